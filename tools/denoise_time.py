"""Device time of the denoise post-pass (mcpt_denoise: one k_denoise_prepare and
`iterations` k_denoise_iter launches) at the sizes users run.

    python tools/denoise_time.py [--out profiles/denoise_time.jsonl] [--reps 50] [--windows 5]

cbox, 20 frames rendered once per size; then, after 10 warm-up calls, `windows`
windows of `reps` back-to-back calls each between two device events.  One JSON
line per size and iteration count: the median, fastest and slowest window in ms per call, and the
compulsory-traffic floor beside it: (48 B read + 16 B written) x pixels x
iterations at the measured 6.1 TB/s read peak.  MCPT_LIB_OVERRIDE
times another build of the library (an A/B runs both alternately: --ab LIB)."""
import argparse
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_READ_BPS = 6.1e12
SIZES = ((1024, 1024), (1920, 1080))


def measure(sizes, iteration_counts, reps, windows):
    import torch

    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    from tests import scenes
    rnd = R.Renderer(0)
    dsc = rnd.upload(scenes.cbox())
    cam = S.parse_camera(scenes.CBOX_CAM)
    rows = []
    for (w, h), iterations in itertools.product(sizes, iteration_counts):
        st = rnd.new_state(w, h)
        rnd.render_frames(dsc, cam, st, 8, 20, 20)
        hits = rnd.first_hits(dsc, cam, w, h)
        for _ in range(10):
            rnd.denoise(dsc, hits, st, iterations=iterations)
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                rnd.denoise(dsc, hits, st, iterations=iterations)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        ms.sort()
        floor_ms = 64.0 * w * h * iterations / PEAK_READ_BPS * 1e3
        rows.append({"width": w, "height": h, "iterations": iterations, "reps": reps, "windows": windows,
                     "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1],
                     "floor_ms": floor_ms, "ratio_to_floor": ms[len(ms) // 2] / floor_ms,
                     "lib": os.environ.get("MCPT_LIB_OVERRIDE", "")})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_time.jsonl"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iterations", type=int, nargs="+", default=[5, 3],
                    help="iteration counts to time (5: the size the floor is quoted for; 3: the default)")
    ap.add_argument("--ab", default=None, nargs="+",
                    help="other libmcpt_hip builds: time this one and them, alternately, in child processes")
    ap.add_argument("--rounds", type=int, default=3, help="--ab: alternations")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.ab and not a.child:  # interleaved A/B: a fresh process per arm and round, each loading its library
        rows = []
        for r in range(a.rounds):
            for lib in [""] + list(a.ab):
                env = dict(os.environ)
                env.pop("MCPT_LIB_OVERRIDE", None)
                if lib:
                    env["MCPT_LIB_OVERRIDE"] = lib
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                                      "--windows", str(a.windows), "--iterations"] + [str(i) for i in a.iterations],
                                     env=env, capture_output=True, text=True, timeout=600, check=True).stdout
                for line in out.splitlines():
                    if line.startswith("{"):
                        rows.append(dict(json.loads(line), round=r))
                        print(json.dumps(rows[-1]), flush=True)
    else:
        rows = measure(SIZES, a.iterations, a.reps, a.windows)
        for row in rows:
            print(json.dumps(row), flush=True)
    if not a.child:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
