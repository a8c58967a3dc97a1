"""Cost of smooth shading (profiles/smooth_on.jsonl, profiles/smooth_off_ab.jsonl,
DESIGN.md 3.13).

    python tools/smooth_cost.py on profiles/smooth_on.jsonl
    python tools/smooth_cost.py off PARENT_LIB profiles/smooth_off_ab.jsonl [pairs]

on:  bench.py's C2 call and C4 (the plan tuned once on the flat scene, 5
     warm-up + 20 timed frames, bench.py's own functions), each flat and with
     vertex normals generated at crease 40, interleaved over 3 rounds; one JSON
     line per timed call, with the scene's share of flat-flagged triangles and
     the generator's host seconds.
off: plain `bench.py --gpus 1 --steps 20 --warmup 5` lines of two builds of
     the library, the parent commit's (PARENT_LIB, through MCPT_LIB_OVERRIDE)
     and this tree's, in interleaved pairs (4 by default; the order within a
     pair alternates), each in a process of its own; the lines as bench.py
     prints them, tagged with their build."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARMUP, ROUNDS, CREASE = 20, 5, 3, 40.0


def on(out_path):
    import numpy as np
    import torch  # noqa: F401

    import bench
    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    rnd = R.Renderer(0)
    with open(out_path, "w") as fh:
        for name in ("C2", "C4"):
            wl = bench.WORKLOADS[name]
            data, camj = bench.load_scene(name)
            w, h, depth = wl["w"], wl["h"], wl["depth"]
            cam = S.parse_camera(camj)
            dsc = rnd.upload(data)
            t0 = time.time()
            vn = S.vertex_normals(data.tris, CREASE)
            gen_s = time.time() - t0
            face = np.repeat(data.tris["normal"][:, None, :3], 3, axis=1)
            flat_share = float((vn.view(np.uint32) == face.view(np.uint32)).all(axis=(1, 2)).mean())
            kw = dict(stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
            st = rnd.new_state(w, h, bench.default_seeds(w * h))
            rnd.set_tuning()
            bench.tune_plan(rnd, dsc, cam, st, STEPS, kw, schedule="auto", depth=depth)  # the flat plan, kept for both
            for r in range(ROUNDS):
                for variant in ("flat", "smooth"):
                    if variant == "flat":
                        rnd.clear_vertex_normals(dsc)
                    else:
                        rnd.set_vertex_normals(dsc, vn)
                    st = rnd.new_state(w, h, bench.default_seeds(w * h))
                    elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
                    k = rnd.stats()
                    rec = {"scene": name, "variant": variant, "round": r, "width": w, "height": h, "max_depth": depth,
                           "steps": STEPS, "warmup": WARMUP, "ms_per_step": round(elapsed * 1e3 / STEPS, 4),
                           "kernel_ms": round(k["kernel_ms"], 4), "primary_cache": k["primary_cache"],
                           "node_format": k.get("node_format"),
                           "value": round(float(w * h) * STEPS * depth / elapsed / 1e6, 2), "unit": "Msamples/s",
                           "triangles": int(len(data.tris)), "flat_flagged_share": round(flat_share, 4),
                           "crease_deg": CREASE, "generator_s": round(gen_s, 3), "schedule": dsc.schedule,
                           "tuning": rnd.get_tuning()}
                    print(json.dumps(rec), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
            dsc.close()


def off(parent_lib, out_path, pairs=4):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)]
    with open(out_path, "w") as fh:
        for r in range(pairs):
            order = (("parent", os.path.abspath(parent_lib)), ("this", None))
            for build, lib in (order if r % 2 == 0 else order[::-1]):  # neither build always runs second
                env = dict(os.environ)
                env.pop("MCPT_LIB_OVERRIDE", None)
                if lib:
                    env["MCPT_LIB_OVERRIDE"] = lib
                p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    return p.returncode
                line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
                rec = dict(json.loads(line), build=build, pair=r)
                print(json.dumps({k: rec.get(k) for k in ("build", "pair", "value", "unit", "ms_per_step")}), flush=True)
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "on":
        on(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "off":
        sys.exit(off(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    else:
        sys.exit(__doc__)
