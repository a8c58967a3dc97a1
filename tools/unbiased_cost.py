"""Cost of the opt-in estimator (profiles/unbiased_off_ab.jsonl,
profiles/unbiased_on.jsonl).

    python tools/unbiased_cost.py off PARENT_LIB profiles/unbiased_off_ab.jsonl [pairs]
    python tools/unbiased_cost.py on profiles/unbiased_on.jsonl

off: the estimator off, the parent commit's library (MCPT_LIB_OVERRIDE) against
     this tree's, in interleaved pairs, a process each.  Per pair and build two
     runs: a plain bench.py line (the headline call, "call": "headline"), and
     bench.py's C2 call with jitter on, its plan tuned in that process, 5
     warm-up + 20 timed frames ("call": "jittered").
on:  bench.py's C2 and C4 calls in one process, the plan tuned once for the
     default estimator and kept: the default estimator ("off"), the counted
     history alone ("count_all"), roulette from depth 3 at the workload's own
     max_depth ("roulette3") and at max_depth 64 ("roulette3_d64"), and the
     default estimator at max_depth 64 ("off_d64"), interleaved over 3 rounds;
     each line carries the call's traced segments (mcpt_stats.segments of the
     same call rendered once more with the counters on, untimed)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP, ROUNDS = 20, 5, 3
SETTINGS = (("off", {}, None), ("count_all", dict(unbiased=True), None),
            ("roulette3", dict(unbiased=True, roulette=3), None),
            ("roulette3_d64", dict(unbiased=True, roulette=3), 64), ("off_d64", {}, 64))


def _scene(rnd, name, **tune_kw):
    """Workload `name` uploaded and its plan tuned for the call with `tune_kw`: (scene, camera, shape)."""
    import bench
    from montecarlopathtracing_amd import scene as S
    wl = bench.WORKLOADS[name]
    data, camj = bench.load_scene(name)
    w, h, depth = wl["w"], wl["h"], wl["depth"]
    cam = S.parse_camera(camj)
    dsc = rnd.upload(data)
    kw = dict(stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
    st = rnd.new_state(w, h, bench.default_seeds(w * h))
    rnd.set_tuning()
    bench.tune_plan(rnd, dsc, cam, st, STEPS, dict(kw, **tune_kw), schedule="auto", depth=depth)
    return dsc, cam, (w, h, depth, kw)


def _timed(rnd, dsc, cam, shape, extra, depth=None, segments=False):
    import bench
    w, h, own_depth, kw = shape
    depth = own_depth if depth is None else depth
    kw = dict(kw, **extra)
    st = rnd.new_state(w, h, bench.default_seeds(w * h))
    elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
    k = rnd.stats()
    rec = {"width": w, "height": h, "max_depth": depth, "steps": STEPS, "warmup": WARMUP,
           "ms_per_step": round(elapsed * 1e3 / STEPS, 4), "kernel_ms": round(k["kernel_ms"], 4),
           "primary_cache": k["primary_cache"], "node_format": k.get("node_format"), "schedule": dsc.schedule}
    if segments:  # the same frames once more with the counters on (their kernels are slower: not timed)
        rnd.set_stats(True)
        st = rnd.new_state(w, h, bench.default_seeds(w * h))
        rnd.render_frames(dsc, cam, st, depth, bench.ATTEMPT, WARMUP, **kw)
        rnd.render_frames(dsc, cam, st, depth, bench.ATTEMPT, STEPS, **kw)
        rec["segments"] = int(rnd.stats()["segments"])
        rec["segments_per_step"] = round(rec["segments"] / STEPS, 1)
        rnd.set_stats(False)
    return rec


def one_jittered():
    """A child process of `off`: one JSON line, bench.py's C2 call with jitter on."""
    import torch  # noqa: F401

    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer(0)
    dsc, cam, shape = _scene(rnd, "C2", jitter=True)
    print(json.dumps(dict(_timed(rnd, dsc, cam, shape, dict(jitter=True)), scene="C2", call="jittered")), flush=True)
    dsc.close()


def off(parent_lib, out_path, pairs=4):
    calls = (("headline", [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                           "--warmup", str(WARMUP)]),
             ("jittered", [sys.executable, os.path.abspath(__file__), "one_jittered"]))
    with open(out_path, "w") as fh:
        for r in range(pairs):
            order = (("parent", os.path.abspath(parent_lib)), ("this", None))
            for build, lib in (order if r % 2 == 0 else order[::-1]):  # neither build always runs second
                env = dict(os.environ)
                env.pop("MCPT_LIB_OVERRIDE", None)
                if lib:
                    env["MCPT_LIB_OVERRIDE"] = lib
                for call, cmd in calls:
                    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                    if p.returncode != 0:
                        sys.stderr.write(p.stderr[-3000:])
                        return p.returncode
                    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
                    rec = dict(json.loads(line), build=build, pair=r, call=call)
                    print(json.dumps({k: rec.get(k) for k in ("build", "pair", "call", "value", "ms_per_step")}), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
    return 0


def on(out_path):
    import torch  # noqa: F401

    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer(0)
    with open(out_path, "w") as fh:
        for name in ("C2", "C4"):
            dsc, cam, shape = _scene(rnd, name)
            for r in range(ROUNDS):
                for setting, extra, depth in SETTINGS:
                    rec = dict(_timed(rnd, dsc, cam, shape, extra, depth, segments=(r == 0)), scene=name,
                               estimator=setting, round=r)
                    print(json.dumps({k: rec.get(k) for k in ("scene", "estimator", "max_depth", "round", "ms_per_step",
                                                              "segments_per_step")}), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
            dsc.close()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "on":
        on(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "one_jittered":
        one_jittered()
    elif len(sys.argv) >= 4 and sys.argv[1] == "off":
        sys.exit(off(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    else:
        sys.exit(__doc__)
