"""Cost of environment lighting (profiles/env_on.jsonl).

    python tools/env_cost.py profiles/env_on.jsonl

bench.py's C2 call (the plan tuned once on the unlit scene, 5 warm-up + 20
timed frames, bench.py's own functions) and the open, lightless scene of the
tests (tests/env_ref.py) at 1024^2, each with no environment, a constant one
and a 1024x512 map, interleaved over 3 rounds; one JSON line per timed call."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import bench  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402
from montecarlopathtracing_amd import scene as S  # noqa: E402
from tests import env_ref  # noqa: E402

STEPS, WARMUP, ROUNDS = 20, 5, 3
out_path = sys.argv[1]
rnd = R.Renderer(0)
sky = env_ref.smooth_map(1024, 512)
variants = [("none", None), ("constant", dict(scale=(0.8, 0.9, 1.2))), ("map_1024x512", dict(scale=1.0, map=sky, rotate=37.0))]

wl = bench.WORKLOADS["C2"]
data, camj = bench.load_scene("C2")
scenes = [("C2", data, camj, wl["w"], wl["h"], wl["depth"]),
          ("open_1024", env_ref.open_scene(), env_ref.OPEN_CAM, 1024, 1024, env_ref.OPEN_DEPTH)]
with open(out_path, "w") as fh:
    for name, data, camj, w, h, depth in scenes:
        cam = S.parse_camera(camj)
        dsc = rnd.upload(data)
        kw = dict(stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
        st = rnd.new_state(w, h, bench.default_seeds(w * h))
        rnd.set_tuning()
        bench.tune_plan(rnd, dsc, cam, st, STEPS, kw, schedule="auto", depth=depth)  # the unlit plan, kept for every variant
        for r in range(ROUNDS):
            for vname, env in variants:
                if env is None:
                    rnd.clear_environment(dsc)
                else:
                    rnd.set_environment(dsc, **env)
                st = rnd.new_state(w, h, bench.default_seeds(w * h))
                elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
                k = rnd.stats()
                rec = {"scene": name, "variant": vname, "round": r, "width": w, "height": h, "max_depth": depth,
                       "steps": STEPS, "warmup": WARMUP, "ms_per_step": round(elapsed * 1e3 / STEPS, 4),
                       "kernel_ms": round(k["kernel_ms"], 4), "primary_cache": k["primary_cache"],
                       "value": round(float(w * h) * STEPS * depth / elapsed / 1e6, 2), "unit": "Msamples/s",
                       "lit_pixels": int((st.count > 0).sum().item()), "schedule": dsc.schedule,
                       "tuning": rnd.get_tuning()}
                print(json.dumps(rec), flush=True)
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
        dsc.close()
