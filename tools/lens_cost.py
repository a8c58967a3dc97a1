"""Cost of the thin-lens camera (profiles/lens_off_ab.jsonl,
profiles/lens_jitter_ab.jsonl, profiles/lens_on.jsonl).

    python tools/lens_cost.py off PARENT_LIB profiles/lens_off_ab.jsonl [pairs]
    python tools/lens_cost.py jitter PARENT_LIB profiles/lens_jitter_ab.jsonl [pairs]
    python tools/lens_cost.py on profiles/lens_on.jsonl

off:    tools/smooth_cost.py's: plain bench.py lines of the parent commit's
        library and of this tree's, in interleaved pairs, a fresh process each.
jitter: the same pairs on bench.py's C2 call rendered with jitter and no lens
        (the default launch plan, 5 warm-up + 20 timed frames, bench.py's own
        functions): the jittered forms are the code the lens changed.
on:     the C2 and C4 calls jittered ("jitter") and through a lens ("lens")
        focused on the middle of the scene's box, whose blur disk is 4 pixels
        wide at the box's far end, interleaved over 3 rounds with the default
        launch plan; one JSON line per timed call."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP, ROUNDS, BLUR_PX = 20, 5, 3, 4.0


def scene_lens(data, cam, camj, h):
    """(R, F): focused on the middle of the scene's box along the view axis,
    a blur disk BLUR_PX pixels wide at the box's far end."""
    import numpy as np
    c = cam[0]
    axis = c["direction"][:3].astype(np.float64)
    axis /= np.linalg.norm(axis)
    v = data.tris["v"][:, :, :3].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    depth = (corners - c["center"][:3].astype(np.float64)) @ axis
    focus = float(((lo + hi) / 2 - c["center"][:3].astype(np.float64)) @ axis)
    far = float(depth.max())
    pixel = 2.0 * math.tan(math.radians(float(camj["fov"])) / 2) * far / h
    return BLUR_PX * pixel * focus / (2.0 * (far - focus)), focus


def timed(rnd, dsc, cam, w, h, depth, **kw):
    import bench
    st = rnd.new_state(w, h, bench.default_seeds(w * h))
    kw = dict(kw, stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
    elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
    k = rnd.stats()
    return {"width": w, "height": h, "max_depth": depth, "steps": STEPS, "warmup": WARMUP,
            "ms_per_step": round(elapsed * 1e3 / STEPS, 4), "kernel_ms": round(k["kernel_ms"], 4),
            "primary_cache": k["primary_cache"], "node_format": k.get("node_format"),
            "value": round(float(w * h) * STEPS * depth / elapsed / 1e6, 2), "unit": "Msamples/s",
            "schedule": dsc.schedule}


def on(out_path):
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
            dsc, _ = bench.upload_scene(rnd, data)
            lens = scene_lens(data, cam, camj, h)
            for r in range(ROUNDS):
                for variant in (("jitter", "lens") if r % 2 == 0 else ("lens", "jitter")):
                    kw = {"lens": lens} if variant == "lens" else {"jitter": True}
                    rec = dict(timed(rnd, dsc, cam, w, h, depth, **kw), scene=name, variant=variant, round=r,
                               triangles=int(len(data.tris)), lens=[round(lens[0], 6), round(lens[1], 6)])
                    print(json.dumps(rec), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
            dsc.close()


def jitter_child():
    import torch  # noqa: F401

    import bench
    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    wl = bench.WORKLOADS["C2"]
    data, camj = bench.load_scene("C2")
    rnd = R.Renderer(0)
    dsc, _ = bench.upload_scene(rnd, data)
    rec = timed(rnd, dsc, S.parse_camera(camj), wl["w"], wl["h"], wl["depth"], jitter=True)
    print(json.dumps(dict(rec, scene="C2", variant="jitter")), flush=True)


def jitter_ab(parent_lib, out_path, pairs=4):
    cmd = [sys.executable, os.path.abspath(__file__), "jitter-child"]
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
                rec = dict(json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1]), build=build, pair=r)
                print(json.dumps({k: rec.get(k) for k in ("build", "pair", "value", "unit", "ms_per_step")}), flush=True)
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "on":
        on(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "off":
        import smooth_cost
        sys.exit(smooth_cost.off(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    elif len(sys.argv) >= 4 and sys.argv[1] == "jitter":
        sys.exit(jitter_ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    elif len(sys.argv) == 2 and sys.argv[1] == "jitter-child":
        jitter_child()
    else:
        sys.exit(__doc__)
