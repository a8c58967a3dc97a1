"""Cost of alpha cutouts (profiles/cutout_off_ab.jsonl,
profiles/cutout_tex_ab.jsonl, profiles/cutout_on.jsonl).

    python tools/cutout_cost.py off PARENT_LIB profiles/cutout_off_ab.jsonl [pairs]
    python tools/cutout_cost.py tex PARENT_LIB profiles/cutout_tex_ab.jsonl [pairs]
    python tools/cutout_cost.py on profiles/cutout_on.jsonl

off: tools/smooth_cost.py's: plain bench.py lines of the parent commit's
     library and of this tree's, in interleaved pairs, a process each.
tex: tools/texture_cost.py's "textured" calls (bench.py's C2 call and C4 with
     generated vertex normals and a 1024 x 1024 checker on every triangle, the
     plan tuned in that process, 5 warm-up + 20 timed frames) with no alpha
     set, by the parent's library (MCPT_LIB_OVERRIDE) and by this tree's, in
     interleaved pairs, a process each: the cost of the fourth channel and the
     launch-uniform test on a scene that cuts nothing.
on:  the same calls in one process, without an alpha ("textured") and with a
     checker alpha of the colour checker's cells, half the texels 0 and half 1,
     on every triangle ("cutout"), interleaved over 3 rounds; each line carries
     the call's traced segments (mcpt_stats.segments of the same call rendered
     once more with the counters on, untimed)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP, ROUNDS = 20, 5, 3


def checker_alpha(side, cells=16):
    import numpy as np
    yy, xx = np.mgrid[0:side, 0:side]
    return ((((xx * cells) // side + (yy * cells) // side) & 1) == 0).astype(np.float32)


def _textured(rnd, name):
    """texture_cost.on's textured scene of workload `name`, its plan tuned: (scene, camera, state arguments)."""
    import numpy as np

    import bench
    import texture_cost as TC
    from montecarlopathtracing_amd import scene as S
    wl = bench.WORKLOADS[name]
    data, camj = bench.load_scene(name)
    w, h, depth = wl["w"], wl["h"], wl["depth"]
    cam = S.parse_camera(camj)
    dsc = rnd.upload(data)
    rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, TC.CREASE))
    rnd.set_textures(dsc, TC.box_uvs(data.tris), np.zeros(len(data.tris), np.int32), [TC.checker()])
    kw = dict(stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
    st = rnd.new_state(w, h, bench.default_seeds(w * h))
    rnd.set_tuning()
    bench.tune_plan(rnd, dsc, cam, st, STEPS, kw, schedule="auto", depth=depth)
    return dsc, cam, (w, h, depth, kw, len(data.tris))


def _timed(rnd, dsc, cam, shape, segments=False):
    import bench
    w, h, depth, kw, n_tris = shape
    st = rnd.new_state(w, h, bench.default_seeds(w * h))
    elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
    k = rnd.stats()
    rec = {"width": w, "height": h, "max_depth": depth, "steps": STEPS, "warmup": WARMUP,
           "ms_per_step": round(elapsed * 1e3 / STEPS, 4), "kernel_ms": round(k["kernel_ms"], 4),
           "primary_cache": k["primary_cache"], "node_format": k.get("node_format"),
           "value": round(float(w * h) * STEPS * depth / elapsed / 1e6, 2), "unit": "Msamples/s", "triangles": int(n_tris),
           "schedule": dsc.schedule, "tuning": rnd.get_tuning()}
    if segments:  # the same frames once more with the counters on (their kernels are slower: not timed)
        rnd.set_stats(True)
        st = rnd.new_state(w, h, bench.default_seeds(w * h))
        rnd.render_frames(dsc, cam, st, depth, bench.ATTEMPT, WARMUP, **kw)
        rnd.render_frames(dsc, cam, st, depth, bench.ATTEMPT, STEPS, **kw)
        rec["segments"] = int(rnd.stats()["segments"])
        rnd.set_stats(False)
    return rec


def one():
    """A child process of `tex`: one JSON line per workload, the textured call with no alpha set."""
    import torch  # noqa: F401

    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer(0)
    for name in ("C2", "C4"):
        dsc, cam, shape = _textured(rnd, name)
        print(json.dumps(dict(_timed(rnd, dsc, cam, shape), scene=name, variant="textured")), flush=True)
        dsc.close()


def tex(parent_lib, out_path, pairs=3):
    cmd = [sys.executable, os.path.abspath(__file__), "one"]
    with open(out_path, "w") as fh:
        for r in range(pairs):
            order = (("parent", os.path.abspath(parent_lib)), ("this", None))
            for build, lib in (order if r % 2 == 0 else order[::-1]):  # neither build always runs second
                env = dict(os.environ)
                env.pop("MCPT_LIB_OVERRIDE", None)
                if lib:
                    env["MCPT_LIB_OVERRIDE"] = lib
                p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    return p.returncode
                for line in [x for x in p.stdout.splitlines() if x.startswith("{")]:
                    rec = dict(json.loads(line), build=build, pair=r)
                    print(json.dumps({k: rec.get(k) for k in ("build", "pair", "scene", "value", "ms_per_step")}), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
    return 0


def on(out_path):
    import torch  # noqa: F401

    import texture_cost as TC
    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer(0)
    alpha = checker_alpha(TC.SIDE)
    with open(out_path, "w") as fh:
        for name in ("C2", "C4"):
            dsc, cam, shape = _textured(rnd, name)  # the uncut scene's plan, kept for both
            for r in range(ROUNDS):
                for variant in ("textured", "cutout"):
                    if variant == "cutout":
                        rnd.set_texture_alpha(dsc, [alpha], 0.5)
                    else:
                        rnd.clear_texture_alpha(dsc)
                    rec = dict(_timed(rnd, dsc, cam, shape, segments=True), scene=name, variant=variant, round=r,
                               texture=[TC.SIDE, TC.SIDE], alpha_cut_share=round(float((alpha < 0.5).mean()), 4))
                    rec["ns_per_segment"] = round(rec["ms_per_step"] * STEPS * 1e6 / rec["segments"], 4)
                    print(json.dumps({k: rec.get(k) for k in ("scene", "variant", "round", "ms_per_step", "segments",
                                                              "ns_per_segment")}), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
            dsc.close()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "on":
        on(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "one":
        one()
    elif len(sys.argv) >= 4 and sys.argv[1] == "tex":
        sys.exit(tex(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3))
    elif len(sys.argv) >= 4 and sys.argv[1] == "off":
        import smooth_cost
        sys.exit(smooth_cost.off(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    else:
        sys.exit(__doc__)
