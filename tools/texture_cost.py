"""Cost of diffuse texture maps (profiles/texture_on.jsonl,
profiles/texture_off_ab.jsonl).

    python tools/texture_cost.py on profiles/texture_on.jsonl
    python tools/texture_cost.py off PARENT_LIB profiles/texture_off_ab.jsonl [pairs]

on:  bench.py's C2 call and C4 (the plan tuned once on the smooth scene, 5
     warm-up + 20 timed frames, bench.py's own functions), each with vertex
     normals generated at crease 40 alone ("smooth"), the same with the
     primary-hit cache switched off ("smooth_nocache") and with a 1024 x 1024
     checker on every triangle through generated box-projection UVs as well
     ("textured"), interleaved over 3 rounds; one JSON line per timed call.
     Textured against smooth is the feature's cost as a user meets it; the
     cache-off line shows what the primary-hit cache is worth to either.
off: tools/smooth_cost.py's: plain bench.py lines of the parent commit's
     library and of this tree's, in interleaved pairs."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP, ROUNDS, CREASE, SIDE = 20, 5, 3, 40.0, 1024


def box_uvs(tris):
    """Box projection: each triangle is projected along the axis its face
    normal is closest to, the other two coordinates scaled so that the
    scene's longest side spans four repeats."""
    import numpy as np
    v = tris["v"][:, :, :3].astype(np.float64)
    n = np.abs(tris["normal"][:, :3].astype(np.float64))
    axis = np.argmax(np.nan_to_num(n), axis=1)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    scale = 4.0 / float((hi - lo).max())
    a, b = (axis + 1) % 3, (axis + 2) % 3
    idx = np.arange(len(v))
    uv = np.stack([(v[idx, :, a] - lo[a][:, None]) * scale, (v[idx, :, b] - lo[b][:, None]) * scale], axis=-1)
    return uv.astype(np.float32)


def checker(side=SIDE, cells=16):
    import numpy as np
    yy, xx = np.mgrid[0:side, 0:side]
    on = (((xx * cells) // side + (yy * cells) // side) & 1).astype(bool)
    img = np.empty((side, side, 3), np.float32)
    img[on], img[~on] = (0.9, 0.85, 0.8), (0.25, 0.3, 0.45)
    return img


def on(out_path):
    import numpy as np
    import torch  # noqa: F401

    import bench
    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    rnd = R.Renderer(0)
    img = checker()
    with open(out_path, "w") as fh:
        for name in ("C2", "C4"):
            wl = bench.WORKLOADS[name]
            data, camj = bench.load_scene(name)
            w, h, depth = wl["w"], wl["h"], wl["depth"]
            cam = S.parse_camera(camj)
            dsc = rnd.upload(data)
            rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, CREASE))
            uv = box_uvs(data.tris)
            tri_tex = np.zeros(len(data.tris), np.int32)
            kw = dict(stripe_rows=bench.STRIPE_ROWS, stripe_index=0, stripe_count=1, frames_per_launch=0)
            st = rnd.new_state(w, h, bench.default_seeds(w * h))
            rnd.set_tuning()
            bench.tune_plan(rnd, dsc, cam, st, STEPS, kw, schedule="auto", depth=depth)  # the smooth plan, kept for both
            for r in range(ROUNDS):
                tuned = rnd.get_tuning()
                for variant in ("smooth", "smooth_nocache", "textured"):
                    if variant == "textured":
                        rnd.set_textures(dsc, uv, tri_tex, [img])
                    else:
                        rnd.clear_textures(dsc)
                    rnd.set_tuning(**dict(tuned, primary_cache=2 if variant == "smooth_nocache" else tuned["primary_cache"]))
                    st = rnd.new_state(w, h, bench.default_seeds(w * h))
                    elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, kw, 1, False, depth=depth)
                    k = rnd.stats()
                    rec = {"scene": name, "variant": variant, "round": r, "width": w, "height": h, "max_depth": depth,
                           "steps": STEPS, "warmup": WARMUP, "ms_per_step": round(elapsed * 1e3 / STEPS, 4),
                           "kernel_ms": round(k["kernel_ms"], 4), "primary_cache": k["primary_cache"],
                           "node_format": k.get("node_format"),
                           "value": round(float(w * h) * STEPS * depth / elapsed / 1e6, 2), "unit": "Msamples/s",
                           "triangles": int(len(data.tris)), "texture": [SIDE, SIDE], "crease_deg": CREASE,
                           "schedule": dsc.schedule, "tuning": rnd.get_tuning()}
                    print(json.dumps(rec), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
                rnd.set_tuning(**tuned)
            dsc.close()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "on":
        on(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "off":
        import smooth_cost
        sys.exit(smooth_cost.off(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4))
    else:
        sys.exit(__doc__)
