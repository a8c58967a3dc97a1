"""Quality sweep behind Renderer.denoise's defaults (render.DENOISE_DEFAULTS).

    python tools/denoise_sweep.py [--out profiles/denoise_sigma_sweep.jsonl]

C1 (cbox 256x256, depth 4) and C2 at 512x512 (cbox diffuse-only, depth 8), 20
frames each, against a 4096-frame render of the same view from other seeds.
iterations {3, 4, 5, 6} x sigma_plane {0.005, 0.01, 0.02} x sigma_color {0, 4,
16} x the raw image's mean luminance over the filtered pixels, sigma_normal
0.5.  One JSON line per (scene, setting) with the RMSE over the filtered pixels,
then one "best" line: the setting with the least mean of RMSE / raw RMSE over
the two scenes (sigma_color as its multiple of the mean luminance)."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITER = (3, 4, 5, 6)
SIGMA_PLANE = (0.005, 0.01, 0.02)
SIGMA_COLOR_X = (0.0, 4.0, 16.0)
CASES = (("C1", 256, 4, False), ("C2_512", 512, 8, True))
FRAMES, REF_FRAMES = 20, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_sigma_sweep.jsonl"))
    a = ap.parse_args()
    import torch

    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    from tests import denoise_ref as D
    from tests import scenes
    rnd = R.Renderer(0)
    cam = S.parse_camera(scenes.CBOX_CAM)
    rows, score = [], {}
    for name, size, depth, diffuse in CASES:
        data = scenes.cbox_diffuse() if diffuse else scenes.cbox()
        dsc = rnd.upload(data)
        seeds = R.default_seeds(size * size)
        ref_st = rnd.new_state(size, size, seeds ^ np.uint32(0xA5A5A5A5))
        rnd.render_frames(dsc, cam, ref_st, depth, REF_FRAMES, REF_FRAMES)
        st = rnd.new_state(size, size, seeds)
        rnd.render_frames(dsc, cam, st, depth, FRAMES, FRAMES)
        hits = rnd.first_hits(dsc, cam, size, size)
        torch.cuda.synchronize()
        filt = D.filtered_mask(R.records(hits, L.HIT), data.mats)
        ref = ref_st.hist.cpu().numpy()[filt, :3].astype(np.float64)
        raw = st.hist.cpu().numpy()[filt, :3].astype(np.float64)
        rmse_raw = float(np.sqrt(((raw - ref) ** 2).mean()))
        lum = float((raw @ np.array([0.2126, 0.7152, 0.0722])).mean())
        for it, sx, scx in itertools.product(ITER, SIGMA_PLANE, SIGMA_COLOR_X):
            den = rnd.denoise(dsc, hits, st, iterations=it, sigma_normal=0.5, sigma_plane=sx, sigma_color=scx * lum)
            got = den.cpu().numpy()[filt, :3].astype(np.float64)
            rmse = float(np.sqrt(((got - ref) ** 2).mean()))
            rows.append({"scene": name, "size": size, "frames": FRAMES, "iterations": it, "sigma_normal": 0.5,
                         "sigma_plane": sx, "sigma_color_x_lum": scx, "mean_luminance": lum,
                         "rmse": rmse, "rmse_raw": rmse_raw, "ratio": rmse / rmse_raw})
            print(json.dumps(rows[-1]), flush=True)
            score.setdefault((it, sx, scx), []).append(rmse / rmse_raw)
        dsc.close()
    best = min(score, key=lambda k: (float(np.mean(score[k])), k))
    rows.append({"best": {"iterations": best[0], "sigma_plane": best[1], "sigma_color_x_lum": best[2]},
                 "mean_ratio": float(np.mean(score[best])), "ratios": score[best]})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
