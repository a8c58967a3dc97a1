"""Cost and effect of adaptive sampling (profiles/adaptive_*.jsonl).

    python tools/unbiased_cost.py off PARENT_LIB profiles/adaptive_off_ab.jsonl    (the "off" A/B: that tool's)
    python tools/adaptive_cost.py on profiles/adaptive_on.jsonl
    python tools/adaptive_cost.py kernels profiles/adaptive_kernels.jsonl
    python tools/adaptive_cost.py quality profiles/adaptive_quality.jsonl

on:      bench.py's C2 call (1024 x 1024, 20 frames after 5 warm-up frames, the plan tuned once for the whole
         image) on tile masks: none, all ones, the left half, a checkerboard, a random 10 %, one tile; 3
         interleaved rounds.  Per line the time of the call as bench.py times it (the view's primary-hit pass
         inside: "ms_per_step") and of the same call again over the held cache ("ms_per_step_held"), the active
         fraction, and both times over the whole call's time x that fraction (medians are taken by the reader).
kernels: mcpt_tile_error and mcpt_merge_halves at 1024 x 1024 and 1920 x 1080 on halves of a real render,
         100 calls between two synchronisations, beside the bytes they read and write.
quality: cbox 128 x 128 against a 4096-frame counted render: uniform sampling at N frames and adaptive sampling
         with a budget of 4 N whose threshold the run bisects until it spends N frames per pixel on average
         (within 3 %, 12 steps at most), for (N, min_frames) = (64, 16) and (128, 64); RMSE of both, and where
         the adaptive samples went (a histogram of the per-pixel counts, the mean count of the darker and the
         brighter half of the pixels by the reference image, the tiles whose error read exactly 0 after round 0)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP, ROUNDS = 20, 5, 3


def masks(w, h):
    import numpy as np
    tx, ty = (w + 7) // 8, (h + 7) // 8
    g = np.random.default_rng(1)
    out = {"none": None, "all": np.ones((ty, tx), np.uint8)}
    half = np.zeros((ty, tx), np.uint8)
    half[:, :tx // 2] = 1
    out["half"] = half
    out["checkerboard"] = (np.add.outer(np.arange(ty), np.arange(tx)) % 2).astype(np.uint8)
    tenth = np.zeros(tx * ty, np.uint8)
    tenth[g.permutation(tx * ty)[:tx * ty // 10]] = 1
    out["tenth"] = tenth.reshape(ty, tx)
    one = np.zeros((ty, tx), np.uint8)
    one[ty // 2, tx // 2] = 1
    out["one"] = one
    return out


def on(out_path):
    import torch

    import bench
    import unbiased_cost as UC
    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer(0)
    dsc, cam, shape = UC._scene(rnd, "C2")
    w, h, depth, kw = shape
    recs = []
    with open(out_path, "w") as fh:
        for r in range(ROUNDS):
            for name, mask in masks(w, h).items():
                extra = {} if mask is None else dict(tiles=mask.reshape(-1))
                st = rnd.new_state(w, h, bench.default_seeds(w * h))
                elapsed = bench.timed_render(rnd, dsc, cam, st, STEPS, WARMUP, dict(kw, **extra), 1, False, depth=depth)
                k = rnd.stats()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rnd.render_frames(dsc, cam, st, depth, bench.ATTEMPT, STEPS, **dict(kw, **extra))
                torch.cuda.synchronize()
                held = time.perf_counter() - t0
                rec = {"mask": name, "round": r, "active_fraction": 1.0 if mask is None else float(mask.mean()),
                       "width": w, "height": h, "max_depth": depth, "steps": STEPS, "warmup": WARMUP,
                       "ms_per_step": round(elapsed * 1e3 / STEPS, 4), "ms_per_step_held": round(held * 1e3 / STEPS, 4),
                       "kernel_ms": round(k["kernel_ms"], 4), "launches": k["launches"], "workgroups": k["workgroups"],
                       "frames_per_block": k["frames_per_block"], "primary_cache": k["primary_cache"]}
                recs.append(rec)
                print(json.dumps(rec), flush=True)
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
        import numpy as np
        med = {m: (float(np.median([x["ms_per_step"] for x in recs if x["mask"] == m])),
                   float(np.median([x["ms_per_step_held"] for x in recs if x["mask"] == m]))) for m in masks(w, h)}
        for m, (a, b) in med.items():
            f = [x["active_fraction"] for x in recs if x["mask"] == m][0]
            rec = {"summary": m, "active_fraction": f, "median_ms_per_step": round(a, 4), "median_ms_per_step_held": round(b, 4),
                   "ratio_to_whole_x_fraction": round(a / (med["none"][0] * f), 3),
                   "ratio_to_whole_x_fraction_held": round(b / (med["none"][1] * f), 3)}
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
    dsc.close()


def kernels(out_path):
    import torch

    import bench
    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    rnd = R.Renderer(0)
    data, camj = bench.load_scene("C2")
    dsc = rnd.upload(data)
    cam = S.parse_camera(camj)
    with open(out_path, "w") as fh:
        for w, h in ((1024, 1024), (1920, 1080)):
            a = rnd.new_state(w, h, bench.default_seeds(w * h))
            b = rnd.new_state(w, h, bench.default_seeds(w * h))
            b.seeds = a.seeds
            for half in (a, b):
                rnd.render_frames(dsc, cam, half, 8, 64, 4, frame_begin=half.frames_done, unbiased=True)
            out_h, out_c = rnd.merge_halves(a.hist, a.count, b.hist, b.count)
            n, reps = w * h, 100
            for name, call, bytes_ in (
                    ("mcpt_tile_error", lambda: rnd.tile_error(w, h, a.hist, a.count, b.hist, b.count, 1e-4),
                     40 * n + 4 * ((w + 7) // 8) * ((h + 7) // 8)),
                    ("mcpt_merge_halves", lambda: rnd.merge_halves(a.hist, a.count, b.hist, b.count, out_h, out_c), 60 * n)):
                for _ in range(5):
                    call()
                times = []
                for _ in range(5):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        call()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) / reps)
                times.sort()
                rec = {"kernel": name, "width": w, "height": h, "calls_per_sample": reps, "us_min": round(times[0] * 1e6, 2),
                       "us_median": round(times[2] * 1e6, 2), "us_max": round(times[-1] * 1e6, 2), "bytes": bytes_,
                       "gb_per_s_at_median": round(bytes_ / times[2] / 1e9, 1)}
                print(json.dumps(rec), flush=True)
                fh.write(json.dumps(rec) + "\n")
    dsc.close()


def quality(out_path, ref_frames=4096):
    import numpy as np
    import torch

    from montecarlopathtracing_amd import render as R
    from montecarlopathtracing_amd import scene as S
    from tests import scenes
    rnd = R.Renderer(0)
    dsc = rnd.upload(scenes.cbox())
    cam = S.parse_camera(scenes.CBOX_CAM)
    w = h = 128
    depth = 8
    ref = rnd.new_state(w, h, R.default_seeds(w * h, "msvc15"))  # its own seeds: independent of both arms
    rnd.render_frames(dsc, cam, ref, depth, ref_frames, ref_frames, unbiased=True)
    truth = ref.hist.cpu().numpy()[:, :3].astype(np.float64)

    def rmse(st):
        return float(np.sqrt(((st.hist.cpu().numpy()[:, :3].astype(np.float64) - truth) ** 2).mean()))

    with open(out_path, "w") as fh:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            fh.flush()

        lum = truth.sum(axis=1)
        dark = lum < np.median(lum)  # the darker half of the pixels, by the reference image
        emit({"reference_frames": ref_frames, "width": w, "height": h, "max_depth": depth})
        for n, min_frames in ((64, 16), (128, 64)):
            uni = rnd.new_state(w, h, R.default_seeds(w * h))
            rnd.render_frames(dsc, cam, uni, depth, n, n, unbiased=True)
            emit({"arm": "uniform", "frames": n, "samples_per_pixel": float(n), "rmse": rmse(uni)})
            lo, hi, best = 0.0, 4.0, None
            for it in range(12):  # bisect the threshold to the uniform arm's sample budget
                th = 0.5 * (lo + hi)
                st = rnd.new_state(w, h, R.default_seeds(w * h))
                rep = rnd.render_adaptive(dsc, cam, st, depth, 4 * n, th, min_frames=min_frames, batch=8)
                spp = rep.samples / float(w * h)
                cnt = st.count.cpu().numpy()
                rec = {"arm": "adaptive", "uniform_frames": n, "threshold": th, "budget": 4 * n, "min_frames": min_frames,
                       "batch": 8, "dilate": True, "samples_per_pixel": spp, "fraction_of_budget": rep.fraction,
                       "rounds": len(rep.round_frames), "rmse": rmse(st), "iteration": it,
                       "tiles_quiet_after_round_0": int((rep.errors[0] == 0).sum()) if rep.errors else None,
                       "tiles": int(rep.tiles_x * rep.tiles_y),
                       "count_histogram": {str(int(c)): int(k) for c, k in zip(*np.unique(cnt, return_counts=True))},
                       "mean_count_darker_half": float(cnt[dark].mean()), "mean_count_brighter_half": float(cnt[~dark].mean())}
                emit(rec)
                if best is None or abs(spp - n) < abs(best["samples_per_pixel"] - n):
                    best = rec
                if abs(spp - n) <= 0.03 * n:
                    break
                if spp > n:
                    lo = th
                else:
                    hi = th
            emit(dict(best, arm="adaptive_at_equal_budget"))
    dsc.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] in ("on", "kernels", "quality"):
        {"on": on, "kernels": kernels, "quality": quality}[sys.argv[1]](sys.argv[2])
    else:
        sys.exit(__doc__)
