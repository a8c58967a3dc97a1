"""Test helper (no GPU): the estimator of include/mcpt_hip.h (mcpt_estimator:
the counted history and Russian roulette) restated in numpy float32 and Python
integers, the yardstick of tests/test_gpu_unbiased.py.

  - the LCG draw (shade.cl:1-6) and its inverse, to plant a seed whose k-th
    draw is a chosen value;
  - the roulette decision u < p with u = draw * 2^-15 and p = min(1, max(R)):
    exact, since u is a 15-bit integer times 2^-15 and p a float32, and both
    are exact in float64;
  - the counted running mean in float64.
"""
import collections

import numpy as np

from montecarlopathtracing_amd import _lib as L

LCG_A, LCG_C = 1103515245, 12345
LCG_A_INV = pow(LCG_A, -1, 1 << 32)
TERMINATED = 0xFF000000
DIFFUSE_DRAWS = 2  # randomDirection: the angle and the radius
GLOSSY_DRAWS = 3   # the lobe coin, then randomDirection (a lobe sample that is not rejected)


def lcg(seed):
    """(next seed, 15-bit draw)."""
    seed = (int(seed) * LCG_A + LCG_C) & 0xFFFFFFFF
    return seed, (seed >> 16) & 0x7FFF


def lcg_back(seed):
    """The seed whose successor is `seed`."""
    return (int(seed) - LCG_C) * LCG_A_INV & 0xFFFFFFFF


def draws(seed, k):
    """(seed after k steps, [the k draws])."""
    out = []
    for _ in range(k):
        seed, d = lcg(seed)
        out.append(d)
    return seed, out


def seed_for_kth_draw(value, k, low=0x1234):
    """A seed whose k-th draw (k >= 1) is `value`."""
    s = ((int(value) & 0x7FFF) << 16) | (low & 0xFFFF)
    for _ in range(k):
        s = lcg_back(s)
    assert draws(s, k)[1][-1] == value
    return s


def steps_between(before, after, limit=256):
    """How many LCG steps lead from `before` to `after` (None: more than limit)."""
    s = int(before)
    for k in range(limit + 1):
        if s == int(after):
            return k
        s = lcg(s)[0]
    return None


def survival_probability(R):
    """p = fmin(1.0f, fmax(R.x, fmax(R.y, R.z))) of a float32 reflectance."""
    r = np.asarray(R, np.float32)
    return np.float32(min(np.float32(1.0), max(r[0], max(r[1], r[2]))))


def survives(draw, p):
    """u < p with u = draw * 2^-15: exact in float64."""
    return float(draw) / 32768.0 < float(np.float32(p))


Verdict = collections.namedtuple("Verdict", "applies survives p steps seed")


def predict(mat, seed, depth_before, rr_depth, max_depth, tex=(1.0, 1.0, 1.0)):
    """What mcpt_shade_est does to one live ray that hit material record `mat`
    (an L.MATERIAL row) head on (its glossy lobe sample is never rejected), at
    depth `depth_before`, with the seed `seed`: whether the roulette applies,
    whether the path survives, p, the number of LCG steps and the seed after."""
    t = int(mat["type"])
    new_depth = depth_before + 1
    if t == L.MCPT_DIFFUSE:
        shading, R = DIFFUSE_DRAWS, np.asarray(mat["kd"][:3], np.float32) * np.asarray(tex, np.float32)
    elif t == L.MCPT_GLOSSY:
        shading = GLOSSY_DRAWS
        coin = lcg(seed)[1] & 1
        R = np.asarray(mat["ka_ks"][:3], np.float32) if coin else np.asarray(mat["kd"][:3], np.float32) * np.asarray(
            tex, np.float32)
    elif t == L.MCPT_LIGHT:
        return Verdict(False, True, None, 0, int(seed))
    elif t == L.MCPT_TRANSPARENT:
        return Verdict(False, True, None, None, None)  # the glass's own draws: taken from mcpt_shade
    else:
        return Verdict(False, False, None, 0, int(seed))
    s, _ = draws(seed, shading)
    if not (rr_depth > 0 and new_depth < max_depth and new_depth >= rr_depth):
        return Verdict(False, new_depth < max_depth, None, shading, s)
    p = survival_probability(R)
    s, d = lcg(s)
    return Verdict(True, survives(d, p), p, shading + 1, s)


def counted_mean(samples):
    """The counted history of a (n_frames, n, 4) stack of samples in float64:
    (per-channel sum S, mean S / n_frames, the largest |sample|)."""
    a = np.asarray(samples, np.float64)
    S = a.sum(axis=0)
    return S, S / len(a), float(np.abs(a).max())


def counted_history_f32(samples, max_attempt):
    """history.cl's expression with count_all, one step per frame, in float32
    with a correctly rounded division (the device's is within 2.5 ulp of it):
    (hist, count)."""
    a = np.asarray(samples, np.float32)
    hist = np.zeros(a.shape[1:], np.float32)
    cnt = 0
    for now in a:
        if cnt >= max_attempt:
            break
        hist = ((now + hist * np.float32(cnt)) / np.float32(cnt + 1)).astype(np.float32)
        hist[..., 3] = 0
        cnt += 1
    return hist, cnt


# ------------------------------------------------------------------- debug build
def debug_main():
    """Child process of tests/test_gpu_unbiased.py (python -c): an estimator
    render (counted history, roulette from depth 1) of texture_ref's textured
    room by the MCPT_DEBUG build of the library (MCPT_LIB_OVERRIDE).  Prints
    one JSON line with the violation count and a digest of the result."""
    import hashlib
    import json

    import torch

    from montecarlopathtracing_amd import render as RR
    from montecarlopathtracing_amd import scene as S

    from . import texture_ref as TR
    rnd = RR.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 37, 21, 6, 8
    data, uv, tri_tex, images = TR.room()
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    st = rnd.new_state(w, h, RR.default_seeds(w * h))
    rnd.render_frames(dsc, S.parse_camera(TR.ROOM_CAM), st, TR.ROOM_DEPTH, att, frames, unbiased=True, roulette=1)
    s = rnd.stats()
    torch.cuda.synchronize()
    dg = hashlib.sha256()
    for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
        dg.update(np.ascontiguousarray(a).tobytes())
    print(json.dumps({"violations": s["debug_violations"], "digest": dg.hexdigest()}), flush=True)
