"""The opt-in estimator (mcpt_estimator: the counted history and Russian
roulette; mcpt_render_frames_est, mcpt_shade_est, mcpt_accumulate_all) on the
GPU.  The reference has no such estimator, so the yardsticks are: today's
entry points for "off", float64 sums of the chain's own samples for the
counted history, tests/unbiased_ref.py for the roulette rule ray by ray, the
chain of the project's wavefront kernels (generate -> (intersect, shade_est) x
depth -> accumulate_all) for the fused kernel's bits, and a two-arm comparison
of means for what the roulette must keep.  None of this needs oracle/_ref."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from montecarlopathtracing_amd import _lib as L  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402
from montecarlopathtracing_amd import scene as S  # noqa: E402

from . import scenes  # noqa: E402
from . import shade_cases as SC  # noqa: E402
from . import unbiased_ref as U  # noqa: E402
from .test_jitter_cpu import _entry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
GOLD = os.path.join(ROOT, "tests", "golden")
W, H, FRAMES, ATT = 37, 21, 6, 4  # frame 5 runs past the history's cap (attempt 4)
# scene -> (data, camera, depth, lens (R, F)); the depths leave bounces between rr_depth 3 and the cap
CASES = {"cbox": (scenes.cbox, scenes.CBOX_CAM, 6, (12.0, 1000.0)), "mis": (scenes.mis, scenes.MIS_CAM, 8, (0.25, 13.0))}
RR_DEPTHS = (0, 1, 3)
CUT_ROUNDS = 256  # a cutout scene's chain: at most max_depth + 256 rounds a frame
CACHE_OFF, CACHE_ALWAYS = 2, 1  # mcpt_tuning.primary_cache


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module")
def uploaded(rnd):
    """name -> (DeviceScene, camera, depth, lens), uploaded once."""
    held = {}

    def get(name):
        if name not in held:
            getter, camjson, depth, lens = CASES[name]
            held[name] = (rnd.upload(getter()), S.parse_camera(camjson), depth, lens)
        return held[name]
    yield get
    for dsc, _, _, _ in held.values():
        dsc.close()


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    same = (a.view(np.uint8) == b.view(np.uint8)).reshape(len(a), -1).all(axis=1)
    if not same.all():
        ia = np.nonzero(~same)[0]
        raise AssertionError("%s: %d / %d records differ, first %s\nmine=%r\nref =%r" % (
            what, len(ia), len(a), ia[:8], a[ia[:2]], b[ia[:2]]))


def assert_state_equal(mine, ref, what):
    for k, name in enumerate(("hist", "count", "seeds")):
        assert_bits_equal(mine[k], ref[k], "%s.%s" % (what, name))


def chain(rnd, dsc, cam, w, h, depth, attempt, frames, seeds, mode=L.MODE_EXACT, count_all=True, roulette=0, gen=None,
          cut=False, keep=None):
    """The frame loop out of the wavefront kernels with the estimator:
    generate -> (intersect, shade_est) x depth -> accumulate_all.  gen: None
    (the unjittered generator), "jitter" or a lens (R, F).  cut: a scene with
    cutouts, where a cut hit costs a round and no depth: the rounds go on until
    every ray is terminated.  keep: a list that receives each frame's colours
    (host float32 (n, 4)) as they go into the history."""
    n = w * h
    d_seed = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(rnd.device)
    hist = torch.zeros((n, 4), dtype=torch.float32, device=rnd.device)
    count = torch.zeros(n, dtype=torch.int32, device=rnd.device)
    for f in range(frames):
        colors = torch.ones((n, 4), dtype=torch.float32, device=rnd.device)
        if gen is None:
            rays = rnd.generate_rays(cam, w, h)
        elif gen == "jitter":
            rays = rnd.generate_rays_jittered(cam, w, h, d_seed)
        else:
            rays = rnd.generate_rays_lens(cam, w, h, d_seed, gen)
        hits, rounds = None, 0
        while True:
            if cut:
                if bool(((rays.view(torch.int32).reshape(n, 12)[:, 3] >> 24) != 0).all()):
                    break
                assert rounds < depth + CUT_ROUNDS, "a ray is still live after max_depth + 256 rounds"
            elif rounds == depth:
                break
            hits = rnd.intersect(dsc, rays, hits=hits, mode=mode)
            rnd.shade(dsc, rays, hits, colors, d_seed, depth, roulette=roulette)
            rounds += 1
        if keep is not None:
            keep.append(colors.cpu().numpy())
        if f <= attempt:
            rnd.accumulate(colors, hist, count, attempt, count_all=count_all)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), count.cpu().numpy(), d_seed.cpu().numpy().view(np.uint32)


def state_np(st):
    torch.cuda.synchronize()
    return st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()


def fused(rnd, dsc, cam, w, h, depth, attempt, frames, seeds, **kw):
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(dsc, cam, st, depth, attempt, frames, **kw)
    return state_np(st)


def est_kw(rr):
    return dict(unbiased=True, roulette=rr)


def raw_render(rnd, dsc, cam, st, depth, attempt, frames, jitter=0, lens=None, est=None, frame_begin=0, entry="est"):
    """The C call itself.  lens / est: None (a null pointer) or the struct's
    values.  entry "plain": mcpt_render_frames, "lens": mcpt_render_frames_lens.
    Returns the status."""
    p = L.RenderParams()
    p.width, p.height = st.width, st.height
    p.max_depth, p.max_attempt, p.frame_begin, p.frames = depth, attempt, frame_begin, frames
    p.stripe_rows, p.stripe_index, p.stripe_count = 16, 0, 1
    p.mode, p.frames_per_launch, p.schedule, p.jitter = L.MODE_EXACT, 0, L.SCHED_PAIRED, int(jitter)
    c = np.ascontiguousarray(cam)
    args = [ctypes.byref(p), L.ptr(st.seeds), L.ptr(st.hist), L.ptr(st.count), R._stream()]
    lens_c = None if lens is None else ctypes.byref(L.Lens(*lens))
    if entry == "plain":
        return L.lib().mcpt_render_frames(rnd.ctx, dsc.handle, L.ptr(c), *args)
    if entry == "lens":
        return L.lib().mcpt_render_frames_lens(rnd.ctx, dsc.handle, L.ptr(c), lens_c, *args)
    est_c = None if est is None else ctypes.byref(L.Estimator(*est))
    return L.lib().mcpt_render_frames_est(rnd.ctx, dsc.handle, L.ptr(c), lens_c, est_c, *args)


@pytest.fixture(scope="module")
def chain_ref(rnd, uploaded):
    """(scene, rr_depth, mode, w, h, frames) -> the estimator chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name, rr, mode=L.MODE_EXACT, w=W, h=H, frames=FRAMES):
        key = (name, rr, mode, w, h, frames)
        if key not in held:
            dsc, cam, depth, _ = uploaded(name)
            held[key] = chain(rnd, dsc, cam, w, h, depth, ATT, frames, R.default_seeds(w * h), mode, roulette=rr)
        return held[key]
    return get


# ---------------------------------------------------- 1: off is today's bits
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_null_and_zero_estimator_are_todays_call(rnd, uploaded, name):
    dsc, cam, depth, lens = uploaded(name)
    seeds = R.default_seeds(W * H)
    for jitter, ln, entry in ((0, None, "plain"), (1, None, "plain"), (1, lens, "lens")):
        st = rnd.new_state(W, H, seeds)
        assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, jitter, ln, entry=entry) == 0
        want = state_np(st)
        for what, est in (("a null estimator", None), ("{0, 0}", (0, 0))):
            st = rnd.new_state(W, H, seeds)
            assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, jitter, ln, est) == 0
            assert_state_equal(state_np(st), want, "%s, jitter %d, lens %r: %s" % (name, jitter, ln, what))
    # and the estimator is no no-op: the counted history is another image
    on = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, unbiased=True)
    off = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds)
    assert on[0].tobytes() != off[0].tobytes() and on[1].tobytes() != off[1].tobytes()


def test_null_estimator_call_gives_the_c1_golden(rnd):
    g = np.load(os.path.join(GOLD, "image_c1_cbox.npz"))
    w, h, depth, frames, att = (int(x) for x in g["meta"])
    dsc = rnd.upload(scenes.cbox())
    try:
        for est in (None, (0, 0)):
            st = rnd.new_state(w, h, g["seeds_in"])
            assert raw_render(rnd, dsc, S.parse_camera(scenes.CBOX_CAM), st, depth, att, frames, 0, None, est) == 0
            hist, count, seeds = state_np(st)
            assert_bits_equal(count, g["count"], "count")
            assert_bits_equal(seeds, g["seeds"], "seeds")
            assert_bits_equal(hist, g["hist"], "hist")
    finally:
        dsc.close()


# ------------------------------------------- 2: the counted history, exact part
def test_counted_history_counts_every_frame_and_draws_nothing(rnd, uploaded):
    dsc, cam, _, _ = uploaded("cbox")
    w, h, depth, n = 64, 48, 4, 8
    seeds = R.default_seeds(w * h)
    rnd.set_stats(True)
    try:
        rnd.set_tuning(primary_cache=CACHE_OFF)  # both calls trace every segment themselves
        default = fused(rnd, dsc, cam, w, h, depth, n, n, seeds)
        seg_default = rnd.stats()["segments"]
        counted = fused(rnd, dsc, cam, w, h, depth, n, n, seeds, unbiased=True)
        seg_counted = rnd.stats()["segments"]
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()
    assert (counted[1] == n).all()
    assert (default[1] < n).any()  # the default history skipped samples here: the flag changes something
    assert_bits_equal(counted[2], default[2], "seeds: count_all draws nothing")
    assert seg_counted == seg_default and seg_default > 0  # the same paths, segment for segment
    # the same with the counters compiled out
    assert_state_equal(fused(rnd, dsc, cam, w, h, depth, n, n, seeds, unbiased=True), counted, "without counters")
    # the cnt >= max_attempt stop is unchanged
    capped = fused(rnd, dsc, cam, w, h, depth, 5, n, seeds, unbiased=True)
    assert (capped[1] == 5).all()
    assert_bits_equal(capped[2], default[2], "seeds with max_attempt 5")
    # two stripes of one call each: every pixel of the stripes, and only those
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(dsc, cam, st, depth, n, n, frame_begin=0, stripe_rows=16, stripe_index=0, stripe_count=2,
                      unbiased=True)
    half = state_np(st)[1].reshape(h, w)
    assert (half[0:16] == n).all() and (half[16:32] == 0).all() and (half[32:48] == n).all()


# -------------------------------------- 3: the counted history against float64
def test_counted_history_is_the_float64_mean_of_the_samples(rnd, uploaded):
    dsc, cam, _, _ = uploaded("cbox")
    w, h, depth, n = 64, 48, 4, 8
    seeds = R.default_seeds(w * h)
    samples = []
    hist, count, after = chain(rnd, dsc, cam, w, h, depth, n, n, seeds, keep=samples)
    assert len(samples) == n and (count == n).all()
    S64, mean, M = U.counted_mean(samples)
    bound = 3 * n * 2.0 ** -23 * M
    err = np.abs(hist.astype(np.float64) - mean)[:, :3].max()
    print("counted history: max |hist - S/n| = %.3e (bound %.3e, M = %.4g)" % (err, bound, M))
    assert M > 0 and err <= bound
    assert (hist[:, 3] == 0).all()
    # the fused kernel holds the chain's bits, so the same figure
    got = fused(rnd, dsc, cam, w, h, depth, n, n, seeds, unbiased=True)
    assert_state_equal(got, (hist, count, after), "k_render against the chain")
    # the default history of the same seeds saw the same samples: mean over the non-zero ones
    default = fused(rnd, dsc, cam, w, h, depth, n, n, seeds)
    assert_bits_equal(default[2], after, "seeds")
    nz = np.stack([(s != 0).any(axis=1) for s in samples]).sum(axis=0)
    assert_bits_equal(default[1], nz.astype(np.int32), "the default count: the non-zero samples")
    err_nz = np.abs(default[0].astype(np.float64) * default[1][:, None] - S64)[:, :3].max()
    print("default history: max |hist_nz * count_nz - S| = %.3e (bound %.3e)" % (err_nz, bound * n))
    assert err_nz <= bound * n
    assert (nz < n).mean() > 0.25  # not vacuous: many pixels had zero samples


# ------------------------------------------------ 4: the roulette rule per ray
RULE_RR, RULE_DEPTH = 3, 8
KD_MAX = (0.0, 2.0 ** -15, 0.25, 0.5, 1.0 - 2.0 ** -24, 1.0, 2.0)
RULE_TEX = (0.5, 0.25, 1.0)  # the textured variant's constant texture factor: powers of two, so kd * tex is exact


def _rule_materials():
    mats = []
    for k, v in enumerate(KD_MAX):  # the maximum in another channel each time
        kd = [v / 2, v / 4, v / 8, 0.0]
        kd[k % 3] = v
        mats.append(SC.material(L.MCPT_DIFFUSE, kd=kd))
    glossy = len(mats)
    mats.append(SC.material(L.MCPT_GLOSSY, Ns=20.0, kd=(0.25, 0.125, 0.0625, 0), kaks=(0.5, 0.75, 0.25, 0)))
    light = len(mats)
    mats.append(SC.material(L.MCPT_LIGHT, kaks=(5, 4, 3, 0)))
    glass = len(mats)
    mats.append(SC.material(L.MCPT_TRANSPARENT, Ni=1.5))
    return np.concatenate(mats), glossy, light, glass


def _rule_records():
    """(rays, hits, colors, seeds, mats, rows): every material at depth
    rr - 2, rr - 1, rr and max_depth - 1, head on (d = -n, so no lobe sample is
    rejected), with seeds whose deciding draw is 0, 32767, the two draws around
    p * 2^15, and arbitrary ones."""
    mats, glossy, light, glass = _rule_materials()
    rng = np.random.Generator(np.random.PCG64(77))
    rows = []
    for m in range(len(mats)):
        t = int(mats["type"][m])
        shading = {L.MCPT_DIFFUSE: U.DIFFUSE_DRAWS, L.MCPT_GLOSSY: U.GLOSSY_DRAWS}.get(t, 1)
        deciding = [0, 32767, 1, 8191, 8192, 16383, 16384, 24575, 24576, 32766]
        planted = [U.seed_for_kth_draw(v, shading + 1, low=0x1000 + 7 * i + m) for i, v in enumerate(deciding)]
        planted += [int(x) for x in rng.integers(0, 1 << 32, 6)]
        for depth in (RULE_RR - 2, RULE_RR - 1, RULE_RR, RULE_DEPTH - 1):
            for s in planted:
                rows.append((m, depth, s))
    k = len(rows) | 1  # an odd count; the last record may repeat
    rows = (rows + rows[:1])[:k]
    rays, hits = np.zeros(k, L.RAY), np.zeros(k, L.HIT)
    colors = rng.uniform(0.25, 4.0, (k, 4)).astype(np.float32)
    seeds = np.array([r[2] for r in rows], np.uint32)
    nrm = rng.normal(size=(k, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    hits["normal"][:, :3] = nrm
    hits["point"][:, :3] = rng.uniform(-10, 10, (k, 3)).astype(np.float32)
    hits["t"] = 1.0
    hits["material_id"] = [r[0] for r in rows]
    rays["direction"][:, :3] = -nrm
    rays["origin"][:, :3] = hits["point"][:, :3] + nrm
    rays["origin"][:, 3] = np.array([r[1] for r in rows], np.uint32).view(np.float32)
    rays["direction"][:, 3] = np.arange(k, dtype=np.int32).view(np.float32)
    return rays, hits, colors, seeds, mats, rows


def _run_shade(rnd, dsc, rays, hits, colors, seeds, roulette):
    d_rays, d_hits = R.to_device(rays, rnd.device), R.to_device(hits, rnd.device)
    d_col = torch.from_numpy(colors.copy()).to(rnd.device)
    d_seed = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
    rnd.shade(dsc, d_rays, d_hits, d_col, d_seed, RULE_DEPTH, roulette=roulette)
    torch.cuda.synchronize()
    return R.records(d_rays, L.RAY), d_col.cpu().numpy(), d_seed.cpu().numpy().view(np.uint32)


def _ulps(a, b):
    """|a - b| in units of b's float32 ulp (b: float64, the exact value)."""
    b32 = np.abs(b).astype(np.float32)
    ulp = np.spacing(b32).astype(np.float64)
    return np.abs(a.astype(np.float64) - b) / ulp


@pytest.mark.parametrize("textured", [False, True], ids=["k_shade", "k_shade_tex"])
def test_roulette_rule_per_ray(rnd, textured):
    rays, hits, colors, seeds, mats, rows = _rule_records()
    data = S.SceneData.from_arrays(np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], np.float32), np.zeros(1, np.int32), mats)
    dsc = rnd.upload(data)
    try:
        if textured:  # a constant texture on the dummy triangle: k_shade_tex, whose R on the diffuse lobe is kd * tex
            image = np.broadcast_to(np.array(RULE_TEX, np.float32), (2, 2, 3)).copy()
            rnd.set_textures(dsc, np.zeros((1, 3, 2), np.float32), np.zeros(1, np.int32), [image])
        plain = _run_shade(rnd, dsc, rays, hits, colors, seeds, 0)
        got = _run_shade(rnd, dsc, rays, hits, colors, seeds, RULE_RR)
        low = _run_shade(rnd, dsc, rays, hits, colors, seeds, 1)  # rr_depth 1: every depth here is at or past it
    finally:
        dsc.close()
    flag = lambda r: r["origin"][:, 3].view(np.uint32)  # noqa: E731
    tex = RULE_TEX if textured else (1.0, 1.0, 1.0)
    p_kd = {m: U.survival_probability(mats["kd"][m, :3] * np.array(tex, np.float32)) for m in range(len(KD_MAX))}
    if textured:  # the texture moves p: a roulette that took it from kd alone would decide otherwise
        assert sum(p_kd[m] != U.survival_probability(mats["kd"][m, :3]) for m in p_kd) >= 3
    seen = {"applies": 0, "survives": 0, "killed": 0, "draw0": 0, "draw32767": 0}
    for rr, out in ((RULE_RR, got), (1, low)):
        r, c, s = out
        for i, (m, depth, seed) in enumerate(rows):
            v = U.predict(mats[m], seed, depth, rr, RULE_DEPTH, tex=tex)
            tag = "record %d (material %d, depth %d, seed %#x, rr_depth %d)" % (i, m, depth, seed, rr)
            if not v.applies:  # glass, lights, rays below rr_depth, capped paths: mcpt_shade's bits
                assert r[i].tobytes() == plain[0][i].tobytes() and c[i].tobytes() == plain[1][i].tobytes(), tag
                assert s[i] == plain[2][i], tag
                if v.steps is not None:
                    assert U.steps_between(seed, s[i]) == v.steps and int(s[i]) == v.seed, tag
                continue
            seen["applies"] += 1
            # the input's condition: the shading draws were the ones assumed (no rejected lobe sample)
            assert int(plain[2][i]) == U.lcg_back(v.seed), tag
            assert int(s[i]) == v.seed and U.steps_between(seed, s[i]) == v.steps, tag
            draw = (v.seed >> 16) & 0x7FFF
            seen["draw0"] += draw == 0
            seen["draw32767"] += draw == 32767
            assert r["direction"][i].tobytes() == plain[0]["direction"][i].tobytes(), tag
            assert r["origin"][i, :3].tobytes() == plain[0]["origin"][i, :3].tobytes(), tag
            if v.survives:
                seen["survives"] += 1
                assert flag(r)[i] == flag(plain[0])[i] == depth + 1, tag
                want = plain[1][i].astype(np.float64) / float(v.p)
                assert _ulps(c[i], want).max() <= 3, "%s: colour %r, want %r" % (tag, c[i], want)
            else:
                seen["killed"] += 1
                assert flag(r)[i] == (flag(plain[0])[i] | np.uint32(L.TERMINATED)), tag
                assert not c[i].view(np.uint32).any(), tag
    print("roulette rule:", seen)
    assert seen["survives"] > 100 and seen["killed"] > 100 and seen["draw0"] >= 8 and seen["draw32767"] >= 8
    # p = 0 always ends the path, p >= 1 never does
    r, c, s = low
    mat_of = np.array([m for m, _, _ in rows])
    live_depth = np.array([d for _, d, _ in rows]) < RULE_DEPTH - 1
    assert ((flag(r)[(mat_of == 0) & live_depth] & np.uint32(L.TERMINATED)) != 0).all()
    never = [m for m in p_kd if p_kd[m] > 1.0 - 2.0 ** -15]  # p above the largest u, 1 - 2^-15, never ends a path either
    assert len(never) >= (1 if textured else 3)
    for m in never:
        keep = (mat_of == m) & live_depth
        assert ((flag(r)[keep] & np.uint32(L.TERMINATED)) == 0).all()
        if p_kd[m] == 1.0:
            assert c[keep].tobytes() == plain[1][keep].tobytes()  # over p = 1: the same bits


def test_shade_est_argument_errors(rnd):
    rays, hits, colors, seeds, mats, _ = _rule_records()
    data = S.SceneData.from_arrays(np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], np.float32), np.zeros(1, np.int32), mats)
    dsc = rnd.upload(data)
    try:
        for bad in (-1, 65536):
            d_rays, d_hits = R.to_device(rays, rnd.device), R.to_device(hits, rnd.device)
            d_col = torch.from_numpy(colors.copy()).to(rnd.device)
            d_seed = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
            rc = L.lib().mcpt_shade_est(rnd.ctx, dsc.handle, L.ptr(d_rays), L.ptr(d_hits), L.ptr(d_col), L.ptr(d_seed),
                                        len(rays), RULE_DEPTH, bad, R._stream())
            assert rc == -1 and b"rr_depth" in L.lib().mcpt_last_error()
            torch.cuda.synchronize()
            assert d_col.cpu().numpy().tobytes() == colors.tobytes()
            assert d_seed.cpu().numpy().view(np.uint32).tobytes() == seeds.tobytes()
    finally:
        dsc.close()


# ------------------------------------------------- 5: k_render equals the chain
@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_render_equals_chain(rnd, uploaded, chain_ref, name, mode, rr):
    dsc, cam, depth, _ = uploaded(name)
    ref = chain_ref(name, rr, mode)
    assert (ref[1] == min(FRAMES, ATT)).all()
    for schedule in (L.SCHED_SINGLE, L.SCHED_PAIRED):
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), mode=mode, schedule=schedule,
                    **est_kw(rr))
        assert_state_equal(got, ref, "%s/mode%d/sched%d/rr%d" % (name, mode, schedule, rr))
    if rr:  # the roulette did something: other draws, another image
        off = chain_ref(name, 0, mode)
        assert off[2].tobytes() != ref[2].tobytes() and off[0].tobytes() != ref[0].tobytes()


@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("knobs", [{"quantized": 1}, {"quantized": 2}, {"quantized": 3}, {"stack_window": 1}],
                         ids=lambda k: "%s=%d" % next(iter(k.items())))
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_render_node_formats_and_stack_layouts(rnd, uploaded, chain_ref, name, knobs, rr):
    dsc, cam, depth, _ = uploaded(name)
    try:
        rnd.set_tuning(**knobs)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), **est_kw(rr))
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    if "quantized" in knobs:
        assert s["node_format"] == {1: 1, 2: 0, 3: 2}[knobs["quantized"]]
    else:
        assert s["stack_window"] == 1
    assert_state_equal(got, chain_ref(name, rr), "%r rr%d" % (knobs, rr))


@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("cache", [CACHE_OFF, CACHE_ALWAYS], ids=["never", "always"])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_render_primary_cache_modes(rnd, uploaded, chain_ref, name, cache, rr):
    """rr_depth = 1 puts the roulette on the cached primary hit's shading."""
    dsc, cam, depth, _ = uploaded(name)
    try:
        rnd.set_tuning(primary_cache=cache)
        rnd.drop_caches()
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), **est_kw(rr))
        ran = rnd.stats()["primary_cache"]
    finally:
        rnd.set_tuning()
        rnd.drop_caches()
    assert (ran != 0) == (cache == CACHE_ALWAYS)
    assert_state_equal(got, chain_ref(name, rr), "%s cache %d rr%d" % (name, cache, rr))


@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3)])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_render_tiny_images(rnd, uploaded, chain_ref, name, w, h, rr):
    dsc, cam, depth, _ = uploaded(name)
    got = fused(rnd, dsc, cam, w, h, depth, ATT, FRAMES, R.default_seeds(w * h), **est_kw(rr))
    assert_state_equal(got, chain_ref(name, rr, w=w, h=h), "%s %dx%d rr%d" % (name, w, h, rr))


@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("fpl,split,frames", [(3, ((0, 2), (2, 4)), 6), (2, ((0, 3), (3, 4)), 7)])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_frames_split_across_calls_and_blocks(rnd, uploaded, chain_ref, name, fpl, split, frames, rr):
    """Calls of (frame_begin, frames) in blocks of 2 or 3 frames: the hand-off
    carries the seed past the roulette's draws and the count past the zeros."""
    dsc, cam, depth, _ = uploaded(name)
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for f0, nf in split:
        rnd.render_frames(dsc, cam, st, depth, ATT, nf, frame_begin=f0, frames_per_launch=fpl, **est_kw(rr))
    assert_state_equal(state_np(st), chain_ref(name, rr, frames=frames), "%s split %r rr%d" % (name, split, rr))


@pytest.mark.parametrize("rr", RR_DEPTHS)
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_estimator_two_stripes_one_after_the_other(rnd, uploaded, chain_ref, name, rr):
    dsc, cam, depth, _ = uploaded(name)
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, depth, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k, stripe_count=2,
                          **est_kw(rr))
    assert_state_equal(state_np(st), chain_ref(name, rr), "%s 2 stripes of 8 rows rr%d" % (name, rr))


@pytest.mark.parametrize("rr", [1, 3])
@pytest.mark.parametrize("what", ["lens", "environment", "vertex_normals", "cutouts", "normal_map", "counters"])
def test_estimator_render_equals_chain_with_other_opt_ins(rnd, what, rr):
    """Roulette on with each other opt-in: jitter with a lens, a constant
    environment, vertex normals, textures with cutouts, a normal map; and with
    the counters compiled in.  The chain's kernels read the same scene."""
    from . import bump_cases as BC
    from . import cutout_ref as CR
    seeds = R.default_seeds(W * H)
    gen, cut, kw = None, False, {}
    if what == "cutouts":
        data, uv, tri_tex, images, alphas = CR.room()
        cam, depth = S.parse_camera(CR.ROOM_CAM), CR.ROOM_DEPTH
    else:
        data = scenes.cbox()
        cam, depth = S.parse_camera(scenes.CBOX_CAM), CASES["cbox"][2]
    dsc = rnd.upload(data)
    try:
        if what == "lens":
            gen, kw = CASES["cbox"][3], dict(lens=CASES["cbox"][3])
        elif what == "environment":
            rnd.set_environment(dsc, scale=(0.4, 0.5, 0.7))
        elif what == "vertex_normals":
            rnd.set_vertex_normals(dsc, S.smooth_normals(data.tris, 40.0))
        elif what == "cutouts":
            rnd.set_textures(dsc, uv, tri_tex, images)
            rnd.set_texture_alpha(dsc, alphas, 0.5)
            cut = True
        elif what == "normal_map":
            rnd.set_normal_maps(dsc, *BC.cbox_maps())
        ref = chain(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, roulette=rr, gen=gen, cut=cut)
        off = chain(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, roulette=0, gen=gen, cut=cut)
        if what == "counters":
            rnd.set_stats(True)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, **dict(est_kw(rr), **kw))
        if what == "counters":
            assert rnd.stats()["segments"] > 0
        assert_state_equal(got, ref, "%s rr%d" % (what, rr))
        assert off[2].tobytes() != ref[2].tobytes()  # the roulette drew
    finally:
        rnd.set_stats(False)
        dsc.close()


@pytest.mark.parametrize("rr", RR_DEPTHS)
def test_estimator_render_with_257_materials(rnd, rr):
    """A material table of 257 records: shade_hit reads it from global memory, not from LDS."""
    z = SC.zoo(True, 257)
    dsc = rnd.upload(z.data)
    w = h = 32
    seeds = R.default_seeds(w * h)
    try:
        ref = chain(rnd, dsc, z.cam, w, h, 8, ATT, FRAMES, seeds, roulette=rr)
        got = fused(rnd, dsc, z.cam, w, h, 8, ATT, FRAMES, seeds, **est_kw(rr))
        assert_state_equal(got, ref, "257 materials rr%d" % rr)
        assert (ref[2] != seeds).mean() > 0.9
    finally:
        dsc.close()


# ------------------------------------------------------- 6: argument errors
@pytest.mark.parametrize("est", [(0, 1), (0, 3), (1, -1), (0, -1), (1, 65536), (2, 0), (2, 3), (-1, 0)], ids=repr)
def test_bad_estimator_is_an_argument_error(rnd, uploaded, chain_ref, est):
    dsc, cam, depth, _ = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    before = state_np(st)
    assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, 0, None, est) == -1  # MCPT_ERR_ARG
    msg = L.lib().mcpt_last_error()
    assert b"estimator" in msg or b"roulette" in msg
    assert_state_equal(state_np(st), before, "state after the refused call")
    # a following good call renders correctly
    assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, 0, None, (1, 3)) == 0
    assert_state_equal(state_np(st), chain_ref("cbox", 3), "the good call after")


def test_python_layer_refuses_roulette_without_unbiased(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    with pytest.raises(ValueError, match="unbiased"):
        rnd.render_frames(dsc, cam, st, depth, ATT, 1, roulette=3)
    assert st.frames_done == 0
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b"):
        rnd.render_frames(dsc, cam, st, depth, ATT, 1, unbiased=True, roulette=65536)


# ---------------------------------------------- 7: the roulette keeps the mean
MEAN_W = MEAN_H = 16
MEAN_DEPTH, MEAN_BATCHES = 32, 16
# Frames per batch, chosen on an MI355X so that the roulette-off arm alone has a
# standard error below 1 % of the mean with room to spare (the figures are in
# profiles/unbiased_mean.jsonl and DESIGN.md 3.18).
MEAN_FRAMES = 64
MEAN_ENV = (1.0, 0.9, 0.8)
MEAN_CAM = {"position": [0, 1.0, 0.001], "lookat": [0, 0, 0], "up": [0, 0, -1], "fov": 60.0}


def _quad(y, half):
    a, b, c, d = (-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)
    return [(a, b, c), (a, c, d)]


def mean_scene():
    """A lightless open scene: a diffuse floor (kd max 0.5) that fills the view
    and a facing diffuse quad above the camera (kd max 0.8), under a constant
    environment.  Every path's radiance comes through at least one bounce."""
    verts = np.array(_quad(0.0, 2.0) + _quad(1.5, 1.5), np.float32)
    mats = np.concatenate([SC.material(L.MCPT_DIFFUSE, kd=(0.5, 0.4, 0.3, 0)),
                           SC.material(L.MCPT_DIFFUSE, kd=(0.6, 0.8, 0.7, 0))])
    return S.SceneData.from_arrays(verts, np.array([0, 0, 1, 1], np.int32), mats)


def mean_arms(rnd, frames=MEAN_FRAMES):
    """(batch means with roulette off, with rr_depth = 1): the image-mean
    radiance (r + g + b over every pixel) of MEAN_BATCHES renders per arm, the
    batches' seed sets fixed and distinct."""
    dsc = rnd.upload(mean_scene())
    cam = S.parse_camera(MEAN_CAM)
    n = MEAN_W * MEAN_H
    arms = {0: [], 1: []}
    try:
        rnd.set_environment(dsc, scale=MEAN_ENV)
        for b in range(MEAN_BATCHES):
            for rr in (0, 1):
                seeds = ((np.arange(n, dtype=np.uint64) * 2654435761 + 977 * (2 * b + rr) + 12345)
                         & 0xFFFFFFFF).astype(np.uint32)
                hist, count, _ = fused(rnd, dsc, cam, MEAN_W, MEAN_H, MEAN_DEPTH, frames, frames, seeds,
                                       unbiased=True, roulette=rr)
                assert (count == frames).all()
                arms[rr].append(float(hist[:, :3].astype(np.float64).sum(axis=1).mean()))
    finally:
        dsc.close()
    return np.array(arms[0]), np.array(arms[1])


def mean_figures(off, on):
    """mean and standard error of each arm's batch means, their difference and its sigma."""
    B = len(off)
    m0, m1 = off.mean(), on.mean()
    s0, s1 = off.std(ddof=1) / np.sqrt(B), on.std(ddof=1) / np.sqrt(B)
    return dict(mean_off=m0, mean_on=m1, rel_sigma_off=s0 / m0, rel_sigma_on=s1 / m1, difference=m1 - m0,
                sigma=float(np.hypot(s0, s1)), batches=B)


def test_roulette_keeps_the_mean(rnd):
    """Measured on an MI355X (profiles/unbiased_mean.jsonl): see the module's
    MEAN_FRAMES; the figures are printed before they are asserted."""
    off, on = mean_arms(rnd)
    f = mean_figures(off, on)
    print("roulette mean:", json.dumps({k: float(v) for k, v in f.items()}))
    assert f["mean_off"] > 0
    assert f["rel_sigma_off"] <= 0.01        # the roulette-off arm alone
    assert f["sigma"] <= 0.01 * f["mean_off"]  # so a failure cannot hide in the noise
    assert abs(f["difference"]) <= 5 * f["sigma"]


# ---------------------------------------------------- 8: App from a config key
def test_app_renders_with_roulette_from_config_key(tmp_path):
    from montecarlopathtracing_amd.app import App
    path = tmp_path / "config.json"
    path.write_text(json.dumps(_entry(roulette=3, maxdepth=6)))
    seeds = R.default_seeds(32 * 32)
    app = App(str(path), seeds=seeds, out_dir=str(tmp_path))
    assert app.unbiased is True and app.roulette == 3  # the roulette switched the counted history on
    out = app.run()
    assert os.path.getsize(out) > 0 and app.attempt_count == 4
    got = state_np(app.state)
    assert (got[1] == 3).all()  # four frames into a history of attempt 3: every pixel full
    st = app.renderer.new_state(32, 32, seeds)
    app.renderer.render_frames(app.scene, app.camera, st, 6, 3, 4, unbiased=True, roulette=3)
    assert_state_equal(got, state_np(st), "App with a \"roulette\" key")
    want = tmp_path / "want.hdr"
    S.write_hdr(str(want), st.image(), flip=True)
    assert open(out, "rb").read() == want.read_bytes()
    plain = fused(app.renderer, app.scene, app.camera, 32, 32, 6, 3, 4, seeds)
    assert got[0].tobytes() != plain[0].tobytes()


# ------------------------------------------------------------ 9: debug build
def _digest(state):
    dg = hashlib.sha256()
    for a in state:
        dg.update(np.ascontiguousarray(a).tobytes())
    return dg.hexdigest()


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_debug_build_estimator_bounds_checks_clean(rnd):
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import unbiased_ref; unbiased_ref.debug_main()"], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert len(lines) == 2 and lines[1]["violations"] == 0, lines
    from . import texture_ref as TR
    data, uv, tri_tex, images = TR.room()
    dsc = rnd.upload(data)
    try:
        rnd.set_textures(dsc, uv, tri_tex, images)
        got = fused(rnd, dsc, S.parse_camera(TR.ROOM_CAM), 37, 21, TR.ROOM_DEPTH, 8, 6, R.default_seeds(37 * 21),
                    unbiased=True, roulette=1)
    finally:
        dsc.close()
    assert lines[1]["digest"] == _digest(got)
