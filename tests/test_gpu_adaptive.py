"""Adaptive sampling on the GPU: the tile-subset render (mcpt_render_frames_tiles),
the half-buffer kernels (mcpt_tile_error, mcpt_merge_halves) and the driver
(Renderer.render_adaptive, App).  The reference has none of it; the yardsticks
are the whole-image render of the same frames (a pixel draws from its own seed
chain, so a subset must reproduce its pixels bit for bit and leave every other
pixel's words alone), tests/adaptive_ref.py in float64 for the two kernels and the
selection policy, and plain render_frames calls for the driver's halves.  Images
are at most 64 x 48 and calls a handful of frames."""
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

from . import adaptive_ref as AR  # noqa: E402
from . import bump_cases as BC  # noqa: E402
from . import cutout_ref as CR  # noqa: E402
from . import scenes  # noqa: E402
from .test_jitter_cpu import _entry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W, H = 37, 21        # 5 x 3 tiles, holes on the right and the top edge
PRE, MORE, ATT = 3, 4, 64  # a state that holds 3 frames takes 4 more; no history gate in reach
CASES = {"cbox": (scenes.cbox, scenes.CBOX_CAM, 6, (12.0, 1000.0)), "mis": (scenes.mis, scenes.MIS_CAM, 8, (0.25, 13.0))}


@pytest.fixture(scope="module")
def rnd():
    r = R.Renderer(0)
    yield r
    r.set_tuning()


@pytest.fixture(scope="module")
def uploaded(rnd):
    """name -> (DeviceScene, camera, depth, lens), uploaded once."""
    held = {}

    def get(name):
        if name not in held:
            if name == "room":  # textured, cut out and normal-mapped
                data, uv, tri_tex, images, alphas = CR.room()
                dsc = rnd.upload(data)
                rnd.set_textures(dsc, uv, tri_tex, images)
                rnd.set_texture_alpha(dsc, alphas, 0.5)
                rnd.set_normal_maps(dsc, uv, np.where(tri_tex >= 0, 0, -1).astype(np.int32),
                                    [BC.random_normal_map(4, 4, 40.0, 9)])
                held[name] = (dsc, S.parse_camera(CR.ROOM_CAM), CR.ROOM_DEPTH, None)
            else:
                getter, camjson, depth, lens = CASES[name]
                held[name] = (rnd.upload(getter()), S.parse_camera(camjson), depth, lens)
        return held[name]
    yield get
    for rec in held.values():
        rec[0].close()


def state_np(st):
    torch.cuda.synchronize()
    return st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()


def state_from(rnd, w, h, snap, frames_done):
    st = rnd.new_state(w, h, snap[2])
    st.hist.copy_(torch.from_numpy(snap[0]))
    st.count.copy_(torch.from_numpy(snap[1]))
    st.frames_done = frames_done
    return st


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if len(a) == 0:
        return
    same = (a.view(np.uint8) == b.view(np.uint8)).reshape(len(a), -1).all(axis=1)
    if not same.all():
        ia = np.nonzero(~same)[0]
        raise AssertionError("%s: %d / %d records differ, first %s\nmine=%r\nref =%r" % (
            what, len(ia), len(a), ia[:8], a[ia[:2]], b[ia[:2]]))


def assert_state_equal(mine, ref, what):
    for k, name in enumerate(("hist", "count", "seeds")):
        assert_bits_equal(mine[k], ref[k], "%s.%s" % (what, name))


def tile_masks(w, h):
    """name -> uint8 (tiles_y * tiles_x,): the subsets every setting is rendered on."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    n = tx * ty
    out = {}
    if n > 1:
        one = np.zeros((ty, tx), np.uint8)
        one[ty // 2, tx // 2] = 1
        out["one interior tile"] = one
        corner = np.zeros((ty, tx), np.uint8)
        corner[ty - 1, tx - 1] = 1  # cut by both edges: mostly holes
        out["the corner tile"] = corner
        out["a checkerboard"] = (np.add.outer(np.arange(ty), np.arange(tx)) % 2).astype(np.uint8)
        but = np.ones((ty, tx), np.uint8)
        but[0, min(1, tx - 1)] = 0
        out["all but one tile"] = but
        half = np.zeros(n, np.uint8)
        half[np.random.default_rng(20101).permutation(n)[:n // 2]] = 1
        out["a random half"] = half
    else:
        out["the only tile"] = np.ones(1, np.uint8)
    return {k: (v.reshape(-1) * 7).astype(np.uint8) for k, v in out.items()}  # any nonzero byte means render


def pixel_mask(mask, w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.kron(mask.reshape(ty, tx) != 0, np.ones((8, 8), bool))[:h, :w].reshape(-1)


def check_subsets(rnd, dsc, cam, depth, what, w=W, h=H, **kw):
    """A state that holds PRE frames takes MORE frames on each mask: the active
    pixels come out as the whole-image call's, the others stay as they were."""
    seeds = R.default_seeds(w * h)
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(dsc, cam, st, depth, ATT, PRE, **kw)
    before = state_np(st)
    rnd.render_frames(dsc, cam, st, depth, ATT, MORE, **kw)
    after = state_np(st)
    if kw.get("jitter") or w * h >= 64:  # (a few corner pixels of an unjittered view may draw nothing)
        assert after[2].tobytes() != before[2].tobytes()
    for name, mask in tile_masks(w, h).items():
        sub = state_from(rnd, w, h, before, PRE)
        rnd.render_frames(dsc, cam, sub, depth, ATT, MORE, tiles=mask, **kw)
        got = state_np(sub)
        on = pixel_mask(mask, w, h)
        assert on.any() and sub.frames_done == PRE + MORE
        for k, arr in enumerate(("hist", "count", "seeds")):
            assert_bits_equal(got[k][on], after[k][on], "%s, %s: active %s" % (what, name, arr))
            assert_bits_equal(got[k][~on], before[k][~on], "%s, %s: inactive %s" % (what, name, arr))


def raw_tiles(rnd, dsc, cam, st, depth, frames, tiles="null", jitter=0, lens=None, est=None, frame_begin=0, stripes=1,
              entry="tiles"):
    """The C call itself.  tiles: "null" (a null pointer), or (mask array or None, n_tiles).  Returns the status."""
    p = L.RenderParams()
    p.width, p.height = st.width, st.height
    p.max_depth, p.max_attempt, p.frame_begin, p.frames = depth, ATT, frame_begin, frames
    p.stripe_rows, p.stripe_index, p.stripe_count = 16, 0, stripes
    p.mode, p.frames_per_launch, p.schedule, p.jitter = L.MODE_EXACT, 0, L.SCHED_PAIRED, int(jitter)
    c = np.ascontiguousarray(cam)
    lens_c = None if lens is None else ctypes.byref(L.Lens(*lens))
    est_c = None if est is None else ctypes.byref(L.Estimator(*est))
    tail = [ctypes.byref(p), L.ptr(st.seeds), L.ptr(st.hist), L.ptr(st.count), R._stream()]
    if entry == "est":
        return L.lib().mcpt_render_frames_est(rnd.ctx, dsc.handle, L.ptr(c), lens_c, est_c, *tail)
    if tiles == "null":
        ts = None
    else:
        mask, n = tiles
        ts = ctypes.byref(L.TileSet(None if mask is None else mask.ctypes.data, n, 0))
    return L.lib().mcpt_render_frames_tiles(rnd.ctx, dsc.handle, L.ptr(c), lens_c, est_c, ts, *tail)


# ---------------------------------------------------- G1: off is today's call
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_null_and_full_tile_set_are_todays_call(rnd, uploaded, name):
    dsc, cam, depth, lens = uploaded(name)
    seeds = R.default_seeds(W * H)
    ones = np.full(15, 1, np.uint8)
    for est in (None, (1, 0)):
        for jitter, ln in ((0, None), (1, None), (1, lens)):
            st = rnd.new_state(W, H, seeds)
            assert raw_tiles(rnd, dsc, cam, st, depth, PRE + MORE, jitter=jitter, lens=ln, est=est, entry="est") == 0
            want = state_np(st)
            for what, tiles in (("a null tile set", "null"), ("a mask of ones", (ones, 15))):
                st = rnd.new_state(W, H, seeds)
                assert raw_tiles(rnd, dsc, cam, st, depth, PRE + MORE, tiles, jitter, ln, est) == 0
                assert_state_equal(state_np(st), want, "%s, est %r, jitter %d, lens %r: %s" % (name, est, jitter, ln, what))


# ---------------------------------------------------- G2: subset exactness
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_subset_modes_and_schedules(rnd, uploaded, name, mode, schedule):
    dsc, cam, depth, _ = uploaded(name)
    check_subsets(rnd, dsc, cam, depth, "%s mode %d schedule %d" % (name, mode, schedule), mode=mode, schedule=schedule)


@pytest.mark.parametrize("knobs", [dict(quantized=1), dict(quantized=2), dict(quantized=3), dict(stack_window=1),
                                   dict(primary_cache=2), dict(primary_cache=1), dict(queues=1), dict(queues=8),
                                   dict(pixel_spread=1), dict(pixel_spread=2), dict(tile_order=1), dict(tile_order=2)],
                         ids=lambda k: "-".join("%s%d" % kv for kv in k.items()))
def test_subset_under_every_launch_knob(rnd, uploaded, knobs):
    dsc, cam, depth, _ = uploaded("cbox")
    rnd.set_tuning(**knobs)
    try:
        check_subsets(rnd, dsc, cam, depth, "cbox %r" % (knobs,))
    finally:
        rnd.set_tuning()


@pytest.mark.parametrize("name", ["cbox", "mis"])
@pytest.mark.parametrize("fpl", [2, 3])
def test_subset_through_the_hand_off(rnd, uploaded, fpl, name):
    dsc, cam, depth, _ = uploaded(name)
    check_subsets(rnd, dsc, cam, depth, "%s frames_per_launch %d" % (name, fpl), frames_per_launch=fpl)
    check_subsets(rnd, dsc, cam, depth, "%s frames_per_launch %d, counted" % (name, fpl), frames_per_launch=fpl,
                  unbiased=True)


@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_subset_with_jitter_lens_and_roulette(rnd, uploaded, name):
    dsc, cam, depth, lens = uploaded(name)
    check_subsets(rnd, dsc, cam, depth, name + " jitter", jitter=True)
    check_subsets(rnd, dsc, cam, depth, name + " lens", lens=lens)
    check_subsets(rnd, dsc, cam, depth, name + " roulette 3", unbiased=True, roulette=3)
    check_subsets(rnd, dsc, cam, depth, name + " lens, roulette 3, blocks of 2", lens=lens, unbiased=True, roulette=3,
                  frames_per_launch=2)


def test_subset_of_a_textured_cutout_normal_mapped_scene(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("room")
    for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
        check_subsets(rnd, dsc, cam, depth, "room mode %d" % mode, mode=mode)
    check_subsets(rnd, dsc, cam, depth, "room jitter, blocks of 2", jitter=True, frames_per_launch=2)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (64, 48)])
def test_subset_of_small_and_whole_tile_images(rnd, uploaded, w, h):
    dsc, cam, depth, _ = uploaded("cbox")
    check_subsets(rnd, dsc, cam, depth, "cbox %d x %d" % (w, h), w=w, h=h)
    check_subsets(rnd, dsc, cam, depth, "cbox %d x %d, jittered blocks of 2" % (w, h), w=w, h=h, frames_per_launch=2,
                  jitter=True, unbiased=True)


# ---------------------------------------------------- G3: nothing else is traced
def test_subset_traces_its_own_pixels_only(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("cbox")
    seeds = R.default_seeds(W * H)
    rnd.set_tuning(primary_cache=2)  # both calls trace their primary rays themselves
    rnd.set_stats(True)
    counts = torch.zeros(W * H, dtype=torch.int32, device=rnd.device)
    rnd.set_pixel_segments(counts)
    try:
        st = rnd.new_state(W, H, seeds)
        rnd.render_frames(dsc, cam, st, depth, ATT, MORE)
        total = rnd.stats()["segments"]
        whole = counts.cpu().numpy().astype(np.int64)
        assert total == whole.sum() and (whole >= MORE).all()
        for name, mask in tile_masks(W, H).items():
            counts.zero_()
            st = rnd.new_state(W, H, seeds)
            rnd.render_frames(dsc, cam, st, depth, ATT, MORE, tiles=mask)
            s = rnd.stats()
            got = counts.cpu().numpy().astype(np.int64)
            on = pixel_mask(mask, W, H)
            assert (got[~on] == 0).all(), name
            assert np.array_equal(got[on], whole[on]), name
            assert s["segments"] == whole[on].sum(), name
    finally:
        rnd.set_pixel_segments(None)
        rnd.set_stats(False)
        rnd.set_tuning()


# ---------------------------------------------------- G4: the empty mask, refusals
def test_empty_mask_does_nothing(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    rnd.render_frames(dsc, cam, st, depth, ATT, PRE)
    assert rnd.stats()["launches"] >= 1
    before = state_np(st)
    rnd.render_frames(dsc, cam, st, depth, ATT, MORE, tiles=np.zeros(15, np.uint8))
    assert rnd.stats()["launches"] == 0
    assert_state_equal(state_np(st), before, "an empty mask")


def test_bad_tile_sets_are_refused(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("cbox")
    seeds = R.default_seeds(W * H)
    st = rnd.new_state(W, H, seeds)
    rnd.render_frames(dsc, cam, st, depth, ATT, PRE)
    before = state_np(st)
    mask = tile_masks(W, H)["a checkerboard"]
    bad = {"a null mask": dict(tiles=(None, 15)), "one tile short": dict(tiles=(mask, 14)),
           "one tile long": dict(tiles=(np.append(mask, 1).astype(np.uint8), 16)),
           "no tiles": dict(tiles=(mask, 0)), "two stripes": dict(tiles=(mask, 15), stripes=2)}
    for what, kw in bad.items():
        assert raw_tiles(rnd, dsc, cam, st, depth, MORE, frame_begin=PRE, **kw) == -1, what
        assert b"tile set" in L.lib().mcpt_last_error(), what
        assert_state_equal(state_np(st), before, what)
    # and a good call after them is correct
    assert raw_tiles(rnd, dsc, cam, st, depth, MORE, (mask, 15), frame_begin=PRE) == 0
    got = state_np(st)
    ref = state_from(rnd, W, H, before, PRE)
    rnd.render_frames(dsc, cam, ref, depth, ATT, MORE)
    want = state_np(ref)
    on = pixel_mask(mask, W, H)
    for k in range(3):
        assert_bits_equal(got[k][on], want[k][on], "after the refusals: active")
        assert_bits_equal(got[k][~on], before[k][~on], "after the refusals: inactive")


# ---------------------------------------------------- G5: the half-buffer kernels against float64
def hand_made_halves(w=W, h=H, seed=5):
    """Two halves over 5 x 3 tiles: values log-uniform in [2^-20, 2^10], counts 1..40; tile 0 equal halves,
    tile 1 equal but for one pixel, tile 2 a pixel without samples in B, tile 3 black, tile 5 a pixel without
    samples in A; the right column and the top row of tiles are cut by the image."""
    g = np.random.default_rng(seed)
    a = np.zeros((h, w, 4), np.float32)
    b = np.zeros((h, w, 4), np.float32)
    a[..., :3] = np.exp2(g.uniform(-20, 10, (h, w, 3)))
    b[..., :3] = a[..., :3] * g.uniform(0.5, 1.5, (h, w, 3)).astype(np.float32)
    na = g.integers(1, 41, (h, w)).astype(np.int32)
    nb = g.integers(1, 41, (h, w)).astype(np.int32)
    b[0:8, 0:8] = a[0:8, 0:8]
    b[0:8, 8:16] = a[0:8, 8:16]
    b[3, 11, 1] *= np.float32(1.25)
    nb[5, 20] = 0
    a[0:8, 24:32] = 0
    b[0:8, 24:32] = 0
    na[9, 2] = 0
    return a.reshape(-1, 4), na.reshape(-1), b.reshape(-1, 4), nb.reshape(-1)


def dev(rnd, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(rnd.device)


def test_tile_error_matches_float64(rnd):
    a, na, b, nb = hand_made_halves()
    floor = 1e-4
    ref = AR.tile_error(W, H, a, na, b, nb, np.float32(floor)).reshape(-1)
    da, dna, db, dnb = (dev(rnd, x) for x in (a, na, b, nb))
    got = rnd.tile_error(W, H, da, dna, db, dnb, floor).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (15,)
    assert got[0] == 0.0 and got[3] == 0.0          # equal halves, black halves: exactly 0
    assert np.isposinf(got[2]) and np.isposinf(got[5]) and np.isposinf(ref[2]) and np.isposinf(ref[5])
    assert got[1] > 0.0                             # one differing pixel is seen
    fin = np.isfinite(ref)
    assert fin.sum() == 13 and np.isfinite(got[fin]).all()
    rel = np.abs(got[fin].astype(np.float64) - ref[fin]) / np.maximum(ref[fin], 1e-300)
    rel[ref[fin] == 0] = np.abs(got[fin][ref[fin] == 0])
    print("tile_error: measured %.3g = %.2f * 2^-24, bound %.3g = %.0f * 2^-24" % (
        rel.max(), rel.max() / AR.U, AR.TILE_ERROR_BOUND, AR.TILE_ERROR_BOUND / AR.U))
    assert rel.max() <= AR.TILE_ERROR_BOUND
    # an edge tile averages its in-image pixels only: the corner tile has 5 x 5
    e = AR.pixel_error(a, na, b, nb, np.float32(floor)).reshape(H, W)
    assert abs(got[14] - e[16:, 32:].mean()) <= AR.TILE_ERROR_BOUND * e[16:, 32:].mean()
    assert abs(got[14] - e[16:, 32:].sum() / 64.0) > 0.1 * got[14]
    again = rnd.tile_error(W, H, da, dna, db, dnb, floor).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    for t in (da, dna, db, dnb):  # read-only
        pass
    assert da.cpu().numpy().tobytes() == a.tobytes() and dnb.cpu().numpy().tobytes() == nb.tobytes()


def test_merge_halves_matches_float64(rnd):
    a, na, b, nb = hand_made_halves()
    a[:, 3], b[:, 3] = 3.5, -2.25  # .w is carried only where a half's words are returned whole
    ref, refn = AR.merge(a, na, b, nb)
    da, dna, db, dnb = (dev(rnd, x) for x in (a, na, b, nb))
    hist, count = rnd.merge_halves(da, dna, db, dnb)
    got, gotn = hist.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(gotn, refn.astype(np.int32))
    both = (na > 0) & (nb > 0)
    assert (got[both, 3] == 0).all()
    rel = np.abs(got[both, :3].astype(np.float64) - ref[both, :3]) / np.maximum(ref[both, :3], 1e-300)
    rel[ref[both, :3] == 0] = 0.0
    assert (got[both, :3][ref[both, :3] == 0] == 0).all()
    print("merge_halves: measured %.3g = %.2f * 2^-24, bound %.0f * 2^-24" % (rel.max(), rel.max() / AR.U, AR.MERGE_BOUND / AR.U))
    assert rel.max() <= AR.MERGE_BOUND
    assert_bits_equal(got[nb == 0], a[nb == 0], "nB == 0 returns A's bits")
    assert_bits_equal(got[na == 0], b[na == 0], "nA == 0 returns B's bits")
    # both zero: A's words (zeros for a pixel never sampled)
    z = np.zeros_like(a[:4])
    zn = np.zeros(4, np.int32)
    h0, c0 = rnd.merge_halves(dev(rnd, z), dev(rnd, zn), dev(rnd, z), dev(rnd, zn))
    assert not h0.cpu().numpy().any() and not c0.cpu().numpy().any()
    h2, c2 = rnd.merge_halves(da, dna, db, dnb)
    assert h2.cpu().numpy().tobytes() == got.tobytes() and c2.cpu().numpy().tobytes() == gotn.tobytes()


def test_half_buffer_calls_refuse_bad_arguments(rnd):
    a, na, b, nb = hand_made_halves()
    da, dna, db, dnb = (dev(rnd, x) for x in (a, na, b, nb))
    for floor in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*tile_error"):
            rnd.tile_error(W, H, da, dna, db, dnb, floor)
    skew = torch.zeros(W * H * 4 + 4, dtype=torch.float32, device=rnd.device)[1:1 + W * H * 4]
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*aligned"):
        rnd.tile_error(W, H, skew, dna, db, dnb, 1e-4)
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*aligned"):
        rnd.merge_halves(da, dna, skew, dnb)
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b"):
        rnd.tile_error(0, H, da, dna, db, dnb, 1e-4)


# ---------------------------------------------------- G6: the driver
def halves_by_hand(rnd, dsc, cam, depth, w, h, frames, rounds, **kw):
    """Two halves on one seed chain out of plain whole-image render_frames calls: per round n, n / 2 frames into
    A and then into B.  Returns the merged (hist, count, seeds)."""
    a = rnd.new_state(w, h, R.default_seeds(w * h))
    b = rnd.new_state(w, h, R.default_seeds(w * h))
    b.seeds = a.seeds
    for n in rounds:
        for half in (a, b):
            rnd.render_frames(dsc, cam, half, depth, frames, n // 2, frame_begin=half.frames_done, unbiased=True, **kw)
    hist, count = rnd.merge_halves(a.hist, a.count, b.hist, b.count)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), count.cpu().numpy(), a.seeds_np()


@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_driver_with_an_infinite_threshold_is_round_zero(rnd, uploaded, name):
    dsc, cam, depth, lens = uploaded(name)
    for kw in (dict(), dict(lens=lens, roulette=3)):
        st = rnd.new_state(W, H, R.default_seeds(W * H))
        rep = rnd.render_adaptive(dsc, cam, st, depth, 12, float("inf"), min_frames=6, batch=4, **kw)
        assert st.frames_done == 6 and rep.frames_issued == 6 and rep.round_frames == [6]
        assert len(rep.masks) == 1 and not rep.masks[0].any()
        assert rep.samples == 6 * W * H and rep.fraction == 0.5
        assert_state_equal(state_np(st), halves_by_hand(rnd, dsc, cam, depth, W, H, 12, [6], **kw), name + " inf")


def test_driver_with_a_zero_threshold_runs_whole_image_rounds_to_the_budget(rnd):
    w = h = 21  # 3 x 3 tiles of lit floor (cbox will not do: a dark tile's first samples are all black, its error 0)
    dsc = rnd.upload(AR.horizon_scene())
    try:
        rnd.set_environment(dsc, scale=AR.HORIZON_SKY)
        cam, depth = S.parse_camera(AR.FLOOR_CAM), AR.HORIZON_DEPTH
        st = rnd.new_state(w, h, R.default_seeds(w * h))
        rep = rnd.render_adaptive(dsc, cam, st, depth, 10, 0.0, min_frames=4, batch=4, dilate=False)
        assert rep.round_frames == [4, 4, 2] and st.frames_done == 10  # the last round cut to the budget
        assert len(rep.masks) == 2 and all(m.all() for m in rep.masks)   # every tile of this view is noisy
        assert rep.samples == 10 * w * h and rep.fraction == 1.0
        assert_state_equal(state_np(st), halves_by_hand(rnd, dsc, cam, depth, w, h, 10, [4, 4, 2]), "floor zero")
    finally:
        dsc.close()


def test_driver_leaves_the_sky_alone(rnd):
    w, h, frames, min_frames, batch, threshold = 64, 48, 12, 4, 4, 1e-6
    dsc = rnd.upload(AR.horizon_scene())
    try:
        rnd.set_environment(dsc, scale=AR.HORIZON_SKY)
        st = rnd.new_state(w, h, R.default_seeds(w * h))
        rep = rnd.render_adaptive(dsc, S.parse_camera(AR.HORIZON_CAM), st, AR.HORIZON_DEPTH, frames, threshold,
                                  min_frames=min_frames, batch=batch)
        hist, count, _ = state_np(st)
    finally:
        dsc.close()
    count = count.reshape(h, w)
    assert (count[32:] == min_frames).all()  # sky tiles outside the dilation: rows of tiles 4 and 5
    assert (count[:24] == frames).all()      # floor tiles: rows of tiles 0-2
    assert all((e[4:] == 0).all() for e in rep.errors)  # identical samples: the error is exactly 0
    sky = hist.reshape(h, w, 4)[32:]
    assert (sky[..., :3] == np.asarray(AR.HORIZON_SKY, np.float32)).all()
    want, masks, issued = AR.replay(rep.errors, w, h, frames, threshold, min_frames, batch, True)
    assert np.array_equal(count, want) and issued == st.frames_done == rep.frames_issued
    assert len(masks) == len(rep.masks) and all(np.array_equal(m, r != 0) for m, r in zip(masks, rep.masks))
    assert rep.samples == count.sum() and rep.fraction == count.sum() / float(w * h * frames)


def test_driver_refuses_before_any_call(rnd, uploaded):
    dsc, cam, depth, _ = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    before = state_np(st)
    for kw in (dict(frames=7), dict(min_frames=3), dict(batch=5), dict(min_frames=14), dict(frames=0),
               dict(threshold=-1.0), dict(threshold=float("nan")), dict(floor=0.0), dict(floor=float("inf"))):
        args = dict(frames=12, threshold=0.1, min_frames=4, batch=4, floor=1e-4)
        args.update(kw)
        with pytest.raises(ValueError, match="render_adaptive"):
            rnd.render_adaptive(dsc, cam, st, depth, args.pop("frames"), args.pop("threshold"), **args)
    st.frames_done = 2
    with pytest.raises(ValueError, match="fresh"):
        rnd.render_adaptive(dsc, cam, st, depth, 12, 0.1, min_frames=4)
    assert_state_equal(state_np(st), before, "refused calls")


# ---------------------------------------------------- G7: App
def test_app_renders_adaptively_from_a_config_key(tmp_path):
    from montecarlopathtracing_amd.app import App
    spec = {"threshold": 0.05, "min_frames": 4, "batch": 2, "map": True}
    path = tmp_path / "config.json"
    path.write_text(json.dumps(_entry(adaptive=spec, maxdepth=6, attempt=10)))  # 11 frames: a budget of 10
    seeds = R.default_seeds(32 * 32)
    app = App(str(path), seeds=seeds, out_dir=str(tmp_path))
    assert app.unbiased is True and app.adaptive_budget() == 10
    out = app.run()
    assert out == app.dumped and app.attempt_count == 11 and app.adaptive_report is not None
    st = app.renderer.new_state(32, 32, seeds)
    rep = app.renderer.render_adaptive(app.scene, app.camera, st, 6, 10, 0.05, min_frames=4, batch=2)
    assert_state_equal(state_np(app.state), state_np(st), "App's state")
    assert rep.round_frames == app.adaptive_report.round_frames
    S.write_hdr(str(tmp_path / "want.hdr"), st.image(), flip=True)
    assert open(out, "rb").read() == open(tmp_path / "want.hdr", "rb").read()
    grey = np.zeros((32, 32, 4), np.float32)
    grey[..., :3] = (state_np(st)[1].astype(np.float32) / np.float32(10)).reshape(32, 32, 1)
    S.write_hdr(str(tmp_path / "want_samples.hdr"), grey, flip=True)
    samples = App.samples_path(out)
    assert samples.endswith("cbox_samples.hdr") or samples.endswith("_samples.hdr")
    assert open(samples, "rb").read() == open(tmp_path / "want_samples.hdr", "rb").read()
    again = app.update(5)  # the driver ran once; a later update renders nothing more
    assert again is app.state and app.state.frames_done == st.frames_done


# ---------------------------------------------------- G8: the debug library
def _digest(state):
    dg = hashlib.sha256()
    for a in state:
        dg.update(np.ascontiguousarray(a).tobytes())
    return dg.hexdigest()


def test_debug_build_renders_a_checkerboard_subset_clean(rnd, uploaded):
    assert os.path.exists(DEBUG_LIB), "debug build missing (__graft_entry__.build makes it)"
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import test_gpu_adaptive as t; t.debug_main()"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert len(lines) == 3
    dsc, cam, depth, _ = uploaded("cbox")
    for c in lines[1:]:
        assert c["violations"] == 0, c
        st = rnd.new_state(W, H, R.default_seeds(W * H))
        rnd.render_frames(dsc, cam, st, depth, ATT, MORE, tiles=tile_masks(W, H)["a checkerboard"], frames_per_launch=2,
                          mode=c["mode"])
        assert c["digest"] == _digest(state_np(st)), c


def debug_main():
    """The child of the test above, run with the MCPT_DEBUG build: a checkerboard subset in both modes."""
    r = R.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    getter, camjson, depth, _ = CASES["cbox"]
    dsc = r.upload(getter())
    for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
        st = r.new_state(W, H, R.default_seeds(W * H))
        r.render_frames(dsc, S.parse_camera(camjson), st, depth, ATT, MORE, tiles=tile_masks(W, H)["a checkerboard"],
                        frames_per_launch=2, mode=mode)
        s = r.stats()
        print(json.dumps({"mode": mode, "violations": s["debug_violations"], "digest": _digest(state_np(st))}), flush=True)
    dsc.close()
