"""Diffuse texture maps (opt-in; mcpt_scene_set_textures, mcpt_texture_eval):
the diffuse lobe's kd is multiplied by a bilinear, repeating lookup of the hit
triangle's texture.  The reference has none, so the yardsticks are the
project's own: the float64 restatement of the lookup (tests/texture_ref.py) for
mcpt_texture_eval, and for the fused kernel the chain of wavefront kernels
(tests/test_gpu_jitter.py's harness), whose k_shade applies the same lookup to
the hit k_intersect reports.  None of this needs oracle/_ref."""
import hashlib
import json
import os
import socket
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
from . import smooth_ref as SR  # noqa: E402
from . import texture_ref as T  # noqa: E402
from .test_gpu_jitter import assert_bits_equal, assert_state_equal, chain, fused, state_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W, H, FRAMES, ATT = 48, 40, 6, 4  # 6 frames run past the history's cap (attempt 4)
FLT_MAX = np.float32(3.402823466e+38)


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module")
def rooms(rnd):
    """name -> (textured DeviceScene, camera, depth, SceneData, (uv, tri_tex, images)).
    "closed": textures only; "smooth": with generated vertex normals as well;
    "opened": under a constant environment."""
    held = {}

    def get(name):
        if name not in held:
            data, uv, tri_tex, images = T.room(opened=name == "opened")
            dsc = rnd.upload(data)
            rnd.set_textures(dsc, uv, tri_tex, images)
            if name == "smooth":
                rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, 40.0))
            if name == "opened":
                rnd.set_environment(dsc, scale=(0.8, 0.9, 1.2))
            held[name] = (dsc, S.parse_camera(T.ROOM_CAM), T.ROOM_DEPTH, data, (uv, tri_tex, images))
        return held[name]
    yield get
    for rec in held.values():
        rec[0].close()


@pytest.fixture(scope="module")
def chain_ref(rnd, rooms):
    """(room, mode, frames, jitter, w, h) -> the chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name="closed", mode=L.MODE_EXACT, frames=FRAMES, jitter=False, w=W, h=H):
        key = (name, mode, frames, jitter, w, h)
        if key not in held:
            dsc, cam, depth = rooms(name)[:3]
            held[key] = chain(rnd, dsc, cam, w, h, depth, ATT, [(frames, jitter)], R.default_seeds(w * h), mode)
        return held[key]
    return get


# ------------------------------------------------------ the lookup vs float64
# Largest error of mcpt_texture_eval against tests/texture_ref.py (float64), max
# |gpu - ref| over the components of every query below (texels up to 4.0),
# measured on an MI355X, and the bound held: 8x that, test_gpu_smooth.py's
# margin, since fp32 rounding varies with the query set.  Measured: 1.381e-5
# (UVs reach 3.5 and a 5-texel row, so x reaches 17 with a float32 step of
# 2e-6, times a texel contrast of up to 4).  The mutants' largest errors, each
# of which must stay 1000x above the bound: u/v swapped 2.98, no v flip 3.62,
# nearest texel 2.62, b1/b2 swapped 3.04, clamp instead of wrap 3.71.
LOOKUP_MEASURED = 1.381e-5
LOOKUP_BOUND = 8 * LOOKUP_MEASURED


def lookup_mesh():
    """The 80-triangle icosphere with spherical UVs (seam triangles included)
    on the 5x3 texture; four quads' triangles with UVs below 0 and above 1 on
    the 2x2 and the 1x1; a sliver whose fp32 den is 0; untextured triangles."""
    ball = SR.icosphere(1)
    rng = np.random.Generator(np.random.PCG64(21))
    flat = rng.uniform(-1.0, 1.0, (8, 3, 3)).astype(np.float32) + np.float32(4.0)
    sliver = np.array([[[3, 0, 0], [4, 0, 0], [5, 2.0 ** -13, 0]]], np.float32)
    plain = rng.uniform(-1.0, 1.0, (4, 3, 3)).astype(np.float32) - np.float32(4.0)
    verts = np.concatenate([ball, flat, sliver, plain])
    n = len(verts)
    uv = np.zeros((n, 3, 2), np.float32)
    tri_tex = np.full(n, -1, np.int32)
    nb = len(ball)
    uv[:nb] = T.spherical_uv(ball, (0, 0, 0))
    tri_tex[:nb] = 2
    uv[nb:nb + 8] = rng.uniform(-2.5, 3.5, (8, 3, 2)).astype(np.float32)
    tri_tex[nb:nb + 4], tri_tex[nb + 4:nb + 8] = 1, 0
    tri_tex[nb + 6:nb + 8] = 2  # the 5x3 one far outside [0, 1] too
    uv[nb + 8] = np.array([[0.3, 0.6], [0.9, 0.1], [0.1, 0.9]], np.float32)
    tri_tex[nb + 8] = 2
    rt = np.random.Generator(np.random.PCG64(22))
    images = [rt.uniform(0.0, 4.0, (1, 1, 3)).astype(np.float32), rt.uniform(0.0, 4.0, (2, 2, 3)).astype(np.float32),
              rt.uniform(0.0, 4.0, (3, 5, 3)).astype(np.float32)]
    seams = (uv[:nb, :, 0].max(1) - uv[:nb, :, 0].min(1)) > 0.5
    assert seams.sum() >= 4
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    data = S.SceneData.from_arrays(verts, np.zeros(n, np.int32), mats)
    return data, uv, tri_tex, images, nb + 8


def lookup_queries(data, skip):
    """(tri ids, points) float32: per triangle (but `skip`) interior points,
    its vertices, edge midpoints and points outside that hit the clamps."""
    keep = np.array([i for i in range(len(data.tris)) if i != skip], np.int32)
    v = data.tris["v"][keep][:, :, :3].astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(23))
    bary = [rng.dirichlet((1.0, 1.0, 1.0), (len(keep), 98))]
    fixed = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5],
             [1.05, -.05, 0], [-.05, 1.05, 0], [-.03, -.02, 1.05], [.6, .6, -.2], [-.2, .6, .6], [.55, -.1, .55]]
    bary.append(np.broadcast_to(np.array(fixed, np.float64), (len(keep), len(fixed), 3)))
    b = np.concatenate(bary, axis=1)
    pts = np.einsum("tkc,tcx->tkx", b, v).reshape(-1, 3).astype(np.float32)
    return np.repeat(keep, b.shape[1]), pts


def test_lookup_matches_float64(rnd):
    data, uv, tri_tex, images, sliver = lookup_mesh()
    dsc = rnd.upload(data)
    try:
        rnd.set_textures(dsc, uv, tri_tex, images)
        ids, pts = lookup_queries(data, sliver)
        assert len(ids) >= 10000
        got = rnd.texture_eval(dsc, ids, pts).cpu().numpy()
        assert got.shape == (len(ids), 4) and (got[:, 3] == 1).all() and np.isfinite(got).all()
        verts = data.tris["v"][:, :, :3]
        ref = T.texture_factor(verts, uv, tri_tex, images, ids, pts)
        err = float(np.abs(got - ref).max())
        errs = {m: float(np.abs(got - T.texture_factor(verts, uv, tri_tex, images, ids, pts, mutant=m)).max())
                for m in T.MUTANTS}
        print("lookup: %d queries, max error %.3e (bound %.3e); mutants %s" % (
            len(ids), err, LOOKUP_BOUND, ", ".join("%s %.3e" % kv for kv in errs.items())))
        for m, e in errs.items():
            assert e >= 1000 * LOOKUP_BOUND, m
        assert err <= LOOKUP_BOUND
        # untextured triangles: ones, exactly
        assert (got[tri_tex[ids] < 0] == 1).all() and (tri_tex[ids] < 0).sum() > 400
        # the sliver (fp32 den = 4 - 2 * 2 = 0): corner 0's uv, wherever the point is
        q = np.array([[4, 0, 0], [3.5, 0, 0], [5, 1, 0]], np.float32)
        fb = rnd.texture_eval(dsc, np.full(3, sliver, np.int32), q).cpu().numpy()
        want = T.sample(images[2], uv[sliver, :1, 0], uv[sliver, :1, 1])[0]
        assert np.abs(fb[:, :3] - want).max() <= LOOKUP_BOUND
        assert_bits_equal(fb[1:], fb[:-1], "the sliver's factor does not depend on the point")
        # a point that is not finite reads inside the textures all the same
        bad = rnd.texture_eval(dsc, np.array([0, 0, 0], np.int32),
                               np.array([[np.nan, 0, 0], [np.inf, 1, 1], [-np.inf, np.nan, 0]], np.float32)).cpu().numpy()
        assert np.isfinite(bad).all() and (bad[:, :3] <= 4.0).all()
        # an index outside the scene reads nothing
        assert (rnd.texture_eval(dsc, np.array([-1, len(data.tris)], np.int32), q[:2]).cpu().numpy() == 0).all()
    finally:
        dsc.close()


def test_set_textures_validates_and_leaves_the_scene(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images) = rooms("closed")
    ids = np.arange(len(data.tris), dtype=np.int32)
    pts = data.tris["v"][:, :, :3].mean(1)
    before = rnd.texture_eval(dsc, ids, pts).cpu().numpy()
    assert (before[tri_tex >= 0, :3] != 1).any()

    def with_uv(value):
        u = uv.copy()
        u[int(np.nonzero(tri_tex >= 0)[0][-1]), 1, 0] = value
        return (u, tri_tex, images)

    def with_index(value):
        t = tri_tex.copy()
        t[3] = value
        return (uv, t, images)

    def with_texel(value):
        im = [x.copy() for x in images]
        im[1][2, 3, 1] = value
        return (uv, tri_tex, im)
    cases = [with_uv(np.nan), with_uv(np.inf), with_uv(2.0 ** 20 * 1.5), with_index(len(images)), with_index(-2),
             with_texel(-1.0), with_texel(np.nan), with_texel(np.inf),
             (uv, tri_tex, images + [np.zeros((1, 16385, 3), np.float32)]),
             (uv, tri_tex, images + [np.zeros((16385, 1, 3), np.float32)])]
    for args in cases:
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*set_textures"):
            rnd.set_textures(dsc, *args)
    # more than 2^27 texels in all: refused from the sizes alone, before a texel is read (so a small block can stand in)
    import ctypes
    small = np.zeros(3, np.float32)
    rec = (L.TextureImage * 1)()
    rec[0].rgb, rec[0].width, rec[0].height = L.ptr(small), 16384, 8193
    u32, t32 = np.ascontiguousarray(uv, np.float32), np.full(len(tri_tex), -1, np.int32)
    tx = L.Textures(L.ptr(u32), L.ptr(t32), 1, ctypes.cast(rec, ctypes.c_void_p))
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*2\^27"):
        L.check(L.lib().mcpt_scene_set_textures(rnd.ctx, dsc.handle, ctypes.byref(tx)))
    with pytest.raises(ValueError):
        rnd.set_textures(dsc, uv[:-1], tri_tex, images)
    with pytest.raises(ValueError):
        rnd.set_textures(dsc, uv, tri_tex, [images[0][..., :2]])
    assert_bits_equal(rnd.texture_eval(dsc, ids, pts).cpu().numpy(), before, "a refused call leaves the textures")
    # a nan uv on an untextured triangle is not looked at
    u = uv.copy()
    u[int(np.nonzero(tri_tex < 0)[0][0])] = np.nan
    rnd.set_textures(dsc, u, tri_tex, images)
    assert_bits_equal(rnd.texture_eval(dsc, ids, pts).cpu().numpy(), before, "untextured triangles' uvs")
    rnd.set_textures(dsc, uv, tri_tex, images)
    plain = rnd.upload(data)
    try:
        with pytest.raises(L.MCPTError, match="no textures"):
            rnd.texture_eval(plain, ids, pts)
    finally:
        plain.close()


# ------------------------------------------------- fused kernel equals chain
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
def test_textured_render_equals_chain(rnd, rooms, chain_ref, schedule, mode):
    ref = chain_ref("closed", mode)
    dsc, cam, depth, data, _ = rooms("closed")
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode,
                schedule=schedule)
    assert_state_equal(got, ref, "sched%d/mode%d" % (schedule, mode))
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all() and (got[1] > 0).any()
    # not vacuous: the same scene without textures renders another image
    plain = rnd.upload(data)
    try:
        flat = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode,
                     schedule=schedule)
    finally:
        plain.close()
    assert (got[0].view(np.uint32) != flat[0].view(np.uint32)).any(axis=1).sum() > W


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_textured_smooth_render_equals_chain(rnd, rooms, chain_ref, mode):
    """Vertex normals set as well: the N forms' lookup and the texture's side by side."""
    ref = chain_ref("smooth", mode)
    dsc, cam, depth = rooms("smooth")[:3]
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode)
    assert_state_equal(got, ref, "vertex normals set, mode %d" % mode)
    assert got[0].tobytes() != chain_ref("closed", mode)[0].tobytes()


@pytest.mark.parametrize("window", [1, 2], ids=["window", "whole-stack"])
@pytest.mark.parametrize("quantized,fmt", [(2, 0), (1, 1), (3, 2)], ids=["128B", "quantized", "96B"])
def test_textured_render_node_formats_and_stack_layouts(rnd, rooms, chain_ref, quantized, fmt, window):
    ref = chain_ref("closed")
    dsc, cam, depth = rooms("closed")[:3]
    try:
        rnd.set_tuning(quantized=quantized, stack_window=window)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["node_format"] == fmt and s["stack_window"] == (1 if window == 1 else 0)
    assert_state_equal(got, ref, "quantized=%d stack_window=%d" % (quantized, window))


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
@pytest.mark.parametrize("split,frames", [(((0, 2), (2, 4)), 6), (((0, 2), (2, 5)), 7)])
def test_textured_frames_split_across_calls_and_blocks(rnd, rooms, chain_ref, split, frames, quantized):
    ref = chain_ref("closed", frames=frames)
    dsc, cam, depth = rooms("closed")[:3]
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    launches = 0
    try:
        rnd.set_tuning(quantized=quantized)
        for f0, nf in split:
            rnd.render_frames(dsc, cam, st, depth, ATT, nf, frame_begin=f0, frames_per_launch=3)
            launches += rnd.stats()["frames_per_block"] < nf
    finally:
        rnd.set_tuning()
    assert launches >= 1  # at least one call ran several blocks per pixel
    assert_state_equal(state_np(st), ref, "split %r" % (split,))


def test_textured_two_stripes_one_after_the_other(rnd, rooms, chain_ref):
    ref = chain_ref("closed")
    dsc, cam, depth = rooms("closed")[:3]
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, depth, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k, stripe_count=2)
    assert_state_equal(state_np(st), ref, "2 stripes of 8 rows")


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
@pytest.mark.parametrize("room", ["closed", "smooth"])
@pytest.mark.parametrize("cache,state", [(2, 0), (1, 2), (0, 2)], ids=["off", "always", "auto"])
def test_textured_render_primary_cache_modes(rnd, rooms, chain_ref, cache, state, quantized, room):
    """A cached primary hit of a textured scene holds the finished normal, and
    its texture factor sits in the side array beside it: off, always and auto
    give the chain's bits, with vertex normals and without."""
    ref = chain_ref(room)
    dsc, cam, depth = rooms(room)[:3]
    rnd.drop_caches()
    try:
        rnd.set_tuning(primary_cache=cache, quantized=quantized)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["primary_cache"] == state
    assert_state_equal(got, ref, "%s room, primary_cache=%d quantized=%d" % (room, cache, quantized))


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_textured_jittered_render_equals_chain(rnd, rooms, chain_ref, mode):
    ref = chain_ref("closed", mode, jitter=True)
    dsc, cam, depth = rooms("closed")[:3]
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=True, mode=mode)
    assert_state_equal(got, ref, "jittered, mode %d" % mode)
    assert got[0].tobytes() != chain_ref("closed", mode)[0].tobytes()


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
def test_textured_opened_room_under_a_constant_environment(rnd, rooms, chain_ref, quantized, jitter):
    ref = chain_ref("opened", jitter=jitter)
    dsc, cam, depth = rooms("opened")[:3]
    try:
        rnd.set_tuning(quantized=quantized)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=jitter)
    finally:
        rnd.set_tuning()
    assert_state_equal(got, ref, "opened room, quantized=%d jitter=%d" % (quantized, jitter))


def test_textured_render_with_counters_on(rnd, rooms, chain_ref):
    dsc, cam, depth = rooms("closed")[:3]
    try:
        rnd.set_stats(True)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
    finally:
        rnd.set_stats(False)
    assert s["segments"] > W * H and s["bad_material"] == 0
    assert_state_equal(got, chain_ref("closed"), "stats on")


def test_textured_ragged_image(rnd, rooms, chain_ref):
    ref = chain_ref("closed", w=20, h=13)
    dsc, cam, depth = rooms("closed")[:3]
    got = fused(rnd, dsc, cam, 20, 13, depth, ATT, FRAMES, R.default_seeds(20 * 13), jitter=False)
    assert_state_equal(got, ref, "20 x 13")


def test_intersect_names_the_closest_triangle_in_both_modes(rnd, rooms):
    """On a textured scene Hit.triangle_id is the closest hit's triangle in
    NOPRUNE too, so k_shade looks the texel up where the point lies."""
    dsc, cam, _, data, _ = rooms("closed")
    rays = rnd.generate_rays(cam, W, H)
    exact = R.records(rnd.intersect(dsc, rays), L.HIT)
    lit = R.records(rnd.intersect(dsc, rays, mode=L.MODE_NOPRUNE), L.HIT)
    hit = exact["t"] < FLT_MAX
    assert hit.mean() > 0.99
    assert_bits_equal(lit["t"], exact["t"], "the literal search finds the same hits")
    assert_bits_equal(lit["triangle_id"][hit], exact["triangle_id"][hit], "triangle_id")
    assert_bits_equal(lit["normal"][hit], exact["normal"][hit], "normal")


# --------------------------------------------------------------------- identity
def _golden_c1(rnd, prepare):
    g = np.load(os.path.join(ROOT, "tests", "golden", "image_c1_cbox.npz"))
    w, h, depth, frames, att = (int(x) for x in g["meta"])
    dsc, cam = rnd.upload(scenes.cbox()), S.parse_camera(scenes.CBOX_CAM)
    try:
        rnd.drop_caches()
        prepare(dsc)
        st = rnd.new_state(w, h, g["seeds_in"])
        rnd.render_frames(dsc, cam, st, depth, att, frames)
        torch.cuda.synchronize()
        assert_bits_equal(st.count.cpu().numpy(), g["count"], "count")
        assert_bits_equal(st.seeds_np(), g["seeds"], "seeds")
        assert_bits_equal(st.hist.cpu().numpy(), g["hist"], "hist")
    finally:
        dsc.close()


def _cbox_textures(value=None):
    tris = scenes.cbox().tris
    n = len(tris)
    rng = np.random.Generator(np.random.PCG64(31))
    uv = rng.uniform(-1.0, 2.0, (n, 3, 2)).astype(np.float32)
    img = rng.uniform(0.1, 1.0, (3, 5, 3)).astype(np.float32) if value is None else np.full((3, 5, 3), value, np.float32)
    return uv, np.zeros(n, np.int32), [img]


def test_set_then_clear_renders_the_committed_golden(rnd):
    def prepare(dsc):
        rnd.set_textures(dsc, *_cbox_textures())
        rnd.clear_textures(dsc)
    _golden_c1(rnd, prepare)


def test_all_ones_textures_render_the_committed_golden(rnd):
    """C1 through the textured kernels with a texture of ones on every
    triangle: x * 1.0f is exact, so the bits are the reference's."""
    _golden_c1(rnd, lambda dsc: rnd.set_textures(dsc, *_cbox_textures(1.0)))


def test_all_ones_textures_render_the_untextured_bits(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images) = rooms("closed")
    ones = [np.ones_like(im) for im in images]
    seeds = R.default_seeds(W * H)
    a, b = rnd.upload(data), rnd.upload(data)
    try:
        rnd.set_textures(b, uv, tri_tex, ones)
        for kw in (dict(jitter=False), dict(jitter=True), dict(jitter=False, mode=L.MODE_NOPRUNE)):
            plain = fused(rnd, a, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw)
            got = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw)
            assert_state_equal(got, plain, "ones %r" % (kw,))
            assert (plain[1] > 0).any()
    finally:
        a.close(), b.close()


def test_primary_cache_is_dropped_by_set_and_clear(rnd, rooms):
    dsc, cam, depth, data, tex = rooms("closed")
    seeds = R.default_seeds(W * H)
    plain = rnd.upload(data)
    try:
        rnd.drop_caches()
        first = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # built
        fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 1  # read
        rnd.set_textures(plain, *tex)
        got = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # rebuilt, with the texture factors beside it
        assert got[0].tobytes() != first[0].tobytes()
        again = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 1  # read
        assert_state_equal(again, got, "cached")
        rnd.set_textures(plain, tex[0], tex[1], [im[::-1].copy() for im in tex[2]])
        other = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # other textures: rebuilt
        assert other[0].tobytes() != got[0].tobytes()
        rnd.clear_textures(plain)
        back = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # rebuilt: every set and the clear dropped it
        assert_state_equal(back, first, "after the clear")
    finally:
        plain.close()


# --------------------------------------------------------------- visible effect
def test_red_texel_reflects_no_green_or_blue(rnd):
    """A floor quad under a constant white environment at depth 2: a path is
    camera -> floor -> sky, so a pixel is kd * Tex * cos / 2pi: inside the red
    quarter g and b are exactly 0.  The quarters of red, green, blue and white
    are 2x2 blocks of a 4x4 texture: under the bilinear, repeating filter a
    one-texel quarter is pure at its centre point alone, a 2x2 block wherever
    all four taps fall inside it."""
    quad = np.array([[[-1, 0, -1], [-1, 0, 1], [1, 0, 1]], [[-1, 0, -1], [1, 0, 1], [1, 0, -1]]], np.float32)
    uv = np.stack([(quad[..., 0] + 1) / 2, (quad[..., 2] + 1) / 2], axis=-1).astype(np.float32)
    img = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 1]]], np.float32)  # row 0 (v near 1): red, green
    img = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.8, 0.8, 0.8), (0, 0, 0), 1.0)
    data = S.SceneData.from_arrays(quad, np.zeros(2, np.int32), mats)
    cam = S.parse_camera({"position": [0, 3, 0.001], "lookat": [0, 0, 0], "up": [0, 0, -1], "fov": 40.0})
    dsc = rnd.upload(data)
    try:
        rnd.set_textures(dsc, uv, np.zeros(2, np.int32), [img])
        rnd.set_environment(dsc, scale=(1.0, 1.0, 1.0))
        st = rnd.new_state(W, H, R.default_seeds(W * H))
        rnd.render_frames(dsc, cam, st, 2, ATT, FRAMES)
        hist = state_np(st)[0]
        hits = R.records(rnd.first_hits(dsc, cam, W, H), L.HIT)
        p = hits["point"]
        u, v = (p[:, 0] + 1) / 2, (p[:, 2] + 1) / 2
        on = hits["t"] < FLT_MAX
        # all four taps in the red block: x = 4u - 0.5 in (0, 1), y = 4(1 - v) - 0.5 in (0, 1), with a margin
        red = on & (u > 0.15) & (u < 0.35) & (v > 0.65) & (v < 0.85)
        assert red.sum() >= 20
        assert (hist[red, 1] == 0).all() and (hist[red, 2] == 0).all() and (hist[red, 0] > 0).all()
        white = on & (u > 0.65) & (u < 0.85) & (v > 0.15) & (v < 0.35)
        assert white.sum() >= 20 and (hist[white, :3] > 0).all()
    finally:
        dsc.close()


# -------------------------------------------------------------- debug build
def _digest(state):
    h = hashlib.sha256()
    for a in state:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_debug_build_texture_bounds_checks_clean(rnd, rooms, chain_ref):
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import texture_ref; texture_ref.debug_main()"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert [(c["mode"], c["node_format"]) for c in lines[1:]] == [(0, 0), (0, 1), (0, 2), (1, 0)]
    for c in lines[1:]:
        assert c["violations"] == 0, c
        assert c["digest"] == _digest(chain_ref("closed", c["mode"])), c


# ------------------------------------------------------------------ denoise
def test_denoise_with_albedo_keeps_a_checker_sharp(rnd):
    """hist = albedo * E on one plane, count 1: with the albedo the filter
    sees the constant E and returns hist within 64 ulp (the rounding of the
    division, the weighted means and the product); without it a pixel beside a
    checker edge moves by more than 5 % of the contrast."""
    w, h = 32, 24
    quad = np.array([[[-9, -9, 0], [9, -9, 0], [9, 9, 0]], [[-9, -9, 0], [9, 9, 0], [-9, 9, 0]]], np.float32)
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    data = S.SceneData.from_arrays(quad, np.zeros(2, np.int32), mats)
    cam = S.parse_camera({"position": [0, 0, 5], "lookat": [0, 0, 0], "up": [0, 1, 0], "fov": 40.0})
    dsc = rnd.upload(data)
    try:
        d_hits = rnd.first_hits(dsc, cam, w, h)
        assert (R.records(d_hits, L.HIT)["t"] < FLT_MAX).all()
        yy, xx = np.mgrid[0:h, 0:w]
        lo, hi = np.float32(0.25), np.float32(0.75)
        a = np.where((((xx // 4) + (yy // 4)) & 1) == 0, lo, hi).astype(np.float32).reshape(-1)
        albedo = np.stack([a, a * np.float32(0.5) + np.float32(0.125), np.full_like(a, 0.5), np.ones_like(a)], axis=1)
        e = np.array([0.7, 1.3, 0.4, 0.0], np.float32)
        st = rnd.new_state(w, h, R.default_seeds(w * h))
        hist = (albedo * e).astype(np.float32)
        st.hist.copy_(torch.from_numpy(hist))
        st.count.fill_(1)
        with_a = rnd.denoise(dsc, d_hits, st, albedo=albedo).cpu().numpy()
        ulp = np.abs(with_a[:, :3].view(np.int32).astype(np.int64) - hist[:, :3].view(np.int32).astype(np.int64))
        print("denoise with albedo: max %d ulp" % int(ulp.max()))
        assert ulp.max() <= 64
        without = rnd.denoise(dsc, d_hits, st).cpu().numpy()
        edge = (yy == 10) & (xx == 4)  # the first pixel right of a checker edge
        moved = np.abs(without[edge.reshape(-1), 0] - hist[edge.reshape(-1), 0])
        assert moved[0] > 0.05 * float(hi - lo) * float(e[0])
        # an albedo of ones changes nothing
        ones = rnd.denoise(dsc, d_hits, st, albedo=np.ones((w * h, 3), np.float32)).cpu().numpy()
        assert_bits_equal(ones, without, "albedo 1")
    finally:
        dsc.close()


def test_first_hit_albedo_is_one_off_the_diffuse_and_glossy_surfaces(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images) = rooms("closed")
    d_hits = rnd.first_hits(dsc, cam, W, H)
    hits = R.records(d_hits, L.HIT)
    a = rnd.first_hit_albedo(dsc, d_hits).cpu().numpy()
    ty = data.mats["type"][hits["material_id"]]
    hit = hits["t"] < FLT_MAX
    shaded = hit & ((ty == L.MCPT_DIFFUSE) | (ty == L.MCPT_GLOSSY))
    assert (a[~shaded] == 1).all() and (~shaded).sum() > 20 and (a[:, 3] == 1).all()
    textured = shaded & (tri_tex[hits["triangle_id"]] >= 0)
    assert textured.sum() > 200 and (a[textured, :3] != 1).any()
    want = rnd.texture_eval(dsc, hits["triangle_id"][textured].astype(np.int32), hits["point"][textured]).cpu().numpy()
    assert_bits_equal(a[textured], want, "albedo at the first hits")


# ------------------------------------------------------------ App and CLI
TEX_OBJ = """mtllib t.mtl
v -1 0 -1
v -1 0 1
v 1 0 1
v 1 0 -1
v -0.6 2.5 -0.6
v 0.6 2.5 -0.6
v 0.6 2.5 0.6
v -0.6 2.5 0.6
v -1 0 -1
v 1 0 -1
v 1 2 -1
v -1 2 -1
vt 0 0
vt 0 2
vt 2 2
vt 2 0
usemtl floor
f 1/1 2/2 3/3 4/4
usemtl light
f 5 6 7 8
usemtl wall
f 9/1 10/4 11/3 12/2
"""
TEX_MTL = """newmtl floor
Kd 0.8 0.8 0.8
map_Kd -clamp on tex\\checker.png
newmtl light
Ka 10 10 10
Kd 0 0 0
newmtl wall
Kd 0.7 0.7 0.7
Ks 0.3 0.3 0.3
Ns 20
map_Kd tex/checker.png
"""


def _textured_entry(tmp_path, **extra):
    d = tmp_path / "model"
    os.makedirs(d / "tex")
    (d / "t.obj").write_text(TEX_OBJ)
    (d / "t.mtl").write_text(TEX_MTL)
    yy, xx = np.mgrid[0:6, 0:4]
    img = np.zeros((6, 4, 4), np.float32)
    img[..., 0] = np.where((xx + yy) & 1, 0.9, 0.1)
    img[..., 1] = np.where((xx + yy) & 1, 0.2, 0.8)
    img[..., 2] = 0.5
    S.write_png(str(d / "tex" / "checker.png"), img, flip=False)
    e = {"bvhtype": "hlbvh", "width": 32, "height": 32, "platform": "amd", "directory": str(d) + "/",
         "objname": "t.obj", "maxdepth": 4, "attempt": 3, "raygenerator": "", "intersect": "", "shade": "",
         "camera": {"position": [0, 1.2, 3.5], "lookat": [0, 0.6, 0], "up": [0, 1, 0], "fov": 45.0,
                    "resolution": [32, 32]},
         "opencl": True}
    e.update(extra)
    return {"configid": 0, "config": [e]}


def test_app_cli_and_two_ranks_render_the_configured_textures(tmp_path):
    from montecarlopathtracing_amd.__main__ import main
    from montecarlopathtracing_amd.app import App
    path = tmp_path / "config.json"
    path.write_text(json.dumps(_textured_entry(tmp_path, textures=True)))
    for d in ("app", "cli", "flat", "dist"):
        os.mkdir(tmp_path / d)
    app = App(str(path), out_dir=str(tmp_path / "app"))  # the CLI's default seeds
    app.run()
    assert app.textured
    got = state_np(app.state)
    directory = str(tmp_path / "model") + "/"
    _, mats, idx = S.load_object(directory, "t.obj")
    uv, tri_tex, images = S.load_textures(directory, "t.obj", mats, idx)
    assert tri_tex.tolist() == [0, 0, -1, -1, 0, 0] and len(images) == 1 and images[0].shape == (6, 4, 3)
    app.renderer.set_textures(app.scene, uv, tri_tex, images)
    want = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, R.default_seeds(32 * 32), jitter=False)
    assert_state_equal(got, want, 'App with "textures": true')
    plain = App(str(path), out_dir=str(tmp_path / "flat"), textures=False)
    plain.run()
    assert not plain.textured and state_np(plain.state)[0].tobytes() != got[0].tobytes()
    flat_cfg = tmp_path / "flat.json"
    entry = json.loads(path.read_text())
    del entry["config"][0]["textures"]
    flat_cfg.write_text(json.dumps(entry))
    assert main([str(flat_cfg), "--out", str(tmp_path / "cli"), "--textures"]) == 0
    assert (tmp_path / "cli" / "t.obj.hdr").read_bytes() == (tmp_path / "app" / "t.obj.hdr").read_bytes()
    assert (tmp_path / "cli" / "t.obj.hdr").read_bytes() != (tmp_path / "flat" / "t.obj.hdr").read_bytes()
    # two ranks sharing the GPU over gloo: every rank sets the textures on its own scene
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        "-m", "montecarlopathtracing_amd", str(path), "--out", str(tmp_path / "dist")],
                       cwd=ROOT, env=dict(os.environ, MCPT_DIST_SHARED_GPU="1"), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "dist" / "t.obj.hdr").read_bytes() == (tmp_path / "app" / "t.obj.hdr").read_bytes()
