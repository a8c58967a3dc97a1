"""Bump and normal maps (opt-in; mcpt_scene_set_normal_maps, mcpt_bump_eval): a
hit is shaded with its normal perturbed by the triangle's tangent-space normal
map.  The reference has none, so the yardsticks are the project's own: the
float64 restatement of the definition (tests/bump_ref.py) for mcpt_bump_eval,
and for the fused kernel the chain of wavefront kernels, whose k_intersect
applies the same lookup to the hit it reports.  None of this needs oracle/_ref."""
import hashlib
import json
import math
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

from . import bump_cases as BC  # noqa: E402
from . import bump_ref as B  # noqa: E402
from . import scenes  # noqa: E402
from .test_gpu_jitter import assert_bits_equal, assert_state_equal, fused, state_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W, H, FRAMES, ATT, DEPTH = 24, 20, 6, 4, 5  # 6 frames run past the history's cap (attempt 4)
FLT_MAX = np.float32(3.402823466e+38)
LENS = (12.0, 900.0)


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module")
def boxes(rnd):
    """name -> (mapped cbox DeviceScene, camera).  "maps": normal maps alone
    (no textures, no vertex normals: both views null); "smooth": with generated
    vertex normals; "tex": with textures; "both": with both; "env": maps alone
    under a constant environment."""
    held = {}

    def get(name):
        if name not in held:
            data = scenes.cbox()
            dsc = rnd.upload(data)
            rnd.set_normal_maps(dsc, *BC.cbox_maps())
            if name in ("smooth", "both"):
                rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, 40.0))
            if name in ("tex", "both"):
                rnd.set_textures(dsc, *BC.cbox_textures())
            if name == "env":
                rnd.set_environment(dsc, scale=(0.8, 0.9, 1.2))
            held[name] = (dsc, S.parse_camera(scenes.CBOX_CAM))
        return held[name]
    yield get
    for rec in held.values():
        rec[0].close()


@pytest.fixture(scope="module")
def chain_ref(rnd, boxes):
    """(box, mode, frames, jitter, lens, w, h) -> the chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name="maps", mode=L.MODE_EXACT, frames=FRAMES, jitter=False, lens=None, w=W, h=H):
        key = (name, mode, frames, jitter, lens, w, h)
        if key not in held:
            dsc, cam = boxes(name)
            held[key] = BC.chain(rnd, dsc, cam, w, h, DEPTH, ATT, frames, R.default_seeds(w * h), mode, jitter, lens)
        return held[key]
    return get


def render(rnd, dsc, cam, w=W, h=H, frames=FRAMES, **kw):
    kw.setdefault("jitter", False)
    return fused(rnd, dsc, cam, w, h, DEPTH, ATT, frames, R.default_seeds(w * h), **kw)


# ------------------------------------------------ 1. mcpt_bump_eval vs float64
# Largest error of mcpt_bump_eval against tests/bump_ref.py (float64), max |gpu -
# ref| over the components of every query of bump_cases.lookup_queries that is no
# near-tie (4,080 queries, 1 left out), measured on an MI355X, and the bound
# held: 8x that, the margin of test_gpu_texture.py and test_gpu_lens.py, since
# fp32 rounding varies with the query set.  Measured: 3.508e-6 (median 7.4e-8,
# 99.9th percentile 2.4e-6: UVs reach 3.5 on a 5-texel row, so x reaches 17 with
# a float32 step of 2e-6, times the contrast of neighbouring unit texels, under
# 2); bound 2.807e-5.  The mutants' largest errors, each of which must stay 100x
# above the bound: h ignored 1.79, f ignored 1.79, no Gram-Schmidt 1.18, mx/my
# swapped 1.52, no v flip 1.44.
LOOKUP_MEASURED = 3.508e-6
LOOKUP_BOUND = 8 * LOOKUP_MEASURED


def test_bump_eval_matches_float64(rnd):
    data, uv, tri_map, images = BC.lookup_mesh()
    ids, pts, dirs, nrm = BC.lookup_queries(data)
    verts, ng = BC.mesh_arrays(data)
    dsc = rnd.upload(data)
    try:
        rnd.set_normal_maps(dsc, uv, tri_map, images)
        n4 = np.zeros((len(ids), 4), np.float32)
        n4[:, :3] = nrm
        n4[::2, 3] = np.float32(-0.0)  # N.w's bits are kept
        got = rnd.bump_eval(dsc, ids, pts, dirs, n4).cpu().numpy()
        assert got.shape == (len(ids), 4) and np.isfinite(got).all()
        assert_bits_equal(got[:, 3], n4[:, 3], "n'.w keeps N.w's bits")
        ref, tie = B.bump_normal(verts, ng, uv, tri_map, images, ids, pts, dirs, nrm)
        keep = ~tie
        assert 3000 <= len(ids) and tie.mean() <= 0.02
        err = float(np.abs(got[keep, :3] - ref[keep]).max())
        errs = {m: float(np.abs(got[keep, :3] - B.bump_normal(verts, ng, uv, tri_map, images, ids, pts, dirs, nrm, m)[0][keep]).max())
                for m in B.MUTANTS}
        print("bump_eval: %d queries, %d near-ties left out, max error %.3e (bound %.3e); mutants %s" % (
            len(ids), int(tie.sum()), err, LOOKUP_BOUND, ", ".join("%s %.3e" % kv for kv in errs.items())))
        for m, e in errs.items():
            assert e >= 100 * LOOKUP_BOUND, m
        assert err <= LOOKUP_BOUND
        assert np.abs(np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-5  # unit
        # unmapped and degenerate-UV triangles: N, bit for bit
        t, h, ok = B.tangent_frames(verts, ng, uv, tri_map)
        plain = ~ok[ids]
        assert plain.sum() >= 200 and (tri_map[ids][plain] >= 0).sum() >= 40
        assert_bits_equal(got[plain], n4[plain], "unmapped and degenerate triangles return N")
        # wherever the restatement keeps N (turned away from the viewer), so does the device, bit for bit
        kept = keep & ~plain & (np.abs(ref - nrm).max(1) == 0)
        assert kept.sum() > 50
        assert_bits_equal(got[kept], n4[kept], "turned away from the viewer: N")
        # an index outside the scene reads nothing
        out = rnd.bump_eval(dsc, np.array([-1, len(data.tris)], np.int32), pts[:2], dirs[:2], n4[:2]).cpu().numpy()
        assert (out == 0).all()
        # a point, direction or normal that is not finite reads inside the maps all the same and stays finite or N
        bad = np.array([[np.nan, 0, 0], [np.inf, 1, 1], [-np.inf, np.nan, 0]], np.float32)
        r = rnd.bump_eval(dsc, np.zeros(3, np.int32), bad, dirs[:3], n4[:3]).cpu().numpy()
        assert np.isfinite(r).all()
        r = rnd.bump_eval(dsc, np.zeros(1, np.int32), pts[:1], bad[:1], n4[:1]).cpu().numpy()
        assert_bits_equal(r, n4[:1], "a NaN direction faces nothing: N")
    finally:
        dsc.close()


# ------------------------------------------------------------- 2. off is off
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


def _flat_maps(tri_map=None):
    uv, tm, images = BC.cbox_maps()
    up = [np.broadcast_to(np.array([0, 0, 1], np.float32), im.shape).copy() for im in images]
    return uv, (tm if tri_map is None else tri_map), up


def test_unmapped_unjittered_call_renders_the_committed_golden(rnd):
    _golden_c1(rnd, lambda dsc: None)


def test_set_then_clear_renders_the_committed_golden(rnd):
    def prepare(dsc):
        rnd.set_normal_maps(dsc, *BC.cbox_maps())
        rnd.clear_normal_maps(dsc)
    _golden_c1(rnd, prepare)


def test_straight_up_maps_render_the_committed_golden(rnd):
    """C1 through the mapped kernels with (0, 0, 1) in every texel: the lookup
    returns N bit for bit, so the bits are the reference's."""
    _golden_c1(rnd, lambda dsc: rnd.set_normal_maps(dsc, *_flat_maps()))


def test_all_unmapped_set_renders_the_committed_golden(rnd):
    n = len(scenes.cbox().tris)
    _golden_c1(rnd, lambda dsc: rnd.set_normal_maps(dsc, *_flat_maps(np.full(n, -1, np.int32))))


@pytest.mark.parametrize("how", ["straight-up", "unmapped", "set-clear"])
def test_off_is_off_through_the_new_forms(rnd, how):
    """The unmapped render's hist, count and seeds bits, jittered, in NOPRUNE,
    in blocks, with vertex normals and textures as well."""
    data = scenes.cbox()
    cam = S.parse_camera(scenes.CBOX_CAM)
    n = len(data.tris)
    a, b = rnd.upload(data), rnd.upload(data)
    try:
        for extra in (False, True):
            if extra:
                for d in (a, b):
                    rnd.set_vertex_normals(d, S.vertex_normals(data.tris, 40.0))
                    rnd.set_textures(d, *BC.cbox_textures())
            if how == "straight-up":
                rnd.set_normal_maps(b, *_flat_maps())
            elif how == "unmapped":
                rnd.set_normal_maps(b, *_flat_maps(np.full(n, -1, np.int32)))
            else:
                rnd.set_normal_maps(b, *BC.cbox_maps())
                rnd.clear_normal_maps(b)
            for kw in (dict(jitter=False), dict(jitter=True), dict(jitter=False, mode=L.MODE_NOPRUNE)):
                plain = render(rnd, a, cam, frames_per_launch=3, **kw)
                got = render(rnd, b, cam, frames_per_launch=3, **kw)
                assert_state_equal(got, plain, "%s %r extra=%d" % (how, kw, extra))
                assert (plain[1] > 0).any()
    finally:
        a.close(), b.close()


# --------------------------------------------- 3. fused kernel equals the chain
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
def test_mapped_render_equals_chain(rnd, boxes, chain_ref, schedule, mode):
    ref = chain_ref("maps", mode)
    dsc, cam = boxes("maps")
    got = render(rnd, dsc, cam, mode=mode, schedule=schedule)
    assert_state_equal(got, ref, "sched%d/mode%d" % (schedule, mode))
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all() and (got[1] > 0).any()
    # not vacuous: the same scene without maps renders another image
    plain = rnd.upload(scenes.cbox())
    try:
        flat = render(rnd, plain, cam, mode=mode, schedule=schedule)
    finally:
        plain.close()
    assert (got[0].view(np.uint32) != flat[0].view(np.uint32)).any(axis=1).sum() > W


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("box", ["smooth", "tex", "both"])
def test_mapped_render_with_vertex_normals_and_textures_equals_chain(rnd, boxes, chain_ref, box, mode):
    ref = chain_ref(box, mode)
    dsc, cam = boxes(box)
    assert_state_equal(render(rnd, dsc, cam, mode=mode), ref, "%s, mode %d" % (box, mode))
    assert ref[0].tobytes() != chain_ref("maps", mode)[0].tobytes()


@pytest.mark.parametrize("window", [1, 2], ids=["window", "whole-stack"])
@pytest.mark.parametrize("quantized,fmt", [(2, 0), (1, 1), (3, 2)], ids=["128B", "quantized", "96B"])
@pytest.mark.parametrize("box", ["maps", "both"])
def test_mapped_render_node_formats_and_stack_layouts(rnd, boxes, chain_ref, box, quantized, fmt, window):
    ref = chain_ref(box)
    dsc, cam = boxes(box)
    try:
        rnd.set_tuning(quantized=quantized, stack_window=window)
        got = render(rnd, dsc, cam)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["node_format"] == fmt and s["stack_window"] == (1 if window == 1 else 0)
    assert_state_equal(got, ref, "%s quantized=%d stack_window=%d" % (box, quantized, window))


@pytest.mark.parametrize("w,h", [(7, 3), (20, 13)])
def test_mapped_ragged_images(rnd, boxes, chain_ref, w, h):
    ref = chain_ref("maps", w=w, h=h)
    dsc, cam = boxes("maps")
    assert_state_equal(render(rnd, dsc, cam, w=w, h=h), ref, "%d x %d" % (w, h))


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
@pytest.mark.parametrize("split,frames", [(((0, 2), (2, 4)), 6), (((0, 2), (2, 5)), 7)])
def test_mapped_frames_split_across_calls_and_blocks(rnd, boxes, chain_ref, split, frames, quantized):
    ref = chain_ref("maps", frames=frames)
    dsc, cam = boxes("maps")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    launches = 0
    try:
        rnd.set_tuning(quantized=quantized)
        for f0, nf in split:
            rnd.render_frames(dsc, cam, st, DEPTH, ATT, nf, frame_begin=f0, frames_per_launch=3)
            launches += rnd.stats()["frames_per_block"] < nf
    finally:
        rnd.set_tuning()
    assert launches >= 1  # at least one call ran several blocks per pixel
    assert_state_equal(state_np(st), ref, "split %r" % (split,))


def test_mapped_two_stripes_one_after_the_other(rnd, boxes, chain_ref):
    ref = chain_ref("maps")
    dsc, cam = boxes("maps")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, DEPTH, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k, stripe_count=2)
    assert_state_equal(state_np(st), ref, "2 stripes of 8 rows")


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
@pytest.mark.parametrize("box", ["maps", "both"])
@pytest.mark.parametrize("cache,state", [(2, 0), (1, 2), (0, 2)], ids=["off", "always", "auto"])
def test_mapped_render_primary_cache_modes(rnd, boxes, chain_ref, cache, state, quantized, box):
    """A cached primary hit of a mapped scene holds n' as the finished normal:
    off, always and auto give the chain's bits."""
    ref = chain_ref(box)
    dsc, cam = boxes(box)
    rnd.drop_caches()
    try:
        rnd.set_tuning(primary_cache=cache, quantized=quantized)
        got = render(rnd, dsc, cam)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["primary_cache"] == state
    assert_state_equal(got, ref, "%s, primary_cache=%d quantized=%d" % (box, cache, quantized))


def test_primary_cache_is_dropped_by_set_and_clear(rnd, chain_ref):
    cam = S.parse_camera(scenes.CBOX_CAM)
    plain = rnd.upload(scenes.cbox())
    try:
        rnd.drop_caches()
        first = render(rnd, plain, cam)
        assert rnd.stats()["primary_cache"] == 2  # built
        render(rnd, plain, cam)
        assert rnd.stats()["primary_cache"] == 1  # read
        rnd.set_normal_maps(plain, *BC.cbox_maps())
        got = render(rnd, plain, cam)
        assert rnd.stats()["primary_cache"] == 2  # rebuilt, with the mapped normals
        assert_state_equal(got, chain_ref("maps"), "after the set")
        again = render(rnd, plain, cam)
        assert rnd.stats()["primary_cache"] == 1
        assert_state_equal(again, got, "cached")
        rnd.clear_normal_maps(plain)
        back = render(rnd, plain, cam)
        assert rnd.stats()["primary_cache"] == 2
        assert_state_equal(back, first, "after the clear")
    finally:
        plain.close()


def test_replacing_each_attribute_keeps_both_orderings_in_step(rnd, chain_ref):
    """One scene on the 96-B nodes, whose launches read the tri4-ordered arrays
    (vnrm4, texrec4, bumprec4), against the chain, whose kernels read the
    reference-ordered ones: all three attributes set, each replaced by another
    valid set, one cleared and set again.  After every step the two must give
    the same bits, which they do not when a set frees, keeps or swaps the wrong
    array of a pair."""
    w, h, frames = 20, 13, 2
    data, cam = scenes.cbox(), S.parse_camera(scenes.CBOX_CAM)
    n = len(data.tris)
    rng = np.random.Generator(np.random.PCG64(7))
    uv, tri_tex, images = BC.cbox_textures()
    # (two images on every triangle: the few lit paths of an image this small meet none of the first set's)
    other_textures = (uv[:, ::-1].copy(), (np.arange(n) % 2).astype(np.int32),
                      [rng.uniform(0.1, 1.0, (2, 7, 3)).astype(np.float32), rng.uniform(0.1, 1.0, (4, 3, 3)).astype(np.float32)])
    # (a crease of 100 degrees rounds the boxes' right-angled edges, which 40 leaves sharp)
    steps = [("normals replaced", lambda d: rnd.set_vertex_normals(d, S.vertex_normals(data.tris, 100.0))),
             ("textures replaced", lambda d: rnd.set_textures(d, *other_textures)),
             ("maps replaced", lambda d: rnd.set_normal_maps(d, *BC.cbox_maps(tilt=20.0))),
             ("textures cleared", lambda d: rnd.clear_textures(d)),
             ("textures set again", lambda d: rnd.set_textures(d, uv, tri_tex, images))]
    dsc = rnd.upload(data)
    seen = []
    try:
        rnd.set_tuning(quantized=3)
        rnd.set_normal_maps(dsc, *BC.cbox_maps())
        rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, 40.0))
        rnd.set_textures(dsc, uv, tri_tex, images)
        got = render(rnd, dsc, cam, w=w, h=h, frames=frames)
        assert rnd.stats()["node_format"] == 2
        assert_state_equal(got, chain_ref("both", w=w, h=h, frames=frames), "all three set")
        seen.append(got[0].tobytes())
        for what, step in steps:
            step(dsc)
            ref = BC.chain(rnd, dsc, cam, w, h, DEPTH, ATT, frames, R.default_seeds(w * h))
            got = render(rnd, dsc, cam, w=w, h=h, frames=frames)
            assert rnd.stats()["node_format"] == 2
            assert_state_equal(got, ref, what)
            assert got[0].tobytes() not in seen, what  # not vacuous: every step changes the image
            seen.append(got[0].tobytes())
    finally:
        rnd.set_tuning()
        dsc.close()


def test_mapped_render_with_counters_on(rnd, boxes, chain_ref):
    dsc, cam = boxes("maps")
    try:
        rnd.set_stats(True)
        got = render(rnd, dsc, cam)
        s = rnd.stats()
    finally:
        rnd.set_stats(False)
    assert s["segments"] > W * H and s["bad_material"] == 0
    assert_state_equal(got, chain_ref("maps"), "stats on")


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("box", ["maps", "both"])
def test_mapped_jittered_render_equals_chain(rnd, boxes, chain_ref, box, mode):
    ref = chain_ref(box, mode, jitter=True)
    dsc, cam = boxes(box)
    assert_state_equal(render(rnd, dsc, cam, jitter=True, mode=mode), ref, "%s jittered, mode %d" % (box, mode))
    assert ref[0].tobytes() != chain_ref(box, mode)[0].tobytes()


@pytest.mark.parametrize("quantized", [2, 3], ids=["128B", "96B"])
def test_mapped_render_through_a_lens_equals_chain(rnd, boxes, chain_ref, quantized):
    ref = chain_ref("maps", jitter=True, lens=LENS)
    dsc, cam = boxes("maps")
    try:
        rnd.set_tuning(quantized=quantized)
        got = render(rnd, dsc, cam, jitter=True, lens=LENS)
    finally:
        rnd.set_tuning()
    assert_state_equal(got, ref, "lens, quantized=%d" % quantized)
    assert ref[0].tobytes() != chain_ref("maps", jitter=True)[0].tobytes()


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
def test_mapped_box_under_a_constant_environment(rnd, boxes, chain_ref, quantized, jitter):
    ref = chain_ref("env", jitter=jitter)
    dsc, cam = boxes("env")
    try:
        rnd.set_tuning(quantized=quantized)
        got = render(rnd, dsc, cam, jitter=jitter)
    finally:
        rnd.set_tuning()
    assert_state_equal(got, ref, "environment, quantized=%d jitter=%d" % (quantized, jitter))
    assert ref[0].tobytes() != chain_ref("maps", jitter=jitter)[0].tobytes()


def test_intersect_reports_the_mapped_normal_and_the_closest_triangle(rnd, boxes):
    """mcpt_hit.normal is n' (bump_eval of the unmapped scene's hit) and
    triangle_id the closest hit's triangle in NOPRUNE too."""
    dsc, cam = boxes("maps")
    rays = rnd.generate_rays(cam, W, H)
    exact = R.records(rnd.intersect(dsc, rays), L.HIT)
    lit = R.records(rnd.intersect(dsc, rays, mode=L.MODE_NOPRUNE), L.HIT)
    hit = exact["t"] < FLT_MAX
    assert hit.mean() > 0.6  # (the 24 x 20 view shows black beside the box)
    assert_bits_equal(lit["t"], exact["t"], "the literal search finds the same hits")
    assert_bits_equal(lit["triangle_id"][hit], exact["triangle_id"][hit], "triangle_id")
    assert_bits_equal(lit["normal"][hit], exact["normal"][hit], "normal")
    plain = rnd.upload(scenes.cbox())
    try:
        base = R.records(rnd.intersect(plain, rays), L.HIT)
    finally:
        plain.close()
    d = R.records(rays, L.RAY)["direction"]
    want = rnd.bump_eval(dsc, exact["triangle_id"][hit].astype(np.int32), exact["point"][hit], d[hit],
                         base["normal"][hit]).cpu().numpy()
    assert_bits_equal(exact["normal"][hit], want, "mcpt_hit.normal is bump_eval of the unmapped normal")
    assert (np.abs(exact["normal"][hit] - base["normal"][hit]).max(1) > 0.05).mean() > 0.5


# ---------------------------------------------------------------- 4. refusals
def test_set_normal_maps_validates_and_leaves_the_scene(rnd, boxes):
    dsc, cam = boxes("maps")
    data = scenes.cbox()
    uv, tri_map, images = BC.cbox_maps()
    n = len(data.tris)
    ids = np.arange(n, dtype=np.int32)
    pts = data.tris["v"][:, :, :3].mean(1)
    nrm = data.tris["normal"][:, :3].copy()
    before = rnd.bump_eval(dsc, ids, pts, -nrm, nrm).cpu().numpy()
    assert (np.abs(before[:, :3] - nrm).max(1) > 0).sum() > n // 2

    def with_uv(value):
        u = uv.copy()
        u[int(np.nonzero(tri_map >= 0)[0][-1]), 1, 0] = value
        return (u, tri_map, images)

    def with_index(value):
        t = tri_map.copy()
        t[3] = value
        return (uv, t, images)

    def with_texel(value):
        im = [x.copy() for x in images]
        im[0][1, 2] = value
        return (uv, tri_map, im)
    cases = [with_uv(np.nan), with_uv(np.inf), with_uv(2.0 ** 20 * 1.5), with_index(len(images)), with_index(-2),
             with_texel((0.0, 0.0, 1.01)), with_texel((0.6, 0.0, 0.7)), with_texel((0.6, 0.0, -0.8)),
             with_texel((1.0, 0.0, 0.0)), with_texel((np.nan, 0.0, 1.0)), with_texel((0.0, 0.0, np.inf)),
             (uv, tri_map, images + [np.zeros((0, 4, 3), np.float32)]),
             (uv, tri_map, images + [np.zeros((1, 16385, 3), np.float32)])]
    for args in cases:
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*set_normal_maps"):
            rnd.set_normal_maps(dsc, *args)
    # more than 2^27 texels in all: refused from the sizes alone, before a texel is read (so a small block can stand in)
    import ctypes
    small = np.zeros(3, np.float32)
    rec = (L.NormalMapImage * 1)()
    rec[0].xyz, rec[0].width, rec[0].height = L.ptr(small), 16384, 8193
    u32, t32 = np.ascontiguousarray(uv, np.float32), np.full(n, -1, np.int32)
    nm = L.NormalMaps(L.ptr(u32), L.ptr(t32), 1, ctypes.cast(rec, ctypes.c_void_p))
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*2\^27"):
        L.check(L.lib().mcpt_scene_set_normal_maps(rnd.ctx, dsc.handle, ctypes.byref(nm)))
    with pytest.raises(ValueError):
        rnd.set_normal_maps(dsc, uv[:-1], tri_map, images)
    with pytest.raises(ValueError):
        rnd.set_normal_maps(dsc, uv, tri_map, [images[0][..., :2]])
    assert_bits_equal(rnd.bump_eval(dsc, ids, pts, -nrm, nrm).cpu().numpy(), before, "a refused call leaves the maps")
    # a good call follows; a nan uv on an unmapped triangle is not looked at
    u = uv.copy()
    u[int(np.nonzero(tri_map < 0)[0][0])] = np.nan
    rnd.set_normal_maps(dsc, u, tri_map, images)
    assert_bits_equal(rnd.bump_eval(dsc, ids, pts, -nrm, nrm).cpu().numpy(), before, "unmapped triangles' uvs")
    rnd.set_normal_maps(dsc, uv, tri_map, images)
    plain = rnd.upload(data)
    try:
        with pytest.raises(L.MCPTError, match="no normal maps"):
            rnd.bump_eval(plain, ids, pts, -nrm, nrm)
    finally:
        plain.close()


# --------------------------------------------- 5. visible effect, per sample
LIT_FRAMES = 256  # on an MI355X 37 of the 42 tilted and 40 of the 42 flat pixels then have count > 0 (half are asked for)


def test_tilted_texels_dim_the_quad_by_the_cosine(rnd):
    """Camera -> quad -> light at depth 2: every non-zero sample is kd ka
    dot(w, n') / 2pi (kd, ka: the material records' values) with w a direction from the quad to the light, at most
    theta from +y.  Under the texels tilted a = 60 degrees towards +u the mean
    of those lies in [cos(a + theta), cos(a - theta)], under the (0, 0, 1)
    texels in [cos(theta), 1], and the latter pixels are the unmapped render's
    bit for bit."""
    data, uv, tri_map, images = BC.lit_quad()
    cam = S.parse_camera(BC.LIT_CAM)
    w, h = BC.LIT_W, BC.LIT_H
    a, theta = math.radians(BC.LIT_TILT), BC.lit_theta()
    lo_t, hi_t = math.cos(a + theta), math.cos(a - theta)
    lo_f = math.cos(theta)
    assert hi_t < lo_f and a + theta < math.pi / 2  # the two intervals are disjoint
    dsc, plain = rnd.upload(data), rnd.upload(data)
    try:
        rnd.set_normal_maps(dsc, uv, tri_map, images)
        seeds = R.default_seeds(w * h)
        got = fused(rnd, dsc, cam, w, h, 2, LIT_FRAMES, LIT_FRAMES, seeds, jitter=False)
        flat = fused(rnd, plain, cam, w, h, 2, LIT_FRAMES, LIT_FRAMES, seeds, jitter=False)
        hits = R.records(rnd.first_hits(plain, cam, w, h), L.HIT)
    finally:
        dsc.close(), plain.close()
    (x0, x1), _ = BC.LIT_QUAD
    on = (hits["t"] < FLT_MAX) & (hits["material_id"] == 0)
    x = (hits["point"][:, 0].astype(np.float64) - x0) / (x1 - x0) * 8 - 0.5  # the lookup's x = 8 u - 0.5; taps floor(x), + 1
    tilted = on & (x > 0.01) & (x < 2.99)   # both columns among 0..3 (a column of -1 would wrap to the flat column 7)
    level = on & (x > 4.01) & (x < 6.99)    # both columns among 4..7
    assert tilted.sum() >= 20 and level.sum() >= 20
    # kd and ka as the material records hold them (the loader's kd is the MTL file's Kd / pi)
    unit = float(data.mats[0]["kd"][0]) * float(data.mats[1]["ka_ks"][0]) / (2 * math.pi)
    hist, count = got[0].astype(np.float64), got[1]
    for name, mask, lo, hi in (("tilted", tilted, lo_t, hi_t), ("flat", level, lo_f, 1.0)):
        lit = mask & (count > 0)
        print("%s: %d pixels, %d with samples, ratio %.4f..%.4f in [%.4f, %.4f]" % (
            name, mask.sum(), lit.sum(), (hist[lit, 0] / unit).min(), (hist[lit, 0] / unit).max(), lo, hi))
        assert 2 * lit.sum() >= mask.sum(), name
        for c in range(3):
            r = hist[lit, c] / unit
            assert (r >= lo * (1 - 1e-5)).all() and (r <= hi * (1 + 1e-5)).all(), (name, c)
    for k in range(3):
        assert_bits_equal(got[k][level], flat[k][level], "the flat columns equal the unmapped render")
    assert (got[0][tilted] != flat[0][tilted]).any()


# ------------------------------------------------- 6. application, debug build
def _digest(state):
    h = hashlib.sha256()
    for a in state:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _app_render(tmp_path):
    from montecarlopathtracing_amd.app import App
    path = tmp_path / "config.json"
    path.write_text(json.dumps(BC.write_model(tmp_path, bump=2.0)))
    os.mkdir(tmp_path / "app"), os.mkdir(tmp_path / "flat")
    app = App(str(path), out_dir=str(tmp_path / "app"))
    app.run()
    assert app.mapped
    return path, app, state_np(app.state)


def test_app_renders_the_configured_bump_maps(tmp_path):
    from montecarlopathtracing_amd.app import App
    path, app, got = _app_render(tmp_path)
    directory = str(tmp_path / "model") + "/"
    _, mats, idx = S.load_object(directory, "b.obj")
    uv, tri_map, images = S.load_bump_maps(directory, "b.obj", mats, idx, 2.0)
    assert tri_map.tolist() == [0, 0, -1, -1, 1, 1] and len(images) == 2
    app.renderer.set_normal_maps(app.scene, uv, tri_map, images)
    want = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, R.default_seeds(32 * 32), jitter=False)
    assert_state_equal(got, want, 'App with "bump": 2.0')
    plain = App(str(path), out_dir=str(tmp_path / "flat"), bump=False)
    plain.run()
    assert not plain.mapped and state_np(plain.state)[0].tobytes() != got[0].tobytes()
    other = App(str(path), out_dir=str(tmp_path / "flat"), bump=True)  # another scale: other slopes on the floor
    other.run()
    assert other.mapped and state_np(other.state)[0].tobytes() != got[0].tobytes()


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_debug_build_renders_the_model_with_no_violations(tmp_path):
    path, app, got = _app_render(tmp_path)
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "import sys; from tests import bump_cases; bump_cases.debug_main(sys.argv[1])",
                        str(path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert [c["node_format"] for c in lines[1:]] == [0, 1, 2]
    for c in lines[1:]:
        assert c["violations"] == 0, c
        assert c["digest"] == _digest(got), c
