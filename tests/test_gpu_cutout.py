"""Alpha cutouts (opt-in; mcpt_scene_set_texture_alpha): a hit whose texture
alpha is below the scene's threshold is cut and the ray goes on through it.
The reference has none, so the yardsticks are the project's own: the float64
restatement (tests/cutout_ref.py) for the alpha at a hit, a mesh with the cut
triangles deleted for a hole, and for the fused kernel the chain of wavefront
kernels, whose k_shade applies the same test to the hit k_intersect reports.
None of this needs oracle/_ref."""
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

from . import bump_cases as BC  # noqa: E402
from . import cutout_ref as CR  # noqa: E402
from .test_gpu_jitter import assert_bits_equal, assert_state_equal, fused, state_np  # noqa: E402
from .test_gpu_texture import LOOKUP_BOUND, _cbox_textures, _golden_c1, lookup_mesh, lookup_queries  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W, H, FRAMES, ATT = 32, 24, 4, 2  # 4 frames run past the history's cap (attempt 2)
FLT_MAX = np.float32(3.402823466e+38)
LIGHT = np.array([5, 4, 3], np.float32)  # cutout_ref.hole_scene's light: what a path that reaches it carries
LENS = (0.05, 3.0)
CUT_ROUNDS = 256  # the chain's loop: at most max_depth + 256 rounds (255 passes and the depth's bounces)


def sees_light(state):
    """Pixels whose every counted sample was the light's radiance (the running
    mean of equal samples, within the rounding of history's division)."""
    return (np.abs(state[0][:, :3] - LIGHT).max(axis=1) < 1e-5) & (state[1] > 0)


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


def cut_chain(rnd, dsc, cam, w, h, depth, attempt, frames, seeds, mode=L.MODE_EXACT, jitter=False, lens=None):
    """The frame loop out of the wavefront kernels on a scene with cutouts:
    generate -> (intersect -> shade) until every ray is terminated -> accumulate.
    A cut hit costs a round and no depth, so the rounds are not the depth's; the
    loop is bounded by depth + 256.  Returns ((hist, count, seeds), most rounds
    a frame took)."""
    n = w * h
    d_seed = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(rnd.device)
    hist = torch.zeros((n, 4), dtype=torch.float32, device=rnd.device)
    count = torch.zeros(n, dtype=torch.int32, device=rnd.device)
    most = 0
    for f in range(frames):
        colors = torch.ones((n, 4), dtype=torch.float32, device=rnd.device)
        if lens is not None:
            rays = rnd.generate_rays_lens(cam, w, h, d_seed, lens)
        elif jitter:
            rays = rnd.generate_rays_jittered(cam, w, h, d_seed)
        else:
            rays = rnd.generate_rays(cam, w, h)
        hits, rounds = None, 0
        while True:
            td = rays.view(torch.int32).reshape(n, 12)[:, 3]
            if bool(((td >> 24) != 0).all()):
                break
            assert rounds < depth + CUT_ROUNDS, "a ray is still live after max_depth + 256 rounds"
            hits = rnd.intersect(dsc, rays, hits=hits, mode=mode)
            rnd.shade(dsc, rays, hits, colors, d_seed, depth)
            rounds += 1
        most = max(most, rounds)
        if f <= attempt:
            rnd.accumulate(colors, hist, count, attempt)
    torch.cuda.synchronize()
    return (hist.cpu().numpy(), count.cpu().numpy(), d_seed.cpu().numpy().view(np.uint32)), most


# ------------------------------------------------------ 1: the lookup vs float64
def lookup_alphas():
    """One alpha per texture of test_gpu_texture.lookup_mesh (1x1, 2x2, 5x3): not constant where a size allows."""
    rng = np.random.Generator(np.random.PCG64(71))
    return [np.full((1, 1), 0.3, np.float32), rng.uniform(0.0, 1.0, (2, 2)).astype(np.float32),
            rng.uniform(0.0, 1.0, (3, 5)).astype(np.float32)]


def test_alpha_lookup_matches_float64(rnd):
    """texture_eval's .w against the restatement on test_gpu_texture.py's query
    families, inside the bound that file commits for rgb (the same filter on the
    same inputs; alphas lie in [0, 1], its texels reach 4)."""
    data, uv, tri_tex, images, sliver = lookup_mesh()
    alphas = lookup_alphas()
    dsc = rnd.upload(data)
    try:
        rnd.set_textures(dsc, uv, tri_tex, images)
        ids, pts = lookup_queries(data, sliver)
        assert len(ids) >= 10000
        before = rnd.texture_eval(dsc, ids, pts).cpu().numpy()
        assert (before[:, 3] == 1).all()  # no alpha set: 1.0f exactly
        rnd.set_texture_alpha(dsc, [np.ones_like(a) for a in alphas])
        ones = rnd.texture_eval(dsc, ids, pts).cpu().numpy()
        assert_bits_equal(ones, before, "an alpha of ones is 1.0f exactly, and the colour is what it was")
        rnd.set_texture_alpha(dsc, alphas)
        got = rnd.texture_eval(dsc, ids, pts).cpu().numpy()
        assert_bits_equal(got[:, :3], before[:, :3], "the colour lanes do not see the alpha")
        verts = data.tris["v"][:, :, :3]
        ref = CR.alpha_at(verts, uv, tri_tex, alphas, ids, pts)
        err = float(np.abs(got[:, 3] - ref).max())
        errs = {m: float(np.abs(got[:, 3] - CR.alpha_at(verts, uv, tri_tex, alphas, ids, pts, mutant=m)).max())
                for m in CR.MUTANTS}
        print("alpha lookup: %d queries, max error %.3e (bound %.3e); mutants %s" % (
            len(ids), err, LOOKUP_BOUND, ", ".join("%s %.3e" % kv for kv in errs.items())))
        assert err <= LOOKUP_BOUND
        for m, e in errs.items():
            assert e > LOOKUP_BOUND, m
        assert np.isfinite(got).all() and got[:, 3].min() >= 0 and got[:, 3].max() <= 1
        # untextured triangles: 1, exactly; the 1x1 texture: its value, exactly (four equal texels)
        assert (got[tri_tex[ids] < 0, 3] == 1).all() and (tri_tex[ids] < 0).sum() > 400
        assert (got[tri_tex[ids] == 0, 3] == np.float32(0.3)).all() and (tri_tex[ids] == 0).sum() > 100
        # the sliver: corner 0's uv, wherever the point is
        q = np.array([[4, 0, 0], [3.5, 0, 0], [5, 1, 0]], np.float32)
        fb = rnd.texture_eval(dsc, np.full(3, sliver, np.int32), q).cpu().numpy()
        want = CR.T.sample(np.repeat(alphas[2][..., None], 3, 2), uv[sliver, :1, 0], uv[sliver, :1, 1])[0, 0]
        assert np.abs(fb[:, 3] - want).max() <= LOOKUP_BOUND
        assert_bits_equal(fb[1:], fb[:-1], "the sliver's alpha does not depend on the point")
        rnd.clear_texture_alpha(dsc)
        assert_bits_equal(rnd.texture_eval(dsc, ids, pts).cpu().numpy(), before, "cleared: 1.0f again")
    finally:
        dsc.close()


# ------------------------------------------------- 2, 3, 7: a hole is a hole
def _hole(rnd, alpha_image=None, delete=False, left_kd=0.7, alpha=True):
    data, uv, tri_tex, images, alphas, verts = CR.hole_scene(alpha_image, delete, left_kd)
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    if alpha:
        rnd.set_texture_alpha(dsc, alphas)
    rnd.set_environment(dsc, scale=CR.HOLE_ENV)
    return dsc, (uv, tri_tex, images, alphas, verts)


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_a_hole_is_a_hole(rnd, mode):
    """The quad whose alpha is 0 renders as the mesh without it does, bit for
    bit and in every pixel: behind it lie a light and the environment, whose
    values do not depend on the hit point's rounding, and a cut draws nothing."""
    w, h = CR.HOLE_W, CR.HOLE_H
    cam, seeds = CR.hole_camera(), R.default_seeds(w * h)
    cut, _ = _hole(rnd)
    gone, _ = _hole(rnd, delete=True)
    solid, _ = _hole(rnd, alpha=False)
    try:
        got = fused(rnd, cut, cam, w, h, CR.HOLE_DEPTH, ATT, FRAMES, seeds, jitter=False, mode=mode)
        want = fused(rnd, gone, cam, w, h, CR.HOLE_DEPTH, ATT, FRAMES, seeds, jitter=False, mode=mode)
        assert_state_equal(got, want, "cut against deleted, mode %d" % mode)
        # not vacuous: the left half sees the light, the right half (kd 0) is black and never counted
        x = R.records(rnd.generate_rays(cam, w, h), L.RAY)["origin"][:, 0]
        left = x < 0
        assert left.sum() == w * h // 2
        assert sees_light(got)[left].all() and (got[1][left] == ATT).all()
        assert (got[0][~left] == 0).all() and (got[1][~left] == 0).all()
        assert (got[2][left] == seeds[left]).all() and (got[2][~left] != seeds[~left]).all()
        # and without the alpha the quad is opaque
        opaque = fused(rnd, solid, cam, w, h, CR.HOLE_DEPTH, ATT, FRAMES, seeds, jitter=False, mode=mode)
        assert not sees_light(opaque)[left].any() and (opaque[2][left] != seeds[left]).all()
    finally:
        cut.close(), gone.close(), solid.close()


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_an_edge_inside_a_triangle(rnd, mode):
    """A 4x4 alpha whose left two columns are 0 on the (kd 0) quad: every pixel
    sees the light or is black with count 0 as the float64 alpha at its hit
    says; pixels within 1e-3 of the threshold are left out, at most 5 %."""
    w, h = CR.HOLE_W, CR.HOLE_H
    cam, seeds = CR.hole_camera(), R.default_seeds(w * h)
    dsc, (uv, tri_tex, images, alphas, verts) = _hole(rnd, CR.edge_alpha(), left_kd=0.0)
    try:
        got = fused(rnd, dsc, cam, w, h, CR.HOLE_DEPTH, ATT, FRAMES, seeds, jitter=False, mode=mode)
        hits = R.records(rnd.intersect(dsc, rnd.generate_rays(cam, w, h), mode=mode), L.HIT)  # the closest triangle, cut or not
        assert (hits["t"] < FLT_MAX).all() and (hits["triangle_id"] < 4).all()
        al = CR.alpha_at(verts, uv, tri_tex, alphas, hits["triangle_id"].astype(np.int64), hits["point"][:, :3])
        judged = np.abs(al - 0.5) >= 1e-3
        assert (~judged).sum() <= 0.05 * w * h
        print("edge: %d of %d pixels left out, %d cut" % ((~judged).sum(), w * h, (al < 0.5).sum()))
        sees = sees_light(got)
        black = (got[0] == 0).all(axis=1) & (got[1] == 0)
        assert (sees | black).all()
        assert (sees[judged] == (al[judged] < 0.5)).all()
        assert 0 < (al < 0.5).sum() < (hits["triangle_id"] < 2).sum()  # the edge runs inside the quad's triangles
    finally:
        dsc.close()


def test_first_hits_and_autofocus_see_through_the_hole(rnd):
    from montecarlopathtracing_amd.app import resolve_lens
    w, h = CR.HOLE_W, CR.HOLE_H
    cam = CR.hole_camera()
    dsc, (uv, tri_tex, images, alphas, verts) = _hole(rnd)
    try:
        x = R.records(rnd.generate_rays(cam, w, h), L.RAY)["origin"][:, 0]
        left = x < 0
        hits = R.records(rnd.first_hits(dsc, cam, w, h), L.HIT)
        assert (hits["material_id"][left] == 2).all() and np.abs(hits["point"][left, 2] + 2).max() < 1e-5  # the light behind the hole
        assert np.abs(hits["t"][left] - 6.0).max() < 1e-5  # the distance along the pixel's ray
        assert (hits["material_id"][~left] == 1).all() and np.abs(hits["t"][~left] - 4.0).max() < 1e-5
        px = int(np.nonzero(left)[0][0]) % w
        spec = {"aperture": 0.1, "focus": None, "focus_at": (px, 3)}
        assert abs(resolve_lens(rnd, dsc, cam, w, h, spec)[1] - 6.0) < 1e-5  # --focus-at on the hole: the light
        assert abs(rnd.autofocus(dsc, cam, w, h, w - 1 - px, 3) - 4.0) < 1e-5
        rnd.clear_texture_alpha(dsc)
        closed = R.records(rnd.first_hits(dsc, cam, w, h), L.HIT)
        assert (closed["material_id"][left] == 0).all() and abs(rnd.autofocus(dsc, cam, w, h, px, 3) - 4.0) < 1e-5
    finally:
        dsc.close()


# --------------------------------------------------------------- 5: the cap
_CAP = {}


def _stack(rnd):
    data, uv, tri_tex, images, alphas = CR.stack_scene(300)
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    rnd.set_texture_alpha(dsc, alphas)
    return dsc


def test_the_pass_cap_through_the_chain(rnd):
    """300 alpha-0 quads in front of a light: 255 are passed, the 256th is
    shaded as if opaque, and every ray is terminated within max_depth + 256
    rounds of the test's own loop (every launch of the chain is finite)."""
    w = h = 4
    depth = 3
    cam, seeds = CR.hole_camera(), R.default_seeds(w * h)
    dsc = _stack(rnd)
    try:
        n = w * h
        d_seed = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(rnd.device)
        colors = torch.ones((n, 4), dtype=torch.float32, device=rnd.device)
        rays = rnd.generate_rays(cam, w, h)
        hits, rounds = None, 0
        while rounds < depth + CUT_ROUNDS:
            r = R.records(rays, L.RAY)
            td = r["origin"][:, 3].copy().view(np.uint32)
            if ((td >> 24) != 0).all():
                break
            if rounds <= CR.PASS_CAP:  # after k rounds: k quads passed, nothing else happened
                assert (td == (rounds << 8)).all(), rounds
                assert (d_seed.cpu().numpy().view(np.uint32) == seeds).all() and bool((colors == 1).all())
                if rounds:
                    assert np.abs(r["origin"][:, 2] + 0.01 * (rounds - 1)).max() < 1e-5
            hits = rnd.intersect(dsc, rays, hits=hits)
            rnd.shade(dsc, rays, hits, colors, d_seed, depth)
            rounds += 1
        r = R.records(rays, L.RAY)
        td = r["origin"][:, 3].copy().view(np.uint32)
        assert ((td >> 24) != 0).all(), "every ray is terminated within max_depth + 256 rounds"
        assert CR.PASS_CAP + 1 <= rounds <= depth + CUT_ROUNDS
        assert (((td >> 8) & 0xFF) == CR.PASS_CAP).all()  # the count stops at 255 ...
        assert (d_seed.cpu().numpy().view(np.uint32) != seeds).all()  # ... and the 256th quad was shaded: it drew
        assert ((td & 0xFF) >= 1).all() and ((td & 0xFF) <= depth).all()
        ref, most = cut_chain(rnd, dsc, cam, w, h, depth, ATT, 2, seeds)
        assert CR.PASS_CAP + 1 <= most <= depth + CUT_ROUNDS
        _CAP["ref"] = ref
    finally:
        dsc.close()


def test_the_pass_cap_in_the_fused_kernel(rnd):
    """The same scene through k_render, once, after the chain has shown that
    every path on it ends: the chain's bits."""
    assert "ref" in _CAP, "the chain's cap test has to pass first: the fused kernel is not run on this scene without it"
    w = h = 4
    dsc = _stack(rnd)
    try:
        got = fused(rnd, dsc, CR.hole_camera(), w, h, 3, ATT, 2, R.default_seeds(w * h), jitter=False)
        assert_state_equal(got, _CAP["ref"], "the cap, fused")
    finally:
        dsc.close()


# ------------------------------------------------- 4: fused kernel equals chain
VARIANTS = {
    "closed": dict(),
    "one": dict(threshold=1.0),
    "smooth": dict(smooth=True),
    "bump": dict(bump=True),
    "opened": dict(opened=True),
}


@pytest.fixture(scope="module")
def rooms(rnd):
    """variant -> (DeviceScene with textures and alpha set, camera, depth, SceneData, (uv, tri_tex, images, alphas))."""
    held = {}

    def get(name):
        if name not in held:
            v = VARIANTS[name]
            data, uv, tri_tex, images, alphas = CR.room(opened=v.get("opened", False))
            dsc = rnd.upload(data)
            rnd.set_textures(dsc, uv, tri_tex, images)
            rnd.set_texture_alpha(dsc, alphas, v.get("threshold", 0.5))
            if v.get("smooth"):
                rnd.set_vertex_normals(dsc, S.vertex_normals(data.tris, 40.0))
            if v.get("bump"):
                rnd.set_normal_maps(dsc, uv, np.where(tri_tex >= 0, 0, -1).astype(np.int32), [BC.random_normal_map(4, 4, 40.0, 9)])
            if v.get("opened"):
                rnd.set_environment(dsc, scale=(0.8, 0.9, 1.2))
            held[name] = (dsc, S.parse_camera(CR.ROOM_CAM), CR.ROOM_DEPTH, data, (uv, tri_tex, images, alphas))
        return held[name]
    yield get
    for rec in held.values():
        rec[0].close()


@pytest.fixture(scope="module")
def chain_ref(rnd, rooms):
    """(room, mode, frames, jitter, lens, w, h) -> the chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name="closed", mode=L.MODE_EXACT, frames=FRAMES, jitter=False, lens=None, w=W, h=H):
        key = (name, mode, frames, jitter, lens, w, h)
        if key not in held:
            dsc, cam, depth = rooms(name)[:3]
            held[key], most = cut_chain(rnd, dsc, cam, w, h, depth, ATT, frames, R.default_seeds(w * h), mode, jitter, lens)
            assert most > depth or name == "one"  # pass-through is followed by real bounces: more rounds than the depth
        return held[key]
    return get


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
def test_cutout_render_equals_chain(rnd, rooms, chain_ref, schedule, mode):
    ref = chain_ref("closed", mode)
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode, schedule=schedule)
    assert_state_equal(got, ref, "sched%d/mode%d" % (schedule, mode))
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all() and (got[1] > 0).any()
    # not vacuous: the same textured scene without the alpha renders another image
    plain = rnd.upload(data)
    try:
        rnd.set_textures(plain, uv, tri_tex, images)
        flat = fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode, schedule=schedule)
    finally:
        plain.close()
    assert (got[0].view(np.uint32) != flat[0].view(np.uint32)).any(axis=1).sum() > W


@pytest.mark.parametrize("name", ["one", "smooth", "bump", "opened"])
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_cutout_render_variants_equal_chain(rnd, rooms, chain_ref, mode, name):
    """Threshold 1.0 (everything below an alpha of 1 is cut), vertex normals
    set, bump maps set, a constant environment over the opened room."""
    ref = chain_ref(name, mode)
    dsc, cam, depth = rooms(name)[:3]
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode)
    assert_state_equal(got, ref, "%s, mode %d" % (name, mode))
    assert got[0].tobytes() != chain_ref("closed", mode)[0].tobytes()


@pytest.mark.parametrize("window", [1, 2], ids=["window", "whole-stack"])
@pytest.mark.parametrize("quantized,fmt", [(2, 0), (1, 1), (3, 2)], ids=["128B", "quantized", "96B"])
def test_cutout_render_node_formats_and_stack_layouts(rnd, rooms, chain_ref, quantized, fmt, window):
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
@pytest.mark.parametrize("room", ["closed", "smooth", "bump"])
@pytest.mark.parametrize("cache,state", [(2, 0), (1, 2), (0, 2)], ids=["off", "always", "auto"])
def test_cutout_render_primary_cache_modes(rnd, rooms, chain_ref, cache, state, quantized, room):
    """A cached primary hit's alpha sits in the .w of its texture factor: a cut
    first segment passes through exactly as a traced one does."""
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


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
def test_cutout_frames_split_across_calls_and_blocks(rnd, rooms, chain_ref, quantized):
    ref = chain_ref("closed", frames=7)
    dsc, cam, depth = rooms("closed")[:3]
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    launches = 0
    try:
        rnd.set_tuning(quantized=quantized)
        for f0, nf in ((0, 2), (2, 5)):
            rnd.render_frames(dsc, cam, st, depth, ATT, nf, frame_begin=f0, frames_per_launch=3)
            launches += rnd.stats()["frames_per_block"] < nf
    finally:
        rnd.set_tuning()
    assert launches >= 1  # at least one call ran several 3-frame blocks per pixel
    assert_state_equal(state_np(st), ref, "split calls, 3-frame blocks")


def test_cutout_two_stripes_one_after_the_other(rnd, rooms, chain_ref):
    ref = chain_ref("closed")
    dsc, cam, depth = rooms("closed")[:3]
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, depth, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k, stripe_count=2)
    assert_state_equal(state_np(st), ref, "2 stripes of 8 rows")


@pytest.mark.parametrize("lens", [None, LENS], ids=["jitter", "lens"])
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
def test_cutout_jittered_render_and_lens_equal_chain(rnd, rooms, chain_ref, mode, lens):
    ref = chain_ref("closed", mode, jitter=True, lens=lens)
    dsc, cam, depth = rooms("closed")[:3]
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=True, mode=mode, lens=lens)
    assert_state_equal(got, ref, "jittered, lens %r, mode %d" % (lens, mode))
    assert got[0].tobytes() != chain_ref("closed", mode)[0].tobytes()


@pytest.mark.parametrize("quantized", [2, 1, 3], ids=["128B", "quantized", "96B"])
def test_cutout_ragged_image(rnd, rooms, chain_ref, quantized):
    ref = chain_ref("closed", w=20, h=13)
    dsc, cam, depth = rooms("closed")[:3]
    try:
        rnd.set_tuning(quantized=quantized)
        got = fused(rnd, dsc, cam, 20, 13, depth, ATT, FRAMES, R.default_seeds(20 * 13), jitter=False)
    finally:
        rnd.set_tuning()
    assert_state_equal(got, ref, "20 x 13, quantized=%d" % quantized)


def test_cutout_render_with_counters_on(rnd, rooms, chain_ref):
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    plain = rnd.upload(data)
    try:
        rnd.set_textures(plain, uv, tri_tex, images)
        rnd.set_stats(True)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
        fused(rnd, plain, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s0 = rnd.stats()
    finally:
        rnd.set_stats(False)
        plain.close()
    assert s["bad_material"] == 0 and s["segments"] > W * H
    assert s["segments"] != s0["segments"]  # a cut hit is a traced segment of its own
    assert_state_equal(got, chain_ref("closed"), "stats on")


# ------------------------------------------------------------- 6: invariance
def test_alpha_of_ones_and_set_then_clear_render_the_textured_bits(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    seeds = R.default_seeds(W * H)
    a, b = rnd.upload(data), rnd.upload(data)
    try:
        rnd.set_textures(a, uv, tri_tex, images)
        rnd.set_textures(b, uv, tri_tex, images)
        for kw in (dict(jitter=False), dict(jitter=True), dict(jitter=False, mode=L.MODE_NOPRUNE)):
            plain = fused(rnd, a, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw)
            rnd.set_texture_alpha(b, [None if x is None else np.ones_like(x) for x in alphas])
            got = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw)
            assert_state_equal(got, plain, "an alpha of ones %r" % (kw,))
            rnd.set_texture_alpha(b, [None] * len(alphas), 1.0)
            assert_state_equal(fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw), plain,
                               "no alpha image, threshold 1 %r" % (kw,))
            rnd.set_texture_alpha(b, alphas)
            cut = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw)
            assert cut[0].tobytes() != plain[0].tobytes()
            rnd.clear_texture_alpha(b)
            assert_state_equal(fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, frames_per_launch=3, **kw), plain,
                               "set then clear %r" % (kw,))
        # a later set_textures drops the alpha
        rnd.set_texture_alpha(b, alphas)
        rnd.set_textures(b, uv, tri_tex, images)
        assert_state_equal(fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False, frames_per_launch=3),
                           fused(rnd, a, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False, frames_per_launch=3),
                           "set_textures drops the alpha")
    finally:
        a.close(), b.close()


def test_alpha_of_ones_renders_the_committed_golden(rnd):
    """C1 through the textured kernels with a texture of ones and an alpha of
    ones on every triangle: the reference's bits."""
    def prepare(dsc):
        rnd.set_textures(dsc, *_cbox_textures(1.0))
        rnd.set_texture_alpha(dsc, [np.ones((3, 5), np.float32)])
    _golden_c1(rnd, prepare)


def test_alpha_set_then_cleared_renders_the_committed_golden(rnd):
    def prepare(dsc):
        rnd.set_textures(dsc, *_cbox_textures(1.0))
        rnd.set_texture_alpha(dsc, [np.zeros((3, 5), np.float32)])
        rnd.clear_texture_alpha(dsc)
    _golden_c1(rnd, prepare)


def test_set_texture_alpha_validates_and_leaves_the_scene(rnd, rooms):
    import ctypes
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    seeds = R.default_seeds(W * H)
    before = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)

    def with_value(v):
        a = [None if x is None else x.copy() for x in alphas]
        a[3][1, 2] = v
        return a
    for bad in (with_value(1.5), with_value(np.nan), with_value(-0.25), with_value(np.inf), alphas[:-1], alphas + [None]):
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*set_texture_alpha"):
            rnd.set_texture_alpha(dsc, bad)
    for th in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*threshold"):
            rnd.set_texture_alpha(dsc, alphas, th)
    ta = L.TextureAlpha(len(alphas), None, 0.5, 0.0)
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b"):
        L.check(L.lib().mcpt_scene_set_texture_alpha(rnd.ctx, dsc.handle, ctypes.byref(ta)))
    with pytest.raises(ValueError):
        rnd.set_texture_alpha(dsc, [np.zeros(3, np.float32)] + alphas[1:])
    assert_state_equal(fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False), before,
                       "a refused call leaves the scene rendering its previous bits")
    # a scene without textures has no alpha to set
    plain = rnd.upload(data)
    try:
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*no textures"):
            rnd.set_texture_alpha(plain, alphas)
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*no textures"):
            rnd.clear_texture_alpha(plain)
    finally:
        plain.close()


def test_max_depth_above_255_is_refused_with_cutouts_only(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    st = rnd.new_state(8, 8, R.default_seeds(64))
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*255"):
        rnd.render_frames(dsc, cam, st, 256, ATT, 1)
    rays = rnd.generate_rays(cam, 8, 8)
    hits = rnd.intersect(dsc, rays)
    colors = torch.ones((64, 4), dtype=torch.float32, device=rnd.device)
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*255"):
        rnd.shade(dsc, rays, hits, colors, st.seeds, 256)
    rnd.render_frames(dsc, cam, st, 255, ATT, 1)  # 255 is fine
    plain = rnd.upload(data)
    try:
        rnd.set_textures(plain, uv, tri_tex, images)
        rnd.render_frames(plain, cam, rnd.new_state(8, 8, R.default_seeds(64)), 256, ATT, 1)  # no cutouts: MCPT_DEPTH_MASK's range
        torch.cuda.synchronize()
    finally:
        plain.close()


def test_primary_cache_is_dropped_by_set_and_clear(rnd, rooms):
    dsc, cam, depth, data, (uv, tri_tex, images, alphas) = rooms("closed")
    seeds = R.default_seeds(W * H)
    b = rnd.upload(data)
    try:
        rnd.set_textures(b, uv, tri_tex, images)
        rnd.drop_caches()
        first = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # built
        fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 1  # read
        rnd.set_texture_alpha(b, alphas)
        got = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2  # rebuilt, with the alpha in the factors' .w
        assert got[0].tobytes() != first[0].tobytes()
        rnd.clear_texture_alpha(b)
        back = fused(rnd, b, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == 2
        assert_state_equal(back, first, "after the clear")
    finally:
        b.close()


# -------------------------------------------------------------- debug build
def _digest(state):
    h = hashlib.sha256()
    for a in state:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_debug_build_renders_the_cutout_room_clean(rnd, rooms, chain_ref):
    assert os.path.exists(DEBUG_LIB), "debug build missing (__graft_entry__.build makes it)"
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import cutout_ref; cutout_ref.debug_main()"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert [(c["mode"], c["node_format"]) for c in lines[1:]] == [(0, 0), (0, 1), (0, 2), (1, 0)]
    for c in lines[1:]:
        assert c["violations"] == 0, c
        assert c["digest"] == _digest(chain_ref("closed", c["mode"])), c
