"""The thin-lens camera (opt-in depth of field; mcpt_render_frames_lens,
mcpt_generate_rays_lens) on the GPU.  The reference has no lens, so there are
two yardsticks: the float64 restatement of the definition (tests/lens_ref.py)
for the ray generator, and, for the fused kernel, the chain of the project's
own wavefront kernels (tests/test_gpu_jitter.py's, each pinned to the
reference's kernels by tests/test_gpu_parity.py) with the lens generator in
front, whose bits k_render must give.  None of this needs oracle/_ref."""
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

from . import lens_ref as LR  # noqa: E402
from . import scenes  # noqa: E402
from .test_jitter_cpu import ZERO_DRAW_SEEDS, _entry, jitter_draws, lcg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
GOLD = os.path.join(ROOT, "tests", "golden")
W, H, FRAMES, ATT = 37, 21, 6, 4  # frames 5 runs past the history's cap (attempt 4)
# scene -> (data, camera, depth, lens (R, F)): focused near the scene's middle, a blur of a few pixels beyond
CASES = {"cbox": (scenes.cbox, scenes.CBOX_CAM, 4, (12.0, 1000.0)), "mis": (scenes.mis, scenes.MIS_CAM, 12, (0.25, 13.0))}
# the ray generator's cameras and a lens for each (R / F about 0.02 and up: the mutants' distance, below)
RAY_CAMS = {"cbox": (scenes.CBOX_CAM, (20.0, 1000.0)), "mis": (scenes.MIS_CAM, (0.4, 13.0)),
            "dining": (scenes.DINING_CAM, (0.15, 5.0))}

# The largest ray_error (tests/lens_ref.py) of mcpt_generate_rays_lens against the float64 restatement
# measured on an MI355X over every case of test_lens_rays_against_float64, and the bound: 8 x that
# (DESIGN.md 3.15).  Each of the four mutant restatements sits at least 100 x the bound away.
MEASURED_RAY_ERROR = 1.671e-7  # 1.670e-7 at dining 37x21, pinhole, scaled axes; the mutants sit at 1.8e-3 to 6e-2
RAY_BOUND = 8 * MEASURED_RAY_ERROR


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


def chain(rnd, dsc, cam, w, h, depth, attempt, calls, seeds, mode=L.MODE_EXACT):
    """tests/test_gpu_jitter.py's frame loop out of the wavefront kernels,
    with the lens generator.  calls: [(frames, lens)], lens (R, F), "jitter"
    or None (the unjittered generator), run one after the other on one state."""
    n = w * h
    d_seed = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(rnd.device)
    hist = torch.zeros((n, 4), dtype=torch.float32, device=rnd.device)
    count = torch.zeros(n, dtype=torch.int32, device=rnd.device)
    f = 0
    for frames, lens in calls:
        for _ in range(frames):
            colors = torch.ones((n, 4), dtype=torch.float32, device=rnd.device)
            if lens is None:
                rays = rnd.generate_rays(cam, w, h)
            elif lens == "jitter":
                rays = rnd.generate_rays_jittered(cam, w, h, d_seed)
            else:
                rays = rnd.generate_rays_lens(cam, w, h, d_seed, lens)
            hits = None
            for _b in range(depth):
                hits = rnd.intersect(dsc, rays, hits=hits, mode=mode)
                rnd.shade(dsc, rays, hits, colors, d_seed, depth)
            if f <= attempt:
                rnd.accumulate(colors, hist, count, attempt)
            f += 1
    torch.cuda.synchronize()
    return hist.cpu().numpy(), count.cpu().numpy(), d_seed.cpu().numpy().view(np.uint32)


def state_np(st):
    torch.cuda.synchronize()
    return st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()


def fused(rnd, dsc, cam, w, h, depth, attempt, frames, seeds, **kw):
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(dsc, cam, st, depth, attempt, frames, **kw)
    return state_np(st)


def raw_render(rnd, dsc, cam, st, depth, attempt, frames, jitter, lens, frame_begin=0, entry="lens"):
    """The C call itself: lens = None (a null pointer) or (R, F), whatever
    `jitter` says.  entry "plain": mcpt_render_frames.  Returns the status."""
    p = L.RenderParams()
    p.width, p.height = st.width, st.height
    p.max_depth, p.max_attempt, p.frame_begin, p.frames = depth, attempt, frame_begin, frames
    p.stripe_rows, p.stripe_index, p.stripe_count = 16, 0, 1
    p.mode, p.frames_per_launch, p.schedule, p.jitter = L.MODE_EXACT, 0, L.SCHED_PAIRED, int(jitter)
    c = np.ascontiguousarray(cam)
    args = [L.ptr(st.seeds), L.ptr(st.hist), L.ptr(st.count), R._stream()]
    if entry == "plain":
        return L.lib().mcpt_render_frames(rnd.ctx, dsc.handle, L.ptr(c), ctypes.byref(p), *args)
    lens_c = None if lens is None else ctypes.byref(L.Lens(*lens))
    return L.lib().mcpt_render_frames_lens(rnd.ctx, dsc.handle, L.ptr(c), lens_c, ctypes.byref(p), *args)


@pytest.fixture(scope="module")
def chain_ref(rnd, uploaded):
    """(scene, mode, w, h, frames) -> the lens chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name, mode=L.MODE_EXACT, w=W, h=H, frames=FRAMES):
        key = (name, mode, w, h, frames)
        if key not in held:
            dsc, cam, depth, lens = uploaded(name)
            held[key] = chain(rnd, dsc, cam, w, h, depth, ATT, [(frames, lens)], R.default_seeds(w * h), mode)
        return held[key]
    return get


# ------------------------------------------------------ 1: rays against float64
def _rho_zero_seeds(k=4):
    """Seeds whose third 15-bit draw is 0: rho = 0, the lens point is the centre."""
    s = np.arange(1 << 20, dtype=np.uint32)
    r1 = LR.lens_draws(s)[2]
    return s[r1 == 0][:k]


def _planted_seeds(n):
    """default seeds with the zero-jitter seeds (jx = jy = 0) and rho = 0 seeds planted."""
    seeds = R.default_seeds(n).copy()
    zero_jitter = np.array([0, n // 3, n // 2 + 5, n - 1])
    seeds[zero_jitter] = np.array(ZERO_DRAW_SEEDS, np.uint32)
    centre = np.array([1, n // 4, n // 2 + 6, n - 2])
    seeds[centre] = _rho_zero_seeds(4)
    return seeds, zero_jitter, centre


def _ray_cam(name, ortho, scaled):
    cam = S.parse_camera(RAY_CAMS[name][0]).copy()
    if ortho:
        cam["camera_type"] = 1
        cam["arg"] = np.float32({"cbox": 500.0, "mis": 9.5, "dining": 4.0}[name])
    if scaled:  # horizontal and up are not unit vectors in general: generateRay scales them, the lens normalises
        cam["horizontal"] *= np.float32(1.5)
        cam["up"] *= np.float32(0.75)
    return cam


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("ortho", [False, True], ids=["pinhole", "ortho"])
@pytest.mark.parametrize("w,h", [(64, 48), (37, 21)])
@pytest.mark.parametrize("name", ["cbox", "mis", "dining"])
def test_lens_rays_against_float64(rnd, name, w, h, ortho, scaled):
    cam = _ray_cam(name, ortho, scaled)
    lens = RAY_CAMS[name][1]
    seeds, zero_jitter, centre = _planted_seeds(w * h)
    d_seed = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
    got = R.records(rnd.generate_rays_lens(cam, w, h, d_seed, lens), L.RAY)
    after = d_seed.cpu().numpy().view(np.uint32)
    want_o, want_d, want_after = LR.lens_rays(cam, w, h, seeds, *lens)
    # the advanced seeds are exactly four draws on
    assert_bits_equal(after, want_after, "seeds after four draws")
    assert_bits_equal(after, lcg(lcg(jitter_draws(seeds)[2])), "two draws past the jitter's")
    # o.w (term_depth 0) and d.w (the pixel id) carry the bits they carried
    assert (got["origin"][:, 3].view(np.uint32) == 0).all()
    assert_bits_equal(got["direction"][:, 3].view(np.int32), np.arange(w * h, dtype=np.int32), "pixel id")
    err = LR.ray_error(got["origin"][:, :3], got["direction"][:, :3], want_o, want_d)
    print("lens rays %s %dx%d ortho=%d scaled=%d: error %.3e (bound %.3e)" % (name, w, h, ortho, scaled, err, RAY_BOUND))
    assert err <= RAY_BOUND
    # rho = 0: the lens point is the centre, so the origin is the jittered ray's, bit for bit
    d_seed2 = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
    jit = R.records(rnd.generate_rays_jittered(cam, w, h, d_seed2), L.RAY)
    assert (LR.lens_draws(seeds)[2][centre] == 0).all()
    assert_bits_equal(got["origin"][centre], jit["origin"][centre], "origin at rho = 0")
    assert (jitter_draws(seeds)[0][zero_jitter] == 0).all()
    # the four mutants: each at least two orders above the bound ("unnormalised" needs non-unit axes, "focus_along_ray" rays off the axis)
    for m in LR.MUTANTS:
        if m == "unnormalised" and not scaled:
            continue
        if m == "focus_along_ray" and ortho:
            continue  # every orthographic ray runs along the view axis: there the mutant is the definition
        mo, md, _ = LR.lens_rays(cam, w, h, seeds, *lens, mutant=m)
        merr = LR.ray_error(got["origin"][:, :3], got["direction"][:, :3], mo, md)
        print("  mutant %s: %.3e" % (m, merr))
        assert merr >= 100 * RAY_BOUND, m


# ------------------------------------------------------------- 2: off is off
def test_null_lens_and_zero_radius_are_the_jittered_call(rnd, uploaded):
    dsc, cam, depth, lens = uploaded("cbox")
    seeds = R.default_seeds(W * H)
    want = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=True)
    for what, ln in (("a null lens", None), ("R == 0", (0.0, lens[1]))):
        st = rnd.new_state(W, H, seeds)
        assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, 1, ln) == 0
        assert_state_equal(state_np(st), want, what)
    # and through the Python layer, where lens=(0, F) still switches the jitter on
    assert_state_equal(fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, lens=(0.0, lens[1])), want, "lens=(0, F)")
    # R == 0 without jitter: the unjittered call
    plain = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False)
    st = rnd.new_state(W, H, seeds)
    assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, 0, (0.0, lens[1])) == 0
    assert_state_equal(state_np(st), plain, "R == 0, jitter 0")
    assert plain[0].tobytes() != want[0].tobytes()


def test_generate_rays_lens_with_zero_radius_is_the_jittered_generator(rnd):
    cam = S.parse_camera(scenes.MIS_CAM)
    seeds, _, _ = _planted_seeds(W * H)
    d0 = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
    want = R.records(rnd.generate_rays_jittered(cam, W, H, d0), L.RAY)
    for ln in (None, (0.0, 13.0)):
        d1 = torch.from_numpy(seeds.view(np.int32).copy()).to(rnd.device)
        got = R.records(rnd.generate_rays_lens(cam, W, H, d1, ln), L.RAY)
        assert_bits_equal(got["origin"], want["origin"], "origin")
        assert_bits_equal(got["direction"], want["direction"], "direction")
        assert_bits_equal(d1.cpu().numpy(), d0.cpu().numpy(), "seeds: two draws")


def test_unjittered_null_lens_call_gives_the_c1_golden(rnd):
    g = np.load(os.path.join(GOLD, "image_c1_cbox.npz"))
    w, h, depth, frames, att = (int(x) for x in g["meta"])
    dsc = rnd.upload(scenes.cbox())
    try:
        st = rnd.new_state(w, h, g["seeds_in"])
        assert raw_render(rnd, dsc, S.parse_camera(scenes.CBOX_CAM), st, depth, att, frames, 0, None) == 0
        hist, count, seeds = state_np(st)
        assert_bits_equal(count, g["count"], "count")
        assert_bits_equal(seeds, g["seeds"], "seeds")
        assert_bits_equal(hist, g["hist"], "hist")
    finally:
        dsc.close()


# ------------------------------------------------- 3: k_render equals the chain
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_lens_render_equals_chain(rnd, uploaded, chain_ref, name, schedule, mode):
    dsc, cam, depth, lens = uploaded(name)
    ref = chain_ref(name, mode)
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), mode=mode, schedule=schedule, lens=lens)
    assert rnd.stats()["primary_cache"] == 0
    assert_state_equal(got, ref, "%s/sched%d/mode%d" % (name, schedule, mode))
    assert (ref[1] > 0).any()
    # and the lens did something: the jitter-only render is another image
    jit = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), mode=mode, jitter=True)
    assert jit[0].tobytes() != got[0].tobytes() and jit[2].tobytes() != got[2].tobytes()


@pytest.mark.parametrize("knobs", [{"quantized": 1}, {"quantized": 2}, {"quantized": 3}, {"stack_window": 1},
                                   {"stack_window": 2}], ids=lambda k: "%s=%d" % next(iter(k.items())))
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_lens_render_node_formats_and_stack_layouts(rnd, uploaded, chain_ref, name, knobs):
    dsc, cam, depth, lens = uploaded(name)
    try:
        rnd.set_tuning(**knobs)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), lens=lens)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    if "quantized" in knobs:
        assert s["node_format"] == {1: 1, 2: 0, 3: 2}[knobs["quantized"]]
    else:
        assert s["stack_window"] == (1 if knobs["stack_window"] == 1 else 0)
    assert_state_equal(got, chain_ref(name), repr(knobs))


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3)])
@pytest.mark.parametrize("name", ["cbox", "mis"])
def test_lens_render_equals_chain_tiny_images(rnd, uploaded, chain_ref, name, w, h):
    dsc, cam, depth, lens = uploaded(name)
    got = fused(rnd, dsc, cam, w, h, depth, ATT, FRAMES, R.default_seeds(w * h), lens=lens)
    assert_state_equal(got, chain_ref(name, w=w, h=h), "%s %dx%d" % (name, w, h))


@pytest.mark.parametrize("split,frames", [(((0, 2), (2, 4)), 6), (((0, 2), (2, 5)), 7)])
def test_lens_frames_split_across_calls_and_blocks(rnd, uploaded, chain_ref, split, frames):
    """Calls of (frame_begin, frames) with 3-frame blocks: the hand-off carries
    the seed past the lens draws."""
    dsc, cam, depth, lens = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for f0, nf in split:
        rnd.render_frames(dsc, cam, st, depth, ATT, nf, frame_begin=f0, frames_per_launch=3, lens=lens)
        assert rnd.stats()["primary_cache"] == 0
    assert_state_equal(state_np(st), chain_ref("cbox", frames=frames), "split %r" % (split,))


def test_lens_two_stripes_one_after_the_other(rnd, uploaded, chain_ref):
    dsc, cam, depth, lens = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, depth, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k,
                          stripe_count=2, lens=lens)
    assert_state_equal(state_np(st), chain_ref("cbox"), "2 stripes of 8 rows")


def _cbox_textures(data):
    """UVs from the vertices' x and y (they repeat across the box) and one checker for every triangle."""
    from .texture_ref import checker
    v = data.tris["v"][:, :, :3]
    uv = np.stack([v[..., 0] / 200.0, v[..., 1] / 150.0 + v[..., 2] / 400.0], axis=-1).astype(np.float32)
    return uv, np.zeros(len(v), np.int32), [checker(5, 3)]


@pytest.mark.parametrize("what", ["environment", "vertex_normals", "textures", "counters"])
def test_lens_render_equals_chain_with_other_opt_ins(rnd, what):
    """A constant environment, vertex normals, textures, counters on: the
    chain's kernels read the same scene, so it stays the yardstick."""
    data = scenes.cbox()
    dsc, cam = rnd.upload(data), S.parse_camera(scenes.CBOX_CAM)
    _, _, depth, lens = CASES["cbox"]
    seeds = R.default_seeds(W * H)
    try:
        if what == "environment":
            rnd.set_environment(dsc, scale=(0.4, 0.5, 0.7))
        elif what == "vertex_normals":
            rnd.set_vertex_normals(dsc, S.smooth_normals(data.tris, 40.0))
        elif what == "textures":
            rnd.set_textures(dsc, *_cbox_textures(data))
        ref = chain(rnd, dsc, cam, W, H, depth, ATT, [(FRAMES, lens)], seeds)
        if what == "counters":
            rnd.set_stats(True)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, lens=lens)
        if what == "counters":
            assert rnd.stats()["segments"] > 0
        assert_state_equal(got, ref, what)
    finally:
        rnd.set_stats(False)
        dsc.close()


def test_lens_call_between_cached_calls(rnd, uploaded):
    """A lens call neither reads, builds nor invalidates the primary-hit cache
    of the unjittered calls around it, whose bits are unchanged."""
    dsc, cam, depth, lens = uploaded("cbox")
    seeds = R.default_seeds(W * H)
    ref = chain(rnd, dsc, cam, W, H, depth, ATT, [(2, None), (2, lens), (1, None)], seeds)
    rnd.drop_caches()
    st = rnd.new_state(W, H, seeds)
    seen = []
    for frames, ln in ((2, None), (2, lens), (1, None)):
        rnd.render_frames(dsc, cam, st, depth, ATT, frames, lens=ln)
        seen.append(rnd.stats()["primary_cache"])
    assert seen == [2, 0, 1]  # built; untouched; still there to be read
    assert_state_equal(state_np(st), ref, "unjittered, lens, unjittered")


# ------------------------------------------------------- 4: argument errors
@pytest.mark.parametrize("jitter,lens", [
    (0, (1.0, 10.0)),                                                   # R > 0 without jitter
    (1, (-1.0, 10.0)),                                                  # R < 0
    (1, (1.0, 0.0)), (1, (1.0, -5.0)), (1, (0.0, 0.0)),                 # F <= 0 (also with R == 0)
    (1, (float("nan"), 10.0)), (1, (1.0, float("nan"))),
    (1, (float("inf"), 10.0)), (1, (1.0, float("inf"))), (1, (1.0, float("-inf"))),
], ids=repr)
def test_bad_lens_is_an_argument_error(rnd, uploaded, chain_ref, jitter, lens):
    dsc, cam, depth, good = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    before = state_np(st)
    assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, jitter, lens) == -1  # MCPT_ERR_ARG
    assert b"lens" in L.lib().mcpt_last_error()
    assert_state_equal(state_np(st), before, "state after the refused call")
    if jitter:  # the generator refuses the same values
        d_seed = torch.from_numpy(before[2].view(np.int32).copy()).to(rnd.device)
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*lens"):
            rnd.generate_rays_lens(cam, W, H, d_seed, lens)
        assert_bits_equal(d_seed.cpu().numpy().view(np.uint32), before[2], "seeds after the refused call")
    # a following good call renders correctly
    assert raw_render(rnd, dsc, cam, st, depth, ATT, FRAMES, 1, good) == 0
    assert_state_equal(state_np(st), chain_ref("cbox"), "the good call after")


def test_python_layer_refuses_a_lens_with_jitter_off(rnd, uploaded):
    dsc, cam, depth, lens = uploaded("cbox")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    with pytest.raises(ValueError, match="jitter"):
        rnd.render_frames(dsc, cam, st, depth, ATT, 1, jitter=False, lens=lens)
    assert st.frames_done == 0


# ------------------------------------------ 5: the visible effect, predicted exactly
@pytest.mark.parametrize("where", ["at_F", "at_2F"])
def test_lit_half_space_blurs_as_predicted(rnd, where):
    """One emissive rectangle over x >= 0 and nothing else: count = the frames
    whose lens ray hit it, replayed per pixel and frame in float64
    (lens_ref.edge_predict).  In focus the edge is as sharp as the jitter-only
    render's; at twice the focus distance it is blurred over the lens disk."""
    w, h, frames = LR.EDGE_W, LR.EDGE_H, LR.EDGE_FRAMES
    depth = LR.EDGE_F if where == "at_F" else 2 * LR.EDGE_F
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (1, 1, 1), (0, 0, 0), (0, 0, 0), 1.0)
    assert int(mats[0]["type"]) == L.MCPT_LIGHT
    cam = S.parse_camera(LR.EDGE_CAM)
    seeds = R.default_seeds(w * h)
    want, near, want_seeds = LR.edge_predict(cam, seeds, depth)
    assert near.sum() <= 0.02 * w * h  # a condition on the chosen geometry (tests/test_lens_cpu.py checks it too)
    dsc = rnd.upload(S.SceneData.from_arrays(LR.edge_rect(depth), np.zeros(2, np.int32), mats))
    try:
        hist, count, after = fused(rnd, dsc, cam, w, h, 2, frames, frames, seeds, lens=(LR.EDGE_R, LR.EDGE_F))
        pinhole = fused(rnd, dsc, cam, w, h, 2, frames, frames, seeds, jitter=True)[1]
    finally:
        dsc.close()
    assert_bits_equal(after, want_seeds, "seeds: four draws a frame")
    keep = ~near
    wrong = np.nonzero(keep & (count != want))[0]
    print("%s: %d pixels left out, %d lit, %d partly" % (where, near.sum(), (count == frames).sum(),
                                                       ((count > 0) & (count < frames)).sum()))
    assert len(wrong) == 0, "count differs from the prediction at pixels %s: got %s, want %s" % (
        wrong[:8], count[wrong[:8]], want[wrong[:8]])
    assert (count == frames).any() and (count == 0).any()
    partial = ((count > 0) & (count < frames)).reshape(h, w).sum(axis=1)
    sharp = ((pinhole > 0) & (pinhole < frames)).reshape(h, w).sum(axis=1)
    if where == "at_F":
        assert partial.max() <= 2, partial
    else:
        diameter = LR.edge_blur_diameter_px(depth)
        assert partial.min() >= diameter - 2, (partial, diameter)
        assert sharp.max() <= 2, sharp  # the same rectangle through the pinhole: an edge, not a ramp


# ---------------------------------------------------- 6: App from a config key
def test_app_renders_with_a_lens_from_config_key(tmp_path):
    from montecarlopathtracing_amd.app import App
    path = tmp_path / "config.json"
    path.write_text(json.dumps(_entry(lens={"aperture": 12.0, "focus_at": [16, 12]})))
    seeds = R.default_seeds(32 * 32)
    app = App(str(path), seeds=seeds, out_dir=str(tmp_path))
    assert app.jitter is True  # the lens switched it on
    out = app.run()
    assert os.path.getsize(out) > 0 and app.attempt_count == 4
    focus = app.renderer.autofocus(app.scene, app.camera, 32, 32, 16, 12)
    assert app.lens == (12.0, focus) and 800 < focus < 1400  # the box stands 800 to 1360 ahead of the camera
    # the arithmetic of the autofocus, from the records themselves
    rays = R.records(app.renderer.generate_rays(app.camera, 32, 32), L.RAY)
    hits = R.records(app.renderer.first_hits(app.scene, app.camera, 32, 32), L.HIT)
    k = 12 * 32 + 16
    assert focus == R.focus_from_hit(hits["t"][k], rays["direction"][k], app.camera[0]["direction"])
    got = state_np(app.state)
    want = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, seeds, lens=(12.0, focus))
    assert_state_equal(got, want, "App with a \"lens\" key")
    jit = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, seeds, jitter=True)
    assert got[0].tobytes() != jit[0].tobytes()
    # a pixel that sees nothing cannot be focused on
    dsc = app.renderer.upload(S.SceneData.from_arrays(LR.edge_rect(10.0), np.zeros(2, np.int32), app.scene.data.mats[:1]))
    try:
        with pytest.raises(ValueError, match=r"\(47, 3\)"):
            app.renderer.autofocus(dsc, S.parse_camera(LR.EDGE_CAM), 48, 16, 47, 3)
    finally:
        dsc.close()


# ------------------------------------------------------------ 7: debug build
def _digest(state):
    dg = hashlib.sha256()
    for a in state:
        dg.update(np.ascontiguousarray(a).tobytes())
    return dg.hexdigest()


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_debug_build_lens_bounds_checks_clean(rnd):
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", "from tests import lens_ref; lens_ref.debug_main()"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert len(lines) == 2 and lines[1]["violations"] == 0 and lines[1]["primary_cache"] == 0, lines
    from . import texture_ref as TR
    data, uv, tri_tex, images = TR.room()
    dsc = rnd.upload(data)
    try:
        rnd.set_textures(dsc, uv, tri_tex, images)
        got = fused(rnd, dsc, S.parse_camera(TR.ROOM_CAM), W, H, TR.ROOM_DEPTH, ATT, FRAMES, R.default_seeds(W * H),
                    lens=LR.ROOM_LENS)
    finally:
        dsc.close()
    assert lines[1]["digest"] == _digest(got)
