"""Environment lighting (opt-in; mcpt_scene_set_environment, mcpt_env_eval): a
ray that leaves the scene picks up scale * map(direction) instead of black.
The reference has no environment, so the yardsticks are the project's own:
the float64 restatement of the lookup (tests/env_ref.py) for mcpt_env_eval, and
for the fused kernel the chain of wavefront kernels (generate, intersect,
shade, accumulate; tests/test_gpu_jitter.py's harness), whose k_shade applies
the same lookup in its miss branch.  None of this needs oracle/_ref."""
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

from . import env_ref, scenes  # noqa: E402
from .test_gpu_jitter import assert_bits_equal, assert_state_equal, chain, fused, state_np  # noqa: E402
from .test_jitter_cpu import _entry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W, H, FRAMES, ATT = 48, 40, 6, 4  # 6 frames run past the history's cap (attempt 4)
CASES = {"open": (env_ref.open_scene, env_ref.OPEN_CAM, env_ref.OPEN_DEPTH), "cbox": (scenes.cbox, scenes.CBOX_CAM, 4)}
ENVS = env_ref.lit_environments()


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module")
def lit(rnd):
    """(scene, environment name or None) -> (DeviceScene, camera, depth): the
    scene uploaded once, its environment set (or cleared) for this use."""
    held = {}

    def get(name, env):
        if name not in held:
            getter, camjson, depth = CASES[name]
            held[name] = (rnd.upload(getter()), S.parse_camera(camjson), depth)
        dsc = held[name][0]
        if env is None:
            rnd.clear_environment(dsc)
        else:
            rnd.set_environment(dsc, **ENVS[env])
        return held[name]
    yield get
    for dsc, _, _ in held.values():
        dsc.close()


@pytest.fixture(scope="module")
def chain_ref(rnd, lit):
    """(scene, environment, mode, frames, jitter) -> the chain's (hist, count, seeds), computed once."""
    held = {}

    def get(name, env, mode=L.MODE_EXACT, frames=FRAMES, jitter=False):
        key = (name, env, mode, frames, jitter)
        if key not in held:
            dsc, cam, depth = lit(name, env)
            held[key] = chain(rnd, dsc, cam, W, H, depth, ATT, [(frames, jitter)], R.default_seeds(W * H), mode)
        return held[key]
    return get


# ------------------------------------------------------ the lookup vs float64
# Largest error of mcpt_env_eval against tests/env_ref.py (float64) over the
# cases below, |gpu - ref| / max(|ref|, mean |ref|), measured on an MI355X, and
# the bound held: 8x that, the margin DESIGN.md 3.11 uses for fp32 against float64.
# Measured per case: 1.9e-7 to 2.8e-7 (the 7x5 map at rotation 0 the largest);
# the half-texel shift and the clamp sit at 2.5e-2 to 3.4e-1, four orders above the bound.
LOOKUP_MEASURED = 2.763e-7
LOOKUP_BOUND = 8 * LOOKUP_MEASURED


def lookup_directions():
    """About 4 K unit directions as float32: random ones, the six axes (the
    poles among them), near-polar ones, the seam (atan2 = +pi and -pi: d.x =
    +0 and -0 at d.z > 0, and a float's step to either side) and d.x = +-0
    opposite it."""
    rng = np.random.default_rng(20)
    v = rng.normal(size=(4000, 3))
    parts = [v / np.sqrt((v * v).sum(axis=1, keepdims=True))]
    parts.append(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64))
    t = np.array([1e-7, 1e-5, 1e-3, 3e-2])
    for sy in (1.0, -1.0):  # around the poles
        for ax, az in ((1, 0), (0, 1), (-1, 0), (0, -1), (0.6, -0.8)):
            parts.append(np.stack([ax * np.sin(t), sy * np.cos(t), az * np.sin(t)], axis=1))
    ys = np.array([-0.999, -0.7, -0.2, 0.0, 0.3, 0.8, 0.9999])
    zs = np.sqrt(1 - ys * ys)
    for x in (0.0, -0.0, 1e-7, -1e-7, 1e-4, -1e-4):
        for sz in (1.0, -1.0):  # sz = 1: the seam; -1: the map's centre column
            parts.append(np.stack([np.full_like(ys, x), ys, sz * zs], axis=1))
    d = np.concatenate(parts).astype(np.float32)
    assert (np.signbit(d[:, 0]) & (d[:, 0] == 0)).any()  # -0 survived
    return d


def eval_on_gpu(rnd, dsc, d):
    rays = np.zeros(len(d), L.RAY)
    rays["direction"][:, :3] = d
    rays["direction"][:, 3] = np.arange(len(d), dtype=np.int32).view(np.float32)  # pixel-id bits: not part of the lookup
    out = rnd.env_eval(dsc, R.to_device(rays, rnd.device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def lookup_error(got, ref):
    ref = np.abs(ref[:, :3])
    return float((np.abs(got[:, :3].astype(np.float64) - ref) / np.maximum(ref, ref.mean())).max())


@pytest.mark.parametrize("rotate", [0.0, 37.0])
@pytest.mark.parametrize("size", [(1, 1), (2, 1), (7, 5), (64, 32)], ids=lambda s: "%dx%d" % s)
def test_lookup_matches_float64(rnd, lit, size, rotate):
    dsc, _, _ = lit("open", None)
    d = lookup_directions()
    texels = env_ref.smooth_map(*size)
    scale = (1.5, 1.0, 0.5)
    rnd.set_environment(dsc, scale=scale, map=texels, rotate=rotate)
    got = eval_on_gpu(rnd, dsc, d)
    assert got.shape == (len(d), 4) and (got[:, 3] == 0).all() and np.isfinite(got).all()
    ref = env_ref.env_radiance(d, scale, texels, rotate)
    err = lookup_error(got, ref)
    print("lookup %dx%d rotate %g: max error %.3e (bound %.3e)" % (size + (rotate, err, LOOKUP_BOUND)))
    # the bound must tell the definition from its near misses: columns moved by
    # half a texel, and the column wrap replaced by a clamp (maps with columns to tell apart)
    if size[0] > 1:
        e_shift = lookup_error(got, env_ref.env_radiance(d, scale, texels, rotate, shift=0.5))
        e_clamp = lookup_error(got, env_ref.env_radiance(d, scale, texels, rotate, wrap=False))
        print("  against the half-texel shift %.3e, against the clamp %.3e" % (e_shift, e_clamp))
        assert e_shift > LOOKUP_BOUND and e_clamp > LOOKUP_BOUND
    assert err <= LOOKUP_BOUND


def test_lookup_constant_environment_and_none(rnd, lit):
    dsc, _, _ = lit("open", "const")
    d = lookup_directions()
    got = eval_on_gpu(rnd, dsc, d)
    want = np.broadcast_to(np.array(ENVS["const"]["scale"] + (0.0,), np.float32), got.shape)
    assert_bits_equal(got, np.ascontiguousarray(want), "constant environment: no arithmetic")
    rnd.clear_environment(dsc)
    assert (eval_on_gpu(rnd, dsc, d) == 0).all()


def test_set_environment_validates(rnd, lit):
    dsc, _, _ = lit("open", "const")
    d = lookup_directions()[:64]
    before = eval_on_gpu(rnd, dsc, d)
    good = env_ref.smooth_map(4, 2)
    bad_map = good.copy()
    bad_map[1, 2, 0] = -1.0
    nan_map = good.copy()
    nan_map[0, 0, 2] = np.nan
    for kw in (dict(scale=(1, -1, 1)), dict(scale=(1, float("inf"), 1)), dict(scale=(1, 1, float("nan"))),
               dict(rotate=float("nan")), dict(map=bad_map), dict(map=nan_map)):
        with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*set_environment"):
            rnd.set_environment(dsc, **kw)
    for shape in ((4, 4), (0, 4, 3), (4, 4, 4)):
        with pytest.raises(ValueError):
            rnd.set_environment(dsc, map=np.zeros(shape, np.float32))
    assert_bits_equal(eval_on_gpu(rnd, dsc, d), before, "a refused call leaves the environment as it was")


# ------------------------------------------------- fused kernel equals chain
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("schedule", [L.SCHED_SINGLE, L.SCHED_PAIRED])
@pytest.mark.parametrize("env", ["const", "map"])
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_render_equals_chain(rnd, lit, chain_ref, name, env, schedule, mode):
    ref = chain_ref(name, env, mode)
    dsc, cam, depth = lit(name, env)
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode,
                schedule=schedule)
    assert_state_equal(got, ref, "%s/%s/sched%d/mode%d" % (name, env, schedule, mode))
    # not vacuous: the environment lights at least one pixel the unlit scene leaves otherwise
    dsc, cam, depth = lit(name, None)
    unlit = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode,
                  schedule=schedule)
    assert (got[0].view(np.uint32) != unlit[0].view(np.uint32)).any(axis=1).sum() >= 1
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all() and (got[0][:, 3] == 0).all()


@pytest.mark.parametrize("quantized", [1, 2])
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_render_both_node_formats(rnd, lit, chain_ref, name, quantized):
    ref = chain_ref(name, "map")
    dsc, cam, depth = lit(name, "map")
    try:
        rnd.set_tuning(quantized=quantized)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["quantized"] == (1 if quantized == 1 else 0)
    assert_state_equal(got, ref, "%s quantized=%d" % (name, quantized))


@pytest.mark.parametrize("split,frames", [(((0, 2), (2, 4)), 6), (((0, 2), (2, 5)), 7)])
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_frames_split_across_calls_and_blocks(rnd, lit, chain_ref, name, split, frames):
    """Calls of (frame_begin, frames) with 3-frame blocks, so a pixel's state
    is handed from lane to lane between lit frames."""
    ref = chain_ref(name, "map", frames=frames)
    dsc, cam, depth = lit(name, "map")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    launches = 0
    for f0, nf in split:
        rnd.render_frames(dsc, cam, st, depth, ATT, nf, frame_begin=f0, frames_per_launch=3)
        launches += rnd.stats()["frames_per_block"] < nf
    assert launches >= 1  # at least one call ran several blocks per pixel
    assert_state_equal(state_np(st), ref, "%s split %r" % (name, split))


@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_two_stripes_one_after_the_other(rnd, lit, chain_ref, name):
    ref = chain_ref(name, "map")
    dsc, cam, depth = lit(name, "map")
    st = rnd.new_state(W, H, R.default_seeds(W * H))
    for k in range(2):
        rnd.render_frames(dsc, cam, st, depth, ATT, FRAMES, frame_begin=0, stripe_rows=8, stripe_index=k,
                          stripe_count=2)
    assert_state_equal(state_np(st), ref, "%s, 2 stripes of 8 rows" % name)


@pytest.mark.parametrize("cache,state", [(2, 0), (1, 2), (0, 2)], ids=["off", "always", "auto"])
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_render_primary_cache_modes(rnd, lit, chain_ref, name, cache, state):
    """A cached primary hit that is a miss is lit too: the lane rebuilds the
    ray from the record before it shades."""
    ref = chain_ref(name, "map")
    dsc, cam, depth = lit(name, "map")
    rnd.drop_caches()
    try:
        rnd.set_tuning(primary_cache=cache)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False)
        s = rnd.stats()
    finally:
        rnd.set_tuning()
    assert s["primary_cache"] == state
    assert_state_equal(got, ref, "%s primary_cache=%d" % (name, cache))


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_NOPRUNE])
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_lit_jittered_render_equals_chain(rnd, lit, chain_ref, name, mode):
    ref = chain_ref(name, "map", mode, jitter=True)
    dsc, cam, depth = lit(name, "map")
    got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=True, mode=mode)
    assert_state_equal(got, ref, "%s jittered, mode %d" % (name, mode))
    assert got[0].tobytes() != chain_ref(name, "map", mode)[0].tobytes()


# ----------------------------------------------------------- all-miss frame
@pytest.mark.parametrize("cache", [2, 1], ids=["traced", "cached"])
@pytest.mark.parametrize("env", ["const", "map"])
def test_all_miss_frame_is_the_background_plate(rnd, env, cache):
    """One triangle behind the camera, one frame: every pixel's sample is
    1 * L of its primary ray, and the history's first mean of it is L."""
    tri = np.array([[[-1, 0, 20], [1, 0, 20], [0, 1, 20]]], np.float32)
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    dsc = rnd.upload(S.SceneData.from_arrays(tri, np.zeros(1, np.int32), mats))
    cam = S.parse_camera(env_ref.OPEN_CAM)
    try:
        rnd.set_environment(dsc, **ENVS[env])
        plate = rnd.env_eval(dsc, rnd.generate_rays(cam, W, H))
        torch.cuda.synchronize()
        plate = plate.cpu().numpy()
        rnd.drop_caches()
        rnd.set_tuning(primary_cache=cache)
        seeds = R.default_seeds(W * H)
        hist, count, after = fused(rnd, dsc, cam, W, H, 4, ATT, 1, seeds, jitter=False)
        assert rnd.stats()["primary_cache"] == (2 if cache == 1 else 0)
    finally:
        rnd.set_tuning()
        dsc.close()
    assert_bits_equal(hist, plate, "hist")
    lit_px = (plate[:, :3] != 0).any(axis=1)
    assert lit_px.all() and (count == lit_px.astype(np.int32)).all()
    assert_bits_equal(after, seeds, "seeds: the lookup draws nothing")
    if env == "map":
        assert len(np.unique(plate[:, 0])) > W  # the plate varies over the image


# ------------------------------------------------------- no change when off
@pytest.mark.parametrize("name", ["open", "cbox"])
def test_zero_scale_gives_the_bits_of_no_environment(rnd, lit, name):
    dsc, cam, depth = lit(name, None)
    seeds = R.default_seeds(W * H)
    unlit = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False, frames_per_launch=3)
    for kw in (dict(scale=0.0), dict(scale=(0, 0, 0), map=env_ref.smooth_map(7, 5), rotate=37.0)):
        rnd.set_environment(dsc, **kw)
        got = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, seeds, jitter=False, frames_per_launch=3)
        assert_state_equal(got, unlit, "%s with a zero environment %r" % (name, sorted(kw)))
    if name == "open":  # no light and no environment: nothing is ever accumulated
        assert (unlit[0] == 0).all() and (unlit[1] == 0).all() and (unlit[2] != seeds).any()


def test_set_then_clear_gives_the_committed_golden(rnd):
    """C1 (tests/golden/image_c1_cbox.npz, the reference's own image): a scene
    whose environment was set and cleared renders the bits of one that never
    had any, and the primary-hit cache built before the environment was set is
    still read after it is cleared (it holds hits, not radiance)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "image_c1_cbox.npz"))
    w, h, depth, frames, att = (int(x) for x in g["meta"])
    dsc, cam = rnd.upload(scenes.cbox()), S.parse_camera(scenes.CBOX_CAM)
    try:
        rnd.drop_caches()
        rnd.render_frames(dsc, cam, rnd.new_state(w, h, g["seeds_in"]), depth, att, frames)
        assert rnd.stats()["primary_cache"] == 2  # built
        rnd.set_environment(dsc, **ENVS["map"])
        st = rnd.new_state(w, h, g["seeds_in"])
        rnd.render_frames(dsc, cam, st, depth, att, frames)
        assert rnd.stats()["primary_cache"] == 1  # read by the lit call
        assert st.hist.cpu().numpy().tobytes() != g["hist"].tobytes()
        rnd.clear_environment(dsc)
        st = rnd.new_state(w, h, g["seeds_in"])
        rnd.render_frames(dsc, cam, st, depth, att, frames)
        assert rnd.stats()["primary_cache"] == 1  # and by the call after the clear
        torch.cuda.synchronize()
        assert_bits_equal(st.count.cpu().numpy(), g["count"], "count")
        assert_bits_equal(st.seeds_np(), g["seeds"], "seeds")
        assert_bits_equal(st.hist.cpu().numpy(), g["hist"], "hist")
    finally:
        dsc.close()


# ------------------------------------------------------------ App and CLI
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_app_cli_and_two_ranks_render_the_configured_environment(tmp_path):
    from montecarlopathtracing_amd.__main__ import main
    from montecarlopathtracing_amd.app import App
    sky = env_ref.smooth_map(16, 8)
    rgba = np.zeros((8, 16, 4), np.float32)
    rgba[..., :3] = sky
    S.write_hdr(str(tmp_path / "sky.hdr"), rgba, flip=False)  # row 0 of the map is the file's first row
    quantized = S.read_hdr(str(tmp_path / "sky.hdr"))
    assert quantized.shape == sky.shape and np.abs(quantized - sky).max() < sky.max() / 128
    env_key = {"map": str(tmp_path / "sky.hdr"), "scale": 0.5, "rotate": 37}
    path = tmp_path / "config.json"
    path.write_text(json.dumps(_entry(environment=env_key)))
    seeds = R.default_seeds(32 * 32)
    app_dir, cli_dir, dist_dir = tmp_path / "app", tmp_path / "cli", tmp_path / "dist"
    for d in (app_dir, cli_dir, dist_dir):
        d.mkdir()
    # the config key: App renders what Renderer.set_environment of the decoded file renders
    app = App(str(path), seeds=seeds, out_dir=str(app_dir))
    out = app.run()
    got = state_np(app.state)
    app.renderer.set_environment(app.scene, scale=0.5, map=quantized, rotate=37.0)
    want = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, seeds, jitter=False)
    assert_state_equal(got, want, 'App with "environment"')
    app.renderer.clear_environment(app.scene)
    unlit = fused(app.renderer, app.scene, app.camera, 32, 32, 4, 3, 4, seeds, jitter=False)
    assert got[0].tobytes() != unlit[0].tobytes()
    # <objname>.hdr through the new reader: the downloaded image, flipped as the writer flips, within RGBE quantisation
    img = app.image()[::-1, :, :3]
    dec = S.read_hdr(out)
    mx = img.max(axis=2)
    step = np.ldexp(1.0, np.frexp(mx.astype(np.float64))[1] - 8)[..., None]
    diff = img.astype(np.float64) - dec
    coded = mx >= np.float32(1e-32)
    assert (dec[~coded] == 0).all() and (diff[coded] >= 0).all() and (diff[coded] < np.broadcast_to(step, diff.shape)[coded]).all()
    # --env overrides the entry's environment
    assert main([str(path), "--out", str(cli_dir), "--env", "0.25,0.5,1"]) == 0
    const = App(str(path), out_dir=str(tmp_path), environment={"color": [0.25, 0.5, 1]})  # the CLI's default seeds
    const.run()
    assert (cli_dir / "cbox.obj.hdr").read_bytes() == (tmp_path / "cbox.obj.hdr").read_bytes()
    assert (cli_dir / "cbox.obj.hdr").read_bytes() != open(out, "rb").read()
    # two ranks sharing the GPU over gloo: every rank lights its own scene (`seeds` are the CLI's default ones)
    env = dict(os.environ, MCPT_DIST_SHARED_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_port()),
                        "-m", "montecarlopathtracing_amd", str(path), "--out", str(dist_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (dist_dir / "cbox.obj.hdr").read_bytes() == (app_dir / "cbox.obj.hdr").read_bytes()


# -------------------------------------------------------------- debug build
def _digest(state):
    h = hashlib.sha256()
    for a in state:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_debug_build_texel_bounds_checks_clean(rnd, lit):
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "env_debug_check.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    modes = {c["mode"]: c for c in lines[1:]}
    assert sorted(modes) == [L.MODE_EXACT, L.MODE_NOPRUNE]
    dsc, cam, depth = lit("open", "map")
    for mode, c in modes.items():
        assert c["violations"] == 0, c
        mine = fused(rnd, dsc, cam, W, H, depth, ATT, FRAMES, R.default_seeds(W * H), jitter=False, mode=mode)
        assert c["digest"] == _digest(mine), mode
