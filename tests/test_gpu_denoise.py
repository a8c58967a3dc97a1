"""The denoise post-pass on the GPU (mcpt_denoise: k_denoise_prepare,
k_denoise_iter) against its float64 restatement (tests/denoise_ref.py) on
synthetic first hits, its exact-bit guarantees, its argument errors, that a
render around it is undisturbed, that it denoises, and the App surface."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from montecarlopathtracing_amd import _lib as L  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402
from montecarlopathtracing_amd import scene as S  # noqa: E402

from . import denoise_ref as D  # noqa: E402
from . import scenes  # noqa: E402
from .test_gpu_jitter import assert_bits_equal, assert_state_equal, state_np  # noqa: E402

# Largest |gpu - ref| / max(|ref|, mean |ref|) over the filtered pixels of every
# case of test_numerics_against_float64_reference, measured on an MI355X:
# 5.475e-7 (37x29, 5 iterations, sigma_color 1; 2.8e-7 to 5.2e-7 on the other
# shapes).  fp32 exp and sum order give a few ulp per tap over 25 taps and 5
# iterations; the bound is 8x the measurement.  The reference without its four
# corner taps is 5.0e-3 or more away on every two-dimensional shape.
MEASURED_REL_ERR = 5.475e-7
TOL = 8 * MEASURED_REL_ERR
SHAPES = [(37, 29), (1, 1), (1, 70), (70, 1), (16, 16), (17, 33)]
SYN = dict(iterations=5, sigma_normal=0.5, sigma_plane=0.05)


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module")
def syn_scene(rnd):
    """The scene the synthetic hits belong to: the material table and the root box."""
    verts, idx = D.synthetic_verts()
    data = S.SceneData.from_arrays(verts, idx, D.synthetic_mats())
    assert abs(D.scene_diagonal(data.nodes) - D.SYN_DIAG) < 1e-12
    dsc = rnd.upload(data)
    yield dsc
    dsc.close()


@pytest.fixture(scope="module")
def cbox_scene(rnd):
    dsc = rnd.upload(scenes.cbox())
    yield dsc
    dsc.close()


def load_state(rnd, w, h, hist, count):
    st = rnd.new_state(w, h)
    st.hist.copy_(torch.from_numpy(np.ascontiguousarray(hist, np.float32)))
    st.count.copy_(torch.from_numpy(np.ascontiguousarray(count, np.int32)))
    return st


def gpu_denoise(rnd, dsc, w, h, hits, hist, count, **params):
    st = load_state(rnd, w, h, hist, count)
    out = rnd.denoise(dsc, R.to_device(hits, rnd.device), st, **params)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


@pytest.fixture(scope="module")
def refs():
    """(w, h, sigma_color) -> (inputs, full reference, corner-dropped reference), computed once."""
    held = {}

    def get(w, h, sc):
        if (w, h, sc) not in held:
            case = D.synthetic_case(w, h)
            args = case + (D.synthetic_mats(), D.SYN_DIAG, w, h)
            held[(w, h, sc)] = (case, D.denoise_ref(*args, sigma_color=sc, **SYN),
                                D.denoise_ref(*args, sigma_color=sc, drop_corners=True, **SYN))
        return held[(w, h, sc)]
    return get


# ------------------------------------------------------------- 1: numerics
@pytest.mark.parametrize("sc", [0.0, 1.0])
@pytest.mark.parametrize("w,h", SHAPES)
def test_numerics_against_float64_reference(rnd, syn_scene, refs, w, h, sc):
    """37x29 with 5 iterations: the reach of 32 exceeds both sides, so taps
    leave the image on every edge; the one-pixel-wide shapes, one tile and a
    shape that is no multiple of the 64x4 tile.  The bound must also tell the
    reference from the one without its corner taps."""
    (hits, hist, count), ref, dropped = refs(w, h, sc)
    got, _ = gpu_denoise(rnd, syn_scene, w, h, hits, hist, count, sigma_color=sc, **SYN)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    err, err_dropped = D.rel_err(got, ref, filt), D.rel_err(got, dropped, filt)
    print("denoise %dx%d sigma_color %g: rel err %.3e, against the corner-dropped reference %.3e" % (
        w, h, sc, err, err_dropped))
    assert np.isfinite(got[filt]).all()
    assert err <= TOL, (err, TOL)
    if min(w, h) >= 3:  # a corner tap needs two dimensions
        assert err_dropped > TOL, (err_dropped, TOL)
    assert (got[filt, 3] == 0).all()
    assert got[~filt].tobytes() == hist[~filt].tobytes(), "pass-through pixels"


# ----------------------------------------------------------- 2: exact bits
def test_exact_bits(rnd, syn_scene):
    w, h = 37, 29
    hits, hist, count = D.synthetic_case(w, h)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    st = load_state(rnd, w, h, hist, count)
    d_hits = R.to_device(hits, rnd.device)
    before = state_np(st)
    a = rnd.denoise(syn_scene, d_hits, st, sigma_color=1.0, **SYN).cpu().numpy()
    # another image in between: the context's scratch holds nothing the next call relies on
    gpu_denoise(rnd, syn_scene, 70, 1, *D.synthetic_case(70, 1), sigma_color=0.0, **SYN)
    b = rnd.denoise(syn_scene, d_hits, st, sigma_color=1.0, **SYN).cpu().numpy()
    zero = rnd.denoise(syn_scene, d_hits, st, iterations=0).cpu().numpy()
    assert_bits_equal(a, b, "two calls")
    assert_bits_equal(a[~filt], hist[~filt], "pass-through pixels")
    assert (a[filt, :3] != hist[filt, :3]).any()
    assert_bits_equal(zero, hist, "iterations = 0")
    assert_state_equal(state_np(st), before, "state after denoise")
    assert_bits_equal(before[0], hist, "hist as loaded")


# ------------------------------------------------------ 3: all counts zero
@pytest.mark.parametrize("sc", [0.0, 1.0])
def test_all_counts_zero(rnd, syn_scene, sc):
    w, h = 37, 29
    hits, hist, count = D.synthetic_case(w, h, all_zero=True)
    got, _ = gpu_denoise(rnd, syn_scene, w, h, hits, hist, count, sigma_color=sc, **SYN)
    assert np.isfinite(got).all() and (got == 0).all()


# ------------------------------------------------------ 4: argument errors
def test_argument_errors(rnd, syn_scene):
    w, h = 16, 16
    hits, hist, count = D.synthetic_case(w, h)
    st = load_state(rnd, w, h, hist, count)
    d_hits = R.to_device(hits, rnd.device)
    out = torch.full((w * h, 4), -7.0, dtype=torch.float32, device=rnd.device)
    good = dict(ctx=rnd.ctx, scene=syn_scene.handle, hits=L.ptr(d_hits), hist=L.ptr(st.hist), count=L.ptr(st.count),
                width=w, height=h, iterations=3, sigma_normal=0.5, sigma_plane=0.05, sigma_color=0.0,
                out=L.ptr(out))

    def call(**change):
        a = dict(good, **change)
        p = L.DenoiseParams(a["iterations"], a["sigma_normal"], a["sigma_plane"], a["sigma_color"])
        params = None if change.get("params_null") else ctypes.byref(p)
        return L.lib().mcpt_denoise(a["ctx"], a["scene"], a["hits"], a["hist"], a["count"], a["width"], a["height"],
                                    params, a["out"], None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(scene=None), dict(hits=None), dict(hist=None), dict(count=None), dict(out=None),
           dict(params_null=True), dict(width=0), dict(width=-3), dict(height=0), dict(height=-1),
           dict(iterations=-1), dict(iterations=9),
           dict(sigma_normal=0.0), dict(sigma_normal=-0.5), dict(sigma_normal=nan), dict(sigma_normal=inf),
           dict(sigma_plane=0.0), dict(sigma_plane=-0.01), dict(sigma_plane=nan), dict(sigma_plane=inf),
           dict(sigma_color=-1.0), dict(sigma_color=nan), dict(sigma_color=inf),
           dict(out=L.ptr(st.hist))]
    for change in bad:
        assert call(**change) == -1, change  # MCPT_ERR_ARG
        assert L.lib().mcpt_last_error().decode().startswith("denoise:"), change
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()  # nothing was launched
    assert_bits_equal(st.hist.cpu().numpy(), hist, "hist after the refused calls")
    # the wrapper raises, and the edge values are accepted
    with pytest.raises(L.MCPTError, match=r"mcpt error -1\b.*iterations"):
        rnd.denoise(syn_scene, d_hits, st, iterations=9)
    with pytest.raises(L.MCPTError, match="hits"):
        rnd.denoise(syn_scene, d_hits[:-48], st)
    assert call(iterations=8) == 0 and call(iterations=0) == 0 and call(sigma_color=0.0) == 0
    torch.cuda.synchronize()


# --------------------------------------------- 5: a render is undisturbed
@pytest.mark.parametrize("jitter", [False, True])
def test_render_resumed_after_denoise_is_unaffected(rnd, cbox_scene, jitter):
    w, h, depth, att = 48, 40, 4, 8
    cam = S.parse_camera(scenes.CBOX_CAM)
    seeds = R.default_seeds(w * h)
    rnd.drop_caches()
    whole = rnd.new_state(w, h, seeds)
    rnd.render_frames(cbox_scene, cam, whole, depth, att, 6, jitter=jitter)
    want = state_np(whole)
    rnd.drop_caches()
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(cbox_scene, cam, st, depth, att, 3, jitter=jitter)
    first = rnd.stats()["primary_cache"]
    hits = rnd.first_hits(cbox_scene, cam, w, h)
    mid = state_np(st)
    den = rnd.denoise(cbox_scene, hits, st)
    assert_state_equal(state_np(st), mid, "state across the denoise")
    rnd.render_frames(cbox_scene, cam, st, depth, att, 3, jitter=jitter)
    # unjittered: the first call built the primary-hit cache and the second still reads it
    assert (first, rnd.stats()["primary_cache"]) == ((0, 0) if jitter else (2, 1))
    assert st.frames_done == 6
    assert_state_equal(state_np(st), want, "3 frames, denoise, 3 frames")
    assert (want[1] > 0).any() and np.isfinite(den.cpu().numpy()).all()


# ---------------------------------------------------------- 6: it denoises
def test_denoised_render_is_closer_to_the_converged_image(rnd, cbox_scene):
    """cbox 64x64, depth 8: 8 frames denoised against 4096 frames from other
    seeds, RMSE over the filtered pixels.  The float64 filter on the CPU
    oracle's render gave 0.032 against 0.084 raw."""
    w = h = 64
    depth = 8
    cam = S.parse_camera(scenes.CBOX_CAM)
    seeds = R.default_seeds(w * h)
    ref_st = rnd.new_state(w, h, seeds ^ np.uint32(0xA5A5A5A5))
    rnd.render_frames(cbox_scene, cam, ref_st, depth, 4096, 4096)
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(cbox_scene, cam, st, depth, 8, 8)
    hits = rnd.first_hits(cbox_scene, cam, w, h)
    den = rnd.denoise(cbox_scene, hits, st, iterations=3, sigma_normal=0.5, sigma_plane=0.01, sigma_color=0.0)
    torch.cuda.synchronize()
    filt = D.filtered_mask(R.records(hits, L.HIT), scenes.cbox().mats)
    ref = ref_st.hist.cpu().numpy()[filt, :3].astype(np.float64)
    raw = st.hist.cpu().numpy()[filt, :3].astype(np.float64)
    got = den.cpu().numpy()[filt, :3].astype(np.float64)
    rmse_raw, rmse_den = np.sqrt(((raw - ref) ** 2).mean()), np.sqrt(((got - ref) ** 2).mean())
    print("cbox 64x64, 8 frames: RMSE raw %.4f, denoised %.4f, ratio %.3f (%d filtered pixels, %.1f %% count 0)" % (
        rmse_raw, rmse_den, rmse_den / rmse_raw, filt.sum(), 100.0 * (st.count.cpu().numpy()[filt] == 0).mean()))
    assert filt.sum() > w * h // 2 and np.isfinite(got).all()
    assert rmse_den < rmse_raw


# ------------------------------------------------------------------ 7: App
def _read_hdr(path):
    """A Radiance .hdr as stbi_write_hdr writes it (new-style RLE scanlines for
    widths 8..32767) -> (H, W, 3) float64, file order (top row first)."""
    data = open(path, "rb").read()
    head, _, rest = data.partition(b"\n\n")
    assert head.startswith(b"#?RADIANCE")
    dims, _, body = rest.partition(b"\n")
    _, hh, _, ww = dims.split()
    h, w = int(hh), int(ww)
    assert 8 <= w < 32768
    b = np.frombuffer(body, np.uint8)
    rgbe = np.zeros((h, w, 4), np.uint8)
    i = 0
    for y in range(h):
        assert b[i] == 2 and b[i + 1] == 2 and (int(b[i + 2]) << 8 | int(b[i + 3])) == w
        i += 4
        for ch in range(4):
            x = 0
            while x < w:
                n = int(b[i])
                if n > 128:
                    rgbe[y, x:x + n - 128, ch] = b[i + 1]
                    x, i = x + n - 128, i + 2
                else:
                    rgbe[y, x:x + n, ch] = b[i + 1:i + 1 + n]
                    x, i = x + n, i + 1 + n
    assert i == len(b)
    scale = np.where(rgbe[..., 3] > 0, np.ldexp(1.0, rgbe[..., 3].astype(np.int32) - 136), 0.0)
    return rgbe[..., :3].astype(np.float64) * scale[..., None]


def test_app_writes_both_files(tmp_path):
    from montecarlopathtracing_amd.app import App
    seeds = R.default_seeds(256 * 256)
    plain_dir, den_dir = tmp_path / "plain", tmp_path / "den"
    plain_dir.mkdir()
    den_dir.mkdir()
    plain = App(scenes.CFG, configid=2, seeds=seeds, out_dir=str(plain_dir))  # C1: cbox 256x256, 16 spp
    raw_path = plain.run()
    assert not os.path.exists(App.denoised_path(raw_path))
    app = App(scenes.CFG, configid=2, seeds=seeds, out_dir=str(den_dir), denoise=True)
    path = app.run()
    den_path = os.path.join(str(den_dir), "cbox.obj_denoised.hdr")
    assert os.path.basename(path) == "cbox.obj.hdr" and os.path.exists(den_path)
    assert open(path, "rb").read() == open(raw_path, "rb").read()
    assert_state_equal(state_np(app.state), state_np(plain.state), "state with and without denoise")
    den = app.denoised()
    assert den.shape == (256, 256, 4) and np.isfinite(den).all()
    assert open(den_path, "rb").read() == S.encode_hdr(den, flip=True)
    assert open(den_path, "rb").read() != open(path, "rb").read()
    # the file decodes to the image: RGBE keeps 8 bits of a pixel's largest channel, truncated
    dec = _read_hdr(den_path)[::-1]
    ulp = np.ldexp(1.0, np.frexp(den[..., :3].max(axis=2).astype(np.float64))[1] - 8)
    assert (np.abs(dec - den[..., :3]) <= ulp[..., None]).all()
    assert dec.max() > 0


def test_dist_cli_denoise_equals_app(tmp_path):
    """The multi-GPU CLI with --denoise: rank 0 runs the same call on the reduced
    image, so both files are byte-identical to App's.  Two ranks on the box's
    one GPU over gloo (MCPT_DIST_SHARED_GPU=1), as tests/test_gpu_dist.py."""
    import json
    import subprocess
    import sys

    from montecarlopathtracing_amd.app import App

    from .test_gpu_dist import ROOT, _port
    from .test_jitter_cpu import _entry
    cfg = _entry(width=96, height=64, maxdepth=5, attempt=7)
    cfg["config"][0]["camera"]["resolution"] = [96, 64]
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    dist_dir, app_dir = tmp_path / "dist", tmp_path / "app"
    dist_dir.mkdir()
    app_dir.mkdir()
    env = dict(os.environ, MCPT_DIST_SHARED_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_port()),
                        "-m", "montecarlopathtracing_amd", str(path), "--out", str(dist_dir), "--denoise"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    App(str(path), out_dir=str(app_dir), denoise=True).run()
    for name in ("cbox.obj.hdr", "cbox.obj_denoised.hdr"):
        assert (dist_dir / name).read_bytes() == (app_dir / name).read_bytes(), name
    assert (app_dir / "cbox.obj.hdr").read_bytes() != (app_dir / "cbox.obj_denoised.hdr").read_bytes()
