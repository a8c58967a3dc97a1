"""The thin-lens camera (opt-in depth of field), the parts that need no GPU:
the config key and command line with every refusal, the float64 restatement's
own properties (tests/lens_ref.py), the autofocus arithmetic, and the geometry
the GPU test of the visible effect relies on."""
import math
import os

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C
from montecarlopathtracing_amd import scene as S

from . import lens_ref as LR
from .test_jitter_cpu import ZERO_DRAW_SEEDS, _entry, jitter_draws, lcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ 1: the surface
def test_abi_mirror_has_the_lens_struct_and_entry_points():
    import ctypes
    assert ctypes.sizeof(L.Lens) == 16
    assert [f[0] for f in L.Lens._fields_] == ["radius", "focus_distance", "pad"]
    rf, rl = L.SIGNATURES["mcpt_render_frames"][1], L.SIGNATURES["mcpt_render_frames_lens"][1]
    assert rl == rf[:3] + [L._P] + rf[3:]
    gj, gl = L.SIGNATURES["mcpt_generate_rays_jittered"][1], L.SIGNATURES["mcpt_generate_rays_lens"][1]
    assert gl == gj[:2] + [L._P] + gj[2:]
    hdr = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in hdr and L.ABI_VERSION == 5
    for name in ("typedef struct mcpt_lens", "mcpt_render_frames_lens(", "mcpt_generate_rays_lens("):
        assert name in hdr


def test_config_reads_the_lens_key():
    assert C.Config(_entry()).LENS() is None
    assert C.Config(_entry(lens={"aperture": 2, "focus": 7.5})).LENS() == {
        "aperture": 2.0, "focus": 7.5, "focus_at": None}
    assert C.Config(_entry(lens={"aperture": 0.25, "focus_at": [3, 4]})).LENS() == {
        "aperture": 0.25, "focus": None, "focus_at": (3, 4)}
    # the committed config.json's entries are the reference's: none has a lens
    root = C.Config(os.path.join(ROOT, "config.json")).root
    for i in range(len(root["config"])):
        assert C.Config(root, configid=i).LENS() is None


@pytest.mark.parametrize("bad", [
    True, 3, [1, 2], "wide",                                   # not an object
    {}, {"focus": 2}, {"focus_at": [1, 1]},                    # no aperture
    {"aperture": 1},                                           # neither focus nor focus_at
    {"aperture": 1, "focus": 2, "focus_at": [1, 1]},           # both
    {"aperture": 1, "focus": 2, "fstop": 8},                   # an unknown key
    {"aperture": "1", "focus": 2}, {"aperture": True, "focus": 2}, {"aperture": None, "focus": 2},
    {"aperture": 1, "focus": "2"}, {"aperture": 1, "focus": [2]},
    {"aperture": 0, "focus": 2}, {"aperture": -1, "focus": 2}, {"aperture": 1, "focus": 0},
    {"aperture": 1, "focus": -3}, {"aperture": float("inf"), "focus": 2}, {"aperture": 1, "focus": float("nan")},
    {"aperture": 1, "focus_at": [1]}, {"aperture": 1, "focus_at": [1, 2, 3]}, {"aperture": 1, "focus_at": "1,2"},
    {"aperture": 1, "focus_at": [1.5, 2]}, {"aperture": 1, "focus_at": [-1, 2]}, {"aperture": 1, "focus_at": [True, 2]},
], ids=repr)
def test_config_refuses_a_bad_lens_key(bad):
    with pytest.raises(ValueError, match="lens"):
        C.Config(_entry(lens=bad))


def test_app_takes_the_lens_and_switches_jitter_on():
    from montecarlopathtracing_amd.app import App
    plain = App(C.Config(_entry()))
    assert plain.lens_spec is None and plain.jitter is False
    a = App(C.Config(_entry(lens={"aperture": 5, "focus": 900})))
    assert a.lens_spec["aperture"] == 5.0 and a.jitter is True
    b = App(C.Config(_entry()), lens=(5, 900))
    assert b.lens_spec == a.lens_spec and b.jitter is True
    c = App(C.Config(_entry(lens={"aperture": 5, "focus": 900})), lens={"aperture": 1, "focus_at": [2, 3]})
    assert c.lens_spec == {"aperture": 1.0, "focus": None, "focus_at": (2, 3)}  # the argument wins
    with pytest.raises(ValueError, match="jitter"):
        App(C.Config(_entry()), lens=(5, 900), jitter=False)
    with pytest.raises(ValueError, match="lens"):
        App(C.Config(_entry()), lens=(0, 900))


def test_command_line_parses_the_lens():
    from montecarlopathtracing_amd.__main__ import cli_lens, parser
    p = parser()
    assert cli_lens(p.parse_args(["cfg.json"])) is None
    assert cli_lens(p.parse_args(["cfg.json", "--aperture", "2.5", "--focus", "10"])) == {"aperture": 2.5, "focus": 10.0}
    assert cli_lens(p.parse_args(["--aperture", "2.5", "--focus-at", "12,7"])) == {"aperture": 2.5, "focus_at": [12, 7]}
    for bad in (["--aperture", "2"], ["--focus", "3"], ["--focus-at", "1,2"],
                ["--aperture", "2", "--focus", "3", "--focus-at", "1,2"],
                ["--aperture", "2", "--focus-at", "1"], ["--aperture", "2", "--focus-at", "a,b"]):
        with pytest.raises(ValueError):
            cli_lens(p.parse_args(bad))
    # what passes the command line still has to pass the key's checks
    with pytest.raises(ValueError, match="lens"):
        C.parse_lens(cli_lens(p.parse_args(["--aperture", "-2", "--focus", "3"])))
    assert "--aperture" in p.format_help() and "jitter" in p.format_help()


def test_renderer_refuses_a_lens_without_jitter_before_any_gpu_call():
    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer.__new__(R.Renderer)  # no context: the refusal comes first
    with pytest.raises(ValueError, match="jitter"):
        rnd.render_frames(None, None, None, 1, 1, 1, jitter=False, lens=(1.0, 2.0))
    with pytest.raises(ValueError, match="lens"):
        rnd.render_frames(None, None, None, 1, 1, 1, lens=(1.0,))


# --------------------------------------------------- 2: the restatement itself
def test_draws_are_the_jitters_then_two_more():
    seeds = (np.arange(4096, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5EED)
    jx, jy, r1, r2, after = LR.lens_draws(seeds)
    wx, wy, s2 = jitter_draws(seeds)
    assert (jx == wx).all() and (jy == wy).all()
    s3 = lcg(s2)
    assert (after == lcg(s3)).all()
    assert (r1 == ((s3 >> 16) & 0x7FFF)).all() and (r2 == ((after >> 16) & 0x7FFF)).all()
    assert 0 <= r1.min() and r1.max() < 32768 and 0 <= r2.min() and r2.max() < 32768
    # the planted seeds: zero offsets, and then some lens point (their chain goes on)
    z = LR.lens_draws(np.array(ZERO_DRAW_SEEDS, np.uint32))
    assert (z[0] == 0).all() and (z[1] == 0).all()


def _cam(camjson, ortho=False, scaled=False):
    cam = S.parse_camera(camjson).copy()
    if ortho:
        cam["camera_type"] = 1
        cam["arg"] = np.float32(9.5)
    if scaled:  # horizontal and up need not be unit vectors: generateRay scales them, the lens must not
        cam["horizontal"] *= np.float32(1.5)
        cam["up"] *= np.float32(0.75)
    return cam


@pytest.mark.parametrize("ortho", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_all_lens_rays_of_a_sample_meet_on_the_focus_plane(ortho, scaled):
    from .scenes import MIS_CAM
    cam = _cam(MIS_CAM, ortho, scaled)
    w, h, radius, focus = 37, 21, 0.4, 13.0
    n = w * h
    rng = np.random.default_rng(7)
    sx, sy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    o, d = LR.camera_rays(cam, w, h, sx, sy)
    ch = LR.unit(cam[0]["direction"])
    P0 = None
    for _ in range(8):
        a, b = LR.disk_sample(rng.integers(0, 32768, n), rng.integers(0, 32768, n))
        o2, d2, P = LR.lens_ray(cam, o, d, a, b, radius, focus)
        # the ray from o' along d' passes through P, which lies on the focus plane of the pinhole origin
        t = ((P - o2) * d2).sum(axis=1, keepdims=True)
        assert np.abs(o2 + t * d2 - P).max() < 1e-12 * focus
        assert np.abs(((P - o) * ch).sum(axis=1) - focus).max() < 1e-12 * focus
        assert np.abs((d2 * d2).sum(axis=1) - 1).max() < 1e-14
        # o' lies on the lens: in the plane through o across the view axis (as far as the record's float32
        # axes are orthogonal: a few 2^-24), within the radius
        assert np.abs(((o2 - o) * ch).sum(axis=1)).max() < radius * 1e-6
        assert np.sqrt(((o2 - o) ** 2).sum(axis=1)).max() <= radius * (1 + 1e-12)
        if P0 is not None:
            assert np.abs(P - P0).max() == 0  # P belongs to the sample, not to the lens point
        P0 = P


def test_lens_points_are_uniform_over_the_disk():
    """A stratified subset of the 2^30 (r1, r2) pairs: every 8th r1 with every
    8th r2, 2^24 points.  Uniform over the disk: the fraction within radius q
    is q^2, every one of 16 sectors holds a 16th, and the mean is the centre."""
    r1, r2 = np.meshgrid(np.arange(0, 32768, 8), np.arange(0, 32768, 8), indexing="ij")
    a, b = LR.disk_sample(r1.ravel(), r2.ravel())
    rr = a * a + b * b
    assert rr.max() < 1.0
    n = len(a)
    for q in (0.1, 0.25, 0.5, 0.75, 0.9):
        assert abs((rr < q * q).sum() / n - q * q) < 1e-3
    sector = np.floor((np.arctan2(b, a) % (2 * np.pi)) / (2 * np.pi / 16)).astype(int)
    # rho = 0 (r1 = 0) sits at the centre for every angle: one 4096th of the points, all in sector 0
    counts = np.bincount(sector, minlength=16) / n
    assert np.abs(counts - 1 / 16).max() < 1e-3
    assert abs(a.mean()) < 1e-3 and abs(b.mean()) < 1e-3
    # jointly: the 4 x 4 cells of (radius^2, angle) are equally full
    cell = np.minimum((rr * 4).astype(int), 3) * 4 + sector // 4
    assert np.abs(np.bincount(cell, minlength=16) / n - 1 / 16).max() < 1e-3


def test_a_vanishing_lens_is_the_pinhole():
    from .scenes import CBOX_CAM
    cam = _cam(CBOX_CAM)
    w, h, focus = 37, 21, 900.0
    seeds = (np.arange(w * h, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0xBEEF)
    o0, d0, _ = LR.lens_rays(cam, w, h, seeds, 0.0, focus)
    jx, jy, _ = jitter_draws(seeds)
    idx, idy = (np.arange(w * h) % w).astype(np.float32), (np.arange(w * h) // w).astype(np.float32)
    op, dp = LR.camera_rays(cam, w, h, (idx + jx).astype(np.float64), (idy + jy).astype(np.float64))
    assert np.abs(o0 - op).max() == 0 and np.abs(d0 - dp).max() < 1e-15
    last = None
    for radius in (1.0, 1e-2, 1e-4, 1e-6):
        o, d, _ = LR.lens_rays(cam, w, h, seeds, radius, focus)
        err = max(np.abs(o - op).max(), np.abs(d - dp).max() * focus)
        assert err <= radius * (1 + 1e-9)  # the lens point moves by at most R, the direction by at most R / F
        assert last is None or err < last * 0.011
        last = err


def test_each_mutant_is_another_function():
    from .scenes import MIS_CAM
    cam = _cam(MIS_CAM, scaled=True)
    w, h = 37, 21
    seeds = (np.arange(w * h, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0xF00D)
    o, d, _ = LR.lens_rays(cam, w, h, seeds, 0.4, 13.0)
    for m in LR.MUTANTS:
        om, dm, _ = LR.lens_rays(cam, w, h, seeds, 0.4, 13.0, mutant=m)
        assert LR.ray_error(om, dm, o, d) > 1e-3, m


# ------------------------------------------------------------- 3: autofocus
def test_autofocus_arithmetic_on_a_hand_made_hit():
    from montecarlopathtracing_amd.render import focus_from_hit
    # the camera looks down +z; a ray 3-4-5 off the axis hits at t = 10: 8 along the axis
    assert focus_from_hit(10.0, [0.6, 0.0, 0.8], [0, 0, 1]) == pytest.approx(8.0, rel=1e-15)
    # the camera's direction need not be unit, nor 3 long (the record's float4)
    assert focus_from_hit(10.0, [0.6, 0.0, 0.8, 123.0], [0, 0, 5, 0]) == pytest.approx(8.0, rel=1e-15)
    # on the axis F = t; and the restatement agrees: a point at focus F sits at t = F / dot(d, c^)
    assert focus_from_hit(7.25, [0, 0, 1], [0, 0, 1]) == 7.25
    d = LR.unit(np.array([0.3, -0.2, 0.9]))
    c = LR.unit(np.array([0.1, 0.0, 1.0]))
    assert focus_from_hit(12.0 / float(d @ c), d, c * 3) == pytest.approx(12.0, rel=1e-14)


# ------------------------------------ the visible-effect test's geometry (GPU test 5)
def test_edge_geometry_leaves_out_at_most_two_percent_and_shows_the_blur():
    """What tests/test_gpu_lens.py asserts of the GPU's counts holds for the
    prediction itself: few pixels near the rectangle's boundary, a sharp edge
    at F, a blur of the disk's width at 2 F."""
    from montecarlopathtracing_amd import render as R
    cam = S.parse_camera(LR.EDGE_CAM)
    w, h, frames = LR.EDGE_W, LR.EDGE_H, LR.EDGE_FRAMES
    seeds = R.default_seeds(w * h)
    for depth in (LR.EDGE_F, 2 * LR.EDGE_F):
        count, near, after = LR.edge_predict(cam, seeds, depth)
        assert near.sum() <= 0.02 * w * h
        partial = ((count > 0) & (count < frames)).reshape(h, w).sum(axis=1)
        if depth == LR.EDGE_F:
            assert partial.max() <= 2 and partial.max() >= 1  # the edge falls inside a pixel
        else:
            diameter = LR.edge_blur_diameter_px(depth)
            assert diameter > 3.5
            assert partial.min() >= diameter - 2
        lit = count.reshape(h, w)
        assert (lit[:, :8] == frames).all() or (lit[:, -8:] == frames).all()   # one side is the light
        assert (lit[:, :8] == 0).all() or (lit[:, -8:] == 0).all()             # the other is not
    # sixteen frames of four draws
    s = seeds
    for _ in range(4 * frames):
        s = lcg(s)
    assert (after == s).all()
    assert math.isclose(LR.edge_blur_diameter_px(LR.EDGE_F), 0.0)
