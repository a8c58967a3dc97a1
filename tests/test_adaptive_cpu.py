"""Adaptive sampling without a GPU: the queue and plan arithmetic of a
tile-subset launch walked on the CPU (tests/native/tile_subset_check.cpp), the
ABI mirror, the "adaptive" config key, the command line, the driver's refusals
before any C call, and the selection policy against tests/adaptive_ref.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import adaptive as AD
from montecarlopathtracing_amd import config as C

from . import adaptive_ref as AR
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "native", "tile_subset_check.cpp")


# ---------------------------------------------------- C1: the subset's queues and plan
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_tile_subset_queue_protocol(tmp_path, flags):
    """Every image up to 3 x 3 tiles, every non-empty subset, 1 / 2 / 8 queues, spread 0 / 1, 1-3 blocks: each
    (pixel of an active tile, block) exactly once, nothing else, a pixel's blocks in one queue in order, 64 * active
    items; and the plan of a subset: the grid bound, blocks of at least one frame, 0 = the plan of before."""
    exe = str(tmp_path / "tile_subset_check")  # the two headers alone: no HIP, no library
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, CHECK, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    assert out.stderr == ""  # no sanitizer report


# ---------------------------------------------------- C2: the ABI mirror
def test_tile_set_mirror_and_signatures():
    assert ctypes.sizeof(L.TileSet) == 16
    assert [(n, getattr(L.TileSet, n).offset) for n, _ in L.TileSet._fields_] == [("mask", 0), ("n_tiles", 8), ("pad", 12)]
    assert L.ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in header and "typedef struct mcpt_tile_set {" in header
    for name, n_args in (("mcpt_render_frames_tiles", 11), ("mcpt_tile_error", 10), ("mcpt_merge_halves", 9)):
        assert "int %s(" % name in header
        assert len(L.SIGNATURES[name][1]) == n_args and L.SIGNATURES[name][0] is ctypes.c_int32
    assert L.SIGNATURES["mcpt_tile_error"][1][7] is ctypes.c_float  # floor travels as a float


# ---------------------------------------------------- C2: the config key
def test_adaptive_config_key():
    assert C.Config(_entry()).ADAPTIVE() is None and C.Config(_entry()).UNBIASED() is False
    c = C.Config(_entry(adaptive=0.05))
    assert c.ADAPTIVE() == {"threshold": 0.05, "min_frames": 16, "batch": 8, "floor": 1e-4, "dilate": True, "map": False}
    assert c.UNBIASED() is True and c.unbiased_key is False  # adaptive sampling switches the counted history on
    c = C.Config(_entry(adaptive={"threshold": 1, "min_frames": 4, "batch": 2, "floor": 0.5, "dilate": False, "map": True}))
    assert c.ADAPTIVE() == {"threshold": 1.0, "min_frames": 4, "batch": 2, "floor": 0.5, "dilate": False, "map": True}
    assert C.Config(_entry(adaptive=0.1, unbiased=True, roulette=3)).ROULETTE() == 3
    bad = [0, -0.5, float("inf"), float("nan"), "0.1", True, False, None, [0.1], {}, {"min_frames": 4},
           {"threshold": 0}, {"threshold": "0.1"}, {"threshold": float("inf")}, {"threshold": True},
           {"threshold": 0.1, "min_frames": 3}, {"threshold": 0.1, "min_frames": 0}, {"threshold": 0.1, "min_frames": 4.0},
           {"threshold": 0.1, "min_frames": "4"}, {"threshold": 0.1, "batch": 5}, {"threshold": 0.1, "batch": -2},
           {"threshold": 0.1, "batch": True}, {"threshold": 0.1, "floor": 0}, {"threshold": 0.1, "floor": float("nan")},
           {"threshold": 0.1, "floor": "1e-4"}, {"threshold": 0.1, "dilate": 1}, {"threshold": 0.1, "map": "yes"},
           {"threshold": 0.1, "frames": 64}]
    for v in bad:
        with pytest.raises(ValueError, match="adaptive"):
            C.Config(_entry(adaptive=v))
    with pytest.raises(ValueError, match="unbiased"):
        C.Config(_entry(adaptive=0.1, unbiased=False))
    # and through the file reader, comments included
    cfg = C.Config(C.loads('{"configid": 0, "config": [%s]}' % json.dumps(_entry(adaptive=0.25)["config"][0])))
    assert cfg.ADAPTIVE()["threshold"] == 0.25


# ---------------------------------------------------- C2: the command line and App
def test_command_line_maps_to_the_app_arguments():
    from montecarlopathtracing_amd.__main__ import cli_adaptive, parser
    from montecarlopathtracing_amd.app import App
    p = parser()
    plain, keyed = C.Config(_entry()), C.Config(_entry(adaptive={"threshold": 0.5, "batch": 4}))
    assert cli_adaptive(p.parse_args(["cfg.json"]), plain) == (None, None)  # the entry's key decides
    spec, amap = cli_adaptive(p.parse_args(["cfg.json", "--adaptive"]), plain)
    assert spec == {"threshold": C.DEFAULT_ADAPTIVE_THRESHOLD} and amap is None
    a = p.parse_args(["--adaptive", "0.125", "cfg.json", "--adaptive-map"])
    assert a.config == "cfg.json" and cli_adaptive(a, plain) == ({"threshold": 0.125}, True)
    spec, _ = cli_adaptive(p.parse_args(["--adaptive", "0.125"]), keyed)  # the entry's other values stay
    assert spec["threshold"] == 0.125 and spec["batch"] == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--adaptive", "often"])
    assert "--adaptive" in p.format_help() and "--adaptive-map" in p.format_help()
    # as App takes them: --adaptive implies the counted history
    spec, amap = cli_adaptive(p.parse_args(["--adaptive", "--adaptive-map"]), plain)
    app = App(plain, adaptive=spec, adaptive_map=amap)
    assert app.unbiased is True and app.adaptive["threshold"] == C.DEFAULT_ADAPTIVE_THRESHOLD and app.adaptive["map"] is True
    assert app.adaptive_budget() == 4  # attempt 3: four frames
    app = App(C.Config(_entry(attempt=10)), adaptive=0.1, roulette=True, jitter=True)  # composes with the other opt-ins
    assert app.adaptive_budget() == 10 and app.roulette == 3 and app.jitter is True and app.unbiased is True
    app = App(keyed)
    assert app.adaptive["threshold"] == 0.5 and app.adaptive["map"] is False and app.unbiased is True
    assert App(keyed, adaptive=False).adaptive is None and App(keyed, adaptive=False).unbiased is False
    assert App(plain).adaptive is None and App(plain).unbiased is False
    for kw in (dict(adaptive=0.1, unbiased=False), dict(adaptive=0), dict(adaptive="0.1"), dict(adaptive_map=True)):
        with pytest.raises(ValueError, match="adaptive"):
            App(plain, **kw)
    assert App.samples_path("out/cbox.obj.hdr") == "out/cbox.obj_samples.hdr"


def test_distributed_paths_refuse_adaptive(tmp_path, monkeypatch):
    from montecarlopathtracing_amd import dist as D
    from montecarlopathtracing_amd.__main__ import main
    D.refuse_adaptive(None)
    D.refuse_adaptive(False)
    for v in (0.1, {"threshold": 0.1}, True):
        with pytest.raises(ValueError, match="adaptive sampling is not available on the distributed path"):
            D.refuse_adaptive(v)
    with pytest.raises(ValueError, match="distributed"):  # before the process group is asked anything
        D.render_distributed(None, None, None, 8, 8, 1, 1, 1, None, adaptive=0.1)
    monkeypatch.setenv("WORLD_SIZE", "2")
    keyed, plain = tmp_path / "keyed.json", tmp_path / "plain.json"
    keyed.write_text(json.dumps(_entry(adaptive=0.1)))
    plain.write_text(json.dumps(_entry()))
    for argv in ([str(keyed)], [str(plain), "--adaptive"], [str(plain), "--adaptive-map"]):
        with pytest.raises(ValueError, match="distributed"):
            main(argv)


# ---------------------------------------------------- C2: the driver's refusals
def test_driver_refuses_before_any_c_call():
    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer.__new__(R.Renderer)  # no context: the refusals come first

    class Fresh:
        width, height, frames_done = 16, 16, 0

    good = dict(frames=12, threshold=0.1, min_frames=4, batch=4, floor=1e-4)
    for kw in (dict(frames=7), dict(frames=0), dict(frames=12.0), dict(frames=True), dict(min_frames=3), dict(min_frames=0),
               dict(min_frames=14), dict(batch=5), dict(batch=0), dict(batch="4"), dict(threshold=-1e-9),
               dict(threshold=float("nan")), dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")),
               dict(floor=float("nan"))):
        a = dict(good, **kw)
        with pytest.raises(ValueError, match="render_adaptive"):
            rnd.render_adaptive(None, None, Fresh(), 4, a["frames"], a["threshold"], min_frames=a["min_frames"],
                                batch=a["batch"], floor=a["floor"])
    used = Fresh()
    used.frames_done = 2
    with pytest.raises(ValueError, match="fresh"):
        rnd.render_adaptive(None, None, used, 4, 12, 0.1, min_frames=4)
    with pytest.raises(ValueError, match="roulette"):
        rnd.render_adaptive(None, None, Fresh(), 4, 12, 0.1, min_frames=4, roulette="3")
    with pytest.raises(ValueError, match="lens"):
        rnd.render_adaptive(None, None, Fresh(), 4, 12, 0.1, min_frames=4, lens=(1.0,))
    AD.check_arguments(12, 0.0, 12, 2, 1e-4)            # threshold 0 and inf, min_frames == frames are fine
    AD.check_arguments(2, float("inf"), 2, 64, 1.0)


# ---------------------------------------------------- C2: the policy against its restatement
def sel(err, threshold, dilate):
    err = np.asarray(err, np.float32)
    ty, tx = err.shape
    return AD.select_tiles(err.reshape(-1), threshold, tx, ty, dilate).reshape(ty, tx).astype(bool)


def test_policy_threshold_edge_inf_and_nan():
    t = np.float32(0.125)
    err = np.array([[0.0, t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))],
                    [np.inf, np.nan, -0.0, 1e30]], np.float32)
    want = np.array([[0, 0, 1, 0], [1, 1, 0, 1]], bool)  # above is strict; +inf and NaN are above
    assert np.array_equal(sel(err, t, False), want) and np.array_equal(AR.select(err, t, False), want)
    assert sel(err, np.inf, False).sum() == 1 and AR.select(err, np.inf, False).sum() == 1  # NaN alone
    assert np.array_equal(sel(err, 0.0, False), np.array([[0, 1, 1, 1], [1, 1, 0, 1]], bool))
    m = AD.select_tiles(err.reshape(-1), t, 4, 2, False)
    assert m.dtype == np.uint8 and m.shape == (8,) and set(m.tolist()) == {0, 1}


def test_policy_dilation_at_the_border():
    err = np.zeros((4, 6), np.float32)
    err[0, 0] = err[3, 5] = err[1, 3] = 1
    got = sel(err, 0.5, True)
    want = np.zeros((4, 6), bool)
    want[0:2, 0:2] = True   # a corner grows into the image only
    want[2:4, 4:6] = True
    want[0:3, 2:5] = True   # the 8-neighbourhood, corners included
    assert np.array_equal(got, want) and np.array_equal(AR.select(err, 0.5, True), want)
    assert np.array_equal(sel(err, 0.5, False), err > 0.5)
    assert not sel(np.zeros((3, 3)), 0.5, True).any()
    assert sel(np.ones((1, 1)), 0.5, True).all() and sel(np.ones((1, 5)) * [0, 0, 1, 0, 0], 0.5, True).sum() == 3
    g = np.random.default_rng(11)
    for _ in range(200):
        ty, tx = g.integers(1, 7, 2)
        e = g.uniform(0, 1, (ty, tx)).astype(np.float32)
        e[g.uniform(size=e.shape) < 0.1] = np.inf
        th = float(g.uniform(0.3, 1.0))
        for dilate in (False, True):
            assert np.array_equal(sel(e, th, dilate), AR.select(e, th, dilate))


def test_policy_rounds_and_the_budget():
    assert AD.round_frames(16, 64, 8) == 8 and AD.round_frames(60, 64, 8) == 4  # the last round cut to the budget
    assert AD.round_frames(64, 64, 8) == 0 and AD.round_frames(16, 16, 8) == 0
    assert AD.tile_grid(37, 21) == (5, 3) and AD.tile_grid(64, 48) == (8, 6) and AD.tile_grid(1, 1) == (1, 1)
    # the restated loop: the last round cut, and an empty set stops it
    noisy = np.ones((3, 5))
    count, masks, issued = AR.replay([noisy, noisy], 37, 21, 10, 0.5, 4, 4, False)
    assert issued == 10 and len(masks) == 2 and (count == 10).all()
    quiet = np.zeros((3, 5))
    count, masks, issued = AR.replay([noisy, quiet], 37, 21, 64, 0.5, 4, 4, True)
    assert issued == 8 and len(masks) == 2 and not masks[1].any() and (count == 8).all()
    one = np.zeros((3, 5))
    one[0, 0] = 1
    count, masks, issued = AR.replay([one, one, quiet], 37, 21, 64, 0.5, 4, 2, True)
    assert issued == 8 and (count[:16, :16] == 8).all() and (count[16:] == 4).all() and (count[:, 16:] == 4).all()
    count, _, _ = AR.replay([one, one, quiet], 37, 21, 64, 0.5, 4, 2, False)
    assert (count[:8, :8] == 8).all() and count.sum() == 4 * 37 * 21 + 4 * 64
    with pytest.raises(AssertionError):
        AR.replay([noisy], 37, 21, 64, 0.5, 4, 4, True)  # the loop would have read another map


def test_float64_restatement_on_hand_made_pixels():
    a = np.array([[1, 2, 3, 9], [0.5, 0.5, 0.5, 0], [4, 4, 4, 0], [0, 0, 0, 0]], np.float64)
    b = np.array([[3, 2, 1, 7], [0.5, 0.5, 0.5, 0], [1, 1, 1, 0], [0, 0, 0, 0]], np.float64)
    na, nb = np.array([1, 5, 0, 2]), np.array([3, 5, 2, 0])
    m, n = AR.merge(a, na, b, nb)
    assert np.array_equal(n, [4, 10, 2, 2])
    assert np.allclose(m[0], [2.5, 2.0, 1.5, 0]) and np.array_equal(m[2], b[2]) and np.array_equal(m[3], a[3])
    e = AR.pixel_error(a, na, b, nb, 1.0)
    assert np.isclose(e[0], 0.5 * 4 / np.sqrt(1 + 6.0)) and e[1] == 0 and np.isposinf(e[2]) and np.isposinf(e[3])
    t = AR.tile_error(2, 2, a, np.array([1, 5, 1, 2]), b, np.array([3, 5, 2, 1]), 1.0)
    assert t.shape == (1, 1) and np.isfinite(t).all()
    assert 26 * AR.U < AR.TILE_ERROR_BOUND <= 32 * AR.U
