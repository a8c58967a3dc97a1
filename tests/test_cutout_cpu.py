"""Alpha cutouts, the host half (no GPU): the MTL `map_d` loader
(csrc/mcpt_host.cpp), the PNG reader's alpha channel, load_cutouts' precedence
and resampling (scene.py), the config key and flags, and the float64
restatement (tests/cutout_ref.py) on cases one can compute by hand."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C
from montecarlopathtracing_amd import scene as S

from . import cutout_ref as CR
from .test_jitter_cpu import _entry
from .test_texture_cpu import QUAD, _png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -------------------------------------------------------------------- loaders
def test_mtl_alpha_map_names_options_spaces_and_backslashes(tmp_path):
    mtl = ("newmtl leaf\nKd 0.8 0.8 0.8\nmap_Kd leaf.png\nmap_d leaf_mask.png\n"
           "newmtl plain\nKd 0.5 0.5 0.5\nd 0.3\nTr 0.7\n"
           "newmtl opt\nmap_d -s 2 2 -o 0.5 0.5 0 -clamp on -imfchan m tex\\my mask.png  \r\n"
           "newmtl only\nmap_d -clamp on\n"
           "newmtl colour\nmap_Kd wood.png\n")
    want = ["leaf_mask.png", "", "tex/my mask.png", "", ""]
    assert S.mtl_alpha_maps_from_text(mtl) == want
    assert S.mtl_maps_from_text(mtl) == ["leaf.png", "", "", "", "wood.png"]  # map_Kd's reader is what it was
    assert S.mtl_alpha_maps_from_text("") == [] and S.mtl_alpha_maps_from_text(b"newmtl") == [""]
    for cut in range(len(mtl) + 1):  # truncated text parses
        assert len(S.mtl_alpha_maps_from_text(mtl[:cut])) <= 5
    (tmp_path / "m.mtl").write_text(mtl)
    (tmp_path / "m.obj").write_text("mtllib m.mtl\n" + QUAD + "usemtl opt\nf 1/1 2/2 3/3\n")
    assert S.load_mtl_alpha_maps(str(tmp_path) + "/", "m.obj") == want
    with pytest.raises(L.MCPTError):
        S.load_mtl_alpha_maps(str(tmp_path) + "/", "missing.obj")
    assert not any(S.load_mtl_alpha_maps(os.path.join(ROOT, "scenes", "cbox") + "/", "cbox.obj"))


def test_cutout_host_code_under_address_sanitizer(tmp_path):
    """The `map_d` parser in a stand-alone program built here with
    -fsanitize=address,undefined: truncated and option-only text and empty
    inputs, every buffer a heap block of exactly its size
    (tests/native/cutout_check.cpp)."""
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    exe = str(tmp_path / "cutout_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "cutout_check.cpp"),
                         os.path.join(csrc, "mcpt_host.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------ PNG
def _with_trns(png, trns):
    """`png` with a tRNS chunk put in front of its first IDAT chunk."""
    at = png.index(b"IDAT") - 4
    chunk = struct.pack(">I", len(trns)) + b"tRNS" + trns + struct.pack(">I", zlib.crc32(b"tRNS" + trns) & 0xFFFFFFFF)
    return png[:at] + chunk + png[at:]


@pytest.mark.parametrize("ctype", [4, 6])
def test_decode_png_returns_the_alpha_channel(ctype):
    w, h = 7, 10
    rng = np.random.Generator(np.random.PCG64(10 + ctype))
    bpp = {4: 2, 6: 4}[ctype]
    px = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    px[0, 0, -1], px[0, 1, -1] = 0, 255
    data = _png(w, h, ctype, [px[y].tobytes() for y in range(h)], [0, 1, 2, 3, 4, 4, 3, 2, 1, 0])
    rgb, a = S.decode_png(data, alpha=True)
    assert np.array_equal(rgb, S.decode_png(data)) and rgb.shape == (h, w, 3)  # the colour is what it was
    assert a.dtype == np.float32 and a.shape == (h, w)
    assert a.tobytes() == (px[..., -1].astype(np.float32) / np.float32(255.0)).tobytes()  # raw / 255: no sRGB decode
    assert a[0, 0] == 0.0 and a[0, 1] == 1.0
    assert not np.array_equal(a, S.SRGB_TO_LINEAR[px[..., -1]])


def test_decode_png_palette_alpha_comes_from_trns():
    w, h = 5, 4
    rng = np.random.Generator(np.random.PCG64(3))
    palette = rng.integers(0, 256, (6, 3), dtype=np.uint8)
    px = rng.integers(0, 6, (h, w, 1), dtype=np.uint8)
    px[0, :, 0] = [0, 1, 2, 3, 5]
    plain = _png(w, h, 3, [px[y].tobytes() for y in range(h)], [0, 1, 2, 4], palette.tobytes())
    rgb, a = S.decode_png(plain, alpha=True)
    assert a is None and np.array_equal(rgb, palette[px[..., 0]])  # no tRNS: no alpha
    trns = bytes([0, 128, 255, 7])  # shorter than the palette: entries 4 and 5 are opaque
    rgb2, a2 = S.decode_png(_with_trns(plain, trns), alpha=True)
    assert np.array_equal(rgb2, rgb) and np.array_equal(S.decode_png(_with_trns(plain, trns)), rgb)
    table = np.array([0, 128, 255, 7, 255, 255], np.float32) / np.float32(255.0)
    assert a2.tobytes() == table[px[..., 0]].astype(np.float32).tobytes()
    assert a2[0].tolist() == [0.0, np.float32(128.0) / np.float32(255.0), 1.0, np.float32(7.0) / np.float32(255.0), 1.0]


@pytest.mark.parametrize("ctype", [0, 2])
def test_decode_png_without_an_alpha_channel_returns_none(ctype):
    bpp = {0: 1, 2: 3}[ctype]
    px = np.arange(2 * 3 * bpp, dtype=np.uint8).reshape(2, 3, bpp)
    data = _png(3, 2, ctype, [px[y].tobytes() for y in range(2)], [0, 0])
    rgb, a = S.decode_png(data, alpha=True)
    assert a is None and np.array_equal(rgb, S.decode_png(data))


# --------------------------------------------------------------- load_cutouts
def _write_rgba(path, rgb, a):
    """An 8-bit RGBA PNG (colour type 6) of (h, w, 3) and (h, w) uint8."""
    px = np.concatenate([rgb, a[..., None]], axis=2).astype(np.uint8)
    h, w = a.shape
    path.write_bytes(_png(w, h, 6, [px[y].tobytes() for y in range(h)], [0] * h))


def _write_grey(path, g):
    h, w = g.shape
    path.write_bytes(_png(w, h, 0, [g[y].astype(np.uint8).tobytes() for y in range(h)], [0] * h))


CUT_MTL = """newmtl both
Kd 1 1 1
map_Kd colour_a.png
map_d mask_rgba.png
newmtl own
Kd 1 1 1
map_Kd colour_a.png
newmtl grey
Kd 1 1 1
map_Kd colour_b.png
map_d -clamp on mask_grey.png
newmtl opaque
Kd 1 1 1
map_Kd colour_c.png
newmtl bare
Kd 1 1 1
map_d mask_grey.png
newmtl none
Kd 1 1 1
d 0.25
Tr 0.75
"""
CUT_OBJ = ("mtllib m.mtl\n" + QUAD +
           "usemtl both\nf 1/1 2/2 3/3\nusemtl grey\nf 1/1 3/3 4/4\nusemtl opaque\nf 1/1 2/2 3/3\n"
           "usemtl bare\nf 1/1 2/2 3/3\nf 1 2 3\nusemtl none\nf 1/1 2/2 3/3\nusemtl own\nf 1/1 2/2 4/4\n")


def _cutout_model(tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    files = {}
    files["colour_a"] = (rng.integers(0, 256, (4, 6, 3), dtype=np.uint8), rng.integers(0, 256, (4, 6), dtype=np.uint8))
    files["mask_rgba"] = (rng.integers(0, 256, (4, 6, 3), dtype=np.uint8), rng.integers(0, 256, (4, 6), dtype=np.uint8))
    files["colour_b"] = (rng.integers(0, 256, (6, 4, 3), dtype=np.uint8), np.full((6, 4), 255, np.uint8))
    _write_rgba(tmp_path / "colour_a.png", *files["colour_a"])
    _write_rgba(tmp_path / "mask_rgba.png", *files["mask_rgba"])
    _write_rgba(tmp_path / "colour_b.png", *files["colour_b"])
    grey = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    _write_grey(tmp_path / "mask_grey.png", grey)
    _write_grey(tmp_path / "colour_c.png", rng.integers(0, 256, (2, 2), dtype=np.uint8))
    (tmp_path / "m.mtl").write_text(CUT_MTL)
    (tmp_path / "m.obj").write_text(CUT_OBJ)
    return files, grey


def test_load_cutouts_precedence_and_resampling(tmp_path):
    files, grey = _cutout_model(tmp_path)
    d = str(tmp_path) + "/"
    _, mats, idx = S.load_object(d, "m.obj")
    uv, tri_tex, images, alphas = S.load_cutouts(d, "m.obj", mats, idx)
    uv0, tri0, images0 = S.load_textures(d, "m.obj", mats, idx)
    # the colour textures are load_textures', in its order; the bare map_d material adds one of ones behind them
    assert len(images0) == 3 and len(images) == 4 and len(alphas) == 4 and np.array_equal(uv, uv0)
    for a, b in zip(images, images0):
        assert a.tobytes() == b.tobytes()
    assert tri0.tolist() == [0, 1, 2, -1, -1, -1, 0]
    assert tri_tex.tolist() == [0, 1, 2, 3, -1, -1, 0]  # "bare" with vt: the new texture; without vt: none; "none": none
    f32 = lambda x: x.astype(np.float32) / np.float32(255.0)  # noqa: E731
    # "both" and "own" share colour_a.png: the map_d image's own alpha channel wins over the colour image's
    assert alphas[0].tobytes() == f32(files["mask_rgba"][1]).tobytes()
    assert alphas[0].tobytes() != f32(files["colour_a"][1]).tobytes()
    # "grey": the map_d image has no alpha channel: its first channel, raw, resampled 3x5 -> 6x4
    assert alphas[1].shape == (6, 4) and alphas[1].dtype == np.float32
    want = CR.resample(grey.astype(np.float64) / 255.0, 6, 4)
    assert np.abs(alphas[1].astype(np.float64) - want).max() <= 2.0 ** -22  # float64 arithmetic, rounded once, on /255 in fp32
    assert np.abs(alphas[1].astype(np.float64) - CR.resample(grey.astype(np.float64)[::-1] / 255.0, 6, 4)).max() > 0.05  # rows not flipped
    # "opaque": a grey colour image without alpha and no map_d: none
    assert alphas[2] is None
    # "bare": map_d and no map_Kd: a texture of ones with that alpha, at the mask's own size
    assert images[3].shape == (3, 5, 3) and (images[3] == 1).all() and alphas[3].tobytes() == f32(grey).tobytes()
    for a in alphas:
        assert a is None or (np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1)


def test_load_cutouts_own_alpha_of_the_colour_image_and_no_vt(tmp_path, capsys):
    files, grey = _cutout_model(tmp_path)
    d = str(tmp_path) + "/"
    # without the map_d line the colour image's own alpha channel is taken
    (tmp_path / "m.mtl").write_text(CUT_MTL.replace("map_d mask_rgba.png\n", ""))
    _, mats, idx = S.load_object(d, "m.obj")
    alphas = S.load_cutouts(d, "m.obj", mats, idx)[3]
    assert alphas[0].tobytes() == (files["colour_a"][1].astype(np.float32) / np.float32(255.0)).tobytes()
    # a missing mask names its file
    os.remove(tmp_path / "mask_grey.png")
    with pytest.raises(ValueError, match="mask_grey.png"):
        S.load_cutouts(d, "m.obj", mats, idx)
    # maps but no vt at all: one warning line, no cutouts
    (tmp_path / "n.mtl").write_text("newmtl a\nKd 1 1 1\nmap_d mask_rgba.png\n")
    (tmp_path / "n.obj").write_text("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nusemtl a\nf 1 2 3\n")
    _, mats, idx = S.load_object(d, "n.obj")
    capsys.readouterr()
    uv, tri_tex, images, alphas = S.load_cutouts(d, "n.obj", mats, idx)
    err = capsys.readouterr().err
    assert tri_tex.tolist() == [-1] and images == [] and alphas == [] and err.count("\n") == 1 and "n.obj" in err


def test_resample_alpha_is_the_lookup_at_the_texel_centres():
    rng = np.random.Generator(np.random.PCG64(8))
    a = rng.uniform(0, 1, (3, 5)).astype(np.float32)
    assert S.resample_alpha(a, 3, 5).tobytes() == a.tobytes()  # the same size: the image itself
    for h, w in ((6, 10), (2, 2), (1, 1), (7, 3)):
        got = S.resample_alpha(a, h, w)
        assert got.shape == (h, w) and got.dtype == np.float32
        assert np.abs(got.astype(np.float64) - CR.resample(a, h, w)).max() <= 2.0 ** -23
    # doubling a 1x2 image: by hand, with the wrap
    got = S.resample_alpha(np.array([[0.0, 1.0]], np.float32), 1, 4)
    assert np.allclose(got, [[0.25, 0.25, 0.75, 0.75]], atol=1e-7)


# ------------------------------------------------------------ config, App, CLI
def test_abi_mirror_declares_the_cutout_entry_points():
    assert L.ABI_VERSION == 5  # functions and their own struct only: the revision stays
    so = L.lib()
    for name in ("mcpt_load_mtl_alpha_maps", "mcpt_mtl_alpha_maps_from_text", "mcpt_scene_set_texture_alpha"):
        assert name in L.SIGNATURES and hasattr(so, name)
    assert ctypes.sizeof(L.TextureAlpha) == 24 and L.TextureAlpha.alpha.offset == 8 and L.TextureAlpha.threshold.offset == 16
    hdr = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in hdr and "typedef struct mcpt_texture_alpha" in hdr


def test_config_reads_the_cutouts_key():
    assert C.Config(_entry()).CUTOUTS() is None
    assert C.Config(_entry(cutouts=True)).CUTOUTS() == 0.5
    assert C.Config(_entry(cutouts=False)).CUTOUTS() is None
    assert C.Config(_entry(cutouts=0.25)).CUTOUTS() == 0.25 and C.Config(_entry(cutouts=1)).CUTOUTS() == 1.0
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), "yes", None, [0.5], {"threshold": 0.5}):
        with pytest.raises(ValueError):
            C.Config(_entry(cutouts=bad))
    root = C.loads(open(os.path.join(ROOT, "config.json")).read())
    assert all("cutouts" not in e for e in root["config"])


def test_app_and_command_line_take_cutouts():
    from montecarlopathtracing_amd.__main__ import cli_cutouts, parser
    from montecarlopathtracing_amd.app import App
    app = App(C.Config(_entry()))
    assert app.cutouts is None and app.textures is False
    app = App(C.Config(_entry(cutouts=True)))
    assert app.cutouts == 0.5 and app.textures is True  # cutouts switch the textures on
    assert App(C.Config(_entry()), cutouts=0.75).cutouts == 0.75 and App(C.Config(_entry()), cutouts=0.75).textures is True
    assert App(C.Config(_entry(cutouts=True)), cutouts=False).cutouts is None
    for bad in (0.0, 2.0, "on"):
        with pytest.raises(ValueError):
            App(C.Config(_entry()), cutouts=bad)
    p = parser()
    assert p.parse_args([]).cutouts is None and p.parse_args(["--cutouts"]).cutouts is True
    assert p.parse_args(["--cutouts", "0.3"]).cutouts == 0.3
    assert cli_cutouts(p.parse_args([]), C.Config(_entry(cutouts=0.25))) == 0.25
    assert cli_cutouts(p.parse_args(["--cutouts"]), C.Config(_entry())) == 0.5
    assert cli_cutouts(p.parse_args(["--cutouts", "1"]), C.Config(_entry(cutouts=0.25))) == 1.0
    with pytest.raises(ValueError):
        cli_cutouts(p.parse_args(["--cutouts", "0"]), C.Config(_entry()))


# ------------------------------------------------- the restatement, by hand
def test_restatement_alpha_by_hand_and_the_edge_scene_leaves_no_pixel_out():
    verts = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float64)
    uv = np.array([[[0, 0], [1, 0], [0, 1]]], np.float64)
    a = np.array([[0.0, 1.0], [0.5, 0.25]])  # row 0 the top
    at = lambda x, y, **kw: CR.alpha_at(verts, uv, [0], [a], [0], np.array([[x, y, 0.0]]), **kw)[0]  # noqa: E731
    assert abs(at(0.25, 0.75) - 0.0) < 1e-12 and abs(at(0.75, 0.25) - 0.25) < 1e-12  # texel centres
    assert abs(at(0.5, 0.75) - 0.5) < 1e-12  # between the top row's texels
    assert abs(at(0.25, 0.5) - 0.25) < 1e-12  # between the left column's
    assert abs(at(0.0, 0.75) - 0.5) < 1e-12  # the column wrap
    assert abs(at(0.3, 0.6, mutant="nearest") - 0.0) < 1e-12 and abs(at(0.25, 0.75, mutant="no_flip") - 0.5) < 1e-12
    assert CR.alpha_at(verts, uv, [-1], [a], [0], np.zeros((1, 3)))[0] == 1.0  # untextured
    assert CR.alpha_at(verts, uv, [0], [None], [0], np.zeros((1, 3)))[0] == 1.0  # an opaque texture
    # the edge scene under hole_camera's rays: every pixel of the left quad at least 0.1 from the threshold
    data, uv2, tri_tex, images, alphas, v = CR.hole_scene(CR.edge_alpha(), left_kd=0.0)
    k = np.arange(16)
    xs = (k / 16.0 - 0.5) * 2.0 + 1.0 / 32
    xx, yy = np.meshgrid(xs, xs)
    pts = np.stack([xx.reshape(-1), yy.reshape(-1), np.zeros(256)], axis=1)
    left = pts[:, 0] < 0
    ids = np.where(pts[:, 1] + 1 <= 2 * (pts[:, 0] - np.where(left, -1.0, 0.0)), 0, 1) + np.where(left, 0, 2)
    al = CR.alpha_at(v, uv2, tri_tex, alphas, ids, pts)
    assert (np.abs(al - 0.5) >= 1e-3).all() and np.abs(al[left] - 0.5).min() >= 0.1  # none of 256 left out (at most 5 % may be)
    assert (al[~left] == 1).all() and 0 < (al[left] < 0.5).sum() < left.sum()
