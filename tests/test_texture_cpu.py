"""Diffuse texture maps, the host half (no GPU): the OBJ `vt` and MTL `map_Kd`
loaders (csrc/mcpt_host.cpp), the PNG reader and sRGB table (scene.py), the
config key and flags, and the float64 restatement of the lookup
(tests/texture_ref.py) on cases one can compute by hand."""
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

from . import texture_ref as T
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n"


# -------------------------------------------------------------------- loaders
def test_obj_vt_forms_fans_and_negative_indices(tmp_path):
    text = QUAD + "f 1/1 2/2 3/3 4/4\nf 1/1/1 2/2/1 3/3/1\nf -4/-4 -3/-3 -2/-2\nf 1//1 2//1 3//1\nf 1 2 3\nf 1/1 2/2 3\n"
    (tmp_path / "m.obj").write_text(text)
    uv, has = S.load_obj_uvs(str(tmp_path) + "/", "m.obj")
    uv2, has2 = S.obj_uvs_from_text(text)
    assert np.array_equal(uv, uv2) and np.array_equal(has, has2)
    tris, _, _ = S.load_object(str(tmp_path) + "/", "m.obj")
    assert len(tris) == len(uv) == 7  # the same fan triangulation and order
    assert has.tolist() == [True, True, True, True, False, False, False]
    assert uv[0].tolist() == [[0, 0], [1, 0], [1, 1]] and uv[1].tolist() == [[0, 0], [1, 1], [0, 1]]
    assert uv[2].tolist() == uv[3].tolist() == [[0, 0], [1, 0], [1, 1]]
    assert not uv[4:].any()
    # uv follows the corner's position: corner k of triangle i is vertex k of load_object's triangle i
    assert np.array_equal(tris["v"][:4, :, :2], uv[:4])


@pytest.mark.parametrize("face", ["f 1/5 2/2 3/3", "f 1/-5 2/2 3/3", "f 1/0 2/2 3/3", "f 1/99999999999999999999 2/2 3/3",
                                  "f 1/x 2/2 3/3"])
def test_obj_vt_index_of_zero_or_out_of_range_is_a_parse_error(face):
    with pytest.raises(L.MCPTError, match="-4"):
        S.obj_uvs_from_text(QUAD + face + "\n")


def test_mtl_map_names_options_spaces_and_backslashes(tmp_path):
    mtl = ("newmtl wood\nKd 0.8 0.8 0.8\nmap_Kd wood.png\n"
           "newmtl plain\nKd 0.5 0.5 0.5\n"
           "newmtl opt\nmap_Kd -s 2 2 -o 0.5 0.5 0 -clamp on -bm 0.3 tex\\my file.png  \r\n"
           "newmtl only\nmap_Kd -clamp on\n")
    assert S.mtl_maps_from_text(mtl) == ["wood.png", "", "tex/my file.png", ""]
    assert S.mtl_maps_from_text("") == []
    (tmp_path / "m.mtl").write_text(mtl)
    (tmp_path / "m.obj").write_text("mtllib m.mtl\n" + QUAD + "usemtl opt\nf 1/1 2/2 3/3\n")
    assert S.load_mtl_maps(str(tmp_path) + "/", "m.obj") == ["wood.png", "", "tex/my file.png", ""]
    _, mats, idx = S.load_object(str(tmp_path) + "/", "m.obj")
    assert len(mats) == 4 and idx.tolist() == [2]  # the same material order


def test_shipped_scenes_have_no_maps_and_load_obj_is_unchanged():
    directory = os.path.join(ROOT, "scenes", "cbox") + "/"
    uv, has = S.load_obj_uvs(directory, "cbox.obj")
    tris, mats, idx = S.load_object(directory, "cbox.obj")
    assert len(uv) == len(tris) and not any(S.load_mtl_maps(directory, "cbox.obj"))
    u, t, images = S.load_textures(directory, "cbox.obj", mats, idx)
    assert (t == -1).all() and images == []


def test_texture_host_code_under_address_sanitizer(tmp_path):
    """The `vt` and `map_Kd` parsers in a stand-alone program built here with
    -fsanitize=address,undefined: truncated and malformed text, overflowing
    and out-of-range indices, option-only map lines and empty inputs, every
    buffer a heap block of exactly its size (tests/native/texture_check.cpp)."""
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    exe = str(tmp_path / "texture_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "texture_check.cpp"),
                         os.path.join(csrc, "mcpt_host.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_attribute_host_code_under_address_sanitizer(tmp_path):
    """The host half of mcpt_scene_set_textures and mcpt_scene_set_normal_maps
    (csrc/mcpt_attr.h, a header without HIP) in a stand-alone program built here
    with -fsanitize=address,undefined: every input the setters reject, with its
    message, and a valid two-triangle, two-image set whose records are compared
    with the layouts of mcpt_texture.h and mcpt_bump.h, every buffer a heap
    block of exactly its size (tests/native/attr_check.cpp)."""
    exe = str(tmp_path / "attr_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "attr_check.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------ PNG
def _png(w, h, ctype, rows, filters, palette=None, depth=8, interlace=0):
    """A PNG built here: rows = h byte strings of unfiltered pixels, each
    filtered with filters[y] as the PNG specification defines it."""
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    raw, prev = b"", bytes(len(rows[0]))
    for y, line in enumerate(rows):
        f, out = filters[y], bytearray()
        for i, x in enumerate(line):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if f == 0:
                p = 0
            elif f == 1:
                p = a
            elif f == 2:
                p = b
            elif f == 3:
                p = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out.append((x - p) & 255)
        raw += bytes([f]) + bytes(out)
        prev = line

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    z = zlib.compress(raw, 6)
    body = chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        body += chunk(b"PLTE", bytes(palette))
    body += chunk(b"IDAT", z[:len(z) // 2]) + chunk(b"IDAT", z[len(z) // 2:])  # two IDAT chunks: one stream
    return b"\x89PNG\r\n\x1a\n" + body + chunk(b"IEND", b"")


@pytest.mark.parametrize("ctype", [0, 2, 3, 4, 6])
def test_read_png_every_filter_and_colour_type(ctype):
    w, h = 7, 10  # two rows of each of the five filters
    rng = np.random.Generator(np.random.PCG64(ctype))
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    px = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    palette = None
    if ctype == 3:
        palette = rng.integers(0, 256, (11, 3), dtype=np.uint8)
        px = rng.integers(0, 11, (h, w, 1), dtype=np.uint8)
    filters = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    data = _png(w, h, ctype, [px[y].tobytes() for y in range(h)], filters,
                None if palette is None else palette.tobytes())
    got = S.decode_png(data)
    want = {0: lambda: np.repeat(px, 3, 2), 2: lambda: px, 3: lambda: palette[px[..., 0]],
            4: lambda: np.repeat(px[..., :1], 3, 2), 6: lambda: px[..., :3]}[ctype]()
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, want)


def test_read_png_round_trip_with_write_png(tmp_path):
    rng = np.random.Generator(np.random.PCG64(1))
    img = rng.uniform(0, 1, (9, 13, 4)).astype(np.float32)
    path = S.write_png(str(tmp_path / "a.png"), img, flip=False)
    assert np.array_equal(S.read_png(path), S.preview_rgb8(img, flip=False))
    lin = S.read_texture(path)
    assert lin.dtype == np.float32 and np.array_equal(lin, S.SRGB_TO_LINEAR[S.preview_rgb8(img, flip=False)])


def test_read_png_refuses_what_it_does_not_read(tmp_path):
    row = [bytes(6)] * 2
    for bad in (_png(2, 2, 2, row, [0, 0], interlace=1), _png(2, 2, 2, [bytes(12)] * 2, [0, 0], depth=16),
                _png(2, 2, 2, row, [0, 5]), _png(2, 2, 3, [bytes(2)] * 2, [0, 0]), b"not a png",
                _png(2, 2, 2, row, [0, 0])[:-20], _png(2, 2, 2, [bytes(6)], [0]), b""):
        with pytest.raises(ValueError):
            S.decode_png(bad)
    good = _png(2, 2, 2, row, [0, 0])
    flipped = bytearray(good)
    flipped[40] ^= 1
    with pytest.raises(ValueError):
        S.decode_png(bytes(flipped))
    with pytest.raises(ValueError, match="nothing.png"):
        S.read_texture(str(tmp_path / "nothing.png"))
    (tmp_path / "x.tga").write_bytes(b"\0" * 32)
    with pytest.raises(ValueError, match="x.tga"):
        S.read_texture(str(tmp_path / "x.tga"))


def test_srgb_table_matches_the_formula_bit_for_bit():
    import math
    for i in range(256):
        c = i / 255.0
        want = c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)
        assert S.SRGB_TO_LINEAR[i].tobytes() == np.float32(want).tobytes(), i
    assert S.SRGB_TO_LINEAR.dtype == np.float32 and S.SRGB_TO_LINEAR[0] == 0 and S.SRGB_TO_LINEAR[255] == 1


def test_load_textures_maps_materials_to_images(tmp_path, capsys):
    img = np.zeros((2, 3, 4), np.float32)
    img[..., 0] = 1.0
    S.write_png(str(tmp_path / "red.png"), img, flip=False)
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd red.png\nnewmtl b\nKd 1 1 1\nnewmtl c\nKd 1 1 1\nmap_Kd -clamp on red.png\n")
    obj = "mtllib m.mtl\n" + QUAD + "usemtl a\nf 1/1 2/2 3/3\nf 1 2 3\nusemtl b\nf 1/1 2/2 3/3\nusemtl c\nf 1/1 3/3 4/4\n"
    (tmp_path / "m.obj").write_text(obj)
    d = str(tmp_path) + "/"
    _, mats, idx = S.load_object(d, "m.obj")
    uv, tri_tex, images = S.load_textures(d, "m.obj", mats, idx)
    assert tri_tex.tolist() == [0, -1, -1, 0] and len(images) == 1  # one file, read once
    assert images[0].shape == (2, 3, 3) and (images[0][..., 0] == 1).all() and not images[0][..., 1:].any()
    # a named file that is missing
    os.remove(tmp_path / "red.png")
    with pytest.raises(ValueError, match="red.png"):
        S.load_textures(d, "m.obj", mats, idx)
    # maps but no vt at all: untextured, one warning line
    (tmp_path / "n.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nusemtl a\nf 1 2 3\n")
    _, mats, idx = S.load_object(d, "n.obj")
    capsys.readouterr()
    uv, tri_tex, images = S.load_textures(d, "n.obj", mats, idx)
    err = capsys.readouterr().err
    assert tri_tex.tolist() == [-1] and images == [] and err.count("\n") == 1 and "n.obj" in err


# ------------------------------------------------------------ config, App, CLI
def test_abi_mirror_declares_the_texture_entry_points():
    assert L.ABI_VERSION == 5  # functions and their own struct only: the revision stays
    so = L.lib()
    for name in ("mcpt_load_obj_uvs", "mcpt_obj_uvs_from_text", "mcpt_load_mtl_maps", "mcpt_mtl_maps_from_text",
                 "mcpt_scene_set_textures", "mcpt_texture_eval"):
        assert name in L.SIGNATURES and hasattr(so, name)
    assert ctypes.sizeof(L.RenderParams) == 13 * 4  # mcpt_render_params gained no field
    assert ctypes.sizeof(L.Textures) == 32 and ctypes.sizeof(L.TextureImage) == 16


def test_config_reads_the_textures_key():
    assert C.Config(_entry()).TEXTURES() is False
    assert C.Config(_entry(textures=True)).TEXTURES() is True
    assert C.Config(_entry(textures=False)).TEXTURES() is False
    for bad in (1, 0, "yes", None, [True], 1.0):
        with pytest.raises(ValueError):
            C.Config(_entry(textures=bad))
    root = C.loads(open(os.path.join(ROOT, "config.json")).read())
    assert all("textures" not in e for e in root["config"])


def test_app_and_command_line_take_textures():
    from montecarlopathtracing_amd.__main__ import parser
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).textures is False
    assert App(C.Config(_entry(textures=True))).textures is True
    assert App(C.Config(_entry()), textures=True).textures is True
    assert App(C.Config(_entry(textures=True)), textures=False).textures is False
    with pytest.raises(ValueError):
        App(C.Config(_entry()), textures=1)
    assert parser().parse_args([]).textures is False and parser().parse_args(["--textures"]).textures is True


# ------------------------------------------------- the restatement, by hand
IMG = np.arange(5 * 3 * 3, dtype=np.float64).reshape(3, 5, 3)  # (H, W) = (3, 5); texel (row j, column i) = IMG[j, i]


def _at(u, v, **kw):
    return T.sample(IMG, np.array([u], np.float64), np.array([v], np.float64), **kw)[0]


def test_restatement_texel_centre_returns_the_texel():
    for j in range(3):
        for i in range(5):
            got = _at((i + 0.5) / 5, 1.0 - (j + 0.5) / 3)
            assert np.allclose(got, IMG[j, i], rtol=0, atol=1e-12), (i, j)


def test_restatement_midpoint_of_two_texels_is_their_mean():
    assert np.allclose(_at(2.0 / 5, 1.0 - 0.5 / 3), (IMG[0, 1] + IMG[0, 2]) / 2, atol=1e-12)   # between columns 1 and 2
    assert np.allclose(_at(0.5 / 5, 1.0 - 1.0 / 3), (IMG[0, 0] + IMG[1, 0]) / 2, atol=1e-12)   # between rows 0 and 1
    assert np.allclose(_at(0.0, 1.0 - 0.5 / 3), (IMG[0, 4] + IMG[0, 0]) / 2, atol=1e-12)       # the column wrap
    assert np.allclose(_at(0.5 / 5, 0.0), (IMG[2, 0] + IMG[0, 0]) / 2, atol=1e-12)             # the row wrap


def test_restatement_repeats_and_puts_row_zero_at_the_top():
    for u, v in ((0.13, 0.71), (0.5, 0.5), (0.99, 0.01)):
        assert np.allclose(_at(u, v), _at(u + 1, v), atol=1e-9) and np.allclose(_at(u, v), _at(u - 2, v + 3), atol=1e-9)
    assert np.allclose(_at(0.5 / 5, 1.0 - 0.5 / 3), IMG[0, 0], atol=1e-12)  # v near 1: row 0
    assert np.allclose(_at(0.5 / 5, 0.5 / 3), IMG[2, 0], atol=1e-12)        # v near 0: the last row


def test_restatement_interpolates_uv_and_falls_back_on_a_sliver():
    verts = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[3, 0, 0], [4, 0, 0], [5, 0, 0]]], np.float64)
    uv = np.array([[[1.1, 0.9], [1.5, 0.9], [1.1, 0.5]], [[0.3, 0.5], [0.9, 0.9], [0.9, 0.9]]], np.float64)
    pts = np.array([[0.25, 0.5, 0], [4.5, 0, 0], [0.25, 0.5, 0]], np.float64)
    got = T.texture_factor(verts, uv, np.array([0, 0]), [IMG], [0, 1, 0], pts)
    assert np.allclose(got[0, :3], _at(1.1 + 0.25 * 0.4, 0.9 - 0.5 * 0.4), atol=1e-12) and (got[:, 3] == 1).all()
    assert np.allclose(got[1, :3], _at(0.3, 0.5), atol=1e-12)  # den = 0: corner 0's uv
    none = T.texture_factor(verts, uv, np.array([-1, -1]), [IMG], [0, 1], pts[:2])
    assert (none == 1).all()
    for m in T.MUTANTS:  # every deliberate mistake moves the first query
        assert not np.allclose(T.texture_factor(verts, uv, np.array([0, 0]), [IMG], [0], pts[:1], mutant=m), got[:1], atol=1e-3), m
