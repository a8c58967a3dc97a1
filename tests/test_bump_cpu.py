"""Bump and normal maps, the host half (no GPU): the MTL `map_Bump` / `bump` /
`norm` loader (csrc/mcpt_host.cpp), the height-to-normal conversion and the
normal-image decode (scene.py), the config key and flags, and the float64
restatement of the lookup (tests/bump_ref.py) on cases one can compute by
hand."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C
from montecarlopathtracing_amd import scene as S

from . import bump_cases as BC
from . import bump_ref as B
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, N_, NONE = S.BUMP_HEIGHT, S.BUMP_NORMAL, S.BUMP_NONE


# --------------------------------------------------------------------- MTL maps
@pytest.mark.parametrize("text,want", [
    ("", []),
    ("newmtl a\nKd 1 1 1\n", [("", NONE, 1.0)]),
    ("newmtl a\nmap_Bump a.png\n", [("a.png", H, 1.0)]),
    ("newmtl a\nmap_bump a.png\n", [("a.png", H, 1.0)]),
    ("newmtl a\nbump a.png\n", [("a.png", H, 1.0)]),
    ("newmtl a\nnorm a.png\n", [("a.png", N_, 1.0)]),
    ("newmtl a\nbump -bm 0.25 -s 2 2 -clamp on a.png\n", [("a.png", H, 0.25)]),
    ("newmtl a\nbump -clamp on -o 0.5 0.5 0 -bm 3 my file.png  \r\n", [("my file.png", H, 3.0)]),
    ("newmtl a\nnorm n.png\nbump -bm 2 h.png\n", [("n.png", N_, 1.0)]),
    ("newmtl a\nbump -bm 2 h.png\nnorm -bm 4 n.png\n", [("n.png", N_, 4.0)]),
    ("newmtl a\nbump tex\\sub\\h.png\nnewmtl b\nnewmtl c\nnorm c.png", [("tex/sub/h.png", H, 1.0), ("", NONE, 1.0),
                                                                    ("c.png", N_, 1.0)]),
    ("bump early.png\nnewmtl a\nmap_Kd kd.png\n", [("", NONE, 1.0)]),
])
def test_mtl_bump_maps_from_text(text, want):
    assert S.mtl_bump_maps_from_text(text) == want


def test_load_mtl_bump_maps_follows_the_obj_files_mtllib(tmp_path):
    (tmp_path / "m.obj").write_text("mtllib missing.mtl m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl b\nf 1 2 3\n")
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nnewmtl b\nKd 1 1 1\nmap_Bump -bm 0.5 h.png\n")
    assert S.load_mtl_bump_maps(str(tmp_path) + "/", "m.obj") == [("", NONE, 1.0), ("h.png", H, 0.5)]
    with pytest.raises(L.MCPTError):
        S.load_mtl_bump_maps(str(tmp_path) + "/", "none.obj")


def test_bump_host_code_under_address_sanitizer(tmp_path):
    """The bump-map parser in a stand-alone program built here with
    -fsanitize=address,undefined: truncated and malformed lines, overflowing
    -bm values, long names and short output buffers, every buffer a heap block
    of exactly its size (tests/native/bump_check.cpp)."""
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    exe = str(tmp_path / "bump_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "bump_check.cpp"),
                         os.path.join(csrc, "mcpt_host.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# -------------------------------------------------------------- height to normal
def test_height_to_normal_of_a_constant_map_is_straight_up():
    m = S.height_to_normal(np.full((3, 5), 0.37), 4.0)
    assert m.dtype == np.float32 and m.shape == (3, 5, 3)
    assert (m == np.array([0, 0, 1], np.float32)).all() and not np.signbit(m).any()


def test_height_to_normal_of_a_ramp_and_its_wrap():
    s, k = 0.01, 3.0
    h = np.tile(np.arange(8) * s, (4, 1))  # rises along +u by s per texel
    m = S.height_to_normal(h, k).astype(np.float64)
    want = np.array([-k * s, 0.0, 1.0]) / math.sqrt(1 + (k * s) ** 2)
    assert np.abs(m[:, 1:7] - want).max() < 1e-7  # the interior: gx = s
    # the edges wrap: column 0 sees (h[1] - h[7]) / 2 = -3 s, column 7 (h[0] - h[6]) / 2 = -3 s
    edge = np.array([3 * k * s, 0.0, 1.0]) / math.sqrt(1 + (3 * k * s) ** 2)
    assert np.abs(m[:, 0] - edge).max() < 1e-7 and np.abs(m[:, 7] - edge).max() < 1e-7
    # a ramp that rises towards row 0 (the top, +v): gy = (h[row j-1] - h[row j+1]) / 2 = s, so the normal leans to -v
    hv = np.tile((np.arange(6)[::-1] * s)[:, None], (1, 3))
    mv = S.height_to_normal(hv, k).astype(np.float64)
    assert np.abs(mv[1:5] - np.array([0.0, -k * s, 1.0]) / math.sqrt(1 + (k * s) ** 2)).max() < 1e-7
    # row 0 wraps to row 5: gy = (h[row 5] - h[row 1]) / 2 = (0 - 4 s) / 2
    assert np.abs(mv[0] - np.array([0.0, 2 * k * s, 1.0]) / math.sqrt(1 + (2 * k * s) ** 2)).max() < 1e-7
    # every texel unit within float32 rounding, z > 0: what mcpt_scene_set_normal_maps asks for
    for a in (m, mv):
        assert np.abs(np.sqrt((a * a).sum(2)) - 1).max() < 1e-6 and (a[..., 2] > 0).all()
    with pytest.raises(ValueError):
        S.height_to_normal(np.zeros((2, 2, 3)))
    with pytest.raises(ValueError):
        S.height_to_normal(np.zeros((2, 2)), float("nan"))


def test_normal_image_decode_of_eight_bit_and_float_data():
    px = np.array([[[128, 128, 255], [255, 128, 128], [128, 128, 0], [128, 128, 128]]], np.uint8)
    m = S.decode_normal_image(px).astype(np.float64)
    c = 2 * 128 / 255 - 1
    want = np.array([c, c, 1.0]) / math.sqrt(2 * c * c + 1)
    assert np.abs(m[0, 0] - want).max() < 1e-7 and m[0, 0, 2] < 1.0 and m[0, 0, 0] > 0  # near +z, not +z: raw, no sRGB
    assert np.abs(m[0, 1] - np.array([1.0, c, c]) / math.sqrt(1 + 2 * c * c)).max() < 1e-7  # z = c > 0: kept
    assert (m[0, 2] == (0, 0, 1)).all()   # z = -1 <= 0
    f = S.decode_normal_image(np.array([[[0, 0, 2.0], [3, 0, 4], [0, 0, 0], [1, 1, -1], [np.nan, 0, 1]]], np.float32))
    assert np.allclose(f[0, 0], (0, 0, 1)) and np.allclose(f[0, 1], (0.6, 0, 0.8), atol=1e-7)
    assert (f[0, 2:] == np.array([0, 0, 1], np.float32)).all()


def test_load_bump_maps_reads_the_model(tmp_path, capsys):
    BC.write_model(tmp_path)
    directory = str(tmp_path / "model") + "/"
    _, mats, idx = S.load_object(directory, "b.obj")
    uv, tri_map, images = S.load_bump_maps(directory, "b.obj", mats, idx, 2.0)
    assert tri_map.tolist() == [0, 0, -1, -1, 1, 1] and [im.shape for im in images] == [(6, 4, 3), (5, 3, 3)]
    raw = S.read_png(directory + "tex/height.png")
    want = S.height_to_normal(raw.astype(np.float64).mean(2) / 255.0, 3.0 * 2.0)  # -bm 3 times the scale
    assert np.array_equal(images[0], want) and (images[0][..., :2] != 0).any()
    assert np.array_equal(images[1], S.decode_normal_image(S.read_png(directory + "tex/normal.png")))
    for im in images:
        assert np.abs(np.sqrt((im.astype(np.float64) ** 2).sum(2)) - 1).max() < 1e-6 and (im[..., 2] > 0).all()
    assert capsys.readouterr().err == ""
    # maps but no vt: one warning line, unmapped
    obj = (tmp_path / "model" / "b.obj").read_text()
    (tmp_path / "model" / "novt.obj").write_text("\n".join(
        ln if not ln.startswith(("vt ", "f ")) else " ".join(t.split("/")[0] for t in ln.split())
        for ln in obj.splitlines() if not ln.startswith("vt ")) + "\n")
    _, tm, ims = S.load_bump_maps(directory, "novt.obj", mats, idx)
    assert (tm == -1).all() and ims == []
    assert capsys.readouterr().err.count("\n") == 1
    (tmp_path / "model" / "b.mtl").write_text("newmtl floor\nbump gone.png\nnewmtl light\nnewmtl wall\n")
    with pytest.raises(ValueError, match="gone.png"):
        S.load_bump_maps(directory, "b.obj", mats, idx)


def test_shipped_scenes_have_no_bump_maps():
    directory = os.path.join(ROOT, "scenes", "cbox") + "/"
    tris, mats, idx = S.load_object(directory, "cbox.obj")
    uv, t, images = S.load_bump_maps(directory, "cbox.obj", mats, idx)
    assert (t == -1).all() and images == []


# ------------------------------------------------------------ config, App, CLI
def test_abi_mirror_declares_the_bump_entry_points():
    assert L.ABI_VERSION == 5  # functions and their own struct only: the revision stays
    so = L.lib()
    for name in ("mcpt_load_mtl_bump_maps", "mcpt_mtl_bump_maps_from_text", "mcpt_scene_set_normal_maps", "mcpt_bump_eval"):
        assert name in L.SIGNATURES and hasattr(so, name)
    assert ctypes.sizeof(L.NormalMaps) == 32 and ctypes.sizeof(L.NormalMapImage) == 16


def test_config_reads_the_bump_key():
    assert C.Config(_entry()).BUMP() is None
    assert C.Config(_entry(bump=True)).BUMP() == 1.0
    assert C.Config(_entry(bump=False)).BUMP() is None
    assert C.Config(_entry(bump=2.5)).BUMP() == 2.5 and C.Config(_entry(bump=3)).BUMP() == 3.0
    for bad in ("yes", [1], {"scale": 1}, 0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="bump"):
            C.Config(_entry(bump=bad))
    root = C.loads(open(os.path.join(ROOT, "config.json")).read())
    assert all("bump" not in e for e in root["config"])


def test_app_and_command_line_take_bump():
    from montecarlopathtracing_amd.__main__ import cli_bump, parser
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).bump is None
    assert App(C.Config(_entry(bump=2.0))).bump == 2.0
    assert App(C.Config(_entry()), bump=True).bump == 1.0 and App(C.Config(_entry(bump=True)), bump=False).bump is None
    with pytest.raises(ValueError):
        App(C.Config(_entry()), bump=-2.0)
    with pytest.raises(ValueError):
        App(C.Config(_entry()), bump="on")
    ap = parser()
    assert ap.parse_args([]).bump is None
    assert ap.parse_args(["--bump"]).bump is True and ap.parse_args(["--bump", "0.5"]).bump == 0.5
    assert cli_bump(ap.parse_args(["--bump"]), C.Config(_entry())) == 1.0
    assert cli_bump(ap.parse_args([]), C.Config(_entry(bump=4))) == 4.0
    with pytest.raises(ValueError):
        cli_bump(ap.parse_args(["--bump", "0"]), C.Config(_entry()))
    with pytest.raises(ValueError):
        cli_bump(ap.parse_args(["--bump", "nan"]), C.Config(_entry()))
    with pytest.raises(SystemExit):
        ap.parse_args(["--bump", "steep"])


# ------------------------------------------------- the restatement's properties
TRI = np.array([[[0, 0, 0], [2, 0, 0], [0, 0, -2]]], np.float64)  # in the plane y = 0, face normal +y
UVS = np.array([[[0, 0], [1, 0], [0, 1]]], np.float64)          # u along +x, v along -z: T = +x, B = -z, h = +1
UP = np.array([[0.0, 1.0, 0.0]])


def _eval(m, uv=UVS, N=UP, d=(0.0, -1.0, 0.0), pt=(0.5, 0.0, -0.5), mutant=None, tri=TRI):
    img = np.broadcast_to(np.asarray(m, np.float64), (2, 2, 3))
    ng = B.face_normals(tri)
    out, tie = B.bump_normal(tri, ng, uv, np.zeros(1, np.int32), [img], [0], np.array([pt], np.float64),
                             np.array([d], np.float64), np.asarray(N, np.float64), mutant)
    assert not tie.any()
    return out[0]


def test_restatement_frame_of_the_hand_triangle():
    ng = B.face_normals(TRI)
    assert np.allclose(ng, UP)
    t, h, ok = B.tangent_frames(TRI, ng, UVS, np.zeros(1, np.int32))
    assert ok.all() and np.allclose(t, [[1, 0, 0]]) and h.tolist() == [1.0]
    a = math.radians(30)
    assert np.allclose(_eval((math.sin(a), 0, math.cos(a))), (math.sin(a), math.cos(a), 0), atol=1e-12)   # red: +u = +x
    assert np.allclose(_eval((0, math.sin(a), math.cos(a))), (0, math.cos(a), -math.sin(a)), atol=1e-12)  # green: +v = -z


def test_restatement_is_unit_and_straight_up_returns_n_bit_for_bit():
    rng = np.random.Generator(np.random.PCG64(7))
    for _ in range(50):
        a, p = math.radians(rng.uniform(0, 70)), rng.uniform(0, 2 * math.pi)
        n = _eval((math.sin(a) * math.cos(p), math.sin(a) * math.sin(p), math.cos(a)))
        assert abs(math.sqrt((n * n).sum()) - 1) < 1e-12
    N = np.array([[0.28, 0.96, 0.0]])
    assert _eval((0, 0, 1), N=N).tobytes() == N[0].tobytes()
    assert _eval((0, 0, 1), N=N, uv=UVS[:, [0, 2, 1]]).tobytes() == N[0].tobytes()


def test_restatement_my_zero_stays_in_the_plane_of_n_and_the_tangent():
    N = np.array([[0.3, 0.9, 0.2]]) / np.linalg.norm([0.3, 0.9, 0.2])
    a = math.radians(40)
    n = _eval((math.sin(a), 0, math.cos(a)), N=N)
    tp = np.array([1.0, 0, 0]) - N[0] * N[0, 0]
    assert abs(np.dot(n, np.cross(N[0], tp))) < 1e-12 and np.dot(n, tp) > 0
    assert abs(np.dot(n, N[0]) - math.cos(a)) < 1e-12  # Gram-Schmidt: the tilt is measured from N


def test_restatement_mirrored_uvs_give_the_same_world_normal():
    """The twin has its UVs mirrored in u (u' = 1 - u) and the map mirrored to
    match (mx negated): the same surface, so the same world normal; its h is -1."""
    ng = B.face_normals(TRI)
    mirrored = UVS.copy()
    mirrored[..., 0] = 1.0 - mirrored[..., 0]
    t, h, ok = B.tangent_frames(TRI, ng, mirrored, np.zeros(1, np.int32))
    assert h.tolist() == [-1.0] and np.allclose(t, [[-1, 0, 0]])
    a, p = math.radians(35), 0.7
    m = np.array([math.sin(a) * math.cos(p), math.sin(a) * math.sin(p), math.cos(a)])
    assert np.allclose(_eval(m), _eval(m * (-1, 1, 1), uv=mirrored), atol=1e-12)
    # with h ignored the twin's green axis points the other way
    assert np.abs(_eval(m) - _eval(m * (-1, 1, 1), uv=mirrored, mutant="no_h")).max() > 0.3


def test_restatement_seen_from_the_back_faces_the_ray():
    a, p = math.radians(35), 2.1
    m = np.array([math.sin(a) * math.cos(p), math.sin(a) * math.sin(p), math.cos(a)])
    front = _eval(m)
    back = _eval(m, N=-UP, d=(0.0, 1.0, 0.0))
    assert np.dot(back, (0.0, 1.0, 0.0)) < 0
    # the back shows the front's relief mirrored in the surface: the tangent part is the same, the normal part negated
    assert np.allclose(back, front * (1, -1, 1), atol=1e-12)
    assert np.abs(back - _eval(m, N=-UP, d=(0.0, 1.0, 0.0), mutant="no_f")).max() > 0.3
    # a texel tilted away from the viewer gives N
    away = _eval((math.sin(math.radians(80)), 0, math.cos(math.radians(80))), d=(0.94, -0.34, 0.0))
    assert away.tobytes() == UP[0].tobytes()


def test_restatement_unmapped_and_degenerate_triangles_return_n():
    ng = B.face_normals(TRI)
    N = np.array([[0.6, 0.8, 0.0]])
    img = np.broadcast_to(np.array([0.6, 0, 0.8]), (1, 1, 3))
    args = ([0], np.array([[0.5, 0, -0.5]]), np.array([[0, -1.0, 0]]), N)
    out, _ = B.bump_normal(TRI, ng, UVS, np.array([-1]), [img], *args)
    assert out.tobytes() == N.tobytes()
    out, _ = B.bump_normal(TRI, ng, np.array([[[0, 0], [0.5, 0.5], [1, 1]]], np.float64), np.array([0]), [img], *args)
    assert out.tobytes() == N.tobytes()


def test_lookup_queries_leave_few_near_ties_out():
    """tests/test_gpu_bump.py's generator: the float64 restatement alone leaves
    out at most 2 % of its queries as near-ties, every kind of triangle and
    every branch is among the rest, and the mutants differ visibly."""
    data, uv, tri_map, images = BC.lookup_mesh()
    ids, pts, dirs, nrm = BC.lookup_queries(data)
    verts, ng = BC.mesh_arrays(data)
    assert 3000 <= len(ids) <= 8000
    ref, tie = B.bump_normal(verts, ng, uv, tri_map, images, ids, pts, dirs, nrm)
    assert tie.mean() <= 0.02
    t, h, ok = B.tangent_frames(verts, ng, uv, tri_map)
    assert (h[ok] < 0).sum() >= 8 and (h[ok] > 0).sum() >= 8 and (~ok & (tri_map >= 0)).sum() == 2
    changed = np.abs(ref - nrm).max(1) > 0
    back = (nrm.astype(np.float64) * ng[ids]).sum(1) < 0
    assert (changed & back).sum() > 500 and (changed & ~back).sum() > 500
    assert (~changed & ok[ids]).sum() > 50  # mapped, but turned away from the viewer: N
    assert np.abs(np.sqrt((ref * ref).sum(1)) - 1).max() < 1e-6
    for mutant in B.MUTANTS:
        other, _ = B.bump_normal(verts, ng, uv, tri_map, images, ids, pts, dirs, nrm, mutant)
        assert np.abs(other - ref)[~tie].max() > 0.5, mutant
