"""Smooth shading, host half (no GPU): the vertex-normal generator against its
float64 restatement (tests/smooth_ref.py), the OBJ `vn` parser, both under
AddressSanitizer in a stand-alone program, and the "smooth" key's way through
Config, App and the command line."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C
from montecarlopathtracing_amd import scene as S

from . import smooth_ref as R
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -23  # one float32 step at 1: the generator rounds a float64 unit vector once (half a step) and its
# double arithmetic may order the sum's additions as the restatement does not (far below the other half)


def packed(verts):
    v = np.asarray(verts, np.float32)
    t = np.zeros(len(v), L.TRIANGLE)
    t["v"][:, :, :3] = v
    return S.pack_triangles(t, np.zeros(len(v), np.int32))


def face_normals(p):
    return np.repeat(p["normal"][:, None, :3], 3, axis=1)


def check_against_ref(p, crease):
    got = S.vertex_normals(p, crease)
    ref = R.vertex_normals(p, crease)
    flat_ref = ref.view(np.uint32) == face_normals(p).view(np.uint32)
    # where the flat rule applies the bits are the face normal's
    assert np.array_equal(got.view(np.uint32)[flat_ref], ref.view(np.uint32)[flat_ref])
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)).max(initial=0.0) <= ULP
    return got


def test_cube_is_flat_at_crease_40():
    p = packed(R.cube())
    got = check_against_ref(p, 40.0)
    assert np.array_equal(got.view(np.uint32), face_normals(p).view(np.uint32))


@pytest.mark.parametrize("fold,smooth", [(30.0, True), (50.0, False)])
def test_hinged_quads_smooth_below_the_crease_only(fold, smooth):
    p = packed(R.hinge(fold))
    got = check_against_ref(p, 40.0)
    on_hinge = np.abs(p["v"][:, :, 0]) < 1e-6  # corners on the shared edge x = 0
    changed = (got.view(np.uint32) != face_normals(p).view(np.uint32)).any(2)
    assert not changed[~on_hinge].any()
    assert changed[on_hinge].all() == smooth and changed[on_hinge].any() == smooth
    if smooth:  # both sides of the hinge agree on the normal there
        h = got[on_hinge]
        assert np.abs(h - h[0]).max() <= 2 * ULP


def test_unindexed_duplicate_vertices_weld_and_negative_zero_is_zero():
    v = R.icosphere(0)  # 20 triangles, every vertex repeated in five of them
    v[v == 0] = 0.0
    w = v.copy()
    w[::2][w[::2] == 0] = -0.0  # every other triangle spells its zeros -0
    a, b = check_against_ref(packed(v), 80.0), check_against_ref(packed(w), 80.0)
    assert np.array_equal(a, b)  # (as values: a -0 in the input may sign a zero of the output)
    assert (a.view(np.uint32) != face_normals(packed(v)).view(np.uint32)).any(2).all()  # every corner blended


def test_degenerate_triangle_joins_nothing_and_keeps_its_normal():
    v = list(R.hinge(10.0))
    v.append(np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2]], np.float32))  # zero area, on the hinge
    p = packed(np.array(v))
    assert not np.isfinite(p["normal"][-1, :3]).all()
    got = check_against_ref(p, 40.0)
    assert np.array_equal(got[-1].view(np.uint32), face_normals(p)[-1].view(np.uint32))
    assert np.array_equal(got[:-1].view(np.uint32), S.vertex_normals(p[:-1], 40.0).view(np.uint32))


def test_half_the_faces_wound_the_other_way():
    v = R.icosphere(1)
    v[::2] = v[::2][:, ::-1]
    p = packed(v)
    got = check_against_ref(p, 60.0)
    # an oppositely wound neighbour is excluded: every vertex normal stays on its own face's side
    assert ((got * face_normals(p)).sum(2) > 0.5).all()


def test_icosphere_80_vertex_normals_are_radial():
    v = R.icosphere(1)
    assert len(v) == 80
    got = check_against_ref(packed(v), 60.0).astype(np.float64)
    cosang = np.clip((got * R.radial(v)).sum(2) / np.sqrt((got * got).sum(2)), -1, 1)
    # by symmetry exact; float64 restatement: 9e-7 degrees
    assert np.degrees(np.arccos(cosang)).max() <= 1e-4


def test_icosphere_320_lookup_beats_the_face_normal_fourfold():
    v = R.icosphere(2)
    assert len(v) == 320
    p = packed(v)
    vn = S.vertex_normals(p, 60.0).astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(7))
    k = 50
    b = rng.dirichlet((1.0, 1.0, 1.0), (len(v), k))
    pts = np.einsum("tkc,tcx->tkx", b, v.astype(np.float64)).reshape(-1, 3)
    rep = lambda a: np.repeat(np.asarray(a, np.float64), k, axis=0)  # noqa: E731
    ng = rep(p["normal"][:, :3])
    ns, bad = R.shading_normal(rep(v[:, 0]), rep(v[:, 1]), rep(v[:, 2]), ng, rep(vn[:, 0]), rep(vn[:, 1]), rep(vn[:, 2]),
                               pts, -R.radial(pts))
    assert not bad.any()
    ang = lambda a: np.degrees(np.arccos(np.clip((a * R.radial(pts)).sum(1), -1, 1))).max()  # noqa: E731
    smooth, flat = ang(ns), ang(ng)
    print("smooth %.3f deg, flat %.3f deg" % (smooth, flat))  # measured 0.59 and 10.4
    assert smooth < flat / 4


# ------------------------------------------------------------------ OBJ normals
CUBE_OBJ = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vn 0 0 -2
vn 0 3 0
vn 1 1 0
f 1//1 2//1 3//1
f 1/9/1 3/9/2 4/9/3
f -4//-3 -3//-1 -2//-2
f 1//1 2 3//1
f 1//1 2//2 3//3 4//1
f 1 2 3
f 1/1 2/1 3/1
"""


def load_normals(tmp_path, text, name="m.obj"):
    (tmp_path / name).write_text(text)
    return S.load_obj_normals(str(tmp_path) + "/", name)


def test_obj_vn_forms(tmp_path):
    vn, has = load_normals(tmp_path, CUBE_OBJ)
    tris, _, _ = S.load_object(str(tmp_path) + "/", "m.obj")
    assert len(vn) == len(tris) == 8  # the polygon fans into two, in mcpt_load_obj's order
    n1, n2, n3 = [0, 0, -1], [0, 1, 0], [math.sqrt(0.5), math.sqrt(0.5), 0]
    f32 = lambda rows: np.array(rows, np.float64).astype(np.float32)  # noqa: E731
    assert has.tolist() == [True, True, True, False, True, True, False, False]
    assert np.array_equal(vn[0], f32([n1, n1, n1]))          # v//vn
    assert np.array_equal(vn[1], f32([n1, n2, n3]))          # v/vt/vn, normalised in double
    assert np.array_equal(vn[2], f32([n1, n3, n2]))          # negative indices
    assert not vn[3].any()                                   # one corner lacks its vn
    assert np.array_equal(vn[4], f32([n1, n2, n3]))          # polygon: (0, 1, 2)
    assert np.array_equal(vn[5], f32([n1, n3, n1]))          # then (0, 2, 3)
    # the polygon's triangles are mcpt_load_obj's
    assert np.array_equal(tris["v"][4, :, :3], [[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    assert np.array_equal(tris["v"][5, :, :3], [[0, 0, 0], [1, 1, 0], [0, 1, 0]])


@pytest.mark.parametrize("face", ["f 1//4 2//1 3//1", "f 1//-4 2//1 3//1", "f 1//1 2//1 0//1"])
def test_obj_vn_index_out_of_range_is_a_parse_error(tmp_path, face):
    with pytest.raises(L.MCPTError, match="-4"):
        load_normals(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 0\nvn 1 0 0\n" + face + "\n")


def test_obj_vn_of_zero_length_is_no_normal(tmp_path):
    vn, has = load_normals(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 0\nf 1//1 2//1 3//1\n")
    assert has.tolist() == [False] and not vn.any()


@pytest.mark.parametrize("d,obj", [("cbox", "cbox.obj"), ("veach_mis", "mis.obj"), ("diningroom", "diningroom.obj")])
def test_shipped_scenes_have_no_vn_and_load_obj_is_unchanged(d, obj):
    directory = os.path.join(ROOT, "scenes", d) + "/"
    tris, _, idx = S.load_object(directory, obj)
    g = np.load(os.path.join(GOLD, "tinyobj_%s.npz" % d))
    v = np.ascontiguousarray(tris["v"][:, :, :3].reshape(-1, 9))
    assert np.array_equal(v.view(np.uint32), g["verts"].view(np.uint32)) and np.array_equal(idx, g["matids"])
    vn, has = S.load_obj_normals(directory, obj)
    assert len(vn) == len(tris) and not has.any()


def test_smooth_normals_prefers_authored(tmp_path):
    vn, has = load_normals(tmp_path, "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0.6 0.8\nf 1//1 2//1 3//1\nf 1 3 4\n")
    tris, _, _ = S.load_object(str(tmp_path) + "/", "m.obj")
    p = S.pack_triangles(tris, np.zeros(len(tris), np.int32))
    out = S.smooth_normals(p, 40.0, (vn, has))
    assert np.array_equal(out[0], vn[0]) and np.array_equal(out[1], S.vertex_normals(p, 40.0)[1])


def test_generator_refuses_a_crease_outside_0_180():
    p = packed(R.cube())
    for bad in (-1.0, 180.5, float("nan")):
        with pytest.raises(L.MCPTError):
            S.vertex_normals(p, bad)


def cap_fan(m, slope):
    """m triangles around the apex (0, 0, 1): a cone whose sides fall `slope`
    per unit radius (a shallow cap: a sphere's pole; a steep one: a spire)."""
    a = 2.0 * math.pi * np.arange(m + 1) / m
    ring = np.stack([np.cos(a), np.sin(a), np.full(m + 1, 1.0 - slope)], axis=1)
    apex = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (m, 3))
    return np.stack([apex, ring[:-1], ring[1:]], axis=1).astype(np.float32)


@pytest.mark.parametrize("slope", [0.05, 1.0], ids=["pole", "spire"])
def test_high_valence_vertex_against_the_restatement(slope):
    """A vertex of 300 corners: the shallow cap takes the one-cone path (every
    normal within half the crease of the mean), the spire the pairwise one; both
    are the pairwise rule's values."""
    p = packed(cap_fan(300, slope))
    got = check_against_ref(p, 40.0)
    apex = got[:, 0].astype(np.float64)
    if slope < 0.5:  # every face joins: one normal, the axis
        assert np.abs(apex - apex[0]).max() == 0 and np.abs(apex[0] - [0, 0, 1]).max() < 1e-6
    else:  # only the faces within 40 degrees join: each apex normal leans with its own face
        assert (np.abs(apex[:, 2] - apex[0, 2]) < 1e-6).all() and 0.5 < apex[0, 2] < 0.9


def test_generator_at_scale_with_shared_vertices():
    """A 300 x 300 bumpy grid (179,402 triangles, valence 6) plus a pole shared
    by 100,000 corners: the weld is a sort and the pole one sum, so this is
    work for a second, not for the 10^10 pair tests a pairwise pole would be."""
    n = 300
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    pts = np.stack([x, y, 0.3 * np.sin(0.2 * x) * np.cos(0.15 * y)], axis=2).astype(np.float32)
    a, b, c, d = pts[:-1, :-1], pts[1:, :-1], pts[1:, 1:], pts[:-1, 1:]
    grid = np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])
    pole = cap_fan(100_000, 0.02) - np.float32([4.0, 4.0, 0.0])  # beside the grid, where float32 still tells its ring points apart
    p = packed(np.concatenate([grid, pole]))
    vn = S.vertex_normals(p, 40.0)
    g, f = vn[:len(grid)], face_normals(p)[:len(grid)]
    assert np.isfinite(vn).all() and np.abs(np.sqrt((vn.astype(np.float64) ** 2).sum(2)) - 1).max() < 1e-6
    assert (g.view(np.uint32) != f.view(np.uint32)).any(2).mean() > 0.9  # blended nearly everywhere
    assert ((g * f).sum(2) > 0.99).all()                                 # and close to its face on this gentle surface
    apex = vn[len(grid):, 0]
    assert (apex.view(np.uint32) == apex[0].view(np.uint32)).all() and abs(float(apex[0, 2]) - 1) < 1e-5


def test_generator_bounds_the_pairwise_work():
    """65,537 corners at one vertex with normals spread beyond half the crease:
    refused (MCPT_ERR_LIMIT) instead of 4 x 10^9 pair tests; 180 degrees would be
    the same spread, while the shallow cap of the same size passes (above)."""
    p = packed(cap_fan(65_537, 1.0))
    with pytest.raises(L.MCPTError, match=r"mcpt error -5\b.*65536"):
        S.vertex_normals(p, 40.0)
    with pytest.raises(L.MCPTError, match=r"mcpt error -5\b"):
        S.vertex_normals(p, 0.0)  # crease 0 is pairwise too (bit-equal normals only)


# ------------------------------------------------------- sanitizers (stand-alone)
def test_smooth_host_code_under_address_sanitizer(tmp_path):
    """mcpt_vertex_normals and the OBJ normal parser in a stand-alone program
    built here with -fsanitize=address,undefined: truncated and malformed OBJ
    text, out-of-range indices, empty and degenerate meshes, every input and
    output in a heap block of exactly its size (tests/native/smooth_check.cpp)."""
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    exe = str(tmp_path / "smooth_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "smooth_check.cpp"),
                         os.path.join(csrc, "mcpt_host.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------ config, App, CLI
def test_abi_mirror_declares_the_smooth_entry_points():
    assert L.ABI_VERSION == 5  # functions only: the revision stays
    so = L.lib()
    for name in ("mcpt_vertex_normals", "mcpt_load_obj_normals", "mcpt_obj_normals_from_text",
                 "mcpt_scene_set_vertex_normals", "mcpt_shading_normals"):
        assert name in L.SIGNATURES and hasattr(so, name)
    assert ctypes.sizeof(L.RenderParams) == 13 * 4  # mcpt_render_params gained no field


def test_config_reads_the_smooth_key():
    assert C.Config(_entry()).SMOOTH() is None
    assert C.Config(_entry(smooth=False)).SMOOTH() is None
    assert C.Config(_entry(smooth=True)).SMOOTH() == 40.0 == C.DEFAULT_CREASE == S.DEFAULT_CREASE
    assert C.Config(_entry(smooth=25)).SMOOTH() == 25.0
    assert C.Config(_entry(smooth=0)).SMOOTH() == 0.0
    assert C.Config(_entry(smooth=180.0)).SMOOTH() == 180.0


@pytest.mark.parametrize("bad", ["yes", [40], {"crease": 40}, None, -1, 180.5, float("nan"), float("inf")])
def test_config_refuses_invalid_smooth(bad):
    with pytest.raises(ValueError):
        C.Config(_entry(smooth=bad))


def test_committed_config_has_no_smooth_key():
    root = C.loads(open(os.path.join(ROOT, "config.json")).read())
    assert all("smooth" not in e for e in root["config"])


def test_app_takes_smooth_from_config_or_argument():
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).smooth is None
    assert App(C.Config(_entry(smooth=True))).smooth == 40.0
    assert App(C.Config(_entry()), smooth=True).smooth == 40.0
    assert App(C.Config(_entry(smooth=True)), smooth=30).smooth == 30.0
    assert App(C.Config(_entry(smooth=True)), smooth=False).smooth is None
    with pytest.raises(ValueError):
        App(C.Config(_entry()), smooth=200)


def test_command_line_smooth_flag():
    from montecarlopathtracing_amd.__main__ import cli_smooth, parser
    plain, keyed = C.Config(_entry()), C.Config(_entry(smooth=55))
    assert cli_smooth(parser().parse_args([]), plain) is None
    assert cli_smooth(parser().parse_args([]), keyed) == 55.0
    assert cli_smooth(parser().parse_args(["--smooth"]), plain) == 40.0
    assert cli_smooth(parser().parse_args(["--smooth", "20"]), keyed) == 20.0
    assert cli_smooth(parser().parse_args(["cfg.json", "--smooth"]), plain) == 40.0
    with pytest.raises(ValueError):
        cli_smooth(parser().parse_args(["--smooth", "181"]), plain)
