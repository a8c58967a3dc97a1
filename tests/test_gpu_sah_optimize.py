"""k_render over the optimised SAH search tree (csrc/mcpt_sah.cpp: subtree
reinsertion, collapse under the plain tree's stack need; Renderer.set_sah_optimize)
against the plain tree from the same library: the tree only sets the search's
cost, so images, counts and seed chains are the same bits for every node format,
both equal the reference kernels where those are built, both upload paths emit
the same bytes, and cbox keeps its stack layout and resident waves."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from montecarlopathtracing_amd import render as R  # noqa: E402
from montecarlopathtracing_amd import scene as S  # noqa: E402

from . import intersect_cases as IC  # noqa: E402
from . import refgpu, scenes  # noqa: E402

needs_ref = pytest.mark.skipif(not refgpu.available(), reason="oracle/_ref not built (needs /root/reference at build time)")

W = H = 64
FRAMES, DEPTH, ATTEMPT = 3, 4, 4  # max_attempt 4: one the reference's history kernel is built for
LATTICE_CAM = {"position": [8, 8, 30], "lookat": [8, 8, 0], "up": [0, 1, 0], "fov": 40}
SCENES = {
    "soup": (lambda: S.random_mesh(500, seed=11), S.RANDOM_MESH_CAMERA),
    "lattice": (lambda: IC.lattice().data, LATTICE_CAM),  # axis-aligned quads: flat boxes, coincident planes
    "cbox": (scenes.cbox, scenes.CBOX_CAM),
}
FORMATS = {2: "128-B", 3: "96-B", 1: "quantized"}  # mcpt_tuning.quantized, forced
NODE_FORMAT = {2: 0, 3: 2, 1: 1}  # what stats()["node_format"] then reports


@pytest.fixture(scope="module")
def rnd():
    r = R.Renderer(0)
    yield r
    R.Renderer.set_sah_optimize(3)
    r.close()


def _render(rnd, dsc, camjson, quantized):
    rnd.set_tuning(quantized=quantized)
    try:
        rnd.drop_caches()
        rnd.set_stats(True)
        st = rnd.new_state(W, H, R.default_seeds(W * H))
        rnd.render_frames(dsc, S.parse_camera(camjson), st, DEPTH, ATTEMPT, FRAMES)
        stats = rnd.stats()
        torch.cuda.synchronize()
        return st.hist.cpu().numpy().copy(), st.count.cpu().numpy().copy(), st.seeds_np().copy(), stats
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()


@pytest.fixture(scope="module")
def rendered(rnd):
    """{scene: {(passes, quantized): (hist, count, seeds, stats)}, "trees": {(scene, passes): near4 bytes}}"""
    out, trees = {}, {}
    try:
        for name, (get, camjson) in SCENES.items():
            out[name] = {}
            for passes in (0, 3):
                R.Renderer.set_sah_optimize(passes)
                assert R.Renderer.sah_optimize() == passes
                dsc = rnd.upload(get())
                try:
                    trees[(name, passes)] = (dsc.read("near4").tobytes(), dsc.read("meta").copy())
                    for q in FORMATS:
                        out[name][(passes, q)] = _render(rnd, dsc, camjson, q)
                finally:
                    dsc.close()
    finally:
        R.Renderer.set_sah_optimize(3)
    out["trees"] = trees
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_pass_on_renders_same_bits_as_off(rendered, name):
    res = rendered[name]
    for q, fmt in FORMATS.items():
        off, on = res[(0, q)], res[(3, q)]
        tag = "%s, %s nodes" % (name, fmt)
        assert off[3]["node_format"] == on[3]["node_format"] == NODE_FORMAT[q], tag  # the forced format took
        assert off[1].max() > 0, tag  # something was hit and accumulated
        assert off[0].tobytes() == on[0].tobytes(), tag + ": hist"
        assert np.array_equal(off[1], on[1]), tag + ": count"
        assert np.array_equal(off[2], on[2]), tag + ": seeds"
        assert off[3]["segments"] == on[3]["segments"], tag
    ref = res[(0, 2)]
    for key, v in res.items():  # every format the same bits as well
        assert v[0].tobytes() == ref[0].tobytes() and np.array_equal(v[2], ref[2]), (name, key)


def test_pass_changes_the_tree_not_the_plan(rendered):
    """cbox: the pass gives another tree (or the test above compares a tree with itself), of no larger
    stack need, and k_render runs it with the same stack layout and as many resident waves."""
    (t_off, m_off), (t_on, m_on) = rendered["trees"][("cbox", 0)], rendered["trees"][("cbox", 3)]
    assert t_off != t_on
    assert m_on[1] <= m_off[1]  # stack_depth4
    for q in FORMATS:
        off, on = rendered["cbox"][(0, q)][3], rendered["cbox"][(3, q)][3]
        assert on["stack_window"] == off["stack_window"] == 0, FORMATS[q]  # the whole stack in LDS
        assert on["workgroups"] == off["workgroups"], FORMATS[q]
        assert on["top_levels"] == off["top_levels"], FORMATS[q]
    for name in ("soup", "lattice"):
        assert rendered["trees"][(name, 3)][1][1] <= rendered["trees"][(name, 0)][1][1], name


@needs_ref
@pytest.mark.parametrize("name", sorted(SCENES))
def test_both_trees_equal_the_reference_kernels(rendered, name):
    get, camjson = SCENES[name]
    rh, rc, rs = refgpu.render(get(), S.parse_camera(camjson), W, H, DEPTH, FRAMES, ATTEMPT, R.default_seeds(W * H))
    for key, v in rendered[name].items():
        assert np.array_equal(v[1], rc), (name, key, "count")
        assert np.array_equal(v[2], rs), (name, key, "seeds")
        assert v[0].tobytes() == np.ascontiguousarray(rh).tobytes(), (name, key, "hist")


def test_upload_paths_same_bytes_with_the_pass_on(rnd):
    """mcpt_scene_upload and mcpt_scene_upload_device call the one host function on the same leaves: every
    array of the soup is the same bytes, and the tree is the optimised one."""
    soup = SCENES["soup"][0]()

    class data:  # what DeviceScene reads of a SceneData, over the HLBVH layout the device path expects
        tris, mats, nodes = soup.tris, soup.mats, S.build_hlbvh(soup.tris)
    R.Renderer.set_sah_optimize(0)
    try:
        plain = rnd.upload(data)
        plain_tree = plain.read("near4").tobytes()
        plain.close()
    finally:
        R.Renderer.set_sah_optimize(3)
    host = rnd.upload(data)
    dev = rnd.upload((R.to_device(data.tris, 0), R.to_device(data.nodes, 0), data.mats))
    try:
        assert host.read("near4").tobytes() != plain_tree
        for k in R.DeviceScene.ARRAYS + ("meta",):
            a, b = host.read(k), dev.read(k)
            assert a.tobytes() == b.tobytes(), (k, len(a), len(b))
    finally:
        host.close()
        dev.close()
