"""k_render on the 96-B exact search-tree nodes (csrc/mcpt_node96.h;
mcpt_tuning.quantized = 3) against the 128-B nodes (quantized = 2): the same
bits on every scene and launch plan, the same 96-B arrays from both upload
paths, and no bounds violation in the MCPT_DEBUG build.  Node-step and test
counts are not compared: the 96-B node permutes a node's slots, which moves
the tie-break among equal entry distances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import render as R
from montecarlopathtracing_amd import scene as S
from tests import intersect_cases as IC
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "montecarlopathtracing_amd", "lib", "libmcpt_hip_debug.so")
W = H = 64
FRAMES, DEPTH, ATTEMPT = 4, 8, 1 << 20
LATTICE_CAM = {"position": [8, 8, 30], "lookat": [8, 8, 0], "up": [0, 1, 0], "fov": 40}
SMALL_CAM = {"position": [1.5, 1, 10], "lookat": [1.5, 1, 0], "up": [0, 1, 0], "fov": 40}


def three():
    """Three triangles: the root holds three leaves and one empty slot."""
    return IC._case("three", [[(0, 0, 0), (4, 0, 1), (1, 3, 2)], [(0, 0, 3), (3, 0, 3), (0, 3, 3)],
                              [(1, 1, -1), (3, 1, -1), (1, 3, -2)]]).data


SCENES = {
    "lattice": (lambda: IC.lattice().data, LATTICE_CAM),
    "near_ties": (lambda: scenes.near_ties("cbox", 0.0), scenes.CBOX_CAM),  # forces order fallbacks
    "root_leaf": (lambda: IC.single().data, SMALL_CAM),
    "three": (three, SMALL_CAM),
    "soup": (lambda: S.random_mesh(2000, seed=7), S.RANDOM_MESH_CAMERA),
}
PLANS = [(sched, win) for sched in (L.SCHED_SINGLE, L.SCHED_PAIRED) for win in (1, 2)]


def render_all(rnd, name):
    """{(schedule, stack_window, quantized): (hist, count, seeds, stats)} of one scene."""
    get, camj = SCENES[name]
    dsc = rnd.upload(get())
    cam = S.parse_camera(camj)
    out = {}
    try:
        for sched, win in PLANS:
            for q in (2, 3):
                rnd.set_tuning(quantized=q, stack_window=win)
                rnd.drop_caches()
                rnd.set_stats(True)
                st = rnd.new_state(W, H)
                rnd.render_frames(dsc, cam, st, DEPTH, ATTEMPT, FRAMES, schedule=sched)
                s = rnd.stats()
                torch.cuda.synchronize()
                out[(sched, win, q)] = (st.hist.cpu().numpy().copy(), st.count.cpu().numpy().copy(), st.seeds_np().copy(), s)
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()
        dsc.close()
    return out


@pytest.fixture(scope="module")
def rnd96():
    r = R.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_node96_renders_same_bits(rnd96, name):
    out = render_all(rnd96, name)
    for sched, win in PLANS:
        a, b = out[(sched, win, 2)], out[(sched, win, 3)]
        tag = "%s schedule %d stack_window %d" % (name, sched, win)
        assert a[3]["node_format"] == 0 and b[3]["node_format"] == 2, tag  # the knob took: 128-B, then 96-B nodes
        assert a[3]["quantized"] == 0 and b[3]["quantized"] == 0, tag
        assert a[3]["stack_window"] == b[3]["stack_window"] == (1 if win == 1 else 0), tag
        assert a[0].tobytes() == b[0].tobytes(), tag + ": hist"
        assert np.array_equal(a[1], b[1]), tag + ": count"
        assert np.array_equal(a[2], b[2]), tag + ": seeds"
        assert a[3]["segments"] == b[3]["segments"], tag
    ref = out[(PLANS[0][0], PLANS[0][1], 2)]
    assert ref[1].max() > 0, name  # something was hit and accumulated
    if name == "near_ties":
        assert all(v[3]["order_fallbacks"] > 0 for v in out.values())
    for key, v in out.items():  # every plan the same bits as well
        assert v[0].tobytes() == ref[0].tobytes() and np.array_equal(v[2], ref[2]), (name, key)


@pytest.mark.parametrize("name", ["lattice", "three", "soup"])
def test_node96_upload_paths_same_bytes(name):
    """mcpt_scene_upload's loop and mcpt_scene_upload_device's kernels give the same near4x, tri4 and
    relabelled reference tree; tri4 holds every triangle once, under the leaf its node names."""
    data = SCENES[name][0]()
    nodes = R.treelet_gpu_device(S.build_hlbvh(data.tris))

    class Host:
        tris, mats = data.tris, data.mats
    Host.nodes = nodes
    rnd = R.Renderer(0)
    host = rnd.upload(Host)
    dev = rnd.upload((R.to_device(data.tris, 0), R.to_device(nodes, 0), data.mats))
    try:
        for k in ("near4x", "tri4", "nodes4x"):
            a, b = host.read(k), dev.read(k)
            assert len(a) > 0 or k == "nodes4x", (name, k)
            assert a.tobytes() == b.tobytes(), (name, k, len(a), len(b))
        n = len(host.read("near4x")) // 96
        assert n == len(host.read("near4")) // 128
        t4 = host.read("tri4").view(np.float32).reshape(-1, 16)
        tris = host.read("tris").view(np.float32).reshape(-1, 16)
        assert len(t4) == 4 * n
        used = np.abs(t4[:, :12]).sum(1) > 0
        ids = t4[used, 13].copy().view(np.int32)
        assert sorted(ids) == list(range(len(tris))), name  # every reference triangle exactly once
        assert np.array_equal(t4[used][:, :13].view(np.uint32), tris[ids][:, :13].view(np.uint32))
    finally:
        host.close()
        dev.close()
        rnd.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from tests import test_gpu_node96 as T
from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import render as R
rnd = R.Renderer(0)
print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
for name in sorted(T.SCENES):
    for key, v in T.render_all(rnd, name).items():
        if key[2] == 3:
            print(json.dumps({"scene": name, "plan": key[:2], "violations": v[3]["debug_violations"],
                              "node_format": v[3]["node_format"]}), flush=True)
"""


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="debug build missing (__graft_entry__.build makes it)")
def test_node96_debug_build_clean():
    """The MCPT_DEBUG build's stack, node and triangle bounds checks on the 96-B form (child ids decoded
    from plane bytes, tri4 indices from node ids): zero violations on every scene and plan."""
    env = dict(os.environ, MCPT_LIB_OVERRIDE=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert "MCPT_DEBUG" in lines[0]["version"]
    assert len(lines) == 1 + len(SCENES) * len(PLANS)
    for c in lines[1:]:
        assert c["violations"] == 0 and c["node_format"] == 2, c
