"""The SAH search tree's optimisation (csrc/mcpt_sah.cpp: subtree reinsertion on
the binary tree, then the least-cost 4-wide collapse under a stack-need cap),
checked on the CPU by tests/native/sah_optimize_check.cpp, which is compiled
with mcpt_sah.cpp and the host loader alone.

For every leaf set, with the pass on and off: sah_check.cpp's invariants (every
leaf once with its own box, every slot box the exact union of its child's,
children after parents, the reported stack need), need(on) <= need(off),
collapse cost(on) <= cost(off), the same tree for 1 and 8 threads, passes = 0
equal to the call without options, and a forced cap of 1 (infeasible from three
leaves on) giving the plain tree back.  The plain cbox tree's hash is the one the
commit before the pass produced."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")

# FNV-1a over the 128-B nodes build_sah4 emitted for cbox's reference leaves before the pass existed
# (12,781 nodes, need 36), recorded from that commit's mcpt_sah.cpp
PARENT_CBOX_HASH = "9881204fd4b4c8ab"
PARENT_CBOX_NODES, PARENT_CBOX_NEED = 12781, 36

SCENES = {"cbox": ("scenes/cbox/", "cbox.obj"), "mis": ("scenes/veach_mis/", "mis.obj"),
          "dining": ("scenes/diningroom/", "diningroom.obj")}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sahopt") / "sah_optimize_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "sah_optimize_check.cpp"), os.path.join(CSRC, "mcpt_sah.cpp"),
                    os.path.join(CSRC, "mcpt_host.cpp"), "-o", out], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    print(r.stdout.strip())
    return dict(kv.split("=") for kv in r.stdout.split()[1:])


@pytest.mark.parametrize("n,seed,clustered", [(1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (5, 3, 1), (1000, 2, 1)])
def test_generated_leaves(exe, n, seed, clustered):
    f = run(exe, "gen", n, seed, clustered)
    assert int(f["need_on"]) <= int(f["need_off"])
    if n > 1:
        assert float(f["cost_on"]) <= float(f["cost_off"])
    if n == 1000:  # the pass does something here: a third of the centroids coincide, the binned build splits them by count
        assert f["optimized"] == "1" and int(f["moved"]) > 0 and float(f["cost_on"]) < float(f["cost_off"])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_leaves(exe, name):
    f = run(exe, "obj", *SCENES[name])
    assert int(f["need_on"]) <= int(f["need_off"])
    assert float(f["cost_on"]) <= float(f["cost_off"])
    assert f["optimized"] == "1" and float(f["cost_on"]) < float(f["cost_off"])
    if name == "cbox":
        assert (int(f["nodes_off"]), int(f["need_off"])) == (PARENT_CBOX_NODES, PARENT_CBOX_NEED)
        assert f["hash_off"] == PARENT_CBOX_HASH  # the pass off: the parent's bytes


def test_estimated_search_cost_cbox(exe):
    """tools/top_pop_sim.cpp's estimator with a triangle-test counter, seed 1, 30,000 camera paths of up to
    8 uniform-hemisphere bounces in cbox: node steps per segment with the pass on are at most 0.95 x off,
    triangle tests per segment at most 1.03 x off."""
    f = run(exe, "sim", *SCENES["cbox"], 278, 273, -800, 278, 273, -799, 39.3077, 30000)
    assert f["segments_on"] == f["segments_off"]
    steps = float(f["steps_on"]) / float(f["steps_off"])
    tests = float(f["tests_on"]) / float(f["tests_off"])
    print("steps on/off %.4f, tests on/off %.4f" % (steps, tests))
    assert steps <= 0.95
    assert tests <= 1.03
    assert int(f["need_on"]) <= int(f["need_off"])
