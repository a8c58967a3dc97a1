"""The 96-B exact search-tree node (csrc/mcpt_node96.h) on the CPU: the
stand-alone program tests/native/node96_check.cpp over the cbox tree, a
500-triangle soup and hand-made nodes of every slot pattern, built plain and
under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def cbox_leaves(tmp_path_factory):
    """The reference leaves of cbox as mcpt::LeafRef records: box = (minx maxx miny maxy minz maxz), triangle."""
    nodes = scenes.cbox().nodes
    leaf = nodes[nodes["left"] == nodes["right"]]
    rec = np.zeros(len(leaf), np.dtype([("box", np.float32, 6), ("tri", np.int32)]))
    rec["box"][:, 0::2] = leaf["bbmin"][:, :3]
    rec["box"][:, 1::2] = leaf["bbmax"][:, :3]
    rec["tri"] = leaf["left"]
    assert sorted(rec["tri"]) == list(range(len(scenes.cbox().tris)))
    path = str(tmp_path_factory.mktemp("node96") / "cbox_leaves.bin")
    rec.tofile(path)
    return path


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_node96_check(tmp_path, cbox_leaves, flags):
    """Leaf boxes bit-equal; internal planes outward by at most 256 floats on the
    three id floats, one float on a flat axis (both sides), exact elsewhere; ids
    and leaf records decode back; every triangle once in tri4; over 1 M slab
    tests with zero and denormal direction components and origins on box planes:
    a slot passes whenever the exact slot does, leaf slots agree bit for bit,
    empty slots are never entered."""
    exe = str(tmp_path / "node96_check")
    subprocess.run(["g++", "-std=c++17", "-pthread", "-Wall", "-ffp-contract=off"] + flags +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "native", "node96_check.cpp"),
                    os.path.join(CSRC, "mcpt_sah.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, cbox_leaves], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "\nok slab_tests=" in out.stdout and "scene: nodes=" in out.stdout, out.stdout + out.stderr
