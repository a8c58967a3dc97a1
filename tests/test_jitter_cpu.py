"""Sub-pixel jitter (opt-in antialiasing), the parts that need no GPU: the ABI
mirror, the config key, the App / command-line surface, and the arithmetic of
the seeds the GPU tests plant."""
import json
import os

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# seeds whose first two 15-bit draws are both 0 (tests/test_gpu_jitter.py plants them)
ZERO_DRAW_SEEDS = (0xfc77a683, 0x8d6a4dc2, 0x7c77a683, 0x0d6a4dc2)


def lcg(s):
    """shade.cl's generator on uint32 arrays: s * 1103515245 + 12345 mod 2^32."""
    return ((np.asarray(s, np.uint64) * np.uint64(1103515245) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def jitter_draws(seeds):
    """The jittered frame start's two draws: (jx, jy, seeds after), jx = the
    first 15-bit draw * 2^-15 (exact in float32), jy the second."""
    s1 = lcg(seeds)
    s2 = lcg(s1)
    scale = np.float32(2.0 ** -15)
    jx = ((s1 >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.float32) * scale
    jy = ((s2 >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.float32) * scale
    return jx, jy, s2


def _entry(**extra):
    e = {"bvhtype": "hlbvh", "width": 32, "height": 32, "platform": "amd",
         "directory": os.path.join(ROOT, "scenes", "cbox") + "/", "objname": "cbox.obj",
         "maxdepth": 4, "attempt": 3, "raygenerator": "", "intersect": "", "shade": "",
         "camera": {"position": [278, 273, -800], "lookat": [278, 273, -799], "up": [0, 1, 0],
                    "fov": 39.3077, "resolution": [32, 32]},
         "opencl": True}
    e.update(extra)
    return {"configid": 0, "config": [e]}


def test_planted_seeds_draw_zero_offsets():
    jx, jy, after = jitter_draws(np.array(ZERO_DRAW_SEEDS, np.uint32))
    assert (jx == 0).all() and (jy == 0).all()
    assert (after != np.array(ZERO_DRAW_SEEDS, np.uint32)).all()
    # and the draw is in [0, 1), exact: 15 bits scaled by a power of two
    jx, jy, _ = jitter_draws(np.arange(1 << 16, dtype=np.uint32) * np.uint32(2654435761))
    assert 0 <= jx.min() and jx.max() < 1 and 0 <= jy.min() and jy.max() < 1
    assert ((jx.astype(np.float64) * 32768) % 1 == 0).all()


def test_render_params_end_with_jitter_and_abi_5():
    assert L.RenderParams._fields_[-1][0] == "jitter"
    assert L.RenderParams().jitter == 0  # a zero-initialised struct: off
    assert L.ABI_VERSION == 5
    assert L.SIGNATURES["mcpt_generate_rays_jittered"][1] == L.SIGNATURES["mcpt_generate_rays"][1][:4] + [
        L._P] + L.SIGNATURES["mcpt_generate_rays"][1][4:]
    hdr = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in hdr


def test_config_reads_jitter_key_default_false(tmp_path):
    assert C.Config(_entry()).JITTER() is False
    assert C.Config(_entry(jitter=True)).JITTER() is True
    assert C.Config(_entry(jitter=False)).JITTER() is False
    with pytest.raises(ValueError):
        C.Config(_entry(jitter=2))
    # the committed config.json's entries are the reference's: none asks for jitter
    root = C.Config(os.path.join(ROOT, "config.json")).root
    for i in range(len(root["config"])):
        assert C.Config(root, configid=i).JITTER() is False
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(_entry(jitter=True)) + "\n# a comment, as the reference's parser allows\n")
    assert C.Config(str(path)).JITTER() is True


def test_app_takes_jitter_from_config_or_argument():
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).jitter is False
    assert App(C.Config(_entry(jitter=True))).jitter is True
    assert App(C.Config(_entry()), jitter=True).jitter is True    # --jitter forces it on
    assert App(C.Config(_entry(jitter=True)), jitter=None).jitter is True


def test_command_line_parses_jitter():
    from montecarlopathtracing_amd.__main__ import parser
    assert parser().parse_args(["cfg.json"]).jitter is False
    a = parser().parse_args(["cfg.json", "--jitter", "--frames", "3"])
    assert a.jitter is True and a.frames == 3 and a.config == "cfg.json"
