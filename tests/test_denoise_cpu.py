"""The denoise post-pass (mcpt_denoise), the parts that need no GPU: the ABI
mirror, the config key, the App / command-line surface, and properties of the
float64 reference (tests/denoise_ref.py) the GPU tests compare against."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C

from . import denoise_ref as D
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 29


def test_config_reads_denoise_key_default_false():
    assert C.Config(_entry()).DENOISE() is False
    assert C.Config(_entry(denoise=True)).DENOISE() is True
    assert C.Config(_entry(denoise=False)).DENOISE() is False
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError):
            C.Config(_entry(denoise=bad))
    root = C.Config(os.path.join(ROOT, "config.json")).root
    for i in range(len(root["config"])):
        assert "denoise" not in root["config"][i]
        assert C.Config(root, configid=i).DENOISE() is False


def test_command_line_parses_denoise():
    from montecarlopathtracing_amd.__main__ import parser
    assert parser().parse_args(["cfg.json"]).denoise is False
    a = parser().parse_args(["cfg.json", "--denoise", "--preview", "p.png"])
    assert a.denoise is True and a.preview == "p.png" and a.jitter is False


def test_app_takes_denoise_from_config_or_argument():
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).denoise is False
    assert App(C.Config(_entry(denoise=True))).denoise is True
    assert App(C.Config(_entry()), denoise=True).denoise is True
    assert App(C.Config(_entry(denoise=True)), denoise=None).denoise is True
    assert App.denoised_path("out/cbox.obj.hdr") == "out/cbox.obj_denoised.hdr"


def test_denoise_params_struct_and_signature(tmp_path):
    assert ctypes.sizeof(L.DenoiseParams) == 16
    assert [f for f, _ in L.DenoiseParams._fields_] == ["iterations", "sigma_normal", "sigma_plane", "sigma_color"]
    res, args = L.SIGNATURES["mcpt_denoise"]
    assert res is L._I32 and args == [L._P, L._P, L._P, L._P, L._P, L._I32, L._I32, L._P, L._P, L._P]
    assert L.ABI_VERSION == 5  # a new struct and a new entry point change no existing one
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpt_hip.h"\nint main(void) { '
                   'printf("%zu %zu %zu %d\\n", sizeof(mcpt_denoise_params), offsetof(mcpt_denoise_params, sigma_normal), '
                   'offsetof(mcpt_denoise_params, sigma_color), MCPT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, L.DenoiseParams.sigma_normal.offset, L.DenoiseParams.sigma_color.offset, 5]
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "mcpt_denoise")


def test_render_defaults_are_the_documented_ones():
    from montecarlopathtracing_amd import render as R
    assert set(R.DENOISE_DEFAULTS) == {"iterations", "sigma_normal", "sigma_plane", "sigma_color"}
    assert 0 <= R.DENOISE_DEFAULTS["iterations"] <= 8
    assert R.DENOISE_DEFAULTS["sigma_normal"] > 0 and R.DENOISE_DEFAULTS["sigma_plane"] > 0
    assert R.DENOISE_DEFAULTS["sigma_color"] >= 0


# ------------------------------------------------ the reference's own properties
PARAMS = dict(iterations=5, sigma_normal=0.5, sigma_plane=0.05, sigma_color=0.0)


def _ref(hits, hist, count, **kw):
    return D.denoise_ref(hits, hist, count, D.synthetic_mats(), D.SYN_DIAG, W, H, **dict(PARAMS, **kw))


def test_synthetic_case_has_every_kind_of_pixel():
    hits, hist, count = D.synthetic_case(W, H)
    mats = D.synthetic_mats()
    filt = D.filtered_mask(hits, mats)
    mid = hits["material_id"]
    assert filt.any() and (~filt).any()
    for m in range(len(mats)):
        assert (mid == m).any(), m
    assert (mid >= len(mats)).sum() == 2 and (hits["t"] == D.FLT_MAX).any()
    assert not filt[mid >= 2].any() and not filt[hits["t"] == D.FLT_MAX].any()
    assert filt[(mid < 2) & (hits["t"] < D.FLT_MAX)].all()
    assert 0.4 < (count == 0).mean() < 0.6 and count.max() == 5
    assert np.isnan(hits["normal"][~filt]).any()  # garbage guides on the misses
    assert abs(D.SYN_DIAG - np.sqrt(200.0)) < 1e-12


def test_reference_keeps_a_constant_image_constant():
    hits, hist, count = D.synthetic_case(W, H)
    hist[:, :3] = np.array([0.25, 0.5, 0.75], np.float32)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    for sc in (0.0, 1.0):
        out = _ref(hits, hist, count, sigma_color=sc)
        assert np.abs(out[filt, :3] - np.array([0.25, 0.5, 0.75])).max() < 1e-14
        assert (out[filt, 3] == 0).all()


def test_reference_all_counts_zero_stays_zero():
    hits, hist, count = D.synthetic_case(W, H, all_zero=True)
    out = _ref(hits, hist, count)
    assert np.isfinite(out).all() and (out == 0).all()
    # and with colours under the zero counts: no tap counts, every colour stays, no NaN
    hits, hist, _ = D.synthetic_case(W, H)
    out = _ref(hits, hist, count, sigma_color=1.0)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    assert np.isfinite(out).all() and (out[filt, :3] == hist[filt, :3]).all() and (out[filt, 3] == 0).all()


def test_reference_passes_through_and_zero_iterations_copy():
    hits, hist, count = D.synthetic_case(W, H)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    out = _ref(hits, hist, count)
    assert (out[~filt] == hist[~filt]).all()
    assert (out[filt, :3] != hist[filt, :3]).any()
    assert (_ref(hits, hist, count, iterations=0) == hist).all()
    # a pass-through pixel is no tap: changing its colour, count or guides changes no other pixel
    hist2, count2, hits2 = hist.copy(), count.copy(), hits.copy()
    hist2[~filt] = 1e6
    count2[~filt] = 1000
    hits2["normal"][~filt] = 0.0
    hits2["point"][~filt] = 0.0
    assert (_ref(hits2, hist2, count2)[filt] == out[filt]).all()


def test_reference_notices_dropped_corner_taps():
    hits, hist, count = D.synthetic_case(W, H)
    filt = D.filtered_mask(hits, D.synthetic_mats())
    full = _ref(hits, hist, count)
    dropped = D.denoise_ref(hits, hist, count, D.synthetic_mats(), D.SYN_DIAG, W, H, drop_corners=True, **PARAMS)
    assert D.rel_err(dropped, full, filt) > 1e-3
    assert D.rel_err(full.astype(np.float32), full, filt) < 1e-7
