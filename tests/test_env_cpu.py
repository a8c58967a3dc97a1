"""Environment lighting (opt-in; mcpt_scene_set_environment), the parts that
need no GPU: the Radiance RGBE reader (mcpt_decode_hdr) against the committed
stb goldens and on malformed files, the same under AddressSanitizer in a
stand-alone program, the "environment" config key with the App / command-line
surface, and the float64 reference of the lookup (tests/env_ref.py)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C
from montecarlopathtracing_amd import scene as S

from . import env_ref
from .test_jitter_cpu import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def _golden(name):
    with open(os.path.join(GOLD, name + ".hdr"), "rb") as fh:
        return fh.read()


# ------------------------------------------------------------------ decoder
@pytest.mark.parametrize("name", ["stb_synthetic", "stb_narrow"])
def test_decoder_reencodes_to_the_golden_bytes(name):
    data = _golden(name)
    img = S.decode_hdr(data)
    assert img.dtype == np.float32 and img.ndim == 3 and img.shape[2] == 3
    assert S.read_hdr(os.path.join(GOLD, name + ".hdr")).tobytes() == img.tobytes()
    rgba = np.zeros(img.shape[:2] + (4,), np.float32)
    rgba[..., :3] = img
    assert S.encode_hdr(rgba, flip=False) == data  # rows are in file order: no flip on the way back


@pytest.mark.parametrize("name", ["stb_synthetic", "stb_narrow"])
def test_decoder_within_one_mantissa_step_of_the_writers_input(name):
    """The golden file is stbi_write_hdr (flipping) of the committed input:
    RGBE truncates each channel to 8 bits under the texel's shared exponent
    e, so 0 <= input - decoded < 2^(e - 136), one mantissa step; a texel the
    writer zeroed (e = 0: its largest channel below 1e-32) decodes to 0."""
    src = np.load(os.path.join(GOLD, name + "_input.npy")).astype(np.float32)
    src = src[::-1, :, :3]  # flipped as the writer flips; the file has no alpha
    img = S.decode_hdr(_golden(name))
    assert img.shape == src.shape
    mx = src.max(axis=2)
    coded = mx >= np.float32(1e-32)
    _, e = np.frexp(mx.astype(np.float64))       # the writer's exponent: byte e + 128
    step = np.ldexp(1.0, e - 8)[..., None]       # 2^((e + 128) - 136)
    diff = src.astype(np.float64) - img.astype(np.float64)
    assert (img[~coded] == 0).all()
    assert (diff[coded] >= 0).all() and (diff[coded] < np.broadcast_to(step, diff.shape)[coded]).all()
    assert coded.any() and (img > 0).any()


def _rle_file(res, body):
    return HEAD + res + bytes(body)


RLE_BODY = [2, 2, 0, 8, 0x88, 10, 0x88, 20, 0x88, 30, 8, 128, 128, 128, 128, 129, 129, 129, 129]


def _patched(idx, value):
    b = list(RLE_BODY)
    b[idx] = value
    return b


def test_decoder_reads_rle_and_flat_scanlines():
    img = S.decode_hdr(_rle_file(b"-Y 1 +X 8\n", RLE_BODY))
    assert img.shape == (1, 8, 3)
    assert img[0, 0].tolist() == [10 / 256, 20 / 256, 30 / 256] and img[0, 7].tolist() == [10 / 128, 20 / 128, 30 / 128]
    flat = HEAD + b"-Y 1 +X 8\n" + b"".join(bytes([k + 1, 0, 0, 136]) for k in range(8))
    assert S.decode_hdr(flat)[0, :, 0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert S.decode_hdr(HEAD + b"-Y 1 +X 1\n" + bytes([128, 64, 0, 0])).tolist() == [[[0, 0, 0]]]  # e == 0: black


MALFORMED = {
    "run longer than the scanline": _rle_file(b"-Y 1 +X 8\n", _patched(4, 0x89)),
    "literal run longer than the scanline": _rle_file(b"-Y 1 +X 8\n", _patched(10, 9)),
    "run of zero length": _rle_file(b"-Y 1 +X 8\n", _patched(4, 0x80)),
    "scanline width disagrees with the header": _rle_file(b"-Y 1 +X 8\n", _patched(3, 9)),
    "second scanline not RLE": _rle_file(b"-Y 2 +X 8\n", RLE_BODY + [1, 2, 3, 4]),
    "no magic": b"FORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\nabcd",
    "wrong magic": b"#?RADIANT\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\nabcd",
    "no FORMAT line": b"#?RADIANCE\n\n-Y 1 +X 1\nabcd",
    "other format": b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\nabcd",
    "+Y resolution": HEAD + b"+Y 1 +X 1\nabcd",
    "zero width": HEAD + b"-Y 1 +X 0\nabcd",
    "negative height": HEAD + b"-Y -1 +X 1\nabcd",
    "trailing text": HEAD + b"-Y 1 +X 1 junk\nabcd",
    "product beyond 2^26": HEAD + b"-Y 8193 +X 8192\nabcd",
    "product overflowing int32": HEAD + b"-Y 2147483647 +X 2147483647\nabcd",
    "no empty line": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n-Y 1 +X 1\nabcd",
    "empty": b"",
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_decoder_refuses_malformed_input(what):
    with pytest.raises(L.MCPTError):
        S.decode_hdr(MALFORMED[what])


def test_decoder_refuses_every_truncation_of_the_narrow_file():
    data = _golden("stb_narrow")
    assert S.decode_hdr(data).size > 0
    for n in range(len(data)):
        with pytest.raises(L.MCPTError):
            S.decode_hdr(data[:n])


def test_decoder_under_address_sanitizer(tmp_path):
    """The same cases (and every fifth truncation of the RLE golden) in a
    stand-alone program built here with -fsanitize=address,undefined (no
    recovery; the flags tests/native/Makefile gives host_asan), inputs and
    outputs in heap blocks of exactly their size (tests/native/hdr_decode_check.cpp)."""
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    exe = str(tmp_path / "hdr_asan")
    cc = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
                         "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                         os.path.join(ROOT, "tests", "native", "hdr_decode_check.cpp"),
                         os.path.join(csrc, "mcpt_host.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------- ABI mirror, config
def test_abi_mirror_declares_the_environment_entry_points():
    assert L.ABI_VERSION == 5  # a new struct with new entry points: the revision stays
    assert ctypes_size(L.Environment) == 40
    for name in ("mcpt_scene_set_environment", "mcpt_env_eval", "mcpt_decode_hdr"):
        assert name in L.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in hdr and "typedef struct mcpt_environment" in hdr


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_config_reads_both_environment_forms():
    assert C.Config(_entry()).ENVIRONMENT() is None
    e = C.Config(_entry(environment={"color": [0.5, 1, 2]})).ENVIRONMENT()
    assert e == {"scale": (0.5, 1.0, 2.0), "map": None, "rotate": 0.0}
    e = C.Config(_entry(environment={"map": "sky.hdr"})).ENVIRONMENT()
    assert e == {"scale": (1.0, 1.0, 1.0), "map": "sky.hdr", "rotate": 0.0}
    e = C.Config(_entry(environment={"map": "sky.hdr", "scale": 2, "rotate": 37})).ENVIRONMENT()
    assert e == {"scale": (2.0, 2.0, 2.0), "map": "sky.hdr", "rotate": 37.0}
    e = C.Config(_entry(environment={"map": "a/sky.hdr", "scale": [1, 0, 0.25], "rotate": -90.5})).ENVIRONMENT()
    assert e == {"scale": (1.0, 0.0, 0.25), "map": "a/sky.hdr", "rotate": -90.5}
    assert C.Config(_entry(environment={"color": [0, 0, 0]})).ENVIRONMENT()["scale"] == (0.0, 0.0, 0.0)
    # the committed config.json's entries are the reference's: none has an environment
    root = C.Config(os.path.join(ROOT, "config.json")).root
    for i in range(len(root["config"])):
        assert C.Config(root, configid=i).ENVIRONMENT() is None


@pytest.mark.parametrize("bad", [
    True, [1, 1, 1], "sky.hdr", {},
    {"color": [1, 1]}, {"color": 1}, {"color": [1, 1, "1"]}, {"color": [1, 1, True]}, {"color": [1, -0.5, 1]},
    {"color": [1, 1, float("inf")]}, {"color": [1, float("nan"), 1]}, {"color": [1, 1, 1], "rotate": 3},
    {"color": [1, 1, 1], "map": "sky.hdr"},
    {"map": 3}, {"map": ""}, {"map": "sky.hdr", "scale": -1}, {"map": "sky.hdr", "scale": [1, 1]},
    {"map": "sky.hdr", "scale": "2"}, {"map": "sky.hdr", "scale": [1, -1, 1]}, {"map": "sky.hdr", "scale": float("inf")},
    {"map": "sky.hdr", "rotate": "90"}, {"map": "sky.hdr", "rotate": float("nan")}, {"map": "sky.hdr", "rotate": None},
    {"map": "sky.hdr", "colour": [1, 1, 1]}, {"scale": 2}, {"map": "sky.hdr", "scale": None},
], ids=repr)
def test_config_refuses_invalid_environment(bad):
    with pytest.raises(ValueError):
        C.Config(_entry(environment=bad))


def test_config_environment_from_a_file_with_json_infinity(tmp_path):
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(_entry(environment={"color": [1, 1, 1]})).replace("[1, 1, 1]", "[1, Infinity, 1]"))
    with pytest.raises(ValueError):
        C.Config(str(path))


def test_app_takes_environment_from_config_or_argument():
    from montecarlopathtracing_amd.app import App
    assert App(C.Config(_entry())).environment is None
    assert App(C.Config(_entry(environment={"color": [1, 2, 3]}))).environment["scale"] == (1.0, 2.0, 3.0)
    over = App(C.Config(_entry(environment={"color": [1, 2, 3]})), environment={"map": "sky.hdr", "rotate": 5})
    assert over.environment == {"scale": (1.0, 1.0, 1.0), "map": "sky.hdr", "rotate": 5.0}
    with pytest.raises(ValueError):
        App(C.Config(_entry()), environment={"color": [1, 2]})


def test_command_line_environment_flags():
    from montecarlopathtracing_amd.__main__ import cli_environment, parser
    plain = C.Config(_entry())
    mapped = C.Config(_entry(environment={"map": "sky.hdr", "scale": 2, "rotate": 10}))
    a = parser().parse_args(["cfg.json"])
    assert (a.env, a.env_map, a.env_scale, a.env_rotate) == (None, None, None, None)
    assert cli_environment(a, plain) is None and cli_environment(a, mapped) is None  # the entry's own stands
    a = parser().parse_args(["cfg.json", "--env", "0.5,1,2"])
    assert cli_environment(a, mapped) == {"color": [0.5, 1.0, 2.0]}
    a = parser().parse_args(["cfg.json", "--env-map", "sky.hdr", "--env-scale", "3", "--env-rotate", "-45"])
    assert cli_environment(a, plain) == {"map": os.path.abspath("sky.hdr"), "scale": 3.0, "rotate": -45.0}
    a = parser().parse_args(["cfg.json", "--env-scale", "1,2,3"])
    assert cli_environment(a, mapped) == {"map": "sky.hdr", "scale": [1.0, 2.0, 3.0], "rotate": 10.0}
    for argv in (["--env", "1,2"], ["--env", "a,b,c"], ["--env", "1,1,1", "--env-map", "x.hdr"],
                 ["--env", "1,1,1", "--env-rotate", "3"], ["--env-map", "x.hdr", "--env-scale", "1,2"]):
        with pytest.raises(ValueError):
            cli_environment(parser().parse_args(["cfg.json"] + argv), plain)
    with pytest.raises(ValueError):
        cli_environment(parser().parse_args(["cfg.json", "--env-rotate", "3"]), plain)  # nothing to rotate
    # every result is a valid config key
    assert C.parse_environment(cli_environment(parser().parse_args(["c", "--env", "0,0,0"]), plain))["scale"] == (0.0,) * 3


# ----------------------------------------------------------- the reference
def _dirs(az_deg, el=0.0):
    """Unit vectors at azimuth az (atan2(x, -z)) and elevation el, degrees."""
    az, el = np.radians(np.atleast_1d(az_deg).astype(np.float64)), np.radians(el)
    return np.stack([np.sin(az) * np.cos(el), np.full_like(az, np.sin(el)), -np.cos(az) * np.cos(el)], axis=1)


def _random_dirs(n, seed=5):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def test_reference_one_texel_map_is_the_constant():
    d = _random_dirs(500)
    one = np.array([[[0.25, 1.5, 3.0]]], np.float32)
    got = env_ref.env_radiance(d, (2.0, 1.0, 0.5), one, rotate_deg=37.0)
    want = env_ref.env_radiance(d, (0.5, 1.5, 1.5))
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * 3.0
    assert (got[:, 3] == 0).all() and (want[:, 3] == 0).all()


def test_reference_poles_read_the_first_and_last_row():
    m = env_ref.smooth_map(7, 5).astype(np.float64)
    m[0], m[-1] = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]  # constant rows: any column mix reads the row's value
    up = env_ref.env_radiance([[0, 1, 0], [1e-9, 1, -1e-9]], texels=m)
    down = env_ref.env_radiance([[0, -1, 0]], texels=m, rotate_deg=123.0)
    assert np.allclose(up[:, :3], [1, 2, 3], rtol=0, atol=1e-12)
    assert np.allclose(down[:, :3], [4, 5, 6], rtol=0, atol=1e-12)


def test_reference_is_continuous_across_the_seam():
    """atan2 = +pi and -pi are one direction: d.x = +0 and -0 at d.z > 0 read
    the same value (u = 1 and u = 0, columns width - 1 and 0 wrapped)."""
    m = env_ref.smooth_map(7, 5)
    for el in (-60.0, 0.0, 35.0):
        c = math.cos(math.radians(el))
        plus = env_ref.env_radiance([[0.0, math.sin(math.radians(el)), c]], texels=m)
        minus = env_ref.env_radiance([[-0.0, math.sin(math.radians(el)), c]], texels=m)
        assert np.abs(plus - minus).max() <= 1e-12
        near = env_ref.env_radiance(_dirs([180.0 - 1e-7, -180.0 + 1e-7], el), texels=m)
        assert np.abs(near[0] - near[1]).max() <= 1e-6
        # and the clamp instead of the wrap is another function there
        assert np.abs(env_ref.env_radiance(_dirs([179.9], el), texels=m, wrap=False)
                      - env_ref.env_radiance(_dirs([179.9], el), texels=m)).max() > 1e-3


def test_reference_full_turn_is_no_rotation():
    m = env_ref.smooth_map(64, 32)
    d = _random_dirs(2000)
    a = env_ref.env_radiance(d, texels=m, rotate_deg=0.0)
    b = env_ref.env_radiance(d, texels=m, rotate_deg=360.0)
    # float64 rounding: sin(2 pi) in double is -2.4e-16, which stays that size as a float; times the map's slope
    assert np.abs(a - b).max() <= 1e-9
    # a quarter turn about +Y moves the lookup: the map is not read where it was
    assert np.abs(a - env_ref.env_radiance(d, texels=m, rotate_deg=90.0)).max() > 0.1
    # rotate = 90 at direction +X reads what rotate = 0 reads at d' = (c d.x + s d.z, d.y, -s d.x + c d.z)
    c, s = env_ref.rotation(90.0)
    dx = np.array([[1.0, 0.0, 0.0]])
    moved = np.array([[c * 1.0, 0.0, -s * 1.0]])
    assert np.abs(env_ref.env_radiance(dx, texels=m, rotate_deg=90.0) - env_ref.env_radiance(moved, texels=m)).max() <= 1e-12


def test_reference_texel_centres_and_bilinear_midpoints():
    """x = u * width - 0.5: a direction through a texel's centre reads that
    texel alone, one midway between two centres their mean."""
    w, h = 8, 4
    m = env_ref.smooth_map(w, h).astype(np.float64)
    for j in range(h):
        el = 90.0 - (j + 0.5) * 180.0 / h
        for i in range(w):
            az = ((i + 0.5) / w - 0.5) * 360.0
            got = env_ref.env_radiance(_dirs([az], el), texels=m)[0, :3]
            assert np.abs(got - m[j, i]).max() <= 1e-9
            mid = env_ref.env_radiance(_dirs([az + 180.0 / w], el), texels=m)[0, :3]
            assert np.abs(mid - 0.5 * (m[j, i] + m[j, (i + 1) % w])).max() <= 1e-9
    assert env_ref.smooth_map(64, 32).min() > 0
