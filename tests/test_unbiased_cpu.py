"""The opt-in estimator (counted history, Russian roulette), the parts that
need no GPU: the ABI mirror, the config keys and command line with every
refusal, the Python layer's refusal of roulette without the counted history,
and the restatement's own sanity cases (tests/unbiased_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import config as C

from . import unbiased_ref as U
from .test_jitter_cpu import _entry
from .test_jitter_cpu import lcg as lcg_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ 1: the surface
def test_abi_mirror_has_the_estimator_struct_and_entry_points():
    assert ctypes.sizeof(L.Estimator) == 16
    assert [f[0] for f in L.Estimator._fields_] == ["count_all", "rr_depth", "pad"]
    e = L.Estimator()
    assert (e.count_all, e.rr_depth) == (0, 0)  # a zero-initialised struct: off
    rl, re = L.SIGNATURES["mcpt_render_frames_lens"][1], L.SIGNATURES["mcpt_render_frames_est"][1]
    assert re == rl[:4] + [L._P] + rl[4:]
    sh, se = L.SIGNATURES["mcpt_shade"][1], L.SIGNATURES["mcpt_shade_est"][1]
    assert se == sh[:8] + [L._I32] + sh[8:]
    assert L.SIGNATURES["mcpt_accumulate_all"] == L.SIGNATURES["mcpt_accumulate"]
    hdr = open(os.path.join(ROOT, "include", "mcpt_hip.h")).read()
    assert "#define MCPT_ABI_VERSION 5" in hdr and L.ABI_VERSION == 5
    for name in ("typedef struct mcpt_estimator", "mcpt_render_frames_est(", "mcpt_shade_est(", "mcpt_accumulate_all("):
        assert name in hdr


def test_config_reads_the_estimator_keys():
    c = C.Config(_entry())
    assert c.UNBIASED() is False and c.ROULETTE() == 0
    assert C.Config(_entry(unbiased=True)).UNBIASED() is True
    assert C.Config(_entry(unbiased=True)).ROULETTE() == 0
    assert C.Config(_entry(unbiased=False)).UNBIASED() is False
    assert C.Config(_entry(roulette=True)).ROULETTE() == 3
    assert C.Config(_entry(roulette=False)).ROULETTE() == 0
    assert C.Config(_entry(roulette=False)).UNBIASED() is False
    assert C.Config(_entry(roulette=1)).ROULETTE() == 1
    assert C.Config(_entry(roulette=7, unbiased=True)).ROULETTE() == 7
    assert C.Config(_entry(roulette=65535)).ROULETTE() == 65535
    # the committed config.json's entries are the reference's: none changes the estimator
    root = C.Config(os.path.join(ROOT, "config.json")).root
    for i in range(len(root["config"])):
        c = C.Config(root, configid=i)
        assert c.UNBIASED() is False and c.ROULETTE() == 0


@pytest.mark.parametrize("depth", [True, 1, 3, 64])
def test_roulette_key_implies_unbiased(depth):
    assert C.Config(_entry(roulette=depth)).UNBIASED() is True
    with pytest.raises(ValueError, match="roulette"):
        C.Config(_entry(roulette=depth, unbiased=False))


@pytest.mark.parametrize("bad", [0, -1, -3, 65536, 2.0, 2.5, "3", "on", [3], None, {"depth": 3}], ids=repr)
def test_config_refuses_a_bad_roulette_key(bad):
    with pytest.raises(ValueError, match="roulette"):
        C.Config(_entry(roulette=bad))


@pytest.mark.parametrize("bad", [0, 1, "yes", None, 1.0, [True]], ids=repr)
def test_config_refuses_a_bad_unbiased_key(bad):
    with pytest.raises(ValueError, match="unbiased"):
        C.Config(_entry(unbiased=bad))


def test_app_takes_the_estimator_from_config_or_argument():
    from montecarlopathtracing_amd.app import App
    plain = App(C.Config(_entry()))
    assert plain.unbiased is False and plain.roulette == 0
    assert App(C.Config(_entry(unbiased=True))).unbiased is True
    a = App(C.Config(_entry(roulette=True)))
    assert a.unbiased is True and a.roulette == 3
    b = App(C.Config(_entry()), unbiased=True)
    assert b.unbiased is True and b.roulette == 0
    c = App(C.Config(_entry()), roulette=5)
    assert c.unbiased is True and c.roulette == 5  # roulette switches the counted history on
    d = App(C.Config(_entry(roulette=5)), roulette=2)
    assert d.roulette == 2  # the argument wins
    e = App(C.Config(_entry(roulette=5)), roulette=False)
    assert e.roulette == 0 and e.unbiased is False  # roulette off again: the default estimator
    f = App(C.Config(_entry(roulette=5, unbiased=True)), roulette=False)
    assert f.roulette == 0 and f.unbiased is True   # the entry's own "unbiased" key stays
    g = App(C.Config(_entry(roulette=5)), roulette=False, unbiased=True)
    assert g.roulette == 0 and g.unbiased is True
    with pytest.raises(ValueError, match="unbiased"):
        App(C.Config(_entry()), roulette=3, unbiased=False)
    for bad in (0, -2, 1.5, "3"):
        with pytest.raises(ValueError, match="roulette"):
            App(C.Config(_entry()), roulette=bad)


def test_command_line_maps_to_the_app_arguments():
    from montecarlopathtracing_amd.__main__ import cli_estimator, parser
    p = parser()
    assert cli_estimator(p.parse_args(["cfg.json"])) == (None, None)  # the entry's keys decide
    assert cli_estimator(p.parse_args(["cfg.json", "--unbiased"])) == (True, None)
    a = p.parse_args(["cfg.json", "--roulette"])
    assert cli_estimator(a) == (True, True) and a.config == "cfg.json"  # --roulette switches --unbiased on
    a = p.parse_args(["--roulette", "5", "cfg.json", "--frames", "3"])
    assert cli_estimator(a) == (True, 5) and a.config == "cfg.json" and a.frames == 3
    assert cli_estimator(p.parse_args(["--unbiased", "--roulette", "1"])) == (True, 1)
    with pytest.raises(SystemExit):
        p.parse_args(["--roulette", "2.5"])
    # and as App takes them
    from montecarlopathtracing_amd.app import App
    u, r = cli_estimator(p.parse_args(["--roulette"]))
    app = App(C.Config(_entry()), unbiased=u, roulette=r)
    assert app.unbiased is True and app.roulette == 3
    u, r = cli_estimator(p.parse_args([]))
    app = App(C.Config(_entry(roulette=4)), unbiased=u, roulette=r)
    assert app.unbiased is True and app.roulette == 4
    # what passes the command line still has to pass the key's checks
    u, r = cli_estimator(p.parse_args(["--roulette", "0"]))
    with pytest.raises(ValueError, match="roulette"):
        App(C.Config(_entry()), unbiased=u, roulette=r)
    assert "--unbiased" in p.format_help() and "--roulette" in p.format_help()


def test_renderer_refuses_roulette_without_unbiased_before_any_c_call():
    from montecarlopathtracing_amd import render as R
    rnd = R.Renderer.__new__(R.Renderer)  # no context: the refusal comes first
    with pytest.raises(ValueError, match="unbiased"):
        rnd.render_frames(None, None, None, 1, 1, 1, roulette=3)
    with pytest.raises(ValueError, match="unbiased"):
        rnd.render_frames(None, None, None, 1, 1, 1, unbiased=False, roulette=True)
    with pytest.raises(ValueError, match="roulette"):
        rnd.render_frames(None, None, None, 1, 1, 1, unbiased=True, roulette="3")
    assert R._estimator_struct(False, 0) is None  # the default estimator: the call of before
    e = R._estimator_struct(True, 0)
    assert (e.count_all, e.rr_depth) == (1, 0)
    e = R._estimator_struct(True, True)
    assert (e.count_all, e.rr_depth) == (1, 3)
    e = R._estimator_struct(True, 64)
    assert (e.count_all, e.rr_depth) == (1, 64)


# --------------------------------------------------- 2: the restatement itself
def test_lcg_restatement_and_its_inverse():
    seeds = (np.arange(512, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5EED)
    nxt = lcg_np(seeds)
    for s, n in zip(seeds[:64], nxt[:64]):
        s2, d = U.lcg(s)
        assert s2 == int(n) and d == (int(n) >> 16) & 0x7FFF and 0 <= d < 32768
        assert U.lcg_back(s2) == int(s)
    assert U.lcg(0) == (12345, 0)  # shade.cl:1-6 on seed 0
    for k in (1, 3, 4):
        for v in (0, 1, 16384, 32767):
            s = U.seed_for_kth_draw(v, k)
            after, ds = U.draws(s, k)
            assert ds[-1] == v and U.steps_between(s, after) == k
    assert U.steps_between(5, 5) == 0 and U.steps_between(5, 6, limit=8) is None


def test_survival_probability_and_the_exact_decision():
    f = np.float32
    assert U.survival_probability((0.2, 0.5, 0.3)) == f(0.5)
    assert U.survival_probability((0, 0, 0)) == 0
    assert U.survival_probability((2, 0.1, 0.1)) == 1          # clamped
    assert U.survival_probability((0.1, 0.1, 1.0)) == 1
    below_one = np.nextafter(f(1), f(0))
    assert U.survival_probability((below_one, 0, 0)) == below_one
    # p = 0 always ends the path, p = 1 never does
    assert not any(U.survives(d, 0.0) for d in (0, 1, 32767))
    assert all(U.survives(d, 1.0) for d in (0, 1, 32767))
    # the edge: u < p is strict
    assert U.survives(0, f(2.0 ** -15)) and not U.survives(1, f(2.0 ** -15))
    assert U.survives(16383, 0.5) and not U.survives(16384, 0.5)
    assert U.survives(32767, below_one) and U.survives(8191, 0.25) and not U.survives(8192, 0.25)
    # the expected weight of a survivor is one: sum over all 2^15 draws of [u < p] / p
    for p in (f(0.25), f(0.5), f(0.8), below_one):
        alive = sum(U.survives(d, p) for d in range(32768))
        assert abs(alive / 32768.0 / float(p) - 1) <= 2.0 ** -15 / float(p)


def _mat(type_, kd=(0, 0, 0), ks=(0, 0, 0)):
    m = np.zeros(1, L.MATERIAL)
    m["type"] = type_
    m["kd"][0, :3] = kd
    m["ka_ks"][0, :3] = ks
    return m[0]


def test_predict_applies_only_where_the_rule_says():
    diffuse = _mat(L.MCPT_DIFFUSE, kd=(0.5, 0.25, 0.1))
    seed = U.seed_for_kth_draw(16383, 3)  # two shading draws, then u just below 0.5
    v = U.predict(diffuse, seed, depth_before=2, rr_depth=3, max_depth=8)
    assert v.applies and v.survives and v.p == np.float32(0.5) and v.steps == 3 and v.seed == U.draws(seed, 3)[0]
    v = U.predict(diffuse, U.seed_for_kth_draw(16384, 3), 2, 3, 8)
    assert v.applies and not v.survives and v.steps == 3
    # below rr_depth, roulette off, or ended by the cap: no draw
    for depth_before, rr, cap in ((1, 3, 8), (0, 3, 8), (2, 0, 8), (2, 3, 3)):
        v = U.predict(diffuse, seed, depth_before, rr, cap)
        assert not v.applies and v.steps == 2 and v.seed == U.draws(seed, 2)[0]
    assert U.predict(diffuse, seed, 2, 3, 3).survives is False  # the cap ended it
    # the texture factor scales kd
    v = U.predict(diffuse, seed, 2, 3, 8, tex=(0.5, 1, 1))
    assert v.p == np.float32(0.25) and not v.survives
    # glossy: R is ks where the coin took the Phong lobe, else kd
    glossy = _mat(L.MCPT_GLOSSY, kd=(0.25, 0.25, 0.25), ks=(0.75, 0.5, 0.5))
    odd, even = U.seed_for_kth_draw(1, 1), U.seed_for_kth_draw(2, 1)
    assert U.predict(glossy, odd, 0, 1, 8).p == np.float32(0.75) and U.predict(glossy, odd, 0, 1, 8).steps == 4
    assert U.predict(glossy, even, 0, 1, 8).p == np.float32(0.25)
    # lights and unknown materials: nothing drawn
    assert U.predict(_mat(L.MCPT_LIGHT, ks=(5, 5, 5)), seed, 5, 1, 8) == U.Verdict(False, True, None, 0, seed)
    assert U.predict(_mat(7), seed, 5, 1, 8).applies is False
    assert U.predict(_mat(L.MCPT_TRANSPARENT), seed, 5, 1, 8).applies is False


def test_counted_mean_counts_the_zero_samples():
    rng = np.random.default_rng(5)
    n, px = 8, 33
    samples = rng.uniform(0, 4, (n, px, 4)).astype(np.float32)
    samples[..., 3] = 0
    samples[rng.uniform(size=(n, px)) < 0.6] = 0  # most samples are black
    S, mean, M = U.counted_mean(samples)
    assert S.shape == (px, 4) and M == float(samples.max())
    hist, cnt = U.counted_history_f32(samples, 100)
    assert cnt == n
    assert np.abs(hist - mean).max() <= 3 * n * 2.0 ** -23 * M  # the GPU test's bound holds for the float32 recurrence
    # the default history is another number wherever a zero sample fell
    nz = (samples[..., :3] != 0).any(axis=2).sum(axis=0)
    some_zero = (nz > 0) & (nz < n)
    assert some_zero.any()
    default = S[some_zero] / nz[some_zero][:, None]
    assert (np.abs(default - mean[some_zero]).max(axis=1) > 1e-3).all()
    # the stop at max_attempt
    hist5, cnt5 = U.counted_history_f32(samples, 5)
    assert cnt5 == 5 and np.abs(hist5 - samples[:5].astype(np.float64).mean(axis=0)).max() <= 3 * 5 * 2.0 ** -23 * M
    # a pixel that is all black stays black and is still counted
    z = np.zeros((4, 3, 4), np.float32)
    h, c = U.counted_history_f32(z, 10)
    assert c == 4 and not h.any()
