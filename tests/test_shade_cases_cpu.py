"""CPU checks of tests/shade_cases.py: the inputs of
tests/test_gpu_shade_edges.py are what they claim to be, and the float64
restatement of shade.cl and history.cl agrees with the CPU oracle (the plain-C
restatement, oracle.shade / oracle.accumulate) wherever it claims to decide.

The float baseline that test_gpu_shade_edges uses where the reference kernels
are absent is measured here (test_oracle_gives_the_float64_answer).
"""
import numpy as np
import pytest

from montecarlopathtracing_amd import _lib as L

from . import oracle
from . import shade_cases as SC

needs_oracle = pytest.mark.skipif(not oracle.available(), reason="oracle/liboracle.so not built")


@pytest.fixture(scope="module")
def f64s():
    return [SC.shade_f64(b) for b in SC.batches()]


def flags_of(rays):
    return rays["origin"][:, 3].view(np.uint32)


def test_generators_are_deterministic():
    SC.batches.cache_clear()
    first = SC.batches()
    SC.batches.cache_clear()
    for a, b in zip(first, SC.batches()):
        assert a.family == b.family and a.max_depth == b.max_depth
        for x, y in zip(a[1:6], b[1:6]):
            assert x.tobytes() == y.tobytes()
    for a, b in zip(SC.accumulate_cases(), SC.accumulate_cases()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_batches_keep_the_rules():
    lengths = []
    for b in SC.batches():
        k = len(b.rays)
        lengths.append(k)
        assert 1 <= k <= 4000 and k % 2 == 1 and k % 64 != 0
        assert len(b.hits) == k and b.colors.shape == (k, 4) and b.seeds.shape == (k,) and b.seeds.dtype == np.uint32
        assert (b.hits["material_id"] < len(b.mats)).all()
        assert (b.hits["triangle_id"] == 0).all()
        for a in (b.rays["origin"][:, :3], b.rays["direction"][:, :3], b.hits["normal"], b.hits["point"], b.hits["t"],
                  b.colors, b.mats["kd"], b.mats["ka_ks"], b.mats["Ni"], b.mats["Ns"]):
            assert np.isfinite(a).all()
        assert (b.rays["direction"][:, 3].view(np.int32) == np.arange(k)).all()
        assert (b.mats["Ni"] != 0).all()
        assert 1 <= b.max_depth <= 16
        if b.family != "dead/miss":
            assert SC.live(b.rays).all()
    assert 1 in lengths
    assert {b.family for b in SC.batches()} == set(SC.FAMILIES)
    assert sorted(b.max_depth for b in SC.batches() if b.family == "depth") == [1, 8]


def _first_draws(seeds, n):
    out = []
    for s in seeds:
        s, row = int(s), []
        for _ in range(n):
            s, v = SC.lcg(s)
            row.append(v)
        out.append(row)
    return np.array(out)


def test_diffuse_normals_reach_what_they_name():
    b = SC.batches()[0]
    assert b.family == "diffuse/normals" and (b.mats["type"] == L.MCPT_DIFFUSE).all()
    n = b.hits["normal"][:, :3]
    d = b.rays["direction"][:, :3]
    assert ((n.astype(np.float64) * d).sum(1) <= 0).all()  # face-forward
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for a in range(3):
        for s in (1.0, -1.0):
            want = np.zeros(3, np.float32)
            want[a] = s
            assert (n == want).all(1).any()
    z = n[:, 2]
    assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any()
    for k in SC.TINY_K:
        e = np.ldexp(np.float32(1), -k)
        for first in (0, 1):  # (+-1, 0, +-2^-k) and (0, +-1, +-2^-k)
            for sz in (e, -e):
                assert ((np.abs(n[:, first]) == 1) & (n[:, 1 - first] == 0) & (z == sz)).any(), (k, first)
    # from k = 64 on the first cross product of (+-1, 0, +-2^-k) underflows: normalize's rescaling branch
    tiny = (np.abs(n[:, 0]) == 1) & (n[:, 1] == 0) & (z != 0) & (np.abs(z) <= 2.0 ** -64)
    c = np.cross(np.array([1.0, 0, 0]), n[tiny].astype(np.float64))
    assert tiny.sum() >= 6 * 4 and ((c * c).sum(1) < 2.0 ** -126).all() and ((c * c).sum(1) > 0).all()
    draws = _first_draws(b.seeds, 2)
    for a in SC.ANGLE_DRAWS:
        assert (draws[:, 0] == a).any()
        for r in SC.RADIUS_DRAWS:
            assert ((draws[:, 0] == a) & (draws[:, 1] == r)).any()
    kd = b.mats["kd"][b.hits["material_id"]]
    assert (kd[:, :3] == 0).any(1).any() and (kd == 0).all(1).any()
    assert ((kd[:, 3] != 0) & (b.colors == 1).all(1)).any()  # kd.w against the chain's starting colour (1, 1, 1, 1)


def test_glossy_lobe_reaches_what_it_names(f64s):
    i = [b.family for b in SC.batches()].index("glossy/lobe")
    b, f = SC.batches()[i], f64s[i]
    assert (b.mats["type"] == L.MCPT_GLOSSY).all()
    nd = (b.hits["normal"][:, :3].astype(np.float64) * b.rays["direction"][:, :3]).sum(1)
    assert (nd <= -SC.MIN_COS).all()  # the hard condition: the normal faces the ray
    for c in SC.GLOSSY_COS:
        assert (np.abs(-nd - np.float32(c)) <= 1e-6 * c).any(), c
    ns = b.mats["Ns"][b.hits["material_id"]]
    for v in SC.GLOSSY_NS:
        sel = ns == np.float32(v)
        assert (f.branch[sel] == SC.LOBE).any() and (f.branch[sel] == SC.GLOSSY_DIFFUSE).any(), v
    assert ((ns < 0) | (ns > 65536)).any()  # the ocml fallback of cl_pow_lobe
    ks = b.mats["ka_ks"][b.hits["material_id"]]
    assert (ks[:, :3] == 0).any(1).any()
    assert 1 <= f.draws.max() <= SC.MAX_DRAWS and (f.draws[f.branch == SC.LOBE] > 1).any()  # the loop did reject
    # grazing incidence rejects about every other draw
    graze = (f.branch == SC.LOBE) & (-nd < 2.0 ** -8)
    assert f.draws[graze].mean() > 1.5


def _pairs(b):
    return b.hits["material_id"], flags_of(b.rays) & np.uint32(SC.INSIDE)


def test_glass_reaches_what_it_names(f64s):
    fam = [b.family for b in SC.batches()]
    for name, nis in (("glass", SC.GLASS_NI), ("glass/extreme", SC.EXTREME_NI)):
        b, f = SC.batches()[fam.index(name)], f64s[fam.index(name)]
        assert (b.mats["type"] == L.MCPT_TRANSPARENT).all()
        assert (b.mats["Ni"] == np.array(nis, np.float32)).all()
        m, bits = _pairs(b)
        exact = (b.rays["direction"][:, :3] == -b.hits["normal"][:, :3]).all(1)
        draws = _first_draws(b.seeds, 1)[:, 0]
        for k in range(len(nis)):
            for v in SC.INSIDE_BITS:
                sel = (m == k) & (bits == v)
                assert sel.sum() >= 20 and (sel & exact).any(), (name, k, v)
                assert (sel & (draws == 0)).any() and (sel & (draws == 32767)).any()
        cos_i = -(b.hits["normal"][:, :3].astype(np.float64) * b.rays["direction"][:, :3]).sum(1)
        assert (cos_i < 2.0 ** -9).any() and (cos_i > 0.999).any()
        for br in (SC.TIR, SC.TRANSMIT, SC.REFLECT):
            assert (f.branch == br).sum() >= 20, (name, br)
    assert 1.0 in SC.GLASS_NI and SC.GLASS_NI[1] == 1.0 + 2.0 ** -23 and {0.75, 0.5} <= set(SC.GLASS_NI)
    # glass/critical: both signs of temp at every (Ni, side) pair, none of them decided by much
    b, f = SC.batches()[fam.index("glass/critical")], f64s[fam.index("glass/critical")]
    m, bits = _pairs(b)
    pairs = SC.critical_pairs()
    assert len(pairs) == 5 * 3 + 3  # Ni > 1 from inside (three bit patterns), Ni < 1 from outside
    for k, ni, v in pairs:
        t = f.temp[(m == k) & (bits == v)]
        assert (t < 0).any() and (t >= 0).any(), (ni, hex(v))
        assert np.abs(t).min() < 1e-6 * max(1.0, SC._eta(ni, v != 0) ** 2)
    # glass/fresnel: the coin on both sides of the threshold, draws next to fresnel * 32768
    b, f = SC.batches()[fam.index("glass/fresnel")], f64s[fam.index("glass/fresnel")]
    assert set(np.unique(f.branch)) == {SC.TRANSMIT, SC.REFLECT}
    assert (f.margin < 2.0 / 32768).mean() > 0.5 and (f.margin <= SC.MARGIN).any()
    on = f.margin == 0  # the coin drawn on the threshold itself (Ni = 1: 0, Ni = 3: 0.25): `>=` transmits
    assert on.sum() == 6 * 4 * 2 and (f.branch[on] == SC.TRANSMIT).all()
    assert set(b.mats["Ni"][b.hits["material_id"][on]]) == {1.0, 3.0}


def test_light_depth_dead_unknown_reach_what_they_name(f64s):
    fam = [b.family for b in SC.batches()]
    b = SC.batches()[fam.index("light")]
    ka, col = b.mats["ka_ks"], b.colors
    assert (ka == 0).all(1).any() and (ka == np.float32(2.0 ** -140)).any() and (ka == np.float32(2.0 ** 100)).any()
    assert ((ka[:, :3] == 0).all(1) & (ka[:, 3] == 1)).any()
    den = (np.abs(col) > 0) & (np.abs(col) < np.float32(2.0 ** -126))
    assert den.any() and (col == np.float32(2.0 ** 100)).any()
    for b in (x for x in SC.batches() if x.family == "depth"):
        low, bits = flags_of(b.rays) & np.uint32(0xFFFF), flags_of(b.rays) & np.uint32(SC.INSIDE)
        md = b.max_depth
        for v in {max(md - 2, 0), md - 1} | {md, md + 5}:
            assert ((low == v) & (bits != 0)).any() and ((low == v) & (bits == 0)).any(), (md, v)
        if md >= 2:
            assert (low == md - 2).any()
    b, f = SC.batches()[fam.index("dead/miss")], f64s[fam.index("dead/miss")]
    dead = ~SC.live(b.rays)
    assert dead[::3].all() and not dead[1::3].any() and not dead[2::3].any()
    assert (b.colors[dead].view(np.uint8) == SC.SENTINEL).all()
    assert len({int(v) for v in flags_of(b.rays)[dead]}) == 3
    assert (f.branch[dead] == SC.SKIPPED).all()
    t = b.hits["t"][~dead]
    assert (t == SC.FLT_MAX).sum() >= 50 and (t == np.nextafter(SC.FLT_MAX, np.float32(0))).sum() >= 50
    assert ((f.branch == SC.MISS) == (~dead & (b.hits["t"] == SC.FLT_MAX))).all()
    b, f = SC.batches()[fam.index("unknown")], f64s[fam.index("unknown")]
    assert tuple(b.mats["type"]) == SC.UNKNOWN_TYPES and (f.branch == SC.UNKNOWN).all()
    assert set(b.hits["material_id"]) == {0, 1, 2, 3}


def test_families_are_decided(f64s):
    """At least 90 % of every family is decided, except the two subsets of glass
    that exist to be undecided: a condition on the inputs (float64 only), so
    that no GPU test can drop a failure by calling its record undecided."""
    for b, f in zip(SC.batches(), f64s):
        share = SC.decided(f).mean()
        if b.family not in SC.UNDECIDED_FAMILIES:
            assert share >= 0.90, (b.family, share)


def test_seed_search():
    for v in (0, 1, 16384, 32767):
        assert SC.lcg(SC.seed_for_draw(v))[1] == v
    s = SC.seed_for_draws(24576, 32767)
    s, a = SC.lcg(s)
    assert a == 24576 and SC.lcg(s)[1] == 32767


def test_f64_restatement_on_known_records():
    """shade_f64 itself, on records whose answer is known by hand."""
    mats = [SC.material(L.MCPT_DIFFUSE, kd=(0.5, 0.5, 0.5, 0)), SC.material(L.MCPT_TRANSPARENT, Ni=1.5),
            SC.material(L.MCPT_LIGHT, kaks=(2, 3, 4, 0))]
    R = SC._Records("known", mats, max_depth=8)
    up = (0, 0, 1)
    R.add(up, (0, 0, -1), 0, SC.seed_for_draws(0, 0), point=(1, 2, 3))              # radius 0: the normal itself
    R.add(up, (0, 0, -1), 1, SC.seed_for_draw(32767), point=(1, 2, 3))              # normal incidence, transmitted
    R.add(up, (0, 0, -1), 1, SC.seed_for_draw(0), point=(1, 2, 3))                  # the coin 0 < fresnel: reflected
    R.add(up, (0.8, 0, -0.6), 1, 7, flags=SC.INSIDE, point=(1, 2, 3))               # sin = 0.8 > 1 / 1.5 from inside
    R.add(up, (0, 0, -1), 2, 7, color=(1, 1, 1, 1), flags=3)
    R.add(up, (0, 0, -1), 0, 7, flags=7)                                            # depth 8 reached
    R.add(up, (0, 0, -1), 0, 7, flags=7)
    b = R.batch(np.random.Generator(np.random.PCG64(0)))
    f = SC.shade_f64(b)
    assert list(f.branch) == [SC.DIFFUSE, SC.TRANSMIT, SC.REFLECT, SC.TIR, SC.LIGHT, SC.DIFFUSE, SC.DIFFUSE]
    assert np.allclose(f.direction[0], up) and np.allclose(f.origin[0], (1, 2, 3 + 1e-5))
    assert np.allclose(f.color[0], (0.5 / (2 * np.pi),) * 3 + (0,)) and f.flags[0] == 1
    assert np.allclose(f.direction[1], (0, 0, -1)) and f.flags[1] == (1 | SC.INSIDE) and np.allclose(f.color[1], 1)
    assert np.isclose(f.margin[1], 32767 / 32768 - 0.04)  # Schlick at normal incidence: ((1.5 - 1) / (1.5 + 1))^2
    assert np.allclose(f.direction[2], up) and f.flags[2] == 1
    assert np.allclose(f.direction[3], (0.8, 0, 0.6)) and f.flags[3] == (1 | SC.INSIDE) and f.seeds[3] == 7
    assert np.isclose(f.temp[3], 1 - 2.25 * 0.64, atol=1e-6)
    assert f.flags[4] == (3 | L.TERMINATED) and np.allclose(f.color[4], (2, 3, 4, 0)) and f.seeds[4] == 7
    assert f.flags[5] == (8 | L.TERMINATED) and (f.color[5] == 0).all() and f.seeds[5] != 7
    assert list(SC.decided(f)) == [True] * 7


# The CPU oracle's own error against float64 on the decided records it agrees on, measured here
# (max |direction - d64|, max |colour - c64| / max(|c64|, 2^-100)):
#   diffuse/normals 2.45e-7, 1.29e-3 (a radius draw of 32767 leaves cos = 2^-15: 1e-7 / 3e-5)
#   glossy/lobe     2.73e-7, 2.71e-4     glass          8.31e-7, 0       glass/extreme 2.14e-6, 0
#   light           0,       5.71e-8     depth          2.12e-7, 5.86e-6 dead/miss     1.95e-7, 4.26e-6
# The bounds below are 4 x these, rounded up: a restatement that differs in a term, not a rounding, is far outside.
ORACLE_BOUNDS = {"diffuse/normals": (1e-6, 6e-3), "glossy/lobe": (1.2e-6, 1.2e-3), "glass": (3.5e-6, 1e-7),
                 "glass/extreme": (9e-6, 1e-7), "light": (0.0, 2.5e-7), "depth": (1e-6, 2.5e-5),
                 "dead/miss": (1e-6, 2e-5), "unknown": (0.0, 0.0)}


@needs_oracle
def test_oracle_gives_the_float64_answer(f64s):
    """On decided records the CPU oracle gives shade_f64's seed (so its draw
    count), flag word and branch exactly, and its direction and colour within
    ORACLE_BOUNDS: what keeps a wrong restatement from being trusted.  Every
    glossy record's loop ends within MAX_DRAWS draws on the oracle too."""
    for b, f in zip(SC.batches(), f64s):
        r, c, s = oracle.shade(SC.scene_of(b), b.rays, b.hits, b.colors, b.seeds, b.max_depth)
        dec = SC.decided(f)
        if b.family == "glossy/lobe":
            draws = np.array([_count_draws(b.seeds[i], s[i]) for i in range(len(s))])
            lobe = f.branch == SC.LOBE
            assert (draws[lobe] - 1 <= 2 * SC.MAX_DRAWS).all() and (draws[lobe] % 2 == 1).all()
        if b.family in SC.UNDECIDED_FAMILIES:
            continue  # compared to the reference kernel's bits only
        assert (s[dec] == f.seeds[dec]).all(), b.family
        assert (flags_of(r)[dec] == f.flags[dec]).all(), b.family
        assert (SC.branch_of(b, r, s)[dec] == f.branch[dec]).all(), b.family
        de, ce = SC.errors(f, r, c, dec)
        print("%s (max_depth %d): decided %.3f, oracle max |d - d64| = %.3g, max colour error %.3g" % (
            b.family, b.max_depth, dec.mean(), de, ce))
        assert de <= ORACLE_BOUNDS[b.family][0] and ce <= ORACLE_BOUNDS[b.family][1], (b.family, de, ce)
        kept = np.isin(f.branch, (SC.SKIPPED, SC.MISS, SC.LIGHT, SC.UNKNOWN))  # the ray itself is kept
        assert (r["direction"][kept] == b.rays["direction"][kept]).all()
        assert (r["origin"][kept, :3] == b.rays["origin"][kept, :3]).all()
        dead = f.branch == SC.SKIPPED
        assert (c[dead].view(np.uint8) == b.colors[dead].view(np.uint8)).all() and (s[dead] == b.seeds[dead]).all()


def _count_draws(before, after, limit=4 * SC.MAX_DRAWS + 4):
    s = int(before)
    for k in range(limit):
        if s == int(after):
            return k
        s, _ = SC.lcg(s)
    return limit


def test_accumulate_cases_reach_what_they_name():
    seen_attempts = set()
    for cols, hist, cnt, ma in SC.accumulate_cases():
        seen_attempts.add(ma)
        k = len(cnt)
        assert k % 2 == 1 and k % 64 != 0 and np.isfinite(cols).all() and np.isfinite(hist).all()
        nz = cols != 0
        only = lambda v: (nz.any(1) & ((cols == np.float32(v)) | ~nz).all(1))  # noqa: E731
        assert only(2.0 ** -149).any() and only(2.0 ** -127).any()
        assert ((cols == 0) & np.signbit(cols)).all(1).any()  # -0 in every lane
        assert (cols[:, :3] == np.float32(2.0 ** 100)).all(1).any()
        assert (~nz[:, :3].any(1) & nz[:, 3]).any()  # .w alone
        shown, h, c, skipped = SC.accumulate_f64(cols, hist, cnt, ma)
        assert (skipped == ((cols == 0).all(1) | (cnt >= ma))).all()
        assert not skipped[only(2.0 ** -149) & (cnt < ma)].any()  # a denormal has a length
        assert skipped[((cols == 0) & np.signbit(cols)).all(1)].all()
        assert (c == cnt + ~skipped).all() and (h[~skipped, 3] == 0).all()
        if ma < (1 << 24):
            assert {ma - 1, ma, ma + 1} <= set(cnt.tolist())
        else:
            assert (cnt == (1 << 24) + 1).any()
    assert seen_attempts == {4, 16, 1 << 30}


@needs_oracle
def test_oracle_accumulates_as_float64():
    for cols, hist, cnt, ma in SC.accumulate_cases():
        shown, h, c, skipped = SC.accumulate_f64(cols, hist, cnt, ma)
        oc, oh, on = oracle.accumulate(cols, hist, cnt, ma)
        assert (on == c).all() and ((on == cnt) == skipped).all()
        assert (oh[skipped].view(np.uint32) == hist[skipped].view(np.uint32)).all()
        assert (oc[skipped].view(np.uint32) == hist[skipped].view(np.uint32)).all()
        fin = np.abs(h) < float(SC.FLT_MAX)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(oh.astype(np.float64) - h) / np.maximum(np.abs(h), 2.0 ** -100)
        # one fma and one division in float32 (a count of 2^24 + 1 rounds by 2^-25 more): 2^-22 covers them
        assert err[fin & ~skipped[:, None]].max() <= 2.0 ** -22


@pytest.mark.parametrize("glossy", (True, False))
@pytest.mark.parametrize("n_mats", (256, 257))
def test_zoo_scenes(glossy, n_mats):
    z = SC.zoo(glossy, n_mats)
    t, m = z.data.tris, z.data.mats
    assert 20 <= len(t) <= 64 and len(m) == n_mats
    mid = t["normal"][:, 3].view(np.int32)
    assert mid.max() == 9  # the padding is unused
    assert (m["type"] == L.MCPT_GLOSSY).sum() == (4 if glossy else 0)
    assert tuple(m["Ns"][5:9]) == tuple(np.float32(v) for v in SC.ZOO_NS)
    assert {0.75, np.float32(2.417)} <= set(m["Ni"][m["type"] == L.MCPT_TRANSPARENT])
    assert (m["type"] == L.MCPT_LIGHT).sum() == 2
    assert tuple(m["ka_ks"][z.mat_light2]) == (np.float32(2.0 ** -140), 0, 0, 0)
    for k in z.wall_tris:  # the packed normal of the tilted wall
        n = t["normal"][k, :3]
        assert abs(n[0]) == 1 and n[1] == 0 and 2.0 ** -72 < abs(float(n[2])) < 2.0 ** -68 and mid[k] == z.mat_wall
    assert SC.zoo.__wrapped__(glossy, n_mats).data.tris.tobytes() == t.tobytes()
