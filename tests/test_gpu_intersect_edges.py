"""mcpt_intersect and k_render's own traversal on adversarial rays
(tests/intersect_cases.py): the EXACT search must give the bits of NOPRUNE,
the literal restatement of the reference traversal, and both the reference
kernels' (oracle/_ref, when built), on rays no scene render shoots.

The four arguments of DESIGN.md §3.1-3.3 and the families that attack them:
  1 slab division   (bb - o) * rcp(d) == (bb - o) / d: edge/tinydir (rcp of a
    denormal component is +-inf), edge/axis, and the tiny / huge scenes;
  2 reduced Cramer  x * rcp(det) == x / det: the tiny / huge scenes (det and
    the cofactor quotients near kEps), edge/graze, edge/tmin;
  3 prune margin    2^-10 x diagonal covers the Cramer solve's rounding: the
    graze scene (margin about 10, triangles 2^-4 .. 2^4 margins apart) under
    edge/graze (|n.d| from 2^-24 to 2^-8) and clear;
  4 zero direction  0 * inf = NaN drops only triangles nobody accepts:
    edge/axis (exact +-0, origins on leaf-box planes) and edge/tinydir (the
    same with a denormal component, where the reference computes 0 / d = 0).
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from montecarlopathtracing_amd import _lib as L  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402

from . import intersect_cases as IC  # noqa: E402
from . import oracle, refgpu  # noqa: E402

HIT_FIELDS = ("t", "normal", "point", "material_id")
W = H = 32
DEPTH, ATTEMPT = 4, 4


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


@pytest.fixture(scope="module", params=IC.CASES, ids=lambda f: f.__name__)
def case(request):
    return request.param()


def differing(a, b, fields, rows=None):
    """Indices (within rows) of records whose `fields` differ in any bit."""
    bad = np.zeros(len(a), bool)
    for f in fields:
        x = np.ascontiguousarray(a[f]).view(np.uint8).reshape(len(a), -1)
        y = np.ascontiguousarray(b[f]).view(np.uint8).reshape(len(b), -1)
        bad |= (x != y).any(axis=1)
    if rows is not None:
        bad &= rows
    return np.flatnonzero(bad)


def describe(idx, rays, mine, other):
    i = idx[0]
    return "%d differ, first ray %d o=%r d=%r: t %r / %r, material %d / %d" % (
        len(idx), i, rays["origin"][i, :3].tolist(), rays["direction"][i, :3].tolist(), float(mine["t"][i]),
        float(other["t"][i]), mine["material_id"][i], other["material_id"][i])


def camera_batch(rnd, case):
    """edge/tinydir through the reference's normalize: generate_rays of the
    cameras whose `direction` has tiny components (8 x 8 rays each)."""
    rays = np.concatenate([R.records(rnd.generate_rays(cam, 8, 8), L.RAY) for cam in IC.tinydir_cameras(case)])
    return IC.Batch("edge/tinydir-camera", "edge", rays, case.tmin, None)


def run_intersect(rnd, dsc, b, mode):
    hits = None if b.hits is None else R.to_device(b.hits, rnd.device)
    return R.records(rnd.intersect(dsc, R.to_device(b.rays, rnd.device), hits=hits, tmin=b.tmin, mode=mode), L.HIT)


def test_intersect_families(rnd, case):
    """Every (scene, family), with both search-tree node formats forced:
    EXACT gives NOPRUNE's bits in t, normal, point and material_id on every
    live ray (arguments 1-4: any difference fails); terminated records keep
    the sentinel (intersect.cl:16-18); under oracle/_ref both equal the
    reference kernel on the same tree, NOPRUNE in triangle_id too; decided
    rays of `clear` families name the float64 brute force's triangle with t
    within 4 x the reference kernel's own measured error."""
    dsc = rnd.upload(case.data)
    failures = []
    try:
        for b in IC.batches(case) + [camera_batch(rnd, case)]:
            live = IC.live(b.rays)
            ref = refgpu.intersect(case.data, b.rays, tmin=b.tmin, hits=b.hits) if refgpu.available() else None
            for quantized in (1, 2):
                rnd.set_tuning(quantized=quantized)
                ex = run_intersect(rnd, dsc, b, L.MODE_EXACT)
                nop = run_intersect(rnd, dsc, b, L.MODE_NOPRUNE)
                tag = "%s %s q%d" % (case.name, b.family, quantized)
                bad = differing(ex, nop, HIT_FIELDS, live)
                if len(bad):
                    failures.append("%s EXACT != NOPRUNE: %s" % (tag, describe(bad, b.rays, ex, nop)))
                if b.hits is not None:  # edge/dead: the sentinel records are untouched
                    for name, h in (("EXACT", ex), ("NOPRUNE", nop)):
                        if not (h[~live].view(np.uint8) == IC.SENTINEL).all():
                            failures.append("%s %s wrote a terminated ray's hit" % (tag, name))
                if ref is not None:
                    for name, h, fields in (("EXACT", ex, HIT_FIELDS), ("NOPRUNE", nop, HIT_FIELDS + ("triangle_id",))):
                        bad = differing(h, ref, fields, live)
                        if len(bad):
                            failures.append("%s %s != reference kernel: %s" % (tag, name, describe(bad, b.rays, h, ref)))
                if b.tag == "clear":
                    failures += check_float64(case, b, ex, nop, ref, tag)
    finally:
        rnd.set_tuning()
        dsc.close()
    assert not failures, "\n".join(failures)


def check_float64(case, b, ex, nop, ref, tag):
    out = []
    f64 = IC.closest_hit_f64(case.data.tris, b.rays, b.tmin)
    dec = IC.decided(f64, b.tmin)
    assert dec.mean() >= 0.90  # the inputs' condition (tests/test_intersect_cases_cpu.py asserts it on the CPU)
    hit64 = f64.tri >= 0
    sel = dec & hit64

    def rel_err(h):
        return float((np.abs(h["t"][sel].astype(np.float64) - f64.t[sel]) / f64.t[sel]).max()) if sel.any() else 0.0

    # The bound on t is 4 x the reference's own float error against float64 on these very
    # rays (a 3-term fma dot's error bound is a small multiple of its observed maximum):
    # the reference kernel's where oracle/_ref is built, else the CPU oracle's.  Measured
    # max |t - t64| / t on an MI355X, reference kernel (CPU oracle): lattice 1.47e-7
    # (1.27e-7), lattice_tilted 1.76e-5 (3.08e-5), graze 6.77e-6 (6.77e-6), tiny 2.05e-7
    # (1.96e-7), huge 8.65e-5 (1.26e-4), single 7.13e-5 (3.15e-5); the bound is 4 x the
    # value measured in the run.  EXACT and NOPRUNE measured the reference kernel's values
    # to every digit (they hold its bits).
    base = rel_err(ref if ref is not None else oracle.intersect(case.data, b.rays, tmin=b.tmin))
    bound = 4.0 * base
    for name, h in (("EXACT", ex), ("NOPRUNE", nop)):
        hit = h["t"] < np.float32(3e38)
        wrong = dec & (hit != hit64)
        if wrong.any():
            out.append("%s %s: hit/miss differs from float64 on %d decided rays" % (tag, name, wrong.sum()))
            continue
        wrong = sel & (h["material_id"] != f64.tri)
        if wrong.any():
            out.append("%s %s: %d decided rays name another triangle than float64" % (tag, name, wrong.sum()))
        err = rel_err(h)
        print("%s %s: max |t - t64| / t = %.3g, reference's own %.3g, bound %.3g (%d decided hits)" % (
            tag, name, err, base, bound, sel.sum()))
        if err > bound:
            out.append("%s %s: |t - t64| / t = %.3g above 4 x the reference's own %.3g" % (tag, name, err, base))
    return out


# ------------------------------------------------------------------ k_render
FORMS = list(itertools.product((L.MODE_EXACT, L.MODE_NOPRUNE), (L.SCHED_SINGLE, L.SCHED_PAIRED), (1, 2), (0, 1, 2),
                               (-1, 2, 4)))  # mode, schedule, quantized, stack_window, top_levels
RENDER_CASES = (IC.lattice, IC.lattice_cut, IC.single)


def expectation(rnd, dsc, case, cam, w=W, h=H):
    """Per pixel (hit, ka): generate_rays + intersect(NOPRUNE) for the camera."""
    hits = R.records(rnd.intersect(dsc, rnd.generate_rays(cam, w, h), mode=L.MODE_NOPRUNE), L.HIT)
    hit = hits["t"] < np.float32(3e38)
    ka = np.where(hit[:, None], case.data.mats["ka_ks"][hits["material_id"] % len(case.data.mats), :3], 0.0)
    return hit, ka.astype(np.float32)


def render(rnd, dsc, cam, seeds, frames, mode, schedule=None, w=W, h=H):
    st = rnd.new_state(w, h, seeds)
    rnd.render_frames(dsc, cam, st, DEPTH, ATTEMPT, frames, mode=mode, schedule=schedule)
    torch.cuda.synchronize()
    return st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()


def check_image(tag, out, hit, ka, seeds, frames, failures, held=None):
    """`held`: the pixels the assertion covers (default: every pixel)."""
    hist, count, s = out
    held = np.ones(len(count), bool) if held is None else held
    want = np.where(hit, frames, 0)
    if not (count == want)[held].all():
        failures.append("%s: count differs on %d pixels" % (tag, ((count != want) & held).sum()))
    elif not (hist[:, :3] == ka)[held].all():
        px = np.flatnonzero((hist[:, :3] != ka).any(axis=1) & held)
        failures.append("%s: %d pixels name another triangle, first %d: %d for %d" % (
            tag, len(px), px[0], IC.triangle_of_ka(hist[px[0]]), IC.triangle_of_ka(ka[px[0]])))
    if not (s == seeds).all():
        failures.append("%s: seeds changed" % tag)


def expected_form(dsc, case, mode, quantized, window, top):
    """What mcpt_stats must report when the requested form really ran (select_kernel's rules):
    quantized nodes only in EXACT and only when the scene holds them; stack_window 1 forces the
    window, 2 forbids it, 0 leaves the choice to the occupancy rule (None: not asserted); the LDS
    top levels are EXACT-only, need an internal root (not `single`), -1 is none."""
    exact = mode == L.MODE_EXACT
    has_q = bool(dsc.read("meta")[2])
    tops = 0 if (not exact or len(case.data.tris) == 1) else {-1: 0, 2: 2, 4: 4}[top]
    return {"quantized": int(exact and quantized == 1 and has_q), "stack_window": {0: None, 1: 1, 2: 0}[window],
            "top_levels": tops}


@pytest.mark.parametrize("getter", RENDER_CASES, ids=lambda f: f.__name__)
def test_render_forms(rnd, getter):
    """k_render's own copy of the traversal, in every form (mode x leaf
    schedule x node format x stack layout x LDS top levels), on per-triangle
    LIGHT scenes: one frame, whole image, primary cache off, so count == 1 and
    hist.xyz == ka name each pixel's triangle and count == 0 a miss; seeds
    stay.  Orthographic cameras along +-x, +-y, +-z put every origin on a
    lattice point (arguments 1 and 4: rays along shared edges and through
    shared vertices, origins on leaf-box planes), the same from centre + 0.5,
    and one perspective camera.  lattice has 1548 materials (the table in
    global memory), lattice_cut 200 (the LDS table), single is the root_leaf
    path.  After every render mcpt_stats must name the form that was asked
    for (expected_form), so a quiet fall-back to another form fails; on
    `single` the top levels do not exist (the root is a leaf) and NOPRUNE has
    neither quantized nodes nor top levels: those forms repeat the plain one."""
    case = getter()
    dsc = rnd.upload(case.data)
    seeds = R.default_seeds(W * H)
    failures = []
    try:
        if len(case.data.tris) > 1:
            assert dsc.read("meta")[2] == 1  # the scene holds the quantized nodes, so quantized=1 is honoured
        for name, cam in IC.render_cameras(case):
            rnd.set_tuning()
            hit, ka = expectation(rnd, dsc, case, cam)
            if refgpu.available():
                rh, rc, rs = refgpu.render(case.data, cam, W, H, DEPTH, 1, ATTEMPT, seeds)
                check_image("%s %s reference render" % (case.name, name), (rh, rc, rs), hit, ka, seeds, 1, failures)
            for mode, schedule, quantized, window, top in FORMS:
                rnd.set_tuning(quantized=quantized, stack_window=window, top_levels=top, primary_cache=2)
                tag = "%s %s mode %d schedule %d quantized %d window %d top %d" % (case.name, name, mode, schedule,
                                                                                   quantized, window, top)
                check_image(tag, render(rnd, dsc, cam, seeds, 1, mode, schedule), hit, ka, seeds, 1, failures)
                st = rnd.stats()
                ran = {k: st[k] for k in ("quantized", "stack_window", "top_levels")}
                want = expected_form(dsc, case, mode, quantized, window, top)
                if any(v is not None and ran[k] != v for k, v in want.items()) or st["primary_cache"] != 0:
                    failures.append("%s: ran as %r (primary_cache %d), asked for %r" % (tag, ran, st["primary_cache"],
                                                                                        want))
    finally:
        rnd.set_tuning()
        dsc.close()
    assert not failures, "%d failures\n%s" % (len(failures), "\n".join(failures[:40]))


@pytest.mark.parametrize("getter", RENDER_CASES, ids=lambda f: f.__name__)
def test_render_primary_cache(rnd, getter):
    """primary_cache=1 and two frames: k_primary (or the PRIM form) makes the
    hits and the second frame reads them: count 2 and the same ka; mcpt_stats
    must say that the call had a cache."""
    case = getter()
    dsc = rnd.upload(case.data)
    seeds = R.default_seeds(W * H)
    failures = []
    try:
        for name, cam in IC.render_cameras(case):
            rnd.set_tuning()
            hit, ka = expectation(rnd, dsc, case, cam)
            for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
                rnd.set_tuning(primary_cache=1)
                rnd.drop_caches()
                check_image("%s %s mode %d cached" % (case.name, name, mode), render(rnd, dsc, cam, seeds, 2, mode),
                            hit, ka, seeds, 2, failures)
                if rnd.stats()["primary_cache"] == 0:
                    failures.append("%s %s mode %d: the call ran without the primary-hit cache" % (case.name, name, mode))
    finally:
        rnd.set_tuning()
        dsc.close()
    assert not failures, "\n".join(failures[:40])


@pytest.mark.parametrize("getter", (IC.lattice, IC.lattice_tilted, IC.single), ids=lambda f: f.__name__)
def test_render_denormal_directions(rnd, getter):
    """Arguments 1 and 4 inside k_render and k_primary: 8 x 8 renders of the
    orthographic cameras whose `direction` has components +-2^k (cl_normalize
    keeps a denormal component), primary cache off (k_render traces the
    primary ray) and on (k_primary does), one and two frames.
      - NOPRUNE == generate_rays + intersect(NOPRUNE) on every pixel, and so
        is the reference's own render under oracle/_ref.
      - EXACT == the same on every pixel outside the predicate that
        include/mcpt_hip.h states at mcpt_render_frames (IC.exact_may_differ: a
        component 0 < |d| < 2^-126 AND the origin on a box plane of the tree
        on that axis, computed from the tree's node boxes).  The excluded
        pixels stay in the image; how many of them EXACT got differently is
        printed, not asserted.
    Both node formats run: the quantized nodes' decoded planes are not the
    tree's, and the predicate as stated must still cover them."""
    case = getter()
    dsc = rnd.upload(case.data)
    w = h = 8
    seeds = R.default_seeds(w * h)
    failures = []
    n_excluded = n_denormal_held = n_exact_differs = 0
    try:
        for ci, cam in enumerate(IC.tinydir_cameras(case)):
            rnd.set_tuning()
            rays = R.records(rnd.generate_rays(cam, w, h), L.RAY)
            excluded = IC.exact_may_differ(case, rays)
            n_excluded += excluded.sum()
            n_denormal_held += (IC.denormal_direction(rays) & ~excluded).sum()
            hit, ka = expectation(rnd, dsc, case, cam, w, h)
            if refgpu.available():
                ref = refgpu.render(case.data, cam, w, h, DEPTH, 1, ATTEMPT, seeds)
                check_image("%s camera %d reference render" % (case.name, ci), ref, hit, ka, seeds, 1, failures)
            for cache, frames in ((2, 1), (1, 2)):
                for quantized in (1, 2):
                    for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
                        rnd.set_tuning(primary_cache=cache, quantized=quantized)
                        rnd.drop_caches()
                        out = render(rnd, dsc, cam, seeds, frames, mode, w=w, h=h)
                        tag = "%s camera %d cache %d quantized %d mode %d" % (case.name, ci, cache, quantized, mode)
                        held = ~excluded if mode == L.MODE_EXACT else None
                        check_image(tag, out, hit, ka, seeds, frames, failures, held)
                        if mode == L.MODE_EXACT:
                            n_exact_differs += ((out[1] != np.where(hit, frames, 0)) & excluded).sum()
    finally:
        rnd.set_tuning()
        dsc.close()
    print("%s: %d pixels inside the predicate (EXACT differed on %d pixel-renders of them), %d denormal pixels held"
          % (case.name, n_excluded, n_exact_differs, n_denormal_held))
    assert n_excluded > 0 and n_denormal_held > 0  # the cameras reach both sides of the predicate
    assert not failures, "%d failures\n%s" % (len(failures), "\n".join(failures[:40]))


def test_fallbacks_are_exercised(rnd):
    """Rays through shared vertices and along shared edges of lattice reach the
    order rule (§3.3): the integer-centre orthographic +-z renders, whose
    every ray goes through a lattice vertex, report order_fallbacks > 0 (and
    still give the expectation with the counters compiled in)."""
    case = IC.lattice()
    dsc = rnd.upload(case.data)
    seeds = R.default_seeds(W * H)
    failures = []
    try:
        rnd.set_stats(True)
        for name, cam in IC.render_cameras(case):
            if name not in ("ortho+1z", "ortho-1z"):
                continue
            rnd.set_tuning()
            hit, ka = expectation(rnd, dsc, case, cam)
            rnd.set_tuning(primary_cache=2)
            check_image(name, render(rnd, dsc, cam, seeds, 1, L.MODE_EXACT), hit, ka, seeds, 1, failures)
            st = rnd.stats()
            print("%s: order_fallbacks %d of %d segments" % (name, st["order_fallbacks"], st["segments"]))
            assert st["order_fallbacks"] > 0
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()
        dsc.close()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("getter", (IC.lattice, IC.lattice_cut), ids=lambda f: f.__name__)
def test_unknown_material_type(rnd, getter):
    """A triangle whose material has an unknown type (7): its pixels end black
    with count == 0 and mcpt_stats.bad_material counts them, with the material
    table in global memory (lattice, 1548 materials) and in LDS (lattice_cut)."""
    case = getter()
    name, cam = IC.render_cameras(case)[-1]
    assert name == "perspective"
    dsc = rnd.upload(case.data)
    try:
        hits = R.records(rnd.intersect(dsc, rnd.generate_rays(cam, W, H), mode=L.MODE_NOPRUNE), L.HIT)
    finally:
        dsc.close()
    hit = hits["t"] < np.float32(3e38)
    victim = np.bincount(hits["material_id"][hit]).argmax()
    mats = case.data.mats.copy()
    mats["type"][victim] = 7
    black = hit & (hits["material_id"] == victim)
    assert 0 < black.sum() < hit.sum()
    ka = np.where((hit & ~black)[:, None], mats["ka_ks"][hits["material_id"] % len(mats), :3], 0.0).astype(np.float32)
    dsc = rnd.upload(IC.S.SceneData(case.data.tris, case.data.nodes, mats))
    seeds = R.default_seeds(W * H)
    failures = []
    try:
        rnd.set_stats(True)
        rnd.set_tuning(primary_cache=2)
        for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
            check_image("%s type 7 mode %d" % (case.name, mode), render(rnd, dsc, cam, seeds, 1, mode), hit & ~black, ka,
                        seeds, 1, failures)
            assert rnd.stats()["bad_material"] == black.sum()
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()
        dsc.close()
    assert not failures, "\n".join(failures)
