"""mcpt_shade, mcpt_accumulate and k_render's shading on adversarial hits and
materials (tests/shade_cases.py): hits, normals, incidence angles, Ni, Ns,
inside bits, colours and seeds that no scene render produces.

  - k_shade and k_shade_tex must give the reference kernel's bits (oracle/_ref,
    when built) in origin, direction, colour and seed on every family the
    reference defines, and shade.cl's float64 restatement (shade_cases.shade_f64)
    on every record that restatement decides, whether or not _ref is built;
  - k_accumulate the same against history.cl;
  - k_render, in every shading form (G on / off, the material table in LDS or
    in global memory, the S phase run early or late, with and without the
    primary-hit cache, in one call or two), must give the bits of the chain of
    wavefront kernels on small scenes built from the same edge cases.
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from montecarlopathtracing_amd import _lib as L  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402

from . import oracle, refgpu  # noqa: E402
from . import shade_cases as SC  # noqa: E402
from .test_gpu_jitter import chain  # noqa: E402


@pytest.fixture(scope="module")
def rnd():
    return R.Renderer(0)


def flags_of(rays):
    return rays["origin"][:, 3].view(np.uint32)


def run_shade(rnd, dsc, b):
    rays, hits = R.to_device(b.rays, rnd.device), R.to_device(b.hits, rnd.device)
    colors = torch.from_numpy(b.colors.copy()).to(rnd.device)
    seeds = torch.from_numpy(b.seeds.view(np.int32).copy()).to(rnd.device)
    rnd.shade(dsc, rays, hits, colors, seeds, b.max_depth)
    torch.cuda.synchronize()
    return R.records(rays, L.RAY), colors.cpu().numpy(), seeds.cpu().numpy().view(np.uint32)


def lanes_differ(mine, ref):
    """Per float lane: the bits differ; where the reference's lane is not
    finite, its class (NaN or infinity) and sign differ."""
    a, b = np.ascontiguousarray(mine, np.float32), np.ascontiguousarray(ref, np.float32)
    bits = a.view(np.uint32) != b.view(np.uint32)
    loose = (np.isnan(a) != np.isnan(b)) | (np.isinf(a) != np.isinf(b)) | (np.signbit(a) != np.signbit(b))
    return np.where(np.isfinite(b), bits, loose)


def differing(out, ref):
    """Records whose origin, direction (all four lanes: the flag word and the id
    among them), colour or seed differ from the reference's.  `ratio` is not
    compared: the reference leaves it uninitialised."""
    (r, c, s), (rr, rc, rs) = out, ref
    bad = lanes_differ(r["origin"][:, :3], rr["origin"][:, :3]).any(1)
    bad |= flags_of(r) != flags_of(rr)
    bad |= lanes_differ(r["direction"][:, :3], rr["direction"][:, :3]).any(1)
    bad |= r["direction"][:, 3].view(np.uint32) != rr["direction"][:, 3].view(np.uint32)
    bad |= lanes_differ(c, rc).any(1) | (s != rs)
    return np.flatnonzero(bad)


def describe(b, idx, out, ref):
    i = idx[0]
    return ("%d of %d differ, first record %d (material %d type %d Ni %r Ns %r, n %r, d %r, flags %#x, seed %#x): "
            "direction %r / %r, colour %r / %r, flags %#x / %#x, seed %#x / %#x" % (
                len(idx), len(b.rays), i, b.hits["material_id"][i], b.mats["type"][b.hits["material_id"][i]],
                float(b.mats["Ni"][b.hits["material_id"][i]]), float(b.mats["Ns"][b.hits["material_id"][i]]),
                b.hits["normal"][i, :3].tolist(), b.rays["direction"][i, :3].tolist(), flags_of(b.rays)[i], b.seeds[i],
                out[0]["direction"][i, :3].tolist(), ref[0]["direction"][i, :3].tolist(), out[1][i].tolist(),
                ref[1][i].tolist(), flags_of(out[0])[i], flags_of(ref[0])[i], out[2][i], ref[2][i]))


def check_float64(b, f64, out, base_out, base_name, tag, pooled):
    """Decided records against shade_f64: seed, flag word and branch exactly;
    the direction and colour errors of the kernel and of the float baseline on
    the same records go to pooled[family], which the caller holds to 4 x the
    baseline's once every batch of the family is in (a maximum over the one
    record of the shortest batch bounds nothing)."""
    fails = []
    dec = SC.decided(f64)
    assert dec.mean() >= 0.90  # the inputs' condition (tests/test_shade_cases_cpu.py asserts it on the CPU)
    r, c, s = out
    for name, wrong in (("seed", s != f64.seeds), ("flag word", flags_of(r) != f64.flags),
                        ("branch", SC.branch_of(b, r, s) != f64.branch)):
        if (wrong & dec).any():
            i = np.flatnonzero(wrong & dec)[0]
            fails.append("%s: %s differs from float64 on %d decided records, first %d (margin %.3g)" % (
                tag, name, (wrong & dec).sum(), i, f64.margin[i]))
    # The bound is 4 x the error of the reference kernel (where oracle/_ref is built, else of
    # the CPU oracle) against float64 on these very records, the family's batches taken
    # together.  Measured on an MI355X, reference
    # kernel, max |d - d64| and max |c - c64| / max(|c64|, 2^-100):
    #   diffuse/normals 2.45e-7, 1.29e-3 (a radius draw of 32767 leaves cos = 2^-15; the batch of
    #   one record 8.04e-8, 9.18e-8)       glossy/lobe 2.73e-7, 2.71e-4
    #   glass 8.30e-7, 0                   glass/extreme 2.14e-6, 0      light 0, 5.71e-8
    #   depth 1.81e-7, 4.62e-6 (max_depth 8), 2.12e-7, 5.56e-6 (max_depth 1)
    #   dead/miss 1.89e-7, 4.63e-6
    # (the CPU oracle's, tests/test_shade_cases_cpu.py: the same to two digits bar depth and
    # dead/miss, 1.96e-7, 3.40e-6 / 2.12e-7, 5.86e-6 / 1.95e-7, 4.26e-6).  k_shade and
    # k_shade_tex measured the reference kernel's values to every digit (they hold its bits).
    base = SC.errors(f64, base_out[0], base_out[1], dec)
    mine = SC.errors(f64, r, c, dec)
    print("%s: max |d - d64| = %.3g (%s %.3g), max colour error %.3g (%s %.3g), %d decided of %d" % (
        tag, mine[0], base_name, base[0], mine[1], base_name, base[1], dec.sum(), len(dec)))
    held = pooled.setdefault(b.family, [0.0, 0.0, 0.0, 0.0, base_name])
    held[:4] = [max(x, y) for x, y in zip(held[:4], mine + base)]
    return fails


@pytest.fixture(scope="module")
def f64s():
    return [SC.shade_f64(b) for b in SC.batches()]


def test_shade_families(rnd, f64s):
    """Every batch through k_shade and, with a texture of ones on the dummy
    triangle, through k_shade_tex."""
    failures, pooled = [], {}
    for b, f64 in zip(SC.batches(), f64s):
        data = SC.scene_of(b)
        tag = "%s (%d records, max_depth %d)" % (b.family, len(b.rays), b.max_depth)
        dsc = rnd.upload(data)
        try:
            plain = run_shade(rnd, dsc, b)
            rnd.set_textures(dsc, np.zeros((1, 3, 2), np.float32), np.zeros(1, np.int32), [np.ones((2, 2, 3), np.float32)])
            textured = run_shade(rnd, dsc, b)
        finally:
            dsc.close()
        for k, name in enumerate(("rays", "colours", "seeds")):  # the two kernels: the same bytes, `ratio` included
            if plain[k].tobytes() != textured[k].tobytes():
                failures.append("%s: k_shade_tex's %s differ from k_shade's" % (tag, name))
        dead = f64.branch == SC.SKIPPED
        if dead.any():  # nothing is written for a terminated ray
            kept = (plain[0][dead].tobytes() == b.rays[dead].tobytes() and (plain[2][dead] == b.seeds[dead]).all()
                    and (plain[1][dead].view(np.uint8) == SC.SENTINEL).all())
            if not kept:
                failures.append("%s: a terminated ray's record, colour or seed was written" % tag)
        if b.family == "unknown":
            # what shade_hit documents; the reference stores an uninitialised ray here
            r, c, s = plain
            ok = ((flags_of(r) == (flags_of(b.rays) | np.uint32(L.TERMINATED))).all() and (c == 0).all()
                  and not np.signbit(c).any() and (s == b.seeds).all()
                  and r["origin"][:, :3].tobytes() == b.rays["origin"][:, :3].tobytes()
                  and r["direction"].tobytes() == b.rays["direction"].tobytes())
            if not ok:
                failures.append("%s: an unknown material type must end the path: colour 0, ray and seed kept" % tag)
            continue
        ref = None
        if refgpu.available():
            ref = refgpu.shade(data, b.rays, b.hits, b.colors, b.seeds, b.max_depth)
            bad = differing(plain, ref)
            if len(bad):
                failures.append("%s: k_shade != reference kernel: %s" % (tag, describe(b, bad, plain, ref)))
        if b.family in SC.UNDECIDED_FAMILIES:
            continue  # compared to the reference's bits only
        if ref is not None:
            base, base_name = ref, "reference kernel"
        else:
            base, base_name = oracle.shade(data, b.rays, b.hits, b.colors, b.seeds, b.max_depth), "CPU oracle"
        failures += check_float64(b, f64, plain, base, base_name, tag, pooled)
    for family, (mine_d, mine_c, base_d, base_c, base_name) in pooled.items():
        if mine_d > 4 * base_d or mine_c > 4 * base_c:
            failures.append("%s: direction error %.3g, colour error %.3g above 4 x the %s's own %.3g, %.3g" % (
                family, mine_d, mine_c, base_name, base_d, base_c))
    assert not failures, "%d failures\n%s" % (len(failures), "\n".join(failures))


def test_accumulate_edges(rnd):
    """k_accumulate against history.cl bit for bit, and against accumulate_f64
    in the count and in which records were skipped."""
    failures = []
    for cols, hist, count, max_attempt in SC.accumulate_cases():
        dc, dh = torch.from_numpy(cols.copy()).to(rnd.device), torch.from_numpy(hist.copy()).to(rnd.device)
        dn = torch.from_numpy(count.copy()).to(rnd.device)
        rnd.accumulate(dc, dh, dn, max_attempt)
        torch.cuda.synchronize()
        oc, oh, on = dc.cpu().numpy(), dh.cpu().numpy(), dn.cpu().numpy()
        tag = "max_attempt %d" % max_attempt
        _shown, _h, want_count, skipped = SC.accumulate_f64(cols, hist, count, max_attempt)
        if not (on == want_count).all():
            i = np.flatnonzero(on != want_count)[0]
            failures.append("%s: count differs from float64 on %d records, first %d: colour %r count %d -> %d" % (
                tag, (on != want_count).sum(), i, cols[i].tolist(), count[i], on[i]))
        if not (oh[skipped].tobytes() == hist[skipped].tobytes() and oc[skipped].tobytes() == hist[skipped].tobytes()):
            failures.append("%s: a skipped record must keep its history and show it" % tag)
        if refgpu.available():
            rc, rh, rn = refgpu.accumulate(cols, hist, count, len(count), 1, max_attempt)
            for name, a, b in (("display", oc, rc), ("history", oh, rh)):
                bad = np.flatnonzero(lanes_differ(a, b).any(1))
                if len(bad):
                    i = bad[0]
                    failures.append("%s: %s differs from the reference kernel on %d records, first %d: colour %r "
                                    "hist %r count %d: %r / %r" % (tag, name, len(bad), i, cols[i].tolist(),
                                                                    hist[i].tolist(), count[i], a[i].tolist(),
                                                                    b[i].tolist()))
            if not (on == rn).all():
                failures.append("%s: count differs from the reference kernel on %d records" % (tag, (on != rn).sum()))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ k_render
W = H = 32
DEPTH, FRAMES, ATTEMPT = 8, 6, 4
CACHE_OFF, CACHE_ALWAYS = 2, 1  # mcpt_tuning.primary_cache
FORMS = list(itertools.product((L.MODE_EXACT, L.MODE_NOPRUNE), (L.SCHED_SINGLE, L.SCHED_PAIRED), (1, 64),
                               (CACHE_OFF, CACHE_ALWAYS), ((FRAMES,), (2, FRAMES - 2))))


def state_differs(tag, got, want, failures):
    for name, a, b in zip(("hist", "count", "seeds"), got, want):
        if a.tobytes() != b.tobytes():
            px = np.flatnonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))
            failures.append("%s: %s differs on %d pixels, first %d: %r / %r" % (tag, name, len(px), px[0],
                                                                                 a[px[0]].tolist(), b[px[0]].tolist()))


@pytest.mark.parametrize("n_mats", (256, 257))
@pytest.mark.parametrize("glossy", (True, False), ids=("glossy", "plain"))
def test_zoo_render_forms(rnd, glossy, n_mats):
    """k_render's own copy of the shading, 32 x 32, depth 8, 6 frames, attempt
    4, on the zoo scene: glass of Ni 0.75 and 2.417, a floor at grazing
    incidence in glossy strips of Ns 0, 98, 65536 and 1e6 (`glossy` off: the
    G = false form, with glass in the scene), a wall of normal (1, 0, ~2^-70),
    a light of ka 2^-140; 256 materials (the LDS table, at its limit) or 257
    (the table in global memory).  Every form (mode x leaf schedule x
    shade_threshold 1 / 64, which moves when a rejected glossy lane draws again,
    x primary-hit cache x one call or 2 + 4 frames) must give the bits of the
    chain of wavefront kernels in hist, count and seeds, and so must the
    reference's own render under oracle/_ref."""
    z = SC.zoo(glossy, n_mats)
    dsc = rnd.upload(z.data)
    seeds = R.default_seeds(W * H)
    failures = []
    try:
        rnd.set_tuning()
        want = {mode: chain(rnd, dsc, z.cam, W, H, DEPTH, ATTEMPT, [(FRAMES, False)], seeds, mode)
                for mode in (L.MODE_EXACT, L.MODE_NOPRUNE)}
        assert (want[L.MODE_NOPRUNE][2] != seeds).mean() > 0.9 and (want[L.MODE_NOPRUNE][1] > 0).mean() > 0.25
        if refgpu.available():
            ref = refgpu.render(z.data, z.cam, W, H, DEPTH, FRAMES, ATTEMPT, seeds)
            for mode in want:
                state_differs("chain mode %d against the reference render" % mode, want[mode], ref, failures)
        # the denormal light: its pixels look black and still count as samples
        hits = R.records(rnd.intersect(dsc, rnd.generate_rays(z.cam, W, H), mode=L.MODE_NOPRUNE), L.HIT)
        dim = (hits["t"] < np.float32(3e38)) & (hits["material_id"] == z.mat_light2)
        assert dim.sum() >= 4
        for mode, schedule, shade_threshold, cache, split in FORMS:
            rnd.set_tuning(shade_threshold=shade_threshold, primary_cache=cache)
            rnd.drop_caches()
            tag = "mode %d schedule %d shade_threshold %d cache %d frames %r" % (mode, schedule, shade_threshold, cache,
                                                                                 split)
            st = rnd.new_state(W, H, seeds)
            for frames in split:
                rnd.render_frames(dsc, z.cam, st, DEPTH, ATTEMPT, frames, mode=mode, schedule=schedule)
                ran = rnd.stats()["primary_cache"]  # (waits for the call)
                if (ran != 0) != (cache == CACHE_ALWAYS):
                    failures.append("%s: ran with primary_cache %d" % (tag, ran))
            got = st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()
            state_differs(tag, got, want[mode], failures)
            if not (got[1][dim] == min(FRAMES, ATTEMPT)).all():
                failures.append("%s: a pixel of the 2^-140 light has another count than %d" % (tag, min(FRAMES, ATTEMPT)))
            if not ((got[0][dim, 0] > 0) & (got[0][dim, 0] < np.float32(2.0 ** -126))).all():
                failures.append("%s: the 2^-140 light's pixels must hold a denormal mean" % tag)
        rnd.set_stats(True)  # the counters compiled in: the same bits, and no material fell to bad_material
        for mode in want:
            rnd.set_tuning(primary_cache=CACHE_OFF)
            st = rnd.new_state(W, H, seeds)
            rnd.render_frames(dsc, z.cam, st, DEPTH, ATTEMPT, FRAMES, mode=mode)
            s = rnd.stats()
            state_differs("mode %d with stats" % mode, (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()),
                          want[mode], failures)
            if s["bad_material"] != 0 or s["segments"] == 0:
                failures.append("mode %d with stats: bad_material %d, segments %d" % (mode, s["bad_material"],
                                                                                     s["segments"]))
    finally:
        rnd.set_stats(False)
        rnd.set_tuning()
        dsc.close()
    assert not failures, "%d failures\n%s" % (len(failures), "\n".join(failures[:40]))
