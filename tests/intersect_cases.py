"""Test helper (no GPU): adversarial scenes and ray batches for mcpt_intersect
and k_render's traversal, and a float64 brute-force closest hit.

Every generator is deterministic (numpy PCG64 with a fixed seed).  A scene is
a `Case` (a SceneData from SceneData.from_arrays, at most 2048 triangles, finite
vertices); a ray batch is a `Batch` of L.RAY records (at most 16384), live
unless the family says otherwise (origin.w bits 0), direction.w = ray index.

Every triangle i has its own MCPT_LIGHT material whose ka encodes i as three
small integers (exact in fp32, never all zero), so Hit.material_id names the
accepted triangle and so does hist.xyz of a one-frame render: a path ends at
its first hit and takes no draw.

Families are tagged "clear" (generic rays, also checked against float64) or
"edge" (adversarial rays, compared bit for bit only).  Which of DESIGN.md
§3.1-3.3's four arguments each family attacks:
  1 slab division    x * rcp(d) == x / d      edge/tinydir, edge/axis, tiny/huge scenes
  2 reduced Cramer   x * rcp(det) == x / det  tiny/huge scenes, edge/graze, edge/tmin
  3 prune margin     2^-10 x diagonal         graze scene with edge/graze and clear
  4 zero direction   0 * inf = NaN            edge/axis (exact +-0), edge/tinydir (denormal)
"""
import collections
import functools

import numpy as np

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import scene as S

K_EPS = 1e-5          # objdef.h EPS: |n.d|, |det| and the replace rule
DEFAULT_TMIN = 1e-3   # intersect.cl's tmin as every caller passes it
MAX_TRIS, MAX_RAYS = 2048, 16384
TINY_EXPONENTS = (-20, -64, -100, -125, -126, -127, -130, -140, -149)
SENTINEL = 0xA5       # byte the edge/dead hit buffer is pre-filled with

Case = collections.namedtuple("Case", "name data unit tmin")
Batch = collections.namedtuple("Batch", "family tag rays tmin hits")


# ------------------------------------------------------------------ materials
def light_materials(n):
    """n MCPT_LIGHT records; ka of record i = (1 + (i & 15), 1 + ((i >> 4) & 15), 1 + (i >> 8))."""
    m = np.zeros(n, L.MATERIAL)
    i = np.arange(n)
    m["type"] = L.MCPT_LIGHT
    m["Ni"] = 1.0
    m["Ns"] = 1.0
    m["ka_ks"][:, 0] = 1 + (i & 15)
    m["ka_ks"][:, 1] = 1 + ((i >> 4) & 15)
    m["ka_ks"][:, 2] = 1 + (i >> 8)
    return m


def triangle_of_ka(ka):
    """Inverse of light_materials' code: (..., >=3) float ka -> triangle index."""
    k = np.asarray(ka)[..., :3].astype(np.int64)
    return (k[..., 0] - 1) + 16 * (k[..., 1] - 1) + 256 * (k[..., 2] - 1)


def _case(name, verts, unit=1.0, tmin=DEFAULT_TMIN):
    v = np.asarray(verts, np.float32)
    assert len(v) <= MAX_TRIS and np.isfinite(v).all()
    data = S.SceneData.from_arrays(v, np.arange(len(v), dtype=np.int32), light_materials(len(v)))
    return Case(name, data, float(unit), float(tmin))


# --------------------------------------------------------------------- scenes
def _quad(p, a, b):
    p, a, b = (np.asarray(x, np.float64) for x in (p, a, b))
    return [[p, p + a, p + a + b], [p, p + a + b, p + b]]


def _box(lo, hi):
    """Axis-aligned box of 12 flat triangles (as cbox's blocks)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = np.diag(hi - lo)
    t = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        t += _quad(lo, e[b], e[c]) + _quad(lo + e[a], e[b], e[c])
    return t


def _lattice_verts(n=16, layers=(0, 1, 2), box=((4, 4, 4), (12, 12, 8))):
    t = []
    for z in layers:
        for j in range(n):
            for i in range(n):
                t += _quad((i, j, z), (1, 0, 0), (0, 1, 0))
    if box is not None:
        t += _box(*box)
    return np.array(t, np.float64)


def _rotation():
    """A rotation that keeps no lattice face axis-aligned: 0.7 rad about (1, 2, 3)."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(0.7) * kx + (1 - np.cos(0.7)) * (kx @ kx)


@functools.lru_cache(None)
def lattice():
    """16 x 16 unit quads on integer coordinates in three layers (z = 0, 1, 2)
    plus one axis-aligned box: 1536 + 12 triangles; every leaf box is flat on
    one axis, every edge and vertex sits on integer planes."""
    return _case("lattice", _lattice_verts())


@functools.lru_cache(None)
def lattice_cut():
    """The first 200 triangles of lattice: at most 256 materials (the LDS table)."""
    return _case("lattice_cut", _lattice_verts()[:200])


@functools.lru_cache(None)
def lattice_tilted():
    return _case("lattice_tilted", _lattice_verts() @ _rotation().T)


@functools.lru_cache(None)
def graze():
    """Four large triangles (edges about 1e3) in an extent of diagonal about 1e4
    (prune margin about 10).  Each has a coplanar patch over the part the grazing
    rays aim at, and rows of small triangles before and behind it at distances
    2^-4 .. 2^4 x margin."""
    margin = 1.0e4 / 1024.0
    t = []
    for k in range(4):
        p = np.array([-1200.0 + 700.0 * k, -900.0 + 300.0 * k, -1500.0 + 1000.0 * k])
        a, b = np.array([1000.0, 50.0 * k, 30.0]), np.array([-40.0 * k, 1000.0, -20.0])
        nrm = np.cross(a, b)
        nrm /= np.linalg.norm(nrm)
        t.append([p, p + a, p + b])
        q = p + 0.55 * a + 0.25 * b + nrm * margin * 2.0 ** (3 * k - 4)
        t.append([q, q + 0.15 * a, q + 0.15 * b])  # a coplanar patch 2^-4, 2^-1, 2^2, 2^5 x margin off: GRAZE_PATCH
        for s in range(-4, 5):
            for side in (-1.0, 1.0):
                c = p + a * (0.08 + 0.045 * (s + 4)) + b * (0.1 + 0.04 * (s + 4) * (side > 0)) \
                    + nrm * side * margin * 2.0 ** s
                t.append([c, c + a * 0.02, c + b * 0.02])
    for corner in (-2887.0, 2887.0):  # extent: the diagonal is 1e4
        c = np.array([corner] * 3)
        t.append([c, c - np.sign(corner) * np.array([8.0, 0, 0]), c - np.sign(corner) * np.array([0, 8.0, 0])])
    return _case("graze", np.array(t), unit=100.0)


def _sizes_verts():
    """A tilted plane of triangles with legs 2^0 .. 2^12 and a 4 x 4 unit
    lattice patch, none behind another (so a scaled copy has no near tie)."""
    t, x = [], 0.0
    for k in range(13):
        s = 2.0 ** k
        for _ in range(3):
            t.append([(x, 0, 0), (x + s, 0, 0), (x, s, 0)])
            x += s * 1.25
    for j in range(4):
        for i in range(4):
            t += [[np.array(c) + (0, -8.0, 0) for c in q] for q in _quad((i, j, 0), (1, 0, 0), (0, 1, 0))]
    return np.array(t, np.float64) @ _rotation().T


@functools.lru_cache(None)
def tiny():
    """_sizes_verts x 2^-20: det sweeps through kEps (legs 2^-20 .. 2^-8)."""
    return _case("tiny", _sizes_verts() * 2.0 ** -20, unit=2.0 ** -20, tmin=DEFAULT_TMIN * 2.0 ** -20)


@functools.lru_cache(None)
def huge():
    return _case("huge", _sizes_verts() * 2.0 ** 20, unit=2.0 ** 20)


@functools.lru_cache(None)
def single():
    """One triangle: the root is a leaf (SceneView.root_leaf)."""
    return _case("single", [[(0, 0, 0), (4, 0, 1), (1, 3, 2)]])


CASES = (lattice, lattice_tilted, graze, tiny, huge, single)


# ----------------------------------------------------------------------- rays
def make_rays(o, d, first_index=0):
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    assert len(o) <= MAX_RAYS
    r = np.zeros(len(o), L.RAY)
    r["origin"][:, :3] = o
    r["direction"][:, :3] = d
    r["direction"][:, 3] = (np.arange(len(o), dtype=np.int32) + first_index).view(np.float32)
    return r


def _verts64(case):
    return case.data.tris["v"][:, :, :3].astype(np.float64)


def _extent(case):
    v = _verts64(case).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def _unit_vectors(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _normalize32(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _interior(rng, v, n, by_area=False):
    """n (triangle index, point) with barycentrics b, c in [0.1, 0.8], b + c <= 0.9;
    triangles drawn uniformly, or with probability proportional to their area."""
    if by_area:
        area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
        tri = rng.choice(len(v), n, p=area / area.sum())
    else:
        tri = rng.integers(0, len(v), n)
    bc = rng.uniform(0.1, 0.8, (4 * n + 64, 2))
    bc = bc[bc.sum(1) <= 0.9][:n]
    assert len(bc) == n
    p = v[tri, 0] + bc[:, :1] * (v[tri, 1] - v[tri, 0]) + bc[:, 1:] * (v[tri, 2] - v[tri, 0])
    return tri, p


def clear(case, n=2048, seed=1):
    """Origins outside the scene (two diagonals from its centre), aimed at
    interior points of random triangles, drawn by area: a triangle far smaller
    than the ray is long is not a generic target (fp32 carries t / size x 2^-24
    into its barycentrics)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = _verts64(case)
    lo, hi, diag = _extent(case)
    _, p = _interior(rng, v, n, by_area=True)
    o = ((lo + hi) / 2 + 2.0 * diag * _unit_vectors(rng, n)).astype(np.float32)
    return Batch("clear", "clear", make_rays(o, _normalize32(p - o)), case.tmin, None)


def _some_vertices(case, rng, n):
    pts = np.unique(case.data.tris["v"][:, :, :3].reshape(-1, 3), axis=0)
    return pts[rng.choice(len(pts), min(n, len(pts)), replace=False)].astype(np.float32)


def axis(case, seed=2):
    """Argument 4 (and 1): directions exactly +-x, +-y, +-z, the other components
    +0 or -0, through scene vertices: on the lattice each ray runs along shared
    edges and through shared vertices with its origin on leaf-box planes on
    the two other axes (0 * rcp(+-0) = NaN).  Then the same rays half a unit off."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi, _ = _extent(case)
    pts = _some_vertices(case, rng, 300)
    o, d = [], []
    for a in range(3):
        for sgn in (1.0, -1.0):
            for zeros in ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0)):
                for shift in (0.0, 0.5 * case.unit):
                    for start in ("outside", "vertex"):
                        if start == "vertex" and (np.signbit(zeros[0]) or np.signbit(zeros[1]) or shift):
                            continue  # from the vertex itself: once per direction
                        oo = pts.astype(np.float64) + shift
                        if start == "outside":
                            oo[:, a] = (lo[a] - case.unit) if sgn > 0 else (hi[a] + case.unit)
                        dd = np.zeros((len(pts), 3))
                        dd[:, a], dd[:, (a + 1) % 3], dd[:, (a + 2) % 3] = sgn, zeros[0], zeros[1]
                        o.append(oo)
                        d.append(dd)
    return Batch("edge/axis", "edge", make_rays(np.concatenate(o), np.concatenate(d)), case.tmin, None)


def tiny_directions():
    """The axis directions with one or two other components +-2^k, not renormalised."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for sgn in (1.0, -1.0):
            for k in TINY_EXPONENTS:
                e = np.ldexp(np.float32(1.0), k)
                for sb, sc in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                    d = np.zeros(3, np.float32)
                    d[a], d[b], d[c] = sgn, sb * e, sc * e
                    out.append(d)
    return np.array(out, np.float32)


def tinydir(case, seed=3):
    """Arguments 1 and 4 where they do not cover each other: a direction
    component that is denormal (or nearly) but not zero, whose v_rcp_f32 is
    +-inf (or huge), with the origin exactly on leaf-box planes on that axis
    (0 * inf = NaN against the reference's 0 / d = 0) and a quarter unit off them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi, _ = _extent(case)
    dirs = tiny_directions()
    pts = _some_vertices(case, rng, 12).astype(np.float64)
    o, d = [], []
    for shift in (0.0, 0.25 * case.unit):
        for p in pts:
            oo = np.repeat((p + shift)[None], len(dirs), 0)
            a = np.argmax(np.abs(dirs), axis=1)
            sg = dirs[np.arange(len(dirs)), a]
            oo[np.arange(len(dirs)), a] = np.where(sg > 0, lo[a] - case.unit, hi[a] + case.unit)
            o.append(oo)
            d.append(dirs)
    return Batch("edge/tinydir", "edge", make_rays(np.concatenate(o), np.concatenate(d)), case.tmin, None)


def tinydir_cameras(case, seed=4):
    """Orthographic cameras (8 x 8 rays each, spacing half a unit) whose
    `direction` has tiny components: generate_rays feeds them through the
    reference's normalize.  Centres sit on a scene vertex's coordinates."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi, _ = _extent(case)
    p = _some_vertices(case, rng, 1)[0].astype(np.float64)
    cams = []
    for a, sgn in ((0, 1.0), (1, -1.0), (2, 1.0)):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in TINY_EXPONENTS:
            e = np.ldexp(np.float32(1.0), k)
            cam = np.zeros(1, L.CAMERA)
            cen = p.copy()
            cen[a] = (lo[a] - case.unit) if sgn > 0 else (hi[a] + case.unit)
            cam["center"][0, :3] = cen
            cam["direction"][0, a], cam["direction"][0, b], cam["direction"][0, c] = sgn, e, -e
            cam["horizontal"][0, b] = 1.0
            cam["up"][0, c] = 1.0
            cam["arg"] = 4.0 * case.unit
            cam["camera_type"] = 1
            cams.append(cam)
    return cams


def _ulp_variants(d):
    """Each direction, and the same with its middle component one ulp down and up."""
    d = np.asarray(d, np.float32)
    j = (np.argmax(np.abs(d), axis=1) + 1) % 3
    r = np.arange(len(d))
    dn, up = d.copy(), d.copy()
    dn[r, j] = np.nextafter(d[r, j], np.float32(-np.inf))
    up[r, j] = np.nextafter(d[r, j], np.float32(np.inf))
    return np.concatenate([d, dn, up])


def _aimed(case, rng, targets):
    lo, hi, diag = _extent(case)
    t = np.asarray(targets, np.float32)
    o = ((lo + hi) / 2 + 1.5 * diag * _unit_vectors(rng, len(t))).astype(np.float32)
    d = _normalize32(t.astype(np.float64) - o)
    return np.concatenate([o, o, o]), _ulp_variants(d)


def vertex(case, n=1500, seed=5):
    """Rays from random origins aimed (float64, rounded to fp32) exactly at
    scene vertices, and one fp32 ulp to either side: shared vertices give up to
    six accepted triangles at one t (the order rule, §3.3) or none."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = _some_vertices(case, rng, n)
    o, d = _aimed(case, rng, pts)
    return Batch("edge/vertex", "edge", make_rays(o, d), case.tmin, None)


def edge(case, n=1500, seed=6):
    """As `vertex`, aimed at points on triangle edges (shared ones on the lattices)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = _verts64(case)
    tri = rng.integers(0, len(v), n)
    k = rng.integers(0, 3, n)
    s = rng.integers(1, 16, n)[:, None] / 16.0
    p = v[tri, k] + s * (v[tri, (k + 1) % 3] - v[tri, k])
    o, d = _aimed(case, rng, p)
    return Batch("edge/edge", "edge", make_rays(o, d), case.tmin, None)


def grazing(case, seed=7):
    """Arguments 2 and 3: rays onto the scene's four largest triangles whose
    |n.d| sweeps 2^-24 .. 2^-8 (straddling kEps = 1e-5 = 2^-16.6) from either
    side, aimed at the part (0.55 .. 0.7, 0.25 .. 0.4 of the two legs) over
    which the graze scene holds a coplanar patch close behind or before."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = _verts64(case)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    o, d = [], []
    for i in np.argsort(-area, kind="stable")[:4]:
        n_ = nrm[i] / area[i]
        e1 = (v[i, 1] - v[i, 0]) / np.linalg.norm(v[i, 1] - v[i, 0])
        e2 = np.cross(n_, e1)
        length = 0.3 * np.sqrt(area[i])
        for ex in range(-24, -7):
            for side in (-1.0, 1.0):
                a_, b_ = v[i, 1] - v[i, 0], v[i, 2] - v[i, 0]
                q = v[i, 0] + 0.55 * a_ + 0.25 * b_
                _, p = _interior(rng, np.array([[q, q + 0.15 * a_, q + 0.15 * b_]]), 30)
                phi = rng.uniform(0, 2 * np.pi, (30, 1))
                s = 2.0 ** ex
                dd = np.sqrt(1 - s * s) * (np.cos(phi) * e1 + np.sin(phi) * e2) + side * s * n_
                o.append(p - dd * length)
                d.append(dd)
    return Batch("edge/graze", "edge", make_rays(np.concatenate(o), np.concatenate(d)), case.tmin, None)


def tmin_edge(case, tmin, n=1200, seed=8):
    """Argument 2's t and the t <= tmin test: origins on a triangle and at
    tmin - 1 ulp, tmin, tmin + 1 ulp in front of it along the ray."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = _verts64(case)
    tri, p = _interior(rng, v, n)
    nrm = np.cross(v[tri, 1] - v[tri, 0], v[tri, 2] - v[tri, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = _normalize32(rng.choice([-1.0, 1.0], (n, 1)) * nrm + 0.5 * _unit_vectors(rng, n))
    t32 = np.float32(tmin)
    o = []
    for t0 in (0.0, np.nextafter(t32, np.float32(-np.inf)), t32, np.nextafter(t32, np.float32(np.inf))):
        o.append(p - float(t0) * d.astype(np.float64))
    return Batch("edge/tmin", "edge", make_rays(np.concatenate(o), np.concatenate([d] * 4)), float(tmin), None)


def dead(case, n=1000 + 37, seed=9):
    """Every third ray already terminated (origin.w has MCPT_TERMINATED); the
    hit buffer is pre-filled with SENTINEL bytes; n is not a multiple of 64."""
    b = clear(case, n, seed)
    rays = b.rays.copy()
    w = rays["origin"][:, 3].view(np.uint32)
    w[::3] = np.uint32(L.TERMINATED) | np.uint32(3)
    hits = np.frombuffer(bytes([SENTINEL]) * (n * L.HIT.itemsize), L.HIT).copy()
    return Batch("edge/dead", "edge", rays, case.tmin, hits)


def live(rays):
    return (rays["origin"][:, 3].view(np.uint32) & np.uint32(L.TERMINATED)) == 0


def exact_may_differ(case, rays):
    """The predicate include/mcpt_hip.h states at mcpt_render_frames: rays on
    which k_render's EXACT search may differ from the reference -- a direction
    component with 0 < |d| < 2^-126 AND the origin exactly on a box plane of
    the tree on that axis (every box plane of the search trees is a plane of
    a reference node: leaves keep their boxes, internal boxes are unions)."""
    out = np.zeros(len(rays), bool)
    for a in range(3):
        bits = np.ascontiguousarray(rays["direction"][:, a]).view(np.uint32)
        den = ((bits & np.uint32(0x7F800000)) == 0) & ((bits & np.uint32(0x007FFFFF)) != 0)
        planes = np.unique(np.concatenate([case.data.nodes["bbmin"][:, a], case.data.nodes["bbmax"][:, a]]))
        out |= den & np.isin(rays["origin"][:, a], planes)
    return out


def denormal_direction(rays):
    bits = np.ascontiguousarray(rays["direction"][:, :3]).view(np.uint32)
    return (((bits & np.uint32(0x7F800000)) == 0) & ((bits & np.uint32(0x007FFFFF)) != 0)).any(axis=1)


def batches(case):
    """Every (family, batch) of a scene, in a fixed order."""
    return [clear(case), axis(case), tinydir(case), vertex(case), edge(case), grazing(case),
            tmin_edge(case, DEFAULT_TMIN), tmin_edge(case, 0.0), tmin_edge(case, 0.5), dead(case)]


# ------------------------------------------------------------- render cameras
def ortho_camera(center, a, sgn, arg=32.0):
    """Orthographic camera (camera_type 1) along axis a: with a 32 x 32 image,
    arg = 32 and an integer centre every origin (idx / 32 - 0.5) * 32 is a lattice point."""
    b, c = (a + 1) % 3, (a + 2) % 3
    cam = np.zeros(1, L.CAMERA)
    cam["center"][0, :3] = center
    cam["direction"][0, a] = sgn
    cam["horizontal"][0, b] = 1.0
    cam["up"][0, c] = 1.0
    cam["arg"] = arg
    cam["camera_type"] = 1
    return cam


def render_cameras(case):
    """(name, camera) for the k_render tests: orthographic along +-x, +-y, +-z
    from an integer centre outside the scene, the same from centre + 0.5, and a
    perspective camera at a lattice point looking along +z."""
    lo, hi, _ = _extent(case)
    mid = np.round((lo + hi) / 2)
    out = []
    for half in (0.0, 0.5):
        for a in range(3):
            for sgn in (1.0, -1.0):
                cen = mid + half
                cen[a] = np.floor(lo[a]) - 3 if sgn > 0 else np.ceil(hi[a]) + 3
                out.append(("ortho%+d%s%s" % (int(sgn), "xyz"[a], "h" if half else ""), ortho_camera(cen, a, sgn)))
    pos = [float(mid[0]), float(mid[1]), float(np.floor(lo[2]) - 6)]
    out.append(("perspective", S.parse_camera({"position": pos, "lookat": [pos[0], pos[1], pos[2] + 1],
                                               "up": [0, 1, 0], "fov": 60.0})))
    return out


# ------------------------------------------------------- float64 brute force
F64Hits = collections.namedtuple("F64Hits", "tri t t2 margin")


def closest_hit_f64(tris, rays, tmin):
    """Brute force over all triangles in numpy float64, no tree: per ray the
    nearest accepted triangle (-1: none) and its t, the runner-up's t (inf:
    none) and the smallest relative margin by which any triangle's acceptance
    was decided.  The tests are the reference's (objdef.h:102-221):
    |n.d| >= kEps with the stored fp32 normal, |det| >= kEps, b >= 0, c >= 0,
    b + c <= 1, t > tmin.  A triangle's margin is the least margin of its
    tests when it is accepted, and the largest margin among its failing tests
    when it is rejected (one robust failure settles it)."""
    v = tris["v"][:, :, :3].astype(np.float64)
    nrm = tris["normal"][:, :3].astype(np.float64)
    nab, nac = v[:, 0] - v[:, 1], v[:, 0] - v[:, 2]
    cr = np.cross(nab, nac)
    n = len(rays)
    out = F64Hits(np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf))
    tm = float(np.float32(tmin))
    for s in range(0, n, 256):
        o = rays["origin"][s:s + 256, :3].astype(np.float64)[:, None, :]
        d = rays["direction"][s:s + 256, :3].astype(np.float64)[:, None, :]
        aro = v[None, :, 0] - o
        with np.errstate(all="ignore"):
            nd = np.abs((nrm[None] * d).sum(-1))
            det = (d * cr[None]).sum(-1)
            t = (aro * cr[None]).sum(-1) / det
            b = (d * np.cross(aro, nac[None])).sum(-1) / det
            c = (d * np.cross(nab[None], aro)).sum(-1) / det
            # signed margins: positive = the test passes
            m = np.stack([(nd - K_EPS) / K_EPS, (np.abs(det) - K_EPS) / K_EPS, b, c, 1.0 - b - c,
                          (t - tm) / np.maximum(np.abs(t), max(tm, 1e-300))], 0)
        m = np.where(np.isnan(m), -np.inf, m)  # det == 0: rejected for certain
        ok =(m[0] >= 0) & (m[1] >= 0) & (m[2] >= 0) & (m[3] >= 0) & (m[4] >= 0) & (m[5] > 0)
        tri_margin = np.where(ok, np.abs(m).min(0), np.where(m < 0, -m, 0.0).max(0))
        ta = np.where(ok, t, np.inf)
        best = ta.argmin(1)
        r = np.arange(len(ta))
        t1 = ta[r, best]
        ta[r, best] = np.inf
        out.tri[s:s + 256] = np.where(np.isfinite(t1), best, -1)
        out.t[s:s + 256] = t1
        out.t2[s:s + 256] = ta.min(1)
        out.margin[s:s + 256] = tri_margin.min(1)
    return out


def decided(f64, tmin):
    """A ray the float64 answer settles: every margin exceeds 1e-3 relative,
    the runner-up is at least 1e-3 x t behind, and t > 10 x tmin.  The
    reference replaces a hit only by one at least kEps closer (objdef.h:213),
    an absolute rule, so the runner-up must also be 4 x kEps behind: within
    that the reference's answer is its traversal order's, not the nearest."""
    hit = f64.tri >= 0
    gap = f64.t2 - f64.t
    with np.errstate(invalid="ignore"):
        ok_hit = (gap >= 1e-3 * f64.t) & (gap >= 4 * K_EPS) & (f64.t > 10 * tmin)
    return (f64.margin > 1e-3) & (~hit | ok_hit)
