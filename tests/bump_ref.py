"""Float64 restatement of the bump / normal-map lookup (include/mcpt_hip.h at
mcpt_scene_set_normal_maps; csrc/mcpt_bump.h on the device), the yardstick of
tests/test_gpu_bump.py and tests/test_bump_cpu.py, with the deliberate mistakes
the GPU test must reject."""
import numpy as np

from . import texture_ref as T

MUTANTS = ("no_h", "no_f", "no_gs", "swap_xy", "no_flip")

# queries where the definition branches on a near-tie are left out of a comparison
TIE_TP2 = 1e-6     # |tp|^2 below this
TIE_FACING = 1e-4  # |dot(n', d)| below this
TIE_FLAT = 1e-10   # 0 < mx^2 + my^2 below this


def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.sqrt((a * a).sum(-1, keepdims=True))


def face_normals(verts):
    """normalize(cross(v1 - v0, v2 - v0)) of (n, 3, 3) corners, float64."""
    v = np.asarray(verts, np.float64)
    return _unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))


def tangent_frames(verts, ng, uv, tri_map):
    """The setter's per-triangle frame, in float64: (t (n, 3) rounded once to
    float32, h (n,), mapped (n,) bool).  det zero or not finite, or T zero or
    not finite, makes the triangle unmapped."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    w = np.asarray(uv, np.float32).astype(np.float64)
    ng = np.asarray(ng, np.float32).astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    du1, dv1 = w[:, 1, 0] - w[:, 0, 0], w[:, 1, 1] - w[:, 0, 1]
    du2, dv2 = w[:, 2, 0] - w[:, 0, 0], w[:, 2, 1] - w[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    with np.errstate(all="ignore"):
        tt = (dv2[:, None] * e1 - dv1[:, None] * e2) / det[:, None]
        bb = (du1[:, None] * e2 - du2[:, None] * e1) / det[:, None]
        tl = np.sqrt((tt * tt).sum(1))
        t = tt / tl[:, None]
    ok = np.isfinite(det) & (det != 0) & np.isfinite(tl) & (tl > 0) & (np.asarray(tri_map) >= 0)
    with np.errstate(all="ignore"):
        h = np.where((np.cross(ng, tt) * bb).sum(1) >= 0, 1.0, -1.0)
    t = np.where(ok[:, None], t, 0.0).astype(np.float32).astype(np.float64)
    return t, h, ok


def lookup(verts, uv, tri_map, images, ids, pts, mutant=None):
    """m (q, 3) float64 of each query: texture_ref's barycentrics and bilinear,
    repeating filter over the normal maps (an unmapped triangle gives (0, 0, 1))."""
    ids = np.asarray(ids, np.int64)
    v = np.asarray(verts, np.float64)[ids]
    b0, b1, b2 = T.barycentrics(v[:, 0], v[:, 1], v[:, 2], pts)
    t = np.asarray(uv, np.float64)[ids]
    u = b0 * t[:, 0, 0] + b1 * t[:, 1, 0] + b2 * t[:, 2, 0]
    w = b0 * t[:, 0, 1] + b1 * t[:, 1, 1] + b2 * t[:, 2, 1]
    out = np.zeros((len(ids), 3), np.float64)
    out[:, 2] = 1.0
    tt = np.asarray(tri_map)[ids]
    for k, img in enumerate(images):
        m = tt == k
        if m.any():
            out[m] = T.sample(img, u[m], w[m], "no_flip" if mutant == "no_flip" else None)
    return out


def bump_normal(verts, ng, uv, tri_map, images, ids, pts, dirs, normals, mutant=None):
    """(n' (q, 3) float64, tie (q,) bool) for queries (ids, pts, dirs, N) on a
    mesh: verts (n, 3, 3), ng (n, 3) the packed face normals, uv (n, 3, 2),
    tri_map (n,), images: list of (H, W, 3).  tie marks the queries that sit
    where the definition branches on a near-tie (TIE_*)."""
    ids = np.asarray(ids, np.int64)
    N = np.asarray(normals, np.float64)[:, :3]
    d = np.asarray(dirs, np.float64)[:, :3]
    t, h, ok = tangent_frames(verts, ng, uv, tri_map)
    m = lookup(verts, uv, np.where(ok, np.asarray(tri_map), -1), images, ids, pts, mutant)
    if mutant == "swap_xy":
        m = m[:, [1, 0, 2]]
    g = np.asarray(ng, np.float32).astype(np.float64)[ids]
    t, h, ok = t[ids], h[ids], ok[ids]
    flat2 = m[:, 0] ** 2 + m[:, 1] ** 2
    f = np.where((N * g).sum(1) < 0, -1.0, 1.0)
    if mutant == "no_f":
        f = np.ones_like(f)
    if mutant == "no_h":
        h = np.ones_like(h)
    tp = t - N * (N * t).sum(1, keepdims=True)
    if mutant == "no_gs":
        tp = t.copy()
    tp2 = (tp * tp).sum(1)
    with np.errstate(all="ignore"):
        Tp = tp / np.sqrt(tp2)[:, None]
        Bp = (h * f)[:, None] * np.cross(N, Tp)
        n = m[:, :1] * Tp + m[:, 1:2] * Bp + m[:, 2:3] * N
        n = n / np.sqrt((n * n).sum(1, keepdims=True))
        facing = (n * d).sum(1)
    keep_n = ~ok | (flat2 == 0) | ~(np.isfinite(tp2) & (tp2 > 0)) | ~np.isfinite(n).all(1) | ~(facing < 0)
    out = np.where(keep_n[:, None], N, n)
    with np.errstate(invalid="ignore"):
        tie = ok & (((flat2 > 0) & (flat2 < TIE_FLAT)) | (tp2 < TIE_TP2) | (np.abs(facing) < TIE_FACING))
    return out, tie
