"""Float64 restatement of the diffuse-texture lookup (include/mcpt_hip.h at
mcpt_scene_set_textures; csrc/mcpt_texture.h on the device), the yardstick of
tests/test_gpu_texture.py and tests/test_texture_cpu.py, with the deliberate
mistakes the GPU test must reject, and the textured room both render."""
import math

import numpy as np

from . import smooth_ref as SR

MUTANTS = ("swap_uv", "no_flip", "nearest", "swap_b", "clamp")


def barycentrics(v0, v1, v2, pt, swap=False):
    """(b0, b1, b2) of the smooth lookup for m queries ((m, 3) each), float64;
    den zero or not finite gives b1 = b2 = 0."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    v0, v1, v2, pt = map(f, (v0, v1, v2, pt))
    dot = lambda a, b: (a * b).sum(1)  # noqa: E731
    e1, e2, w = v1 - v0, v2 - v0, pt - v0
    d11, d12, d22, w1, w2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(w, e1), dot(w, e2)
    den = d11 * d22 - d12 * d12
    with np.errstate(all="ignore"):
        b1 = np.clip((d22 * w1 - d12 * w2) / den, 0.0, 1.0)
        b2 = np.clip((d11 * w2 - d12 * w1) / den, 0.0, 1.0)
    bad = ~(np.isfinite(den) & (den != 0))
    b1, b2 = np.where(bad, 0.0, b1), np.where(bad, 0.0, b2)
    if swap:
        b1, b2 = b2, b1
    return np.maximum(0.0, 1.0 - b1 - b2), b1, b2


def sample(image, u, v, mutant=None):
    """The lookup of one texture ((H, W, 3), row 0 the top) at m (u, v) pairs,
    float64: (m, 3)."""
    img = np.asarray(image, np.float64)
    hh, ww = img.shape[:2]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if mutant == "swap_uv":
        u, v = v, u
    if mutant == "clamp":
        u, v = np.clip(u, 0.0, 1.0), np.clip(v, 0.0, 1.0)
    else:
        u, v = u - np.floor(u), v - np.floor(v)
    x = u * ww - 0.5
    y = (v if mutant == "no_flip" else 1.0 - v) * hh - 0.5
    if mutant == "nearest":
        x, y = np.floor(x + 0.5), np.floor(y + 0.5)
    i0, j0 = np.floor(x), np.floor(y)
    fx, fy = (x - i0)[:, None], (y - j0)[:, None]
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    if mutant == "clamp":
        wrap_x = lambda i: np.clip(i, 0, ww - 1)  # noqa: E731
        wrap_y = lambda j: np.clip(j, 0, hh - 1)  # noqa: E731
    else:
        wrap_x = lambda i: i % ww  # noqa: E731
        wrap_y = lambda j: j % hh  # noqa: E731
    i1, j1, i0, j0 = wrap_x(i0 + 1), wrap_y(j0 + 1), wrap_x(i0), wrap_y(j0)
    t00, t10, t01, t11 = img[j0, i0], img[j0, i1], img[j1, i0], img[j1, i1]
    return (1 - fx) * (1 - fy) * t00 + fx * (1 - fy) * t10 + (1 - fx) * fy * t01 + fx * fy * t11


def texture_factor(verts, uv, tri_tex, images, ids, pts, mutant=None):
    """The factor (m, 4) float64 for queries (ids, pts) on a mesh: verts (n, 3,
    3), uv (n, 3, 2), tri_tex (n,), images: list of (H, W, 3)."""
    ids = np.asarray(ids, np.int64)
    v = np.asarray(verts, np.float64)[ids]
    b0, b1, b2 = barycentrics(v[:, 0], v[:, 1], v[:, 2], pts, swap=mutant == "swap_b")
    t = np.asarray(uv, np.float64)[ids]
    u = b0 * t[:, 0, 0] + b1 * t[:, 1, 0] + b2 * t[:, 2, 0]
    w = b0 * t[:, 0, 1] + b1 * t[:, 1, 1] + b2 * t[:, 2, 1]
    out = np.ones((len(ids), 4), np.float64)
    tt = np.asarray(tri_tex)[ids]
    for k, img in enumerate(images):
        m = tt == k
        if m.any():
            out[m, :3] = sample(img, u[m], w[m], mutant)
    return out


# ----------------------------------------------------------------- room scene
ROOM_CAM = SR.ROOM_CAM
ROOM_DEPTH = 6


def spherical_uv(verts, center):
    """(n, 3, 2) lat-long UVs of (n, 3, 3) corners about `center`; a triangle
    across the seam keeps its corners' own u (one corner near 0, the others
    near 1: the seam triangle, interpolated the long way round, as a naive
    exporter writes it)."""
    r = SR.radial(verts, center)
    u = np.arctan2(r[..., 2], r[..., 0]) / (2 * math.pi) + 0.5
    v = np.arccos(np.clip(r[..., 1], -1, 1)) / math.pi
    return np.stack([u, 1.0 - v], axis=-1).astype(np.float32)


def checker(w, h, lo=(0.05, 0.1, 0.9), hi=(0.9, 0.8, 0.1), seed=3):
    """(h, w, 3) float32: a two-colour checker with a small per-texel variation."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.where(((xx + yy) & 1)[..., None] == 0, np.array(lo), np.array(hi))
    return (base * rng.uniform(0.8, 1.0, (h, w, 1))).astype(np.float32)


def room_images():
    return [checker(5, 3), checker(8, 8, (0.9, 0.2, 0.2), (0.2, 0.9, 0.3), 4), checker(2, 2, (1, 1, 1), (0.3, 0.3, 0.9), 5)]


def room(opened=False):
    """smooth_ref.room's closed 4 x 3 x 6 room with textures: the floor is
    glossy and textured (UVs beyond [0, 1]: it repeats), the back and left
    walls diffuse and textured, the right wall, the ceiling and the wall behind
    the camera untextured; the diffuse icosphere carries spherical UVs (with
    their seam triangles), the glossy one too, the glass one none.  Returns
    (SceneData, uv, tri_tex, images)."""
    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import scene as S
    data, first_ball, nb = SR.room(opened=opened)
    n = len(data.tris)
    verts = data.tris["v"][:, :, :3].copy()
    mat_index = np.ascontiguousarray(data.tris["normal"][:, 3]).view(np.int32).copy()
    mats = np.zeros(6, L.MATERIAL)
    mats[:5] = data.mats
    mats[5] = S.classify_material(1.0, (0, 0, 0), (0.6, 0.6, 0.6), (0.4, 0.4, 0.4), 12.0)  # the glossy floor
    assert int(mats[5]["type"]) == L.MCPT_GLOSSY
    mat_index[0:2] = 5
    uv = np.zeros((n, 3, 2), np.float32)
    tri_tex = np.full(n, -1, np.int32)
    uv[0:2, :, 0], uv[0:2, :, 1] = verts[0:2, :, 0] * 0.9 - 0.3, verts[0:2, :, 2] * 0.7 + 0.1  # floor: x, z; repeats
    tri_tex[0:2] = 1
    uv[2:4, :, 0], uv[2:4, :, 1] = verts[2:4, :, 0] * 0.25 + 0.5, verts[2:4, :, 1] / 3.0  # back wall: once across
    tri_tex[2:4] = 0
    uv[4:6, :, 0], uv[4:6, :, 1] = verts[4:6, :, 2] * -0.5, verts[4:6, :, 1] * 1.5  # left wall: negative u
    tri_tex[4:6] = 2
    for k, tex in ((0, 0), (1, 1)):
        s = slice(first_ball + k * nb, first_ball + (k + 1) * nb)
        uv[s] = spherical_uv(verts[s], SR.ROOM_SPHERES[k][0])
        tri_tex[s] = tex
    out = S.SceneData.from_arrays(verts, mat_index, mats)
    return out, uv, tri_tex, room_images()


def debug_main():
    """Child process of tests/test_gpu_texture.py (python -c): the textured
    room rendered by the MCPT_DEBUG build of the library (MCPT_LIB_OVERRIDE),
    whose k_render checks the record and texel indices of every lookup.
    Prints one JSON line per (mode, node format) with the violation count and
    a digest of the result."""
    import hashlib
    import json

    import torch

    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import render as RR
    from montecarlopathtracing_amd import scene as S
    rnd = RR.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 48, 40, 6, 4  # tests/test_gpu_texture.py: W, H, FRAMES, ATT
    data, uv, tri_tex, images = room()
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    for mode, quantized in ((L.MODE_EXACT, 2), (L.MODE_EXACT, 1), (L.MODE_EXACT, 3), (L.MODE_NOPRUNE, 2)):
        rnd.set_tuning(quantized=quantized)
        st = rnd.new_state(w, h, RR.default_seeds(w * h))
        rnd.render_frames(dsc, S.parse_camera(ROOM_CAM), st, ROOM_DEPTH, att, frames, mode=mode)
        s = rnd.stats()
        torch.cuda.synchronize()
        dg = hashlib.sha256()
        for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
            dg.update(np.ascontiguousarray(a).tobytes())
        print(json.dumps({"mode": mode, "quantized": quantized, "node_format": s["node_format"],
                          "violations": s["debug_violations"], "digest": dg.hexdigest()}), flush=True)
    dsc.close()
