"""Inputs of tests/test_gpu_bump.py and tests/test_bump_cpu.py: the query mesh
of the lookup comparison, the mapped Cornell box, the lit quad of the
visible-effect test and the tiny OBJ/MTL/PNG model, all generated from fixed
seeds (nothing here needs a GPU but chain())."""
import math
import os

import numpy as np

from montecarlopathtracing_amd import _lib as L
from montecarlopathtracing_amd import scene as S

from . import scenes
from . import smooth_ref as SR
from . import texture_ref as T

MAX_TILT = 80.0  # degrees, the lookup comparison's steepest texel


def random_normal_map(h, w, max_tilt, seed):
    """(h, w, 3) float32 unit normals with z > 0: tilts uniform in [0, max_tilt]
    degrees, any azimuth."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = np.radians(rng.uniform(0.0, max_tilt, (h, w)))
    p = rng.uniform(0.0, 2 * math.pi, (h, w))
    m = np.stack([np.sin(a) * np.cos(p), np.sin(a) * np.sin(p), np.cos(a)], axis=2)
    return np.ascontiguousarray(m.astype(np.float32))


def lookup_mesh():
    """The 80-triangle icosphere with spherical UVs (seam triangles included)
    on the 5x3 map; eight random triangles with UVs in [-2.5, 3.5] on the 2x2,
    the 1x1 and the 5x3; each of those again with two UV corners exchanged
    (mirrored UVs: h = -1 for one of each pair); two triangles with degenerate
    UVs (det = 0); unmapped triangles.  Returns (SceneData, uv, tri_map, images)."""
    ball = SR.icosphere(1)
    rng = np.random.Generator(np.random.PCG64(41))
    flat = rng.uniform(-1.0, 1.0, (8, 3, 3)).astype(np.float32) + np.float32(4.0)
    degen = rng.uniform(-1.0, 1.0, (2, 3, 3)).astype(np.float32) + np.float32(8.0)
    plain = rng.uniform(-1.0, 1.0, (4, 3, 3)).astype(np.float32) - np.float32(4.0)
    verts = np.concatenate([ball, flat, flat, degen, plain])
    n, nb = len(verts), len(ball)
    uv = np.zeros((n, 3, 2), np.float32)
    tri_map = np.full(n, -1, np.int32)
    uv[:nb] = T.spherical_uv(ball, (0, 0, 0))
    tri_map[:nb] = 2
    fuv = rng.uniform(-2.5, 3.5, (8, 3, 2)).astype(np.float32)
    uv[nb:nb + 8] = fuv
    uv[nb + 8:nb + 16] = fuv[:, [0, 2, 1]]  # the same triangle with mirrored UVs
    for base in (nb, nb + 8):
        tri_map[base:base + 3], tri_map[base + 3:base + 5], tri_map[base + 5:base + 8] = 1, 0, 2
    uv[nb + 16] = np.array([[0.25, 0.125], [0.5, 0.25], [0.75, 0.375]], np.float32)  # collinear UVs: det = 0
    uv[nb + 17] = np.array([[0.5, 0.5], [0.5, 0.5], [0.1, 0.9]], np.float32)
    tri_map[nb + 16:nb + 18] = 2
    images = [random_normal_map(1, 1, MAX_TILT, 42), random_normal_map(2, 2, MAX_TILT, 43),
              random_normal_map(3, 5, MAX_TILT, 44)]
    seams = (uv[:nb, :, 0].max(1) - uv[:nb, :, 0].min(1)) > 0.5
    assert seams.sum() >= 4
    mats = np.zeros(1, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    data = S.SceneData.from_arrays(verts, np.zeros(n, np.int32), mats)
    return data, uv, tri_map, images


def lookup_queries(data):
    """(tri ids, points, dirs, normals) float32: per triangle 40 points (interior,
    corners, edges, outside), each with a ray from the front or the back within
    60 degrees of the face normal; N is the ray-facing face normal for one half
    of the queries and a unit vector up to 35 degrees from it (an interpolated
    normal's place) for the other."""
    nt = len(data.tris)
    v = data.tris["v"][:, :, :3].astype(np.float64)
    ng = data.tris["normal"][:, :3].astype(np.float32).astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(45))
    per = 40
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5],
                      [1.05, -.05, 0], [-.03, -.02, 1.05]], np.float64)
    b = np.concatenate([rng.dirichlet((1.0, 1.0, 1.0), (nt, per - len(fixed))),
                        np.broadcast_to(fixed, (nt, len(fixed), 3))], axis=1)
    pts = np.einsum("tkc,tcx->tkx", b, v).reshape(-1, 3)
    ids = np.repeat(np.arange(nt, dtype=np.int32), per)
    q = len(ids)
    g = ng[ids]

    def cone(axis, max_deg):  # unit vectors within max_deg of each axis
        a = np.radians(rng.uniform(0.0, max_deg, q))
        p = rng.uniform(0.0, 2 * math.pi, q)
        ref = np.where(np.abs(axis[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
        s = np.cross(axis, ref)
        s /= np.sqrt((s * s).sum(1, keepdims=True))
        t = np.cross(axis, s)
        return (np.cos(a)[:, None] * axis + np.sin(a)[:, None] * (np.cos(p)[:, None] * s + np.sin(p)[:, None] * t))
    side = np.where(rng.random(q) < 0.5, 1.0, -1.0)[:, None]  # +1: the ray sees the front
    facing = side * g
    dirs = -cone(facing, 60.0)
    interp = rng.random(q) < 0.5
    normals = np.where(interp[:, None], cone(facing, 35.0), facing)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return ids, f32(pts), f32(dirs), f32(normals)


def mesh_arrays(data):
    """(verts (n, 3, 3), ng (n, 3)) float32 of a SceneData: what bump_ref takes."""
    return data.tris["v"][:, :, :3].copy(), data.tris["normal"][:, :3].copy()


# ------------------------------------------------------------ mapped Cornell box
def box_uv(verts, scale):
    """Box-projection UVs: each triangle's corners projected along the axis its
    face normal is closest to, times `scale`."""
    v = np.asarray(verts, np.float64)
    n = np.abs(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    ax = n.argmax(1)
    ua, va = (ax + 1) % 3, (ax + 2) % 3
    i = np.arange(len(v))[:, None]
    k = np.arange(3)[None, :]
    return (np.stack([v[i, k, ua[:, None]], v[i, k, va[:, None]]], axis=-1) * scale).astype(np.float32)


def cbox_maps(tilt=50.0):
    """(uv, tri_map, images) for scenes.cbox(): box-projection UVs (several
    repeats per wall) and a small random normal map on every triangle but the
    light's, one triangle in eight unmapped."""
    data = scenes.cbox()
    verts = data.tris["v"][:, :, :3]
    uv = box_uv(verts, 1.0 / 170.0)
    n = len(verts)
    tri_map = np.where(np.arange(n) % 8 == 5, -1, np.arange(n) % 2).astype(np.int32)
    images = [random_normal_map(3, 4, tilt, 46), random_normal_map(2, 2, tilt, 47)]
    return uv, tri_map, images


def cbox_textures():
    """(uv, tri_tex, images): a random diffuse texture on the box, on other UVs."""
    n = len(scenes.cbox().tris)
    rng = np.random.Generator(np.random.PCG64(48))
    uv = rng.uniform(-1.0, 2.0, (n, 3, 2)).astype(np.float32)
    return uv, (np.arange(n) % 3 - 1).clip(-1, 0).astype(np.int32), [rng.uniform(0.1, 1.0, (3, 5, 3)).astype(np.float32)]


# ------------------------------------------------------------------ the lit quad
LIT_W, LIT_H = 16, 8
LIT_TILT = 60.0
LIT_KD, LIT_KA = 0.8, 10.0
LIT_CAM = {"position": [0, 3, 0.001], "lookat": [0, 0, 0], "up": [0, 0, -1], "fov": 40.0}
LIT_QUAD = ((-2.0, 2.0), (-1.0, 1.0))      # x and z extent at y = 0
LIT_LIGHT = ((-1.0, 1.0), (-1.0, 1.0), 8.0)  # x and z extent, y


def lit_quad():
    """(SceneData, uv, tri_map, images): a diffuse 4 x 2 quad at y = 0 with UVs
    0..1 across it (u along +x, v along -z... v = (1 - z) / 2), under a 2 x 2
    emissive rectangle at y = 8; an 8x2 map whose left four columns are tilted
    LIT_TILT degrees towards +u and whose right four are (0, 0, 1)."""
    (x0, x1), (z0, z1) = LIT_QUAD
    (lx0, lx1), (lz0, lz1), ly = LIT_LIGHT
    quad = np.array([[[x0, 0, z0], [x0, 0, z1], [x1, 0, z1]], [[x0, 0, z0], [x1, 0, z1], [x1, 0, z0]]], np.float32)
    light = np.array([[[lx0, ly, lz0], [lx1, ly, lz1], [lx0, ly, lz1]], [[lx0, ly, lz0], [lx1, ly, lz0], [lx1, ly, lz1]]],
                     np.float32)
    verts = np.concatenate([quad, light])
    uv = np.zeros((4, 3, 2), np.float32)
    uv[:2, :, 0] = (quad[..., 0] - x0) / (x1 - x0)
    uv[:2, :, 1] = (z1 - quad[..., 2]) / (z1 - z0)
    a = math.radians(LIT_TILT)
    img = np.zeros((2, 8, 3), np.float64)
    img[:, :4] = (math.sin(a), 0.0, math.cos(a))
    img[:, 4:] = (0.0, 0.0, 1.0)
    mats = np.zeros(2, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (LIT_KD,) * 3, (0, 0, 0), 1.0)
    mats[1] = S.classify_material(1.0, (LIT_KA,) * 3, (0, 0, 0), (0, 0, 0), 1.0)
    assert int(mats[0]["type"]) == L.MCPT_DIFFUSE and int(mats[1]["type"]) == L.MCPT_LIGHT
    data = S.SceneData.from_arrays(verts, np.array([0, 0, 1, 1], np.int32), mats)
    return data, uv, np.array([0, 0, -1, -1], np.int32), [img.astype(np.float32)]


def lit_theta():
    """The largest angle (radians) between +y and a direction from a point of
    the quad to a point of the light: attained between corners (the height is
    fixed and the horizontal offset is convex in both points), float64."""
    (x0, x1), (z0, z1) = LIT_QUAD
    (lx0, lx1), (lz0, lz1), ly = LIT_LIGHT
    worst = 0.0
    for px in (x0, x1):
        for pz in (z0, z1):
            for qx in (lx0, lx1):
                for qz in (lz0, lz1):
                    worst = max(worst, math.atan2(math.hypot(qx - px, qz - pz), ly))
    return worst


# ----------------------------------------------------------- OBJ / MTL / PNG model
BUMP_OBJ = """mtllib b.mtl
v -1 0 -1
v -1 0 1
v 1 0 1
v 1 0 -1
v -0.6 2.5 -0.6
v 0.6 2.5 -0.6
v 0.6 2.5 0.6
v -0.6 2.5 0.6
v -1 0 -1
v 1 0 -1
v 1 2 -1
v -1 2 -1
vt 0 0
vt 0 2
vt 2 2
vt 2 0
usemtl floor
f 1/1 2/2 3/3 4/4
usemtl light
f 5 6 7 8
usemtl wall
f 9/1 10/4 11/3 12/2
"""
BUMP_MTL = """newmtl floor
Kd 0.8 0.8 0.8
map_Bump -bm 3 -clamp on tex\\height.png
newmtl light
Ka 10 10 10
Kd 0 0 0
newmtl wall
Kd 0.7 0.7 0.7
bump tex/height.png
norm tex/normal.png
"""


def write_model(tmp_path, **extra):
    """The tiny model in tmp_path/model with an 8-bit height map and an 8-bit
    normal map; returns a config dict with one entry (plus `extra` keys)."""
    d = tmp_path / "model"
    os.makedirs(d / "tex")
    (d / "b.obj").write_text(BUMP_OBJ)
    (d / "b.mtl").write_text(BUMP_MTL)
    yy, xx = np.mgrid[0:6, 0:4]
    hgt = np.zeros((6, 4, 4), np.float32)
    hgt[..., :3] = (((xx * 3 + yy * 5) % 7) / 6.0)[..., None]
    S.write_png(str(d / "tex" / "height.png"), hgt, flip=False)
    nrm = np.zeros((5, 3, 4), np.float32)
    nrm[..., :3] = random_normal_map(5, 3, 50.0, 49) * 0.5 + 0.5
    S.write_png(str(d / "tex" / "normal.png"), nrm, flip=False)
    e = {"bvhtype": "hlbvh", "width": 32, "height": 32, "platform": "amd", "directory": str(d) + "/",
         "objname": "b.obj", "maxdepth": 4, "attempt": 3, "raygenerator": "", "intersect": "", "shade": "",
         "camera": {"position": [0, 1.2, 3.5], "lookat": [0, 0.6, 0], "up": [0, 1, 0], "fov": 45.0,
                    "resolution": [32, 32]},
         "opencl": True}
    e.update(extra)
    return {"configid": 0, "config": [e]}


# ------------------------------------------------------------------------ chain
def chain(rnd, dsc, cam, w, h, depth, attempt, frames, seeds, mode=L.MODE_EXACT, jitter=False, lens=None):
    """The frame loop out of the wavefront kernels (tests/test_gpu_jitter.py's
    chain, with the thin lens as well): generate -> (intersect -> shade) x depth
    -> accumulate.  Returns (hist, count, seeds) as numpy."""
    import torch
    n = w * h
    d_seed = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(rnd.device)
    hist = torch.zeros((n, 4), dtype=torch.float32, device=rnd.device)
    count = torch.zeros(n, dtype=torch.int32, device=rnd.device)
    for f in range(frames):
        colors = torch.ones((n, 4), dtype=torch.float32, device=rnd.device)
        if lens is not None:
            rays = rnd.generate_rays_lens(cam, w, h, d_seed, lens)
        elif jitter:
            rays = rnd.generate_rays_jittered(cam, w, h, d_seed)
        else:
            rays = rnd.generate_rays(cam, w, h)
        hits = None
        for _b in range(depth):
            hits = rnd.intersect(dsc, rays, hits=hits, mode=mode)
            rnd.shade(dsc, rays, hits, colors, d_seed, depth)
        if f <= attempt:
            rnd.accumulate(colors, hist, count, attempt)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), count.cpu().numpy(), d_seed.cpu().numpy().view(np.uint32)


def debug_main(config_path):
    """Child process of tests/test_gpu_bump.py (python -c): the model of
    `config_path` (its "bump" key set) rendered by the MCPT_DEBUG build of the
    library (MCPT_LIB_OVERRIDE), whose k_render checks the record and texel
    indices of every lookup.  Prints one JSON line per node format with the
    violation count and a digest of the result."""
    import hashlib
    import json

    import torch

    from montecarlopathtracing_amd import render as RR
    from montecarlopathtracing_amd.app import App
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    app = App(config_path)
    app.init()
    assert app.mapped
    rnd, cfg = app.renderer, app.cfg
    for quantized in (2, 1, 3):
        rnd.set_tuning(quantized=quantized)
        st = rnd.new_state(app.w, app.h, RR.default_seeds(app.w * app.h))
        rnd.render_frames(app.scene, app.camera, st, cfg.MAXDEPTH(), cfg.MAXATTEPMT(), cfg.MAXATTEPMT() + 1)
        s = rnd.stats()
        torch.cuda.synchronize()
        dg = hashlib.sha256()
        for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
            dg.update(np.ascontiguousarray(a).tobytes())
        print(json.dumps({"quantized": quantized, "node_format": s["node_format"], "violations": s["debug_violations"],
                          "digest": dg.hexdigest()}), flush=True)
