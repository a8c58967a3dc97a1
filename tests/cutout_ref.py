"""Float64 restatement of the alpha cutouts (include/mcpt_hip.h at
mcpt_scene_set_texture_alpha; csrc/mcpt_texture.h on the device), the yardstick
of tests/test_gpu_cutout.py and tests/test_cutout_cpu.py, with the scenes both
use.  The alpha at a hit is the texture lookup of tests/texture_ref.py applied
to a one-channel image; a hit is cut when alpha < a0 (and the pass count is
below 255)."""
import numpy as np

from . import texture_ref as T

MUTANTS = ("nearest", "no_flip")
PASS_CAP = 255  # a path's cut hits: the 256th is shaded as if opaque


def alpha_at(verts, uv, tri_tex, alphas, ids, pts, mutant=None):
    """The alpha (m,) float64 for queries (ids, pts) on a mesh: verts (n, 3, 3),
    uv (n, 3, 2), tri_tex (n,), alphas: one (H, W) image or None (opaque) per
    texture.  An untextured triangle and an opaque texture give 1."""
    imgs = [np.ones((1, 1, 3)) if a is None else np.repeat(np.asarray(a, np.float64)[..., None], 3, axis=2) for a in alphas]
    return T.texture_factor(verts, uv, tri_tex, imgs, ids, pts, mutant=mutant)[:, 0]


def resample(a, height, width):
    """An alpha image at the texel centres of a (height, width) texture: the
    lookup's repeating bilinear filter, float64 (scene.resample_alpha's rule)."""
    u = (np.arange(width, dtype=np.float64) + 0.5) / width
    v = 1.0 - (np.arange(height, dtype=np.float64) + 0.5) / height
    uu, vv = np.meshgrid(u, v)
    img = np.repeat(np.asarray(a, np.float64)[..., None], 3, axis=2)
    return T.sample(img, uu.reshape(-1), vv.reshape(-1))[:, 0].reshape(height, width)


# --------------------------------------------------------------- small scenes
def _quad(x0, x1, y0, y1, z):
    """Two triangles of the rectangle [x0, x1] x [y0, y1] at depth z, and their
    UVs: (0, 0) at (x0, y0), (1, 1) at (x1, y1)."""
    p = lambda x, y: [x, y, z]  # noqa: E731
    v = np.array([[p(x0, y0), p(x1, y0), p(x1, y1)], [p(x0, y0), p(x1, y1), p(x0, y1)]], np.float32)
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    return v, uv


HOLE_ENV = (0.25, 0.5, 0.75)
HOLE_DEPTH = 3
HOLE_W = HOLE_H = 16


def hole_camera():
    """An orthographic camera (camera_type 1) looking down -z at the square
    [-1, 1]^2 from z = 4.  A pixel's ray starts at its corner (idx / W - 0.5)
    * arg, so with arg = 2 and 16 pixels the rays lie 1 / 8 apart; the camera
    stands 1 / 32 right of and above the axis, which keeps every ray 1 / 32 from
    the quads' outer edges and from the edge they share."""
    from montecarlopathtracing_amd import scene as S
    cam = S.parse_camera({"position": [1.0 / 32, 1.0 / 32, 4.0], "lookat": [1.0 / 32, 1.0 / 32, 0.0], "up": [0, 1, 0],
                          "fov": 90.0})
    cam["camera_type"] = 1
    cam["arg"] = 2.0
    return cam


def hole_scene(alpha_image=None, delete=False, left_kd=0.7):
    """Two coplanar quads (z = 0) in front of a light quad (z = -2), to be put
    under a constant environment: the left quad (x in [-1, 0]) carries texture
    0, a 1x1 of ones whose alpha is 0 (or `alpha_image`, any size), the right
    one (x in [0, 1]) texture 1, a 1x1 of ones with alpha 1 on a material whose
    kd is 0.  delete: the mesh without the left quad's triangles.  left_kd: the
    left quad's diffuse kd.  Returns (SceneData, uv, tri_tex, images,
    alphas, verts)."""
    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import scene as S
    lv, luv = _quad(-1.0, 0.0, -1.0, 1.0, 0.0)
    rv, ruv = _quad(0.0, 1.0, -1.0, 1.0, 0.0)
    gv, guv = _quad(-3.0, 3.0, -3.0, 3.0, -2.0)
    mats = np.zeros(3, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (left_kd,) * 3, (0, 0, 0), 1.0)  # the cut quad
    mats[1] = S.classify_material(1.0, (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0)        # kd 0: every path through it is black
    mats[2] = S.classify_material(1.0, (5, 4, 3), (0, 0, 0), (0, 0, 0), 1.0)        # the light
    assert int(mats[2]["type"]) == L.MCPT_LIGHT and int(mats[1]["type"]) == L.MCPT_DIFFUSE
    parts = ([] if delete else [(lv, luv, 0, 0)]) + [(rv, ruv, 1, 1), (gv, guv, 2, -1)]
    verts = np.concatenate([p[0] for p in parts])
    uv = np.concatenate([p[1] for p in parts])
    mat_index = np.concatenate([np.full(2, p[2], np.int32) for p in parts])
    tri_tex = np.concatenate([np.full(2, p[3], np.int32) for p in parts])
    a0 = np.zeros((1, 1), np.float32) if alpha_image is None else np.asarray(alpha_image, np.float32)
    images = [np.ones(a0.shape + (3,), np.float32), np.ones((1, 1, 3), np.float32)]
    alphas = [a0, np.ones((1, 1), np.float32)]
    data = S.SceneData.from_arrays(verts, mat_index, mats)
    return data, uv, tri_tex, images, alphas, verts


def edge_alpha():
    """4x4: the left two columns alpha 0, the right two alpha 1."""
    a = np.ones((4, 4), np.float32)
    a[:, :2] = 0.0
    return a


# The edge test: the left quad maps u = x + 1, and hole_camera's rays cross it
# at u = k / 8 + 1 / 32, so the texel coordinate 4 u - 0.5 is k / 2 - 3 / 8.  The
# alpha crosses 0.5 at texel coordinates 1.5 and 3.5 (the repeat seam), so every
# ray's alpha is at least 0.125 away from the threshold 0.5: the reference
# leaves out no pixel.


def stack_scene(n_quads=300):
    """n parallel alpha-0 quads (z = 0, -0.01, ...) in front of a light quad:
    the cap's scene.  Quad k (from the camera) has material k % 2 (diffuse kd
    0.7 / 0.3), all carry the one 1x1 texture whose alpha is 0."""
    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import scene as S
    vs, uvs = [], []
    for k in range(n_quads):
        v, uv = _quad(-1.5, 1.5, -1.5, 1.5, -0.01 * k)
        vs.append(v), uvs.append(uv)
    gv, guv = _quad(-3.0, 3.0, -3.0, 3.0, -0.01 * n_quads - 1.0)
    verts = np.concatenate(vs + [gv])
    uv = np.concatenate(uvs + [guv])
    mat_index = np.concatenate([np.full(2, k % 2, np.int32) for k in range(n_quads)] + [np.full(2, 2, np.int32)])
    tri_tex = np.concatenate([np.zeros(2 * n_quads, np.int32), np.full(2, -1, np.int32)])
    mats = np.zeros(3, L.MATERIAL)
    mats[0] = S.classify_material(1.0, (0, 0, 0), (0.7, 0.7, 0.7), (0, 0, 0), 1.0)
    mats[1] = S.classify_material(1.0, (0, 0, 0), (0.3, 0.3, 0.3), (0, 0, 0), 1.0)
    mats[2] = S.classify_material(1.0, (5, 4, 3), (0, 0, 0), (0, 0, 0), 1.0)
    data = S.SceneData.from_arrays(verts, mat_index, mats)
    return data, uv, tri_tex, [np.ones((1, 1, 3), np.float32)], [np.zeros((1, 1), np.float32)]


# ----------------------------------------------------------------- room scene
ROOM_CAM = T.ROOM_CAM
ROOM_DEPTH = T.ROOM_DEPTH


def card_alpha(w, h, seed):
    """(h, w) float32: a checker of 0.05 / 0.95 with a per-texel variation, so
    the bilinear alpha crosses 0.5 inside the card and reaches 1.0 nowhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.where((xx + yy) & 1, 0.95, 0.05) * rng.uniform(0.9, 1.0, (h, w))).astype(np.float32)


def room(opened=False):
    """texture_ref.room's textured room with three cutout cards in it: a
    diffuse one in front of the back wall, a glossy one before the spheres and
    a light-coloured diffuse one lying above the floor, each on a texture of
    its own whose alpha is a checker (card_alpha); the textured floor gets an
    alpha too, the other textures none.  Returns (SceneData, uv, tri_tex,
    images, alphas)."""
    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import scene as S
    data, uv, tri_tex, images = T.room(opened=opened)
    verts = data.tris["v"][:, :, :3].copy()
    mat_index = np.ascontiguousarray(data.tris["normal"][:, 3]).view(np.int32).copy()
    nm = len(data.mats)
    mats = np.zeros(nm + 2, L.MATERIAL)
    mats[:nm] = data.mats
    mats[nm] = S.classify_material(1.0, (0, 0, 0), (0.8, 0.7, 0.3), (0, 0, 0), 1.0)
    mats[nm + 1] = S.classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 8.0)
    assert int(mats[nm + 1]["type"]) == L.MCPT_GLOSSY
    cards = []
    # the room is x in [-2, 2], y in [0, 3], z in [-2, 4], the camera at z = 3.6 looking down -z, the spheres
    # at z <= 1: two upright cards between the camera and the spheres
    for z, mat, xs, ys in ((1.5, nm, (-1.5, 0.2), (0.6, 2.2)), (2.3, nm + 1, (-0.2, 1.4), (0.6, 2.0))):
        v, t = _quad(xs[0], xs[1], ys[0], ys[1], z)
        cards.append((v, t * np.float32(1.7) - np.float32(0.2), mat))
    # and one lying flat above the floor, in front of them
    y = 0.4
    fv = np.array([[[-1.2, y, 1.2], [1.2, y, 1.2], [1.2, y, 2.6]], [[-1.2, y, 1.2], [1.2, y, 2.6], [-1.2, y, 2.6]]], np.float32)
    cards.append((fv, _quad(0, 1, 0, 1, 0)[1] * np.float32(2.0), nm))
    images = list(images)
    alphas = [None] * len(images)
    alphas[1] = card_alpha(images[1].shape[1], images[1].shape[0], 40)  # the floor's own texture
    for k, (v, t, mat) in enumerate(cards):
        w, h = ((5, 4), (3, 3), (6, 2))[k]
        images.append(T.checker(w, h, (0.9, 0.9, 0.9), (0.4, 0.6, 0.9), 50 + k))
        alphas.append(card_alpha(w, h, 60 + k))
        verts = np.concatenate([verts, v])
        uv = np.concatenate([uv, t.astype(np.float32)])
        mat_index = np.concatenate([mat_index, np.full(2, mat, np.int32)])
        tri_tex = np.concatenate([tri_tex, np.full(2, len(images) - 1, np.int32)])
    out = S.SceneData.from_arrays(verts, mat_index, mats)
    return out, uv, tri_tex, images, alphas


def debug_main():
    """Child process of tests/test_gpu_cutout.py (python -c): the cutout room
    rendered by the MCPT_DEBUG build of the library (MCPT_LIB_OVERRIDE).  Prints
    one JSON line per (mode, node format) with the violation count and a digest
    of the result."""
    import hashlib
    import json

    import torch

    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import render as RR
    from montecarlopathtracing_amd import scene as S
    rnd = RR.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 32, 24, 4, 2  # tests/test_gpu_cutout.py: W, H, FRAMES, ATT
    data, uv, tri_tex, images, alphas = room()
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    rnd.set_texture_alpha(dsc, alphas, 0.5)
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
