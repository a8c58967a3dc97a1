"""The thin-lens camera of include/mcpt_hip.h (mcpt_render_frames_lens) in
float64, and its draw sequence: the yardstick of mcpt_generate_rays_lens
(tests/test_gpu_lens.py) and the subject of tests/test_lens_cpu.py.  No GPU.

Per pixel and frame the seed chain gives jx, jy (the jitter's draws, taken
from tests/test_jitter_cpu.py) and then r1, r2; the lens sample is
rho = sqrt(r1 / 2^15), phi = 2 pi r2 / 2^15, (a, b) = rho (cos phi, sin phi);
with (o, d) the camera's ray through (idx + jx, idy + jy):

    k = F / dot(d, c^),  P = o + k d,  o' = o + R (a h^ + b u^),  d' = normalize(P - o')

`mutant` swaps one step for a plausible mistake (MUTANTS); the GPU test shows
that its tolerance tells each of them from the definition."""
import numpy as np

from .test_jitter_cpu import jitter_draws, lcg

MUTANTS = ("unnormalised", "focus_along_ray", "rho_linear", "offset_sign")


def lens_draws(seeds):
    """A lens frame start's four draws: (jx, jy, r1, r2, seeds after); jx, jy
    as jitter_draws gives them, r1 and r2 the next two 15-bit draws (ints)."""
    jx, jy, s2 = jitter_draws(seeds)
    s3 = lcg(s2)
    s4 = lcg(s3)
    r1 = ((s3 >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.int64)
    r2 = ((s4 >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.int64)
    return jx, jy, r1, r2, s4


def disk_sample(r1, r2, mutant=None):
    """(a, b): the unit disk's point of two 15-bit draws."""
    u = np.asarray(r1, np.float64) / 32768.0
    rho = u if mutant == "rho_linear" else np.sqrt(u)
    phi = 2.0 * np.pi * np.asarray(r2, np.float64) / 32768.0
    return rho * np.cos(phi), rho * np.sin(phi)


def unit(v):
    v = np.asarray(v, np.float64)[..., :3]
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def camera_rays(cam, w, h, sx, sy):
    """rayGenerator.cl in float64 on sample positions (sx, sy) in pixels:
    (o, d), each (n, 3), d a unit vector.  cam: one L.CAMERA record."""
    c = np.asarray(cam).reshape(-1)[0]
    cdir, chor, cup, ccen = (c[k].astype(np.float64)[:3] for k in ("direction", "horizontal", "up", "center"))
    px, py = (np.asarray(sx, np.float64) / w)[:, None], (np.asarray(sy, np.float64) / h)[:, None]
    ratio, arg = w / h, float(c["arg"])
    if int(c["camera_type"]) == 0:
        dd = cdir * (0.5 / np.tan(arg / 2)) + (px - 0.5) * chor * ratio + (py - 0.5) * cup
        o = np.broadcast_to(ccen, dd.shape).copy()
    else:
        o = ccen + (px - 0.5) * arg * chor * ratio + (py - 0.5) * arg * cup
        dd = np.broadcast_to(cdir, o.shape).copy()
    return o, unit(dd)


def lens_ray(cam, o, d, a, b, radius, focus, mutant=None):
    """The lens ray (o', d') of camera ray (o, d) and disk point (a, b), and
    the sample's focus-plane point P."""
    c = np.asarray(cam).reshape(-1)[0]
    ch, hh, uh = unit(c["direction"]), unit(c["horizontal"]), unit(c["up"])
    if mutant == "unnormalised":
        hh, uh = c["horizontal"].astype(np.float64)[:3], c["up"].astype(np.float64)[:3]
    k = focus / (d * ch).sum(axis=-1, keepdims=True)
    if mutant == "focus_along_ray":
        k = np.full_like(k, focus)
    P = o + k * d
    off = radius * (np.asarray(a)[..., None] * hh + np.asarray(b)[..., None] * uh)
    if mutant == "offset_sign":
        off = -off
    o2 = o + off
    return o2, unit(P - o2), P


def lens_rays(cam, w, h, seeds, radius, focus, mutant=None):
    """mcpt_generate_rays_lens in float64: (o', d', seeds after) for every
    pixel of a w x h image, row-major.  The sample position is formed in
    float32 as the kernel forms it ((float)idx + jx is exact there or rounds
    once), everything after in float64."""
    n = w * h
    jx, jy, r1, r2, after = lens_draws(np.asarray(seeds, np.uint32))
    idx = (np.arange(n) % w).astype(np.float32)
    idy = (np.arange(n) // w).astype(np.float32)
    o, d = camera_rays(cam, w, h, (idx + jx).astype(np.float64), (idy + jy).astype(np.float64))
    a, b = disk_sample(r1, r2, mutant)
    o2, d2, _ = lens_ray(cam, o, d, a, b, radius, focus, mutant)
    return o2, d2, after


def ray_error(got_o, got_d, want_o, want_d):
    """One number for a ray set against the restatement: the largest absolute
    error of a direction component, or of an origin component relative to the
    origins' largest magnitude (at least 1): what float32 can hold of each."""
    scale = max(1.0, float(np.abs(want_o).max()))
    eo = float(np.abs(np.asarray(got_o, np.float64) - want_o).max()) / scale
    ed = float(np.abs(np.asarray(got_d, np.float64) - want_d).max())
    return max(eo, ed)


# ---------------------------------------------------------------- the lit half-space
# One emissive rectangle (two triangles, ka = 1) covering x >= 0 of a pinhole
# camera's view, nothing else: a ray ends on the light or misses, so a frame
# draws exactly four numbers and count = the frames whose lens ray hit.
EDGE_W, EDGE_H, EDGE_FRAMES = 48, 16, 16
EDGE_FOV = 30.0
EDGE_F = 10.0         # focus distance
EDGE_R = 1.3          # lens radius: a blur disk of 2 R at depth 2 F, 3.9 pixels wide.  With 16 frames a
# rim pixel whose share of the disk is under a sixteenth often shows nothing, so a row shows about a pixel
# less than the disk is wide; a wider disk loses more a side and no longer keeps "diameter - 2" in every row
# (checked on the prediction itself, tests/test_lens_cpu.py)
EDGE_X, EDGE_Y = 200.0, 100.0   # the rectangle: 0 <= x <= EDGE_X, |y| <= EDGE_Y (its diagonal leaves the view)
# the camera looks down +z from a little left of the edge, which then falls inside a pixel
EDGE_CAM = {"position": [0.13, 0, 0], "lookat": [0.13, 0, 1], "up": [0, 1, 0], "fov": EDGE_FOV}


def edge_rect(depth):
    """(2, 3, 3) float32 vertices of the rectangle at z = depth."""
    z = float(depth)
    a, b, c, d = [0, -EDGE_Y, z], [EDGE_X, -EDGE_Y, z], [EDGE_X, EDGE_Y, z], [0, EDGE_Y, z]
    return np.array([[a, b, c], [a, c, d]], np.float32)


def edge_blur_diameter_px(depth):
    """The blur disk's diameter in pixels at `depth`: 2 R |depth - F| / F in
    scene units over the pixel width there (the image is W / H wide for a
    vertical extent of 2 tan(fov / 2) at depth 1)."""
    pixel = 2.0 * np.tan(np.radians(EDGE_FOV) / 2) * (EDGE_W / EDGE_H) * depth / EDGE_W
    return 2.0 * EDGE_R * abs(depth - EDGE_F) / EDGE_F / pixel


def edge_predict(cam, seeds, depth, radius=EDGE_R, focus=EDGE_F, frames=EDGE_FRAMES, w=EDGE_W, h=EDGE_H):
    """Replay every pixel's chain in float64: (count, near, seeds after).
    count: the frames whose lens ray hits the rectangle at z = depth; near:
    the pixels with a frame whose ray passes within 1e-5 of the rectangle's
    size (its diagonal's length) of its boundary or of the triangles' shared
    diagonal, where float32 may decide otherwise."""
    seeds = np.asarray(seeds, np.uint32)
    count = np.zeros(w * h, np.int64)
    near = np.zeros(w * h, bool)
    margin = 1e-5 * float(np.hypot(EDGE_X, 2 * EDGE_Y))
    for _ in range(frames):
        o, d, seeds = lens_rays(cam, w, h, seeds, radius, focus)
        t = (depth - o[:, 2]) / d[:, 2]
        x, y = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
        inside = (x >= 0) & (x <= EDGE_X) & (np.abs(y) <= EDGE_Y) & (t > 0)
        count += inside
        # distance to the nearest boundary line, and to the diagonal (0, -Y) - (X, Y)
        to_edge = np.minimum.reduce([np.abs(x), np.abs(x - EDGE_X), np.abs(y - EDGE_Y), np.abs(y + EDGE_Y)])
        to_diag = np.abs(2 * EDGE_Y * x - EDGE_X * (y + EDGE_Y)) / np.hypot(EDGE_X, 2 * EDGE_Y)
        near |= (to_edge < margin) | (to_diag < margin)
    return count, near, seeds


# ------------------------------------------------------------------- debug build
ROOM_LENS = (0.05, 3.6)  # texture_ref.room through a lens focused at its middle


def debug_main():
    """Child process of tests/test_gpu_lens.py (python -c): a lens render of
    texture_ref's textured room by the MCPT_DEBUG build of the library
    (MCPT_LIB_OVERRIDE), whose k_render checks every stack push and node,
    triangle, record and texel index.  Prints one JSON line with the violation
    count and a digest of the result."""
    import hashlib
    import json

    import torch

    from montecarlopathtracing_amd import _lib as L
    from montecarlopathtracing_amd import render as RR
    from montecarlopathtracing_amd import scene as S

    from . import texture_ref as TR
    rnd = RR.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 37, 21, 6, 4  # tests/test_gpu_lens.py: W, H, FRAMES, ATT
    data, uv, tri_tex, images = TR.room()
    dsc = rnd.upload(data)
    rnd.set_textures(dsc, uv, tri_tex, images)
    st = rnd.new_state(w, h, RR.default_seeds(w * h))
    rnd.render_frames(dsc, S.parse_camera(TR.ROOM_CAM), st, TR.ROOM_DEPTH, att, frames, lens=ROOM_LENS)
    s = rnd.stats()
    torch.cuda.synchronize()
    dg = hashlib.sha256()
    for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
        dg.update(np.ascontiguousarray(a).tobytes())
    print(json.dumps({"violations": s["debug_violations"], "primary_cache": s["primary_cache"],
                      "digest": dg.hexdigest()}), flush=True)
