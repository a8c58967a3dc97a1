"""Scene-side host pipeline: the reference's ThirdPartyWrapper::loadObject,
Auxiliary::parseCamera, SceneCL packing and HLBVH<CPU> build, all running in
the native host half of libmcpt_hip.so (csrc/mcpt_host.cpp).

    load_object   MCPT/thirdpartywrapper.cpp:25-99
    parse_camera  MCPT/auxiliary.cpp:20-71
    pack_triangles MCPT/scenebuild.cpp:58-62
    build_hlbvh   MCPT/BVH/hlbvh.cpp:92-200
"""
import ctypes

import numpy as np

from . import _lib as L


def load_object(directory, objname):
    """OBJ + MTL -> (triangles[TRIANGLE], materials[MATERIAL], mat_index[int32])."""
    lib = L.lib()
    nt, nm = ctypes.c_int64(0), ctypes.c_int32(0)
    d, o = directory.encode(), objname.encode()
    L.check(lib.mcpt_load_obj(d, o, None, None, ctypes.byref(nt), None, ctypes.byref(nm)))
    tris = np.zeros(nt.value, L.TRIANGLE)
    idx = np.zeros(nt.value, np.int32)
    mats = np.zeros(max(nm.value, 0), L.MATERIAL)
    L.check(lib.mcpt_load_obj(d, o, L.ptr(tris), L.ptr(idx), ctypes.byref(nt), L.ptr(mats), ctypes.byref(nm)))
    return tris, mats, idx


def classify_material(ior=1.0, ambient=(0, 0, 0), diffuse=(0, 0, 0), specular=(0, 0, 0), shininess=1.0):
    """One MTL record -> Material (thirdpartywrapper.cpp:65-97)."""
    out = np.zeros(1, L.MATERIAL)
    a = np.asarray(ambient, np.float32)
    dfs = np.asarray(diffuse, np.float32)
    s = np.asarray(specular, np.float32)
    L.check(L.lib().mcpt_classify_material(float(ior), L.ptr(a), L.ptr(dfs), L.ptr(s), float(shininess), L.ptr(out)))
    return out[0]


def parse_camera(camera_json):
    """JSON camera object (position/lookat/up/fov) -> Camera record."""
    pos = np.asarray(camera_json["position"], np.float64)
    look = np.asarray(camera_json["lookat"], np.float64)
    up = np.asarray(camera_json["up"], np.float64)
    out = np.zeros(1, L.CAMERA)
    L.check(L.lib().mcpt_parse_camera(L.ptr(pos), L.ptr(look), L.ptr(up), float(camera_json["fov"]), L.ptr(out)))
    return out


def pack_triangles(tris, mat_index):
    """normal = normalize(cross(v1-v0, v2-v0)), normal.w <- material index bits (copy)."""
    t = np.ascontiguousarray(tris.copy())
    m = np.ascontiguousarray(np.asarray(mat_index, np.int32))
    if len(m) != len(t):
        raise ValueError("one material index per triangle")
    L.check(L.lib().mcpt_pack_triangles(L.ptr(t), L.ptr(m), len(t)))
    return t


from .config import DEFAULT_CREASE  # degrees; a quality choice: creases sharper than this stay creases


def vertex_normals(tris, crease=DEFAULT_CREASE):
    """Vertex normals for smooth shading, generated from PACKED triangles
    (mcpt_vertex_normals, include/mcpt_hip.h): (n, 3, 3) float32, corner k of
    triangle i the angle-weighted mean of the face normals around its welded
    vertex that lie within `crease` degrees of triangle i's."""
    t = np.ascontiguousarray(tris)
    out = np.zeros((len(t), 3, 3), np.float32)
    L.check(L.lib().mcpt_vertex_normals(L.ptr(t), len(t), float(crease), L.ptr(out)))
    return out


def load_obj_normals(directory, objname):
    """Authored normals of an OBJ file (its `vn` records): (vn[n, 3, 3] float32,
    has[n] bool) in load_object's triangle order; has[i] is False where a
    corner of triangle i names no usable normal (vn[i] is zero there)."""
    lib = L.lib()
    nt = ctypes.c_int64(0)
    d, o = directory.encode(), objname.encode()
    L.check(lib.mcpt_load_obj_normals(d, o, None, None, ctypes.byref(nt)))
    vn = np.zeros((nt.value, 3, 3), np.float32)
    has = np.zeros(nt.value, np.uint8)
    L.check(lib.mcpt_load_obj_normals(d, o, L.ptr(vn), L.ptr(has), ctypes.byref(nt)))
    return vn, has.astype(bool)


def smooth_normals(tris, crease=DEFAULT_CREASE, authored=None):
    """What a smooth scene uploads: authored normals (load_obj_normals' pair)
    where a triangle has them, generated ones elsewhere."""
    vn = vertex_normals(tris, crease)
    if authored is not None:
        avn, has = authored
        if len(avn) != len(vn):
            raise ValueError("authored normals of another mesh")
        vn[has] = avn[has]
    return vn


def build_hlbvh(tris):
    """HLBVH<CPU>: 2n-1 BVHNode records (root 0, leaves at [n-1, 2n-2])."""
    n = len(tris)
    if n == 0:
        raise ValueError("empty scene")
    nodes = np.zeros(2 * n - 1, L.BVHNODE)
    t = np.ascontiguousarray(tris)
    L.check(L.lib().mcpt_build_hlbvh(L.ptr(t), n, L.ptr(nodes)))
    return nodes


def bvh_stack_depth(nodes):
    d = ctypes.c_int32(0)
    L.check(L.lib().mcpt_bvh_stack_depth(L.ptr(np.ascontiguousarray(nodes)), len(nodes), ctypes.byref(d)))
    return d.value


def encode_hdr(rgba, flip=True):
    """RGBE bytes exactly as stbi_write_hdr writes them (outputPicture flips)."""
    a = np.ascontiguousarray(rgba, np.float32)
    h, w = a.shape[0], a.shape[1]
    n = L.check(L.lib().mcpt_encode_hdr(w, h, L.ptr(a), int(flip), None, 0))
    buf = np.zeros(n, np.uint8)
    L.check(L.lib().mcpt_encode_hdr(w, h, L.ptr(a), int(flip), L.ptr(buf), n))
    return buf.tobytes()


def write_hdr(path, rgba, flip=True):
    """ThirdPartyWrapper::outputPicture (thirdpartywrapper.cpp:14-23)."""
    a = np.ascontiguousarray(rgba, np.float32)
    L.check(L.lib().mcpt_write_hdr(path.encode(), a.shape[1], a.shape[0], L.ptr(a), int(flip)))


def decode_hdr(data):
    """Radiance RGBE bytes -> (height, width, 3) float32, rows in file order
    (mcpt_decode_hdr: RLE and flat scanlines, decoded as stb_image does).  A
    malformed file raises MCPTError."""
    buf = np.frombuffer(bytes(data), np.uint8)
    w, h = ctypes.c_int32(0), ctypes.c_int32(0)
    lib = L.lib()
    L.check(lib.mcpt_decode_hdr(L.ptr(buf), len(buf), ctypes.byref(w), ctypes.byref(h), None, 0))
    out = np.zeros((h.value, w.value, 3), np.float32)
    L.check(lib.mcpt_decode_hdr(L.ptr(buf), len(buf), ctypes.byref(w), ctypes.byref(h), L.ptr(out), out.size))
    return out


def read_hdr(path):
    """A .hdr file as (height, width, 3) float32, row 0 the file's first
    (its top): the layout Renderer.set_environment takes as a map."""
    with open(path, "rb") as fh:
        return decode_hdr(fh.read())


def preview_rgb8(preview, flip=True):
    """8-bit RGB of a gamma-encoded preview (mcpt_gamma_preview's float4s):
    round(clamp(c, 0, 1) * 255) per channel; flip=True puts the image's top
    row first, as the .hdr dump does (row 0 of the render is its bottom)."""
    a = np.asarray(preview, np.float32)[..., :3]
    a = np.nan_to_num(a, nan=0.0, posinf=1.0, neginf=0.0)
    q = np.floor(np.clip(a, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    return np.ascontiguousarray(q[::-1] if flip else q)


def write_png(path, preview, flip=True):
    """The display's gamma-2.2 image as a PNG (the optional
    preview of testkernel.cl's pass): 8-bit RGB, no interlace, zlib-compressed
    rows with filter 0."""
    import struct
    import zlib
    q = preview_rgb8(preview, flip)
    h, w = q.shape[:2]
    raw = b"".join(b"\x00" + q[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(png)
    return path


# ------------------------------------------------------ texture maps (opt-in)
def _srgb_table():
    """8-bit sRGB -> linear float32: c <= 0.04045 ? c / 12.92 : ((c + 0.055) /
    1.055)^2.4 with c = i / 255, computed in float64 and rounded once."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)


SRGB_TO_LINEAR = _srgb_table()


def decode_png(data, alpha=False):
    """PNG bytes -> (height, width, 3) uint8, row 0 the top.  8-bit,
    non-interlaced images of colour types 0 (grey), 2 (RGB), 3 (palette), 4
    (grey + alpha) and 6 (RGBA), all five row filters; alpha is dropped.
    Anything else raises ValueError.  Needs zlib only.
    alpha=True: (rgb, a) instead, a the alpha channel as (height, width)
    float32, raw / 255 (no sRGB decode), of colour types 4 and 6 and of type 3
    with a tRNS chunk (palette entries past its end are opaque); None for an
    image that carries none."""
    import struct
    import zlib
    data = bytes(data)
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, ihdr, plte, trns, idat, ended = 8, None, None, None, [], False
    while pos + 8 <= len(data) and not ended:
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("PNG: truncated %s chunk" % tag.decode("latin-1"))
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError("PNG: bad checksum in %s chunk" % tag.decode("latin-1"))
        if tag == b"IHDR":
            ihdr = body
        elif tag == b"PLTE":
            plte = body
        elif tag == b"tRNS":
            trns = body
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or len(ihdr) != 13 or not idat or not ended:
        raise ValueError("PNG: missing IHDR, IDAT or IEND")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ihdr)
    if depth != 8 or ctype not in (0, 2, 3, 4, 6) or comp != 0 or filt != 0 or lace != 0:
        raise ValueError("PNG: only 8-bit, non-interlaced images of colour type 0, 2, 3, 4 or 6 are read "
                         "(depth %d, colour type %d, interlace %d)" % (depth, ctype, lace))
    if not (1 <= w <= 16384 and 1 <= h <= 16384):
        raise ValueError("PNG: %d x %d is outside 1..16384" % (w, h))
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    stride = w * bpp
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError("PNG: %s" % e)
    if len(raw) != h * (stride + 1):
        raise ValueError("PNG: %d bytes of image data, expected %d" % (len(raw), h * (stride + 1)))
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f == 1:  # Sub: a running sum per byte lane of a pixel
            cur = np.cumsum(line.reshape(w, bpp), axis=0).reshape(-1) & 255
        elif f in (3, 4):  # Average, Paeth: each byte needs the finished one to its left
            cur = np.zeros(stride, np.int32)
            up = prev.tolist()
            ln = line.tolist()
            c = [0] * stride
            for i in range(stride):
                a = c[i - bpp] if i >= bpp else 0
                b = up[i]
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    cc = up[i - bpp] if i >= bpp else 0
                    pp = a + b - cc
                    pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - cc)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                c[i] = (ln[i] + pred) & 255
            cur = np.asarray(c, np.int32)
        else:
            raise ValueError("PNG: row filter %d" % f)
        out[y] = cur
        prev = cur
    px = out.reshape(h, w, bpp)
    if ctype == 3:
        if plte is None or len(plte) % 3 or not plte:
            raise ValueError("PNG: palette image without a palette")
        pal = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        if int(px.max()) >= len(pal):
            raise ValueError("PNG: palette index out of range")
        rgb, a = np.ascontiguousarray(pal[px[..., 0]]), None
        if trns is not None:
            ta = np.full(256, 255, np.uint8)
            ta[:min(len(trns), 256)] = np.frombuffer(trns[:256], np.uint8)
            a = ta[px[..., 0]]
    elif ctype in (0, 4):
        rgb, a = np.ascontiguousarray(np.repeat(px[..., :1], 3, axis=2)), (px[..., 1] if ctype == 4 else None)
    else:
        rgb, a = np.ascontiguousarray(px[..., :3]), (px[..., 3] if ctype == 6 else None)
    if not alpha:
        return rgb
    return rgb, (None if a is None else np.ascontiguousarray(a.astype(np.float32) / np.float32(255.0)))


def read_png(path, alpha=False):
    """A PNG file as (height, width, 3) uint8, row 0 the top (decode_png; with
    alpha=True its (rgb, alpha) pair)."""
    with open(path, "rb") as fh:
        try:
            return decode_png(fh.read(), alpha)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e))


def read_texture(path):
    """A texture image as (height, width, 3) linear float32, row 0 the top:
    .png through read_png and .hdr through read_hdr (taken as linear); other
    formats through Pillow if it is importable.  8-bit data is decoded from
    sRGB with SRGB_TO_LINEAR.  A missing or unreadable file raises ValueError
    naming it."""
    import os
    if not os.path.isfile(path):
        raise ValueError("texture file %s does not exist" % path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        return SRGB_TO_LINEAR[read_png(path)]
    if ext == ".hdr":
        try:
            a = read_hdr(path)
        except L.MCPTError as e:
            raise ValueError("%s: %s" % (path, e))
        return np.ascontiguousarray(np.maximum(np.nan_to_num(a, nan=0.0, posinf=3.0e38), 0.0), np.float32)
    try:
        from PIL import Image
    except ImportError:
        raise ValueError("%s: only .png (8-bit, non-interlaced) and .hdr textures are read without Pillow" % path)
    try:
        with Image.open(path) as im:
            q = np.asarray(im.convert("RGB"), np.uint8)
    except Exception as e:  # Pillow raises its own types for unknown or damaged files
        raise ValueError("%s: %s" % (path, e))
    return SRGB_TO_LINEAR[q]


def load_obj_uvs(directory, objname):
    """Texture coordinates of an OBJ file (its `vt` records): (uv[n, 3, 2]
    float32, has[n] bool) in load_object's triangle order; has[i] is False
    where a corner of triangle i names no finite vt (uv[i] is zero there)."""
    lib = L.lib()
    nt = ctypes.c_int64(0)
    d, o = directory.encode(), objname.encode()
    L.check(lib.mcpt_load_obj_uvs(d, o, None, None, ctypes.byref(nt)))
    uv = np.zeros((nt.value, 3, 2), np.float32)
    has = np.zeros(nt.value, np.uint8)
    L.check(lib.mcpt_load_obj_uvs(d, o, L.ptr(uv), L.ptr(has), ctypes.byref(nt)))
    return uv, has.astype(bool)


def _names(buf, n):
    parts = bytes(buf).split(b"\0")
    return [x.decode("utf-8", "replace") for x in parts[:n]]


def load_mtl_maps(directory, objname):
    """Each material's map_Kd file name ("" without one), in load_object's
    material order (mcpt_load_mtl_maps)."""
    lib = L.lib()
    nb, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    d, o = directory.encode(), objname.encode()
    L.check(lib.mcpt_load_mtl_maps(d, o, None, ctypes.byref(nb), ctypes.byref(nm)))
    buf = np.zeros(max(nb.value, 1), np.uint8)
    L.check(lib.mcpt_load_mtl_maps(d, o, L.ptr(buf), ctypes.byref(nb), ctypes.byref(nm)))
    return _names(buf[:nb.value], nm.value)


def mtl_maps_from_text(text):
    """load_mtl_maps on MTL text (bytes or str) in memory."""
    lib = L.lib()
    t = text.encode() if isinstance(text, str) else bytes(text)
    src = np.frombuffer(t, np.uint8) if t else np.zeros(0, np.uint8)
    nb, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(lib.mcpt_mtl_maps_from_text(L.ptr(src) if len(src) else None, len(src), None, ctypes.byref(nb), ctypes.byref(nm)))
    buf = np.zeros(max(nb.value, 1), np.uint8)
    L.check(lib.mcpt_mtl_maps_from_text(L.ptr(src) if len(src) else None, len(src), L.ptr(buf), ctypes.byref(nb), ctypes.byref(nm)))
    return _names(buf[:nb.value], nm.value)


def obj_uvs_from_text(text):
    """load_obj_uvs on OBJ text (bytes or str) in memory."""
    lib = L.lib()
    t = text.encode() if isinstance(text, str) else bytes(text)
    src = np.frombuffer(t, np.uint8) if t else np.zeros(0, np.uint8)
    sp = L.ptr(src) if len(src) else None
    nt = ctypes.c_int64(0)
    L.check(lib.mcpt_obj_uvs_from_text(sp, len(src), None, None, ctypes.byref(nt)))
    uv = np.zeros((nt.value, 3, 2), np.float32)
    has = np.zeros(nt.value, np.uint8)
    L.check(lib.mcpt_obj_uvs_from_text(sp, len(src), L.ptr(uv), L.ptr(has), ctypes.byref(nt)))
    return uv, has.astype(bool)


def load_textures(directory, objname, mats, mat_index):
    """What Renderer.set_textures takes for an OBJ model: (uv[n, 3, 2]
    float32, tri_tex[n] int32, images: list of (h, w, 3) linear float32).
    tri_tex[i] = -1 where triangle i has no `vt` or its material no map_Kd.
    `mats` (load_object's, for their count) and `mat_index` (one per
    triangle).  A named texture file that is missing raises ValueError naming
    it; a model with maps but no `vt` at all comes back untextured after one
    warning line."""
    import os
    import sys
    uv, has = load_obj_uvs(directory, objname)
    idx = np.asarray(mat_index, np.int32)
    if len(idx) != len(uv):
        raise ValueError("load_textures: %d material indices for %d triangles" % (len(idx), len(uv)))
    names = load_mtl_maps(directory, objname)
    names = (names + [""] * len(mats))[:max(len(mats), len(names))]
    tri_tex = np.full(len(uv), -1, np.int32)
    images, slot = [], {}
    used = sorted(set(int(m) for m in idx[has] if 0 <= m < len(names) and names[m]))
    for m in used:
        path = os.path.join(directory, names[m])
        if path not in slot:
            slot[path] = len(images)
            images.append(read_texture(path))
        tri_tex[has & (idx == m)] = slot[path]
    if any(names) and not has.any():
        print("warning: %s names texture maps but has no texture coordinates (vt): rendering untextured" % objname,
              file=sys.stderr)
    return uv, tri_tex, images


# ------------------------------------------------- alpha cutouts (opt-in)
def load_mtl_alpha_maps(directory, objname):
    """Each material's map_d file name ("" without one), in load_object's
    material order (mcpt_load_mtl_alpha_maps)."""
    lib = L.lib()
    nb, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    d, o = directory.encode(), objname.encode()
    L.check(lib.mcpt_load_mtl_alpha_maps(d, o, None, ctypes.byref(nb), ctypes.byref(nm)))
    buf = np.zeros(max(nb.value, 1), np.uint8)
    L.check(lib.mcpt_load_mtl_alpha_maps(d, o, L.ptr(buf), ctypes.byref(nb), ctypes.byref(nm)))
    return _names(buf[:nb.value], nm.value)


def mtl_alpha_maps_from_text(text):
    """load_mtl_alpha_maps on MTL text (bytes or str) in memory."""
    lib = L.lib()
    t = text.encode() if isinstance(text, str) else bytes(text)
    src = np.frombuffer(t, np.uint8) if t else np.zeros(0, np.uint8)
    sp = L.ptr(src) if len(src) else None
    nb, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(lib.mcpt_mtl_alpha_maps_from_text(sp, len(src), None, ctypes.byref(nb), ctypes.byref(nm)))
    buf = np.zeros(max(nb.value, 1), np.uint8)
    L.check(lib.mcpt_mtl_alpha_maps_from_text(sp, len(src), L.ptr(buf), ctypes.byref(nb), ctypes.byref(nm)))
    return _names(buf[:nb.value], nm.value)


def read_alpha(path, own_only=False):
    """An image file's alpha as (height, width) float32 in [0, 1], row 0 the
    top, raw (no sRGB decode): its alpha channel if it has one; else, unless
    own_only, its first channel (8-bit: / 255); else None.  .png through
    read_png, .hdr (no alpha channel) through read_hdr, other formats through
    Pillow if it is importable."""
    import os
    if not os.path.isfile(path):
        raise ValueError("map file %s does not exist" % path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        rgb, a = read_png(path, alpha=True)
        first = rgb[..., 0].astype(np.float32) / np.float32(255.0)
    elif ext == ".hdr":
        a, first = None, _read_raw_image(path)[..., 0]
    else:
        try:
            from PIL import Image
        except ImportError:
            raise ValueError("%s: only .png (8-bit, non-interlaced) and .hdr maps are read without Pillow" % path)
        try:
            with Image.open(path) as im:
                q = np.asarray(im.convert("RGBA"), np.uint8)
                has_a = "A" in im.getbands() or "transparency" in im.info
        except Exception as e:  # Pillow raises its own types for unknown or damaged files
            raise ValueError("%s: %s" % (path, e))
        a = q[..., 3].astype(np.float32) / np.float32(255.0) if has_a else None
        first = q[..., 0].astype(np.float32) / np.float32(255.0)
    if a is None and not own_only:
        a = first
    if a is None:
        return None
    return np.ascontiguousarray(np.clip(np.nan_to_num(a, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0), np.float32)


def resample_alpha(a, height, width):
    """An alpha image (h, w) at the texel centres of a (height, width) texture:
    the texture lookup's repeating bilinear filter in float64, rounded once."""
    a = np.asarray(a, np.float64)
    h, w = a.shape
    if (h, w) == (height, width):
        return np.ascontiguousarray(a, np.float32)
    x = (np.arange(width, dtype=np.float64) + 0.5) / width * w - 0.5
    y = (np.arange(height, dtype=np.float64) + 0.5) / height * h - 0.5
    i0, j0 = np.floor(x), np.floor(y)
    fx, fy = (x - i0)[None, :], (y - j0)[:, None]
    i0, j0 = i0.astype(np.int64) % w, j0.astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    t00, t10 = a[j0][:, i0], a[j0][:, i1]
    t01, t11 = a[j1][:, i0], a[j1][:, i1]
    r = (1 - fx) * (1 - fy) * t00 + fx * (1 - fy) * t10 + (1 - fx) * fy * t01 + fx * fy * t11
    return np.ascontiguousarray(np.clip(r, 0.0, 1.0), np.float32)


def load_cutouts(directory, objname, mats, mat_index):
    """What Renderer.set_textures and set_texture_alpha take for an OBJ model
    with cutouts: (uv, tri_tex, images, alphas).  The first three are
    load_textures' with, behind them, one texture of ones per map_d image of a
    material that has a map_d but no map_Kd; alphas holds one (h, w) float32
    image or None per texture: from the material's map_d image (its alpha
    channel if it has one, else its first channel, raw), resampled to the
    colour texture's size where they differ (resample_alpha); else from the
    map_Kd image's own alpha channel.  A texture that several materials share
    takes the first such material's map_d.  The scalars `d` and `Tr` are not
    honoured.  Maps without `vt` give one warning line and no cutouts."""
    import os
    import sys
    uv, tri_tex, images = load_textures(directory, objname, mats, mat_index)
    images = list(images)
    has = np.asarray(load_obj_uvs(directory, objname)[1], bool)
    idx = np.asarray(mat_index, np.int32)
    kd = load_mtl_maps(directory, objname)
    md = load_mtl_alpha_maps(directory, objname)
    n = max(len(mats), len(kd), len(md))
    kd, md = (kd + [""] * n)[:n], (md + [""] * n)[:n]
    alphas = [None] * len(images)
    if any(md) and not has.any():
        if not any(kd):  # (load_textures has warned otherwise)
            print("warning: %s names alpha maps but has no texture coordinates (vt): rendering without cutouts" % objname,
                  file=sys.stderr)
        return uv, tri_tex, images, alphas
    # load_textures' slots, rebuilt: one per distinct map_Kd path, in material order
    slot, owner = {}, {}
    for m in sorted(set(int(x) for x in idx[has] if 0 <= x < n and kd[x])):
        path = os.path.join(directory, kd[m])
        if path not in slot:
            slot[path] = len(slot)
        owner.setdefault(slot[path], []).append(m)
    for t, ms in owner.items():
        h, w = images[t].shape[:2]
        named = [m for m in ms if md[m]]
        if named:
            alphas[t] = resample_alpha(read_alpha(os.path.join(directory, md[named[0]])), h, w)
        else:
            path = os.path.join(directory, kd[ms[0]])
            alphas[t] = read_alpha(path, own_only=True) if os.path.splitext(path)[1].lower() != ".hdr" else None
    extra = {}
    for m in sorted(set(int(x) for x in idx[has] if 0 <= x < n and md[x] and not kd[x])):
        path = os.path.join(directory, md[m])
        if path not in extra:
            a = read_alpha(path)
            extra[path] = len(images)
            images.append(np.ones(a.shape + (3,), np.float32))
            alphas.append(a)
        tri_tex[has & (idx == m)] = extra[path]
    return uv, tri_tex, images, alphas


# ------------------------------------------- bump and normal maps (opt-in)
BUMP_NONE, BUMP_HEIGHT, BUMP_NORMAL = 0, 1, 2  # mcpt_load_mtl_bump_maps' kinds


def height_to_normal(hmap, k=1.0):
    """A height map (h, w) -> (h, w, 3) float32 tangent-space unit normals, row
    0 the top, +v up.  Central differences with wrap, per texel: gx = (h[i+1] -
    h[i-1]) / 2, gy = (h[row j-1] - h[row j+1]) / 2, m = normalize(-k gx, -k
    gy, 1) in float64, rounded once.  k = bm * scale: MTL carries no world
    scale, so slopes are per texel and the user's scale stands in for it."""
    h = np.asarray(hmap, np.float64)
    if h.ndim != 2 or h.size == 0:
        raise ValueError("height_to_normal: a (height, width) map, got %r" % (h.shape,))
    k = float(k)
    if not np.isfinite(k):
        raise ValueError("height_to_normal: k must be finite, got %r" % (k,))
    gx = (np.roll(h, -1, axis=1) - np.roll(h, 1, axis=1)) / 2.0
    gy = (np.roll(h, 1, axis=0) - np.roll(h, -1, axis=0)) / 2.0
    m = np.stack([-k * gx, -k * gy, np.ones_like(h)], axis=2)
    m /= np.sqrt((m * m).sum(axis=2, keepdims=True))
    return _clean_normals(m)


def _clean_normals(m):
    """float64 (h, w, 3) vectors -> float32 unit normals; a texel with z <= 0,
    zero length or a non-finite component becomes (0, 0, 1)."""
    m = np.array(m, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l = np.sqrt((m * m).sum(axis=2))
        bad = ~np.isfinite(m).all(axis=2) | ~(l > 0) | ~np.isfinite(l) | ~(m[..., 2] > 0)
        m = m / np.where(bad, 1.0, l)[..., None]
    out = m.astype(np.float32) + np.float32(0.0)  # (-0 -> +0)
    bad |= ~(out[..., 2] > 0)
    out[bad] = (0.0, 0.0, 1.0)
    return np.ascontiguousarray(out)


def decode_normal_image(img):
    """A normal-map image -> (h, w, 3) float32 unit normals.  uint8: 2 c / 255 -
    1 per channel, raw (no sRGB decode), then normalised; float data is taken
    as it is and normalised.  A texel with z <= 0 or zero length becomes
    (0, 0, 1)."""
    a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] < 3:
        raise ValueError("decode_normal_image: (height, width, 3), got %r" % (a.shape,))
    if a.dtype == np.uint8:
        return _clean_normals(2.0 * a[..., :3].astype(np.float64) / 255.0 - 1.0)
    return _clean_normals(a[..., :3].astype(np.float64))


def _read_raw_image(path):
    """An image's raw channels: (h, w, 3) uint8 for 8-bit files, float32 for
    .hdr.  A missing or unreadable file raises ValueError naming it."""
    import os
    if not os.path.isfile(path):
        raise ValueError("map file %s does not exist" % path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        return read_png(path)
    if ext == ".hdr":
        try:
            return np.ascontiguousarray(read_hdr(path), np.float32)
        except L.MCPTError as e:
            raise ValueError("%s: %s" % (path, e))
    try:
        from PIL import Image
    except ImportError:
        raise ValueError("%s: only .png (8-bit, non-interlaced) and .hdr maps are read without Pillow" % path)
    try:
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"), np.uint8)
    except Exception as e:  # Pillow raises its own types for unknown or damaged files
        raise ValueError("%s: %s" % (path, e))


def read_bump_map(path, kind, k=1.0):
    """A map file as (h, w, 3) float32 unit normals.  BUMP_NORMAL:
    decode_normal_image of the raw channels; BUMP_HEIGHT: height_to_normal of
    their mean (8-bit: / 255, no sRGB decode) with slope factor k."""
    raw = _read_raw_image(path)
    if kind == BUMP_NORMAL:
        return decode_normal_image(raw)
    h = raw[..., :3].astype(np.float64).mean(axis=2)
    if raw.dtype == np.uint8:
        h = h / 255.0
    return height_to_normal(np.nan_to_num(h, nan=0.0, posinf=3.0e38, neginf=-3.0e38), k)


def _bump_maps(call, *head):
    nb, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(call(*head, None, None, None, ctypes.byref(nb), ctypes.byref(nm)))
    buf = np.zeros(max(nb.value, 1), np.uint8)
    kinds = np.zeros(max(nm.value, 1), np.int32)
    bm = np.ones(max(nm.value, 1), np.float32)
    L.check(call(*head, L.ptr(buf), L.ptr(kinds), L.ptr(bm), ctypes.byref(nb), ctypes.byref(nm)))
    n = nm.value
    return list(zip(_names(buf[:nb.value], n), [int(x) for x in kinds[:n]], [float(x) for x in bm[:n]]))


def load_mtl_bump_maps(directory, objname):
    """Each material's (file name, kind, -bm value) in load_object's material
    order: kind BUMP_NORMAL for `norm`, BUMP_HEIGHT for `map_Bump`, `map_bump`
    or `bump`, BUMP_NONE with "" (mcpt_load_mtl_bump_maps)."""
    return _bump_maps(L.lib().mcpt_load_mtl_bump_maps, directory.encode(), objname.encode())


def mtl_bump_maps_from_text(text):
    """load_mtl_bump_maps on MTL text (bytes or str) in memory."""
    t = text.encode() if isinstance(text, str) else bytes(text)
    src = np.frombuffer(t, np.uint8) if t else np.zeros(0, np.uint8)
    return _bump_maps(L.lib().mcpt_mtl_bump_maps_from_text, L.ptr(src) if len(src) else None, len(src))


def load_bump_maps(directory, objname, mats, mat_index, scale=1.0):
    """What Renderer.set_normal_maps takes for an OBJ model: (uv[n, 3, 2]
    float32, tri_map[n] int32, images: list of (h, w, 3) float32 unit normals).
    tri_map[i] = -1 where triangle i has no `vt` or its material no map.  A
    height map's slopes are per texel times bm * scale.  A named file that is
    missing raises ValueError naming it; a model with maps but no `vt` at all
    comes back unmapped after one warning line."""
    import os
    import sys
    uv, has = load_obj_uvs(directory, objname)
    idx = np.asarray(mat_index, np.int32)
    if len(idx) != len(uv):
        raise ValueError("load_bump_maps: %d material indices for %d triangles" % (len(idx), len(uv)))
    maps = load_mtl_bump_maps(directory, objname)
    maps = (maps + [("", BUMP_NONE, 1.0)] * len(mats))[:max(len(mats), len(maps))]
    tri_map = np.full(len(uv), -1, np.int32)
    images, slot = [], {}
    used = sorted(set(int(m) for m in idx[has] if 0 <= m < len(maps) and maps[m][0]))
    for m in used:
        name, kind, bm = maps[m]
        key = (os.path.join(directory, name), kind, bm if kind == BUMP_HEIGHT else 1.0)
        if key not in slot:
            slot[key] = len(images)
            images.append(read_bump_map(key[0], kind, bm * float(scale)))
        tri_map[has & (idx == m)] = slot[key]
    if any(m[0] for m in maps) and not has.any():
        print("warning: %s names bump or normal maps but has no texture coordinates (vt): rendering unmapped" % objname,
              file=sys.stderr)
    return uv, tri_map, images


class SceneData:
    """Host-side scene: packed triangles, HLBVH nodes, materials."""

    def __init__(self, tris, nodes, mats):
        self.tris, self.nodes, self.mats = tris, nodes, mats

    def with_nodes(self, nodes):
        """Same triangles and materials over another BVH (e.g. a treelet pass)."""
        return SceneData(self.tris, nodes, self.mats)

    @classmethod
    def from_obj(cls, directory, objname, material_override=None):
        tris, mats, idx = load_object(directory, objname)
        if (idx < 0).any():
            raise ValueError("face without a known material")
        if material_override is not None:
            mats = material_override(mats)
        packed = pack_triangles(tris, idx)
        return cls(packed, build_hlbvh(packed), mats)

    @classmethod
    def from_arrays(cls, verts, mat_index, mats, build=None):
        """verts: (n, 3, 3) float32 triangle corners.  `build` makes the
        HLBVH from the packed triangles (default: the host build_hlbvh;
        render.build_hlbvh_host_nodes builds the same tree on the GPU)."""
        v = np.asarray(verts, np.float32)
        t = np.zeros(len(v), L.TRIANGLE)
        t["v"][:, :, :3] = v
        packed = pack_triangles(t, mat_index)
        return cls(packed, (build or build_hlbvh)(packed), mats)


def diffuse_only(mats):
    """C2's material override (BASELINE.json configs[1]): every non-light
    material becomes DIFFUSE with its kd (already Kd/pi); glass has Kd = 0."""
    m = mats.copy()
    for i in range(len(m)):
        if m[i]["type"] != L.MCPT_LIGHT:
            m[i]["type"] = L.MCPT_DIFFUSE
    return m


# ------------------------------------------------------------- synthetic scenes
RANDOM_MESH_CAMERA = {"position": [50.0, 50.0, -150.0], "lookat": [50.0, 50.0, 50.0], "up": [0, 1, 0], "fov": 45.0}


def random_mesh(n, seed=42, extent=100.0, build=None):
    """BASELINE.json configs[4] / SURVEY.md §8(d) C5: n random triangles,
    centres uniform in [0, extent]^3, corners = centre + U[-h, h]^3 with
    h = 0.5 * extent / n^(1/3); diffuse 0.5; one emissive quad (Ka 10)
    above the volume.  numpy PCG64(seed) stands in for the survey's PCG32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h = 0.5 * extent / float(n) ** (1.0 / 3.0)
    c = rng.uniform(0.0, extent, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-h, h, (n, 3, 3)).astype(np.float32)).astype(np.float32)
    y = np.float32(1.2 * extent)
    lo, hi = np.float32(0.25 * extent), np.float32(0.75 * extent)
    quad = np.array([[[lo, y, lo], [hi, y, lo], [hi, y, hi]], [[lo, y, lo], [hi, y, hi], [lo, y, hi]]], np.float32)
    verts = np.concatenate([v, quad], axis=0)
    mat_index = np.zeros(len(verts), np.int32)
    mat_index[-2:] = 1
    mats = np.zeros(2, L.MATERIAL)
    mats[0] = classify_material(1.0, (0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    mats[1] = classify_material(1.0, (10, 10, 10), (0, 0, 0), (0, 0, 0), 1.0)
    return SceneData.from_arrays(verts, mat_index, mats, build=build)
