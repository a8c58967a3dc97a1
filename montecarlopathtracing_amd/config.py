"""config.json surface of the reference (MCPT/config.cpp:70-124, MCPT/config.json).

The reference reads ``config.json`` from the working directory with a patched
nlohmann/json 3.1.2 in which ``#`` starts a comment wherever the scanner skips
whitespace (MCPT/json.hpp:3037-3043); ``configid`` selects one entry of the
``config`` array.  :class:`Config` exposes the same getters
(MCPT/config.cpp:128-145, MCPT/config.h:8-30) with the same defaults.
"""
import json
import math


def strip_hash_comments(text):
    """Drop ``# ...`` to end of line outside JSON strings (json.hpp:3037-3043)."""
    out, i, n, in_str = [], 0, len(text), False
    while i < n:
        c = text[i]
        if in_str:
            out.append(c)
            if c == "\\" and i + 1 < n:
                out.append(text[i + 1])
                i += 1
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
            out.append(c)
        elif c == "#":
            while i < n and text[i] != "\n":
                i += 1
            continue
        else:
            out.append(c)
        i += 1
    return "".join(out)


def loads(text):
    return json.loads(strip_hash_comments(text))


def _env_number(v, what):
    """A finite JSON number (bool is not one)."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError('config "environment": %s must be a finite number, got %r' % (what, v))
    return float(v)


def _env_rgb(v, what):
    if not isinstance(v, (list, tuple)) or len(v) != 3:
        raise ValueError('config "environment": %s must be [r, g, b], got %r' % (what, v))
    rgb = tuple(_env_number(x, what) for x in v)
    if min(rgb) < 0:
        raise ValueError('config "environment": %s must be >= 0, got %r' % (what, v))
    return rgb


DEFAULT_CREASE = 40.0  # degrees: what "smooth": true means.  A quality choice, not a measured optimum: edges
# sharper than this (a box's 90, a faceted gem's) stay edges, tessellated curves (an icosphere's ~20-37) blend


def parse_smooth(v):
    """The "smooth" extension key of a config entry -> the crease angle in
    degrees, or None (false: face normals).  true is DEFAULT_CREASE; a number
    is the angle, in [0, 180]."""
    if v is False:
        return None
    if v is True:
        return DEFAULT_CREASE
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError('config "smooth" must be true, false or a crease angle in degrees, got %r' % (v,))
    if not (math.isfinite(v) and 0.0 <= v <= 180.0):
        raise ValueError('config "smooth": the crease angle must lie in [0, 180] degrees, got %r' % (v,))
    return float(v)


def parse_textures(v):
    """The "textures" extension key of a config entry -> bool."""
    if not isinstance(v, bool):
        raise ValueError('config "textures" must be true or false, got %r' % (v,))
    return v


def parse_cutouts(v):
    """The "cutouts" extension key of a config entry -> the alpha threshold in
    (0, 1] of the model's cutouts (true: 0.5), or None (false: opaque textures)."""
    if isinstance(v, bool):
        return 0.5 if v else None
    if not isinstance(v, (int, float)):
        raise ValueError('config "cutouts" must be true, false or a threshold in (0, 1], got %r' % (v,))
    v = float(v)
    if not (v > 0.0 and v <= 1.0):
        raise ValueError('config "cutouts" must be a threshold in (0, 1], got %r' % (v,))
    return v


DEFAULT_ROULETTE_DEPTH = 3  # "roulette": true


def parse_unbiased(v):
    """The "unbiased" extension key of a config entry -> bool."""
    if not isinstance(v, bool):
        raise ValueError('config "unbiased" must be true or false, got %r' % (v,))
    return v


def parse_roulette(v):
    """The "roulette" extension key of a config entry -> the depth from which
    Russian roulette runs (true: DEFAULT_ROULETTE_DEPTH), or 0 (false: none).
    A depth is an integer in 1..65535."""
    if isinstance(v, bool):
        return DEFAULT_ROULETTE_DEPTH if v else 0
    if not isinstance(v, int):
        raise ValueError('config "roulette" must be true, false or an integer depth >= 1, got %r' % (v,))
    if not 1 <= v <= 65535:
        raise ValueError('config "roulette" must be a depth in 1..65535, got %r' % (v,))
    return v


DEFAULT_ADAPTIVE_THRESHOLD = 0.02  # --adaptive without a value.  A starting point, not a tuned optimum


def parse_adaptive(v):
    """The "adaptive" extension key of a config entry ->
    {"threshold": t, "min_frames": n, "batch": b, "floor": f, "dilate": bool, "map": bool}
    (Renderer.render_adaptive's arguments; "map": also write the sample map).
    A number is the threshold alone; an object names any of the six, and needs
    "threshold".  ValueError on strings and other types, unknown keys,
    non-positive or non-finite numbers, and counts that are not even integers
    >= 2."""
    out = {"threshold": None, "min_frames": 16, "batch": 8, "floor": 1e-4, "dilate": True, "map": False}

    def positive(x, what):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or not x > 0:
            raise ValueError('config "adaptive": %s must be a finite number > 0, got %r' % (what, x))
        return float(x)

    def even(x, what):
        if isinstance(x, bool) or not isinstance(x, int) or x < 2 or x % 2:
            raise ValueError('config "adaptive": %s must be an even integer >= 2, got %r' % (what, x))
        return x

    def flag(x, what):
        if not isinstance(x, bool):
            raise ValueError('config "adaptive": %s must be true or false, got %r' % (what, x))
        return x

    if not isinstance(v, dict):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError('config "adaptive" must be a threshold > 0 or an object, got %r' % (v,))
        out["threshold"] = positive(v, "the threshold")
        return out
    unknown = set(v) - set(out)
    if unknown:
        raise ValueError('config "adaptive": unknown keys %r' % (sorted(unknown),))
    if "threshold" not in v:
        raise ValueError('config "adaptive" needs "threshold"')
    out["threshold"] = positive(v["threshold"], '"threshold"')
    for k in ("min_frames", "batch"):
        if k in v:
            out[k] = even(v[k], '"%s"' % k)
    if "floor" in v:
        out["floor"] = positive(v["floor"], '"floor"')
    for k in ("dilate", "map"):
        if k in v:
            out[k] = flag(v[k], '"%s"' % k)
    return out


def parse_lens(v):
    """The "lens" extension key of a config entry ->
    {"aperture": R, "focus": F or None, "focus_at": (px, py) or None}.
    {"aperture": R, "focus": F}: a thin lens of radius R focused at distance F
    along the view axis, both > 0 in scene units.  {"aperture": R, "focus_at":
    [px, py]}: focused on what that pixel sees (autofocus, Renderer.autofocus).
    ValueError on wrong types, unknown keys, both or neither of "focus" and
    "focus_at", and non-positive or non-finite values."""
    if not isinstance(v, dict):
        raise ValueError('config "lens" must be an object, got %r' % (v,))
    unknown = set(v) - {"aperture", "focus", "focus_at"}
    if unknown:
        raise ValueError('config "lens": unknown keys %r' % (sorted(unknown),))
    if "aperture" not in v:
        raise ValueError('config "lens" needs "aperture"')
    if ("focus" in v) == ("focus_at" in v):
        raise ValueError('config "lens" needs exactly one of "focus" and "focus_at", got keys %r' % (sorted(v),))

    def positive(x, what):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or not x > 0:
            raise ValueError('config "lens": "%s" must be a finite number > 0, got %r' % (what, x))
        return float(x)

    out = {"aperture": positive(v["aperture"], "aperture"), "focus": None, "focus_at": None}
    if "focus" in v:
        out["focus"] = positive(v["focus"], "focus")
    else:
        at = v["focus_at"]
        if (not isinstance(at, (list, tuple)) or len(at) != 2 or
                any(isinstance(x, bool) or not isinstance(x, int) or x < 0 for x in at)):
            raise ValueError('config "lens": "focus_at" must be a pixel [px, py], got %r' % (at,))
        out["focus_at"] = (int(at[0]), int(at[1]))
    return out


def parse_bump(v):
    """The "bump" extension key of a config entry -> the slope scale of the
    model's height maps (true: 1.0), or None (false: no bump or normal maps)."""
    if isinstance(v, bool):
        return 1.0 if v else None
    if not isinstance(v, (int, float)):
        raise ValueError('config "bump" must be true, false or a scale > 0, got %r' % (v,))
    v = float(v)
    if not (v > 0.0 and v < float("inf")):
        raise ValueError('config "bump" must be a finite scale > 0, got %r' % (v,))
    return v


def parse_environment(e):
    """The "environment" extension key of a config entry ->
    {"scale": (r, g, b), "map": path or None, "rotate": degrees}.
    Form one: {"color": [r, g, b]}, a constant environment.  Form two:
    {"map": "sky.hdr", "scale": s | [r, g, b], "rotate": deg}, a lat-long .hdr
    relative to the entry's "directory" ("scale" defaults to 1, "rotate" to 0).
    ValueError on wrong types, negative or non-finite values, unknown sub-keys
    or a mix of the two forms."""
    if not isinstance(e, dict):
        raise ValueError('config "environment" must be an object, got %r' % (e,))
    if "color" in e:
        if set(e) != {"color"}:
            raise ValueError('config "environment": "color" stands alone, got keys %r' % (sorted(e),))
        return {"scale": _env_rgb(e["color"], '"color"'), "map": None, "rotate": 0.0}
    if "map" not in e:
        raise ValueError('config "environment" needs "color" or "map", got keys %r' % (sorted(e),))
    unknown = set(e) - {"map", "scale", "rotate"}
    if unknown:
        raise ValueError('config "environment": unknown keys %r' % (sorted(unknown),))
    if not isinstance(e["map"], str) or not e["map"]:
        raise ValueError('config "environment": "map" must be a file name, got %r' % (e["map"],))
    s = e.get("scale", 1.0)
    if isinstance(s, (list, tuple)):
        scale = _env_rgb(s, '"scale"')
    else:
        scale = (_env_number(s, '"scale"'),) * 3
        if scale[0] < 0:
            raise ValueError('config "environment": "scale" must be >= 0, got %r' % (s,))
    return {"scale": scale, "map": e["map"], "rotate": _env_number(e.get("rotate", 0.0), '"rotate"')}


class Config:
    """One selected entry of a reference config.json (config.cpp:72-122)."""

    def __init__(self, obj, configid=None):
        if isinstance(obj, str):
            with open(obj, "r") as fh:
                obj = loads(fh.read())
        self.root = obj
        cid = int(obj["configid"] if configid is None else configid)
        c = obj["config"][cid]
        self.entry = c
        self.bvhtype = c.get("bvhtype", "") or "hlbvh"
        self.testall = bool(c.get("testall", False))
        self.directory = c.get("directory", "")
        # extension key (no reference counterpart; like "materials": "diffuse_only"):
        # "jitter": true renders with sub-pixel jitter (antialiasing)
        self.jitter = c.get("jitter", False)
        if not isinstance(self.jitter, bool):
            raise ValueError('config "jitter" must be true or false, got %r' % (self.jitter,))
        # "denoise": true also writes the denoised image (Renderer.denoise)
        self.denoise = c.get("denoise", False)
        if not isinstance(self.denoise, bool):
            raise ValueError('config "denoise" must be true or false, got %r' % (self.denoise,))
        # "environment": what a ray that leaves the scene picks up
        # (Renderer.set_environment); None: the reference's black
        self.environment = parse_environment(c["environment"]) if "environment" in c else None
        # "smooth": true | <crease degrees>: shade with interpolated vertex normals
        # (Renderer.set_vertex_normals); None: the reference's face normals
        self.smooth = parse_smooth(c["smooth"]) if "smooth" in c else None
        # "textures": true: the model's diffuse texture maps (OBJ vt, MTL map_Kd;
        # Renderer.set_textures); false: the materials' Kd alone, as the reference
        self.textures = parse_textures(c["textures"]) if "textures" in c else False
        # "bump": true | <scale > 0>: the model's bump and normal maps (MTL map_Bump,
        # bump, norm; Renderer.set_normal_maps); None: the unmapped normals
        self.bump = parse_bump(c["bump"]) if "bump" in c else None
        # "cutouts": true | <threshold in (0, 1]>: the model's alpha cutouts (MTL map_d, a map_Kd image's
        # alpha channel; Renderer.set_texture_alpha), which take the textures with them; None: opaque
        self.cutouts = parse_cutouts(c["cutouts"]) if "cutouts" in c else None
        # "lens": {"aperture": R, "focus": F | "focus_at": [px, py]}: a thin-lens
        # camera (depth of field; Renderer.render_frames' lens); None: the pinhole
        self.lens = parse_lens(c["lens"]) if "lens" in c else None
        # "unbiased": true: the history counts every sample, the all-zero ones included
        # (Renderer.render_frames' unbiased); "roulette": true | <depth >= 1>: Russian roulette from that
        # depth on (true: 3), which needs the counted history and switches it on
        self.unbiased = parse_unbiased(c["unbiased"]) if "unbiased" in c else False
        self.unbiased_key = self.unbiased  # what the "unbiased" key itself says, whatever the roulette adds
        self.roulette = parse_roulette(c["roulette"]) if "roulette" in c else 0
        if self.roulette:
            if "unbiased" in c and not self.unbiased:
                raise ValueError('config "roulette" needs the counted history: "unbiased": false cannot go with it')
            self.unbiased = True
        # "adaptive": <threshold> | {...}: adaptive sampling by half-buffer error (Renderer.render_adaptive),
        # which runs on the counted history and switches it on; None: every pixel gets every frame
        self.adaptive = parse_adaptive(c["adaptive"]) if "adaptive" in c else None
        if self.adaptive:
            if "unbiased" in c and not self.unbiased:
                raise ValueError('config "adaptive" needs the counted history: "unbiased": false cannot go with it')
            self.unbiased = True
        if self.testall:
            self.objs = c["objname"]
            self.objname = ""
            self.camera = None
            self.width = self.height = 0
            self.testbvh = False
            self.maxdepth = self.attempt = 0
            self.opencl = False
            return
        self.camera = c.get("camera")
        self.objname = c["objname"]
        self.width = int(float(c["width"]))      # read as double, stored as int
        self.height = int(float(c["height"]))
        self.testbvh = bool(c.get("testbvh", False))
        self.objs = None
        if self.testbvh:
            self.maxdepth = self.attempt = 0
            self.opencl = False
            return
        self.platform = c.get("platform", "")
        self.raygenerator = c.get("raygenerator", "")
        self.intersect = c.get("intersect", "")
        self.shade = c.get("shade", "")
        self.opencl = bool(c.get("opencl", False))
        self.maxdepth = int(c["maxdepth"])
        self.attempt = int(c["attempt"])

    # the reference's free-function getters (config.h)
    def WIDTH(self): return self.width
    def HEIGHT(self): return self.height
    def MAXDEPTH(self): return self.maxdepth
    def MAXATTEPMT(self): return self.attempt  # sic, config.h:24
    def GETOBJNAME(self): return self.objname
    def GETDIRECTORY(self): return self.directory
    def GETCAMERA(self): return self.camera
    def BVHTYPE(self): return self.bvhtype
    def TESTBVH(self): return self.testbvh
    def TESTALL(self): return self.testall
    def USEOPENCL(self): return self.opencl
    def GETOBJS(self): return self.objs
    def JITTER(self): return self.jitter  # extension: sub-pixel jitter of the render path
    def DENOISE(self): return self.denoise  # extension: the denoise post-pass
    def ENVIRONMENT(self): return self.environment  # extension: parse_environment's dict, or None
    def SMOOTH(self): return self.smooth  # extension: smooth shading's crease angle in degrees, or None
    def LENS(self): return self.lens  # extension: parse_lens' dict (thin-lens camera), or None
    def UNBIASED(self): return self.unbiased  # extension: the history counts every sample (on with roulette)
    def ROULETTE(self): return self.roulette  # extension: the depth Russian roulette runs from, 0: none
    def ADAPTIVE(self): return self.adaptive  # extension: parse_adaptive's dict (adaptive sampling), or None
    def TEXTURES(self): return self.textures  # extension: the model's map_Kd textures on the diffuse lobe
    def CUTOUTS(self): return self.cutouts  # extension: the alpha threshold of the model's cutouts (textures on), or None
    def BUMP(self): return self.bump  # extension: the height maps' slope scale of the model's bump and normal maps, or None
