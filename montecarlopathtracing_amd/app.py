"""The reference's application loop on the HIP path: OpenCL::init/update
(MCPT/OpenCLApp.cpp:36-82) + ColorOut (MCPT/colorout.cpp:31-73), headless.

    app = App("config.json")      # config.json of the reference (configid selects the entry)
    app.run()                     # attempt+1 frames accumulated, then <objname>.hdr

Frame semantics kept: frames 0..attempt run the history kernel (attemptCount
<= MAX_ATTEMPT), the .hdr is written once after that from the accumulated
frameBuffer, vertically flipped like stbi_flip_vertically_on_write(true).

Extension: a config entry with "jitter": true (or App(..., jitter=True), the
command line's --jitter) renders with sub-pixel jitter, every frame's primary
ray through a drawn point of its pixel's footprint (antialiasing); the
reference has none, and the default keeps its corner ray bit for bit.

Extension: "denoise": true (App(..., denoise=True), --denoise) also writes
<objname>_denoised.hdr, the accumulated image through Renderer.denoise with
its defaults.  <objname>.hdr keeps its bytes, and the render state is not
touched.  The filter's guide is the first hit of each pixel's corner ray,
also when the render is jittered: the geometry a jittered pixel averages over
is within one pixel of it.

Extension: "environment": {"color": [r, g, b]} or {"map": "sky.hdr", "scale":
s | [r, g, b], "rotate": deg} (App(..., environment={...}), --env / --env-map)
lights the rays that leave the scene with a constant or a lat-long .hdr map
instead of the reference's black (Renderer.set_environment).  The denoise
pass needs nothing for it: a pixel whose first hit is a miss passes through,
so the sky stays sharp.

Extension: "smooth": true | <crease degrees> (App(..., smooth=...), --smooth
[DEG]) shades every hit with the normal interpolated from vertex normals (the
OBJ file's `vn` records where it has them, generated ones elsewhere; creases
sharper than the angle, default 40 degrees, stay creases) instead of the
triangle's face normal (Renderer.set_vertex_normals).  The denoise pass's
guide follows: first_hits returns the shading normals.

Extension: "textures": true (App(..., textures=True), --textures) multiplies
the diffuse lobe's Kd by the model's map_Kd texture at each hit (OBJ `vt`
coordinates, bilinear, repeating, no mip levels; Renderer.set_textures).  The
denoise pass then filters the image divided by the first hits' texture factor
and multiplies it back (Renderer.denoise's albedo), so the texture stays sharp.

Extension: "bump": true | <scale > 0> (App(..., bump=...), --bump [SCALE])
shades every hit with its normal perturbed by the model's normal map (MTL
`norm`) or height map (`map_Bump`, `bump`; slopes per texel times -bm times
the scale) at the hit's `vt` coordinates (Renderer.set_normal_maps).  The
denoise pass's guide follows: first_hits returns the mapped normals.

Extension: "cutouts": true | <threshold in (0, 1]> (App(..., cutouts=...),
--cutouts [THRESHOLD]) cuts every hit whose texture alpha (the material's MTL
`map_d` image, else the `map_Kd` image's own alpha channel) is below the
threshold, default 0.5: the ray goes on through the hole
(Renderer.set_texture_alpha).  It switches the textures on.  The scalars `d`
and `Tr` are not honoured.  The denoise pass's guide and a lens' autofocus see
through the holes: first_hits returns the first hit that is not cut.

Extension: "lens": {"aperture": R, "focus": F} or {"aperture": R, "focus_at":
[px, py]} (App(..., lens={...} or (R, F)), --aperture with --focus or
--focus-at) renders through a thin lens of radius R focused at distance F
along the view axis, or on what pixel (px, py) sees (autofocus): depth of field
instead of the reference's pinhole (Renderer.render_frames' lens).  A lens
needs a fresh primary ray every frame, so it switches jitter on (App.jitter
then reads True).  The denoise pass's guide stays the pinhole corner ray's
first hit, as with jitter.

Extension: "unbiased": true (App(..., unbiased=...), --unbiased) counts every
sample in the history, the all-zero ones included, so the image is the mean of
all samples and not of the non-zero ones (Renderer.render_frames' unbiased).
"roulette": true | <depth >= 1> (App(..., roulette=...), --roulette [DEPTH];
true: depth 3) ends diffuse and glossy paths from that depth on with one minus
the bounce's albedo as the probability and divides the survivors' colour by
it; it needs the counted history and switches it on (App.unbiased then reads
True).  App(..., roulette=False) over an entry with a "roulette" key switches
both off again, unless the entry's own "unbiased" key (or the argument) asks
for the counted history.  The denoise pass runs unchanged: it weights every tap by its count,
which is then the frame count everywhere, so a black pixel carries black at
full weight.

Extension: "adaptive": <threshold> or {"threshold": t, "min_frames": n,
"batch": b, "floor": f, "dilate": bool, "map": bool} (App(..., adaptive=...),
--adaptive [THRESHOLD], --adaptive-map) spends the frames where the image is
noisy (Renderer.render_adaptive): after min_frames frames everywhere, only the
8x8 tiles whose half-buffer error estimate is above the threshold (and their
neighbours) go on, in batches, up to the budget of attempt + 1 frames rounded
down to even (min_frames is cut to the budget).  It runs on the counted history
and switches it on (App.unbiased then reads True).  update() runs the whole
render once, whatever its frame argument, and dumps <objname>.hdr; with "map"
also <objname>_samples.hdr, each pixel's count over the budget as grey.  The
denoise pass runs unchanged: it weights every tap by its count, which now
differs by tile.
"""
import os

import numpy as np

from . import config as C
from . import scene as S


def config_scene(cfg, root, device=0, material_override=None):
    """SceneCL's input for a config entry: the OBJ/MTL scene over the tree
    every reference render traverses.  SceneCL's ctor (scenebuild.cpp:66-95):
    whatever bvhtype names, the "hlbvh" and "treelet" branches fall through
    into the GPUBVH block ("treeletGPU" jumps there), which uploads a FRESH
    HLBVH over bvhBuffer and restructures it in place with the GPU treelet
    kernel; intersect reads that buffer (:125).  "treelet"'s TreeletBVH<CPU>
    tree (:70-73) is built and then overwritten, so it is not computed here.
    App.init and the multi-GPU CLI (__main__._main_dist) both load through
    this, so every GPU count renders over the same tree."""
    from . import render as R
    directory = os.path.join(root, cfg.GETDIRECTORY())
    if not directory.endswith("/"):
        directory += "/"
    if material_override is None and cfg.entry.get("materials") == "diffuse_only":
        material_override = S.diffuse_only
    data = S.SceneData.from_obj(directory, cfg.GETOBJNAME(), material_override)
    bvhtype = cfg.BVHTYPE()
    if bvhtype not in ("hlbvh", "treelet", "treeletGPU"):
        raise ValueError("BVH Not Implemented: %r" % bvhtype)  # scenebuild.cpp:77-79
    return data.with_nodes(R.treelet_gpu_device(data.nodes, device))


def apply_environment(renderer, scene, env, cfg, root):
    """Set a config entry's environment (config.parse_environment's dict, or
    None: leave the reference's black) on an uploaded scene; a map's path is
    relative to the entry's directory.  App.init and every rank of the
    multi-GPU CLI go through this."""
    if env is None:
        return
    texels = None
    if env["map"] is not None:
        texels = S.read_hdr(os.path.join(root, cfg.GETDIRECTORY(), env["map"]))
    renderer.set_environment(scene, scale=env["scale"], map=texels, rotate=env["rotate"])


def apply_smooth(renderer, scene, crease, cfg, root):
    """Set a config entry's smooth shading (config.parse_smooth's crease angle,
    or None: leave the face normals) on an uploaded scene: the OBJ file's
    authored normals where a triangle has them, generated ones elsewhere.
    App.init and every rank of the multi-GPU CLI go through this."""
    if crease is None:
        return
    directory = os.path.join(root, cfg.GETDIRECTORY())
    if not directory.endswith("/"):
        directory += "/"
    authored = S.load_obj_normals(directory, cfg.GETOBJNAME())
    renderer.set_vertex_normals(scene, S.smooth_normals(scene.data.tris, crease, authored))


def apply_textures(renderer, scene, on, cfg, root, cutouts=None):
    """Set a config entry's model textures (OBJ vt, MTL map_Kd) on an uploaded
    scene when `on`; returns whether the scene is textured now.  `cutouts`
    (config.parse_cutouts' threshold, or None) switches them on too and sets
    the model's alpha (MTL map_d, a map_Kd image's alpha channel) with that
    threshold.  App.init and every rank of the multi-GPU CLI go through this."""
    if not on and cutouts is None:
        return False
    directory = os.path.join(root, cfg.GETDIRECTORY())
    if not directory.endswith("/"):
        directory += "/"
    tris = scene.data.tris
    mat_index = np.ascontiguousarray(tris["normal"][:, 3]).view(np.int32)  # pack_triangles put it there
    alphas = None
    if cutouts is None:
        uv, tri_tex, images = S.load_textures(directory, cfg.GETOBJNAME(), scene.data.mats, mat_index)
    else:
        uv, tri_tex, images, alphas = S.load_cutouts(directory, cfg.GETOBJNAME(), scene.data.mats, mat_index)
    if not (tri_tex >= 0).any():
        return False
    renderer.set_textures(scene, uv, tri_tex, images)
    if alphas is not None and any(a is not None for a in alphas):
        renderer.set_texture_alpha(scene, alphas, cutouts)
    return True


def apply_bump(renderer, scene, scale, cfg, root):
    """Set a config entry's bump and normal maps (OBJ vt, MTL map_Bump, bump,
    norm) on an uploaded scene when `scale` (config.parse_bump's) is not None;
    returns whether the scene is mapped now.  App.init and every rank of the
    multi-GPU CLI go through this."""
    if scale is None:
        return False
    directory = os.path.join(root, cfg.GETDIRECTORY())
    if not directory.endswith("/"):
        directory += "/"
    tris = scene.data.tris
    mat_index = np.ascontiguousarray(tris["normal"][:, 3]).view(np.int32)  # pack_triangles put it there
    uv, tri_map, images = S.load_bump_maps(directory, cfg.GETOBJNAME(), scene.data.mats, mat_index, scale)
    if not (tri_map >= 0).any():
        return False
    renderer.set_normal_maps(scene, uv, tri_map, images)
    return True


def resolve_lens(renderer, scene, camera, width, height, spec):
    """A lens spec (config.parse_lens' dict, or None) -> (R, F) or None; a
    "focus_at" pixel is focused on through Renderer.autofocus.  App.init and
    every rank of the multi-GPU CLI go through this."""
    if spec is None:
        return None
    if spec["focus"] is not None:
        return (spec["aperture"], spec["focus"])
    px, py = spec["focus_at"]
    return (spec["aperture"], renderer.autofocus(scene, camera, width, height, px, py))


class App:
    def __init__(self, cfg, configid=None, device=0, seeds=None, out_dir=".", root=None,
                 material_override=None, jitter=None, denoise=None, environment=None, smooth=None, textures=None,
                 lens=None, bump=None, cutouts=None, unbiased=None, roulette=None, adaptive=None,
                 adaptive_map=None):
        self.cfg = cfg if isinstance(cfg, C.Config) else C.Config(cfg, configid)
        if self.cfg.TESTBVH() or self.cfg.TESTALL():
            raise ValueError("testbvh/testall modes are BVH-quality tools, not the render path")
        if not self.cfg.USEOPENCL():
            raise ValueError('config has "opencl": false — the reference throws "Not Implemented" here')
        self.root = root if root is not None else (os.path.dirname(os.path.abspath(cfg)) if isinstance(cfg, str) else ".")
        self.device = device
        self.seeds = seeds
        self.out_dir = out_dir
        self.material_override = material_override
        if material_override is None and self.cfg.entry.get("materials") == "diffuse_only":
            self.material_override = S.diffuse_only
        self.jitter = self.cfg.JITTER() if jitter is None else bool(jitter)  # None: the entry's "jitter" key
        self.denoise = self.cfg.DENOISE() if denoise is None else bool(denoise)  # None: the entry's "denoise" key
        # None: the entry's "environment" key; else that key's value ({"color": ..} or {"map": ..})
        self.environment = self.cfg.ENVIRONMENT() if environment is None else C.parse_environment(environment)
        # None: the entry's "smooth" key; else that key's value (True / False / crease degrees)
        self.smooth = self.cfg.SMOOTH() if smooth is None else C.parse_smooth(smooth)
        self.textures = self.cfg.TEXTURES() if textures is None else C.parse_textures(textures)  # None: the entry's key
        # None: the entry's "lens" key; else that key's value, or (R, F).  A lens switches jitter on.
        if lens is None:
            self.lens_spec = self.cfg.LENS()
        elif isinstance(lens, dict):
            self.lens_spec = C.parse_lens(lens)
        else:
            self.lens_spec = C.parse_lens({"aperture": lens[0], "focus": lens[1]})
        if self.lens_spec is not None:
            if jitter is not None and not jitter:
                raise ValueError("a lens needs jitter: jitter=False cannot go with a lens")
            self.jitter = True
        self.lens = None  # (R, F) once init() has resolved the focus
        self.textured = False
        self.bump = self.cfg.BUMP() if bump is None else C.parse_bump(bump)  # None: the entry's "bump" key
        self.mapped = False
        # None: the entry's "cutouts" key; else that key's value (True / False / threshold).  Cutouts switch textures on.
        self.cutouts = self.cfg.CUTOUTS() if cutouts is None else C.parse_cutouts(cutouts)
        if self.cutouts is not None:
            self.textures = True
        # None: the entry's "unbiased" / "roulette" keys; else those keys' values.  The roulette in force switches
        # unbiased on: with roulette=False over an entry's "roulette", unbiased is what the "unbiased" key itself says.
        self.unbiased = self.cfg.unbiased_key if unbiased is None else C.parse_unbiased(unbiased)
        self.roulette = self.cfg.ROULETTE() if roulette is None else C.parse_roulette(roulette)
        if self.roulette:
            if unbiased is not None and not unbiased:
                raise ValueError("roulette needs the counted history: unbiased=False cannot go with it")
            self.unbiased = True
        # None: the entry's "adaptive" key; False: off; else that key's value (a threshold or an object).
        # Adaptive sampling runs on the counted history and switches it on.
        if adaptive is None:
            self.adaptive = self.cfg.ADAPTIVE()
        else:
            self.adaptive = None if adaptive is False else C.parse_adaptive(adaptive)
        if self.adaptive is not None:
            self.adaptive = dict(self.adaptive)
            if adaptive_map is not None:
                self.adaptive["map"] = bool(adaptive_map)
            if unbiased is not None and not unbiased:
                raise ValueError("adaptive sampling needs the counted history: unbiased=False cannot go with it")
            self.unbiased = True
        elif adaptive_map:
            raise ValueError("adaptive_map needs adaptive sampling")
        self.adaptive_report = None  # Renderer.render_adaptive's report once update() has run it
        self.attempt_count = 0
        self.dumped = None
        self._init = False

    def init(self):
        """OpenCL::init: load OBJ, build scene, camera, buffers (OpenCLApp.cpp:36-55)."""
        from . import render as R
        cam = self.cfg.GETCAMERA()
        res = cam.get("resolution", [self.cfg.WIDTH(), self.cfg.HEIGHT()])
        if [int(res[0]), int(res[1])] != [self.cfg.WIDTH(), self.cfg.HEIGHT()]:
            # the reference sizes rays by camera.resolution but colour by width/height
            # (raygeneration.cpp:51-56 vs OpenCLApp.cpp:38-51); a mismatch is undefined there
            raise ValueError("camera.resolution must equal width/height")
        self.w, self.h = self.cfg.WIDTH(), self.cfg.HEIGHT()
        self.data = config_scene(self.cfg, self.root, self.device, self.material_override)
        self.camera = S.parse_camera(cam)
        self.renderer = R.Renderer(self.device)
        self.scene = self.renderer.upload(self.data)
        apply_environment(self.renderer, self.scene, self.environment, self.cfg, self.root)
        apply_smooth(self.renderer, self.scene, self.smooth, self.cfg, self.root)
        self.textured = apply_textures(self.renderer, self.scene, self.textures, self.cfg, self.root, self.cutouts)
        self.mapped = apply_bump(self.renderer, self.scene, self.bump, self.cfg, self.root)
        self.state = self.renderer.new_state(self.w, self.h, self.seeds)
        self.lens = resolve_lens(self.renderer, self.scene, self.camera, self.w, self.h, self.lens_spec)
        self._init = True

    def update(self, frames=1):
        """`frames` display frames of OpenCL::update; dumps the .hdr once the
        history has taken attempt+1 frames (colorout.cpp:56-68)."""
        if not self._init:
            self.init()
        att = self.cfg.MAXATTEPMT()
        if self.adaptive is not None:
            if self.adaptive_report is None:
                self._update_adaptive(att)
            return self.state
        todo = frames
        if frames >= 4096 and not getattr(self, "_tuned", False):  # long runs: time the leaf schedules, S-phase
            # and fetch thresholds on one-block 16-frame calls (7 trials, 112 scratch frames, bit-identical
            # either way).  Not the block sizing nor the tile order: a long call runs max_block_frames-frame
            # blocks whatever block_entries says, and the tile order mostly shortens a launch's tail, so
            # one-block trials of either would tune a regime the run never enters.
            self.renderer.tune(self.scene, self.camera, self.state, self.cfg.MAXDEPTH(), att, frames=16,
                               block_entries=None, last_block=False, tile_orders=None, frames_per_launch=16,
                               jitter=self.jitter, lens=self.lens, unbiased=self.unbiased, roulette=self.roulette)
            self._tuned = True
        while todo > 0:
            n = todo if self.attempt_count > att else min(todo, att + 1 - self.attempt_count)
            self.renderer.render_frames(self.scene, self.camera, self.state, self.cfg.MAXDEPTH(), att, n,
                                        jitter=self.jitter, lens=self.lens, unbiased=self.unbiased,
                                        roulette=self.roulette)
            self.attempt_count += n
            todo -= n
            if self.attempt_count > att and self.dumped is None:
                self.dumped = self.output_picture()
        return self.state

    def adaptive_budget(self):
        """The per-pixel frame budget of an adaptive render: attempt + 1, rounded down to even."""
        return (self.cfg.MAXATTEPMT() + 1) // 2 * 2

    def _update_adaptive(self, att):
        a, budget = self.adaptive, self.adaptive_budget()
        self.adaptive_report = self.renderer.render_adaptive(
            self.scene, self.camera, self.state, self.cfg.MAXDEPTH(), budget, a["threshold"],
            min_frames=min(a["min_frames"], budget), batch=a["batch"], floor=a["floor"], dilate=a["dilate"],
            jitter=self.jitter, lens=self.lens, roulette=self.roulette)
        self.attempt_count = att + 1
        self.dumped = self.output_picture()

    def samples_image(self):
        """An adaptive render's sample map: each pixel's count over the budget as grey, H x W x 4 floats (w = 0)."""
        g = self.state.count.cpu().numpy().astype(np.float32) / np.float32(self.adaptive_budget())
        out = np.zeros((self.h, self.w, 4), np.float32)
        out[..., :3] = g.reshape(self.h, self.w, 1)
        return out

    @staticmethod
    def samples_path(path):
        """<name>.hdr -> <name>_samples.hdr."""
        return (path[:-4] if path.endswith(".hdr") else path) + "_samples.hdr"

    def output_picture(self, path=None):
        """ThirdPartyWrapper::outputPicture(<objname>.hdr, frameBuffer); with
        denoise on also <objname>_denoised.hdr beside it (denoised_path)."""
        path = path or os.path.join(self.out_dir, self.cfg.GETOBJNAME() + ".hdr")
        S.write_hdr(path, self.state.image(), flip=True)
        if self.denoise:
            S.write_hdr(self.denoised_path(path), self.denoised(), flip=True)
        if self.adaptive is not None and self.adaptive["map"]:
            S.write_hdr(self.samples_path(path), self.samples_image(), flip=True)
        return path

    @staticmethod
    def denoised_path(path):
        """<name>.hdr -> <name>_denoised.hdr."""
        return (path[:-4] if path.endswith(".hdr") else path) + "_denoised.hdr"

    def denoised(self):
        """The accumulated image through Renderer.denoise (its defaults), H x W
        x 4 floats (w = 0 on filtered pixels), guided by the corner rays' first
        hits; the state is only read."""
        if not self._init:
            self.init()
        return self._denoise().cpu().numpy().reshape(self.h, self.w, 4)

    def _denoise(self):
        hits = self.renderer.first_hits(self.scene, self.camera, self.w, self.h)
        albedo = self.renderer.first_hit_albedo(self.scene, hits) if self.textured else None
        return self.renderer.denoise(self.scene, hits, self.state, albedo=albedo)

    def run(self):
        self.update(self.cfg.MAXATTEPMT() + 1)
        return self.dumped

    def image(self):
        return self.state.image()

    def preview(self):
        """ColorOut's display pass (testkernel.cl func, colorout.cpp:69-70 once
        the history is complete): the running mean gamma-2.2 encoded, H x W x 4
        floats (w = 0), as the reference writes to its RGBA32F texture.  With
        denoise on it encodes the denoised image."""
        if not self._init:
            self.init()
        src = self.state.hist
        if self.denoise:
            src = self._denoise()
        out = self.renderer.gamma_preview(src)
        return out.cpu().numpy().reshape(self.h, self.w, 4)
