"""Command line: render a reference config.json on the GPU(s) and write the .hdr,
or, for a "testbvh" / "testall" entry, print the BVH metrics (main.cpp:11-25).

    python -m montecarlopathtracing_amd [config.json] [--configid N] [--out DIR] [--preview PNG] [--jitter] [--denoise]
        [--env R,G,B | --env-map FILE [--env-scale S|R,G,B] [--env-rotate DEG]] [--smooth [DEG]]
        [--textures] [--cutouts [THRESHOLD]] [--bump [SCALE]] [--aperture R (--focus F | --focus-at X,Y)]
        [--unbiased] [--roulette [DEPTH]] [--adaptive [THRESHOLD]] [--adaptive-map]
    torchrun --nproc-per-node 8 -m montecarlopathtracing_amd config.json   (row-stripe tiles)
"""
import argparse
import os
import sys
import time


def parser():
    ap = argparse.ArgumentParser(prog="montecarlopathtracing_amd")
    ap.add_argument("config", nargs="?", default="config.json")
    ap.add_argument("--configid", type=int, default=None)
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=None, help="override attempt+1 frames")
    ap.add_argument("--preview", default=None, help="also write the gamma-2.2 display image (testkernel.cl) as PNG")
    ap.add_argument("--jitter", action="store_true",
                    help="sub-pixel jitter (antialiasing) even if the config entry has no \"jitter\": true")
    ap.add_argument("--denoise", action="store_true",
                    help="also write <objname>_denoised.hdr, the count-aware geometry-guided denoise of the image "
                         "(with --preview the PNG shows it), even if the config entry has no \"denoise\": true")
    ap.add_argument("--env", default=None, metavar="R,G,B",
                    help="constant environment: rays that leave the scene pick up this radiance instead of black "
                         "(overrides the config entry's \"environment\")")
    ap.add_argument("--env-map", default=None, metavar="FILE",
                    help="lat-long .hdr environment map (row 0 the top; a path relative to the working directory; "
                         "overrides the config entry's \"environment\")")
    ap.add_argument("--env-scale", default=None, metavar="S|R,G,B",
                    help="factor on the map (--env-map, or the config entry's map)")
    ap.add_argument("--env-rotate", type=float, default=None, metavar="DEG",
                    help="rotation of the map about +Y in degrees (--env-map, or the config entry's map)")
    ap.add_argument("--smooth", nargs="?", type=float, const=True, default=None, metavar="DEG",
                    help="smooth shading from interpolated vertex normals; DEG: the crease angle kept sharp "
                         "(default 40), even if the config entry has no \"smooth\" key")
    ap.add_argument("--textures", action="store_true",
                    help="the model's diffuse texture maps (OBJ vt, MTL map_Kd), even if the config entry has no "
                         "\"textures\" key")
    ap.add_argument("--cutouts", nargs="?", type=float, const=True, default=None, metavar="THRESHOLD",
                    help="alpha cutouts (MTL map_d, a map_Kd image's alpha channel): a hit whose alpha is below "
                         "THRESHOLD (default 0.5, in (0, 1]) lets the ray through; switches --textures on, even if the "
                         "config entry has no \"cutouts\" key")
    ap.add_argument("--bump", nargs="?", type=float, const=True, default=None, metavar="SCALE",
                    help="the model's bump and normal maps (MTL map_Bump, bump, norm); SCALE: factor on a height "
                         "map's per-texel slopes (default 1), even if the config entry has no \"bump\" key")
    ap.add_argument("--aperture", type=float, default=None, metavar="R",
                    help="thin-lens camera (depth of field): the lens radius in scene units; needs --focus or "
                         "--focus-at, switches --jitter on, overrides the config entry's \"lens\"")
    ap.add_argument("--focus", type=float, default=None, metavar="F",
                    help="the distance along the view axis that is in focus, in scene units (with --aperture)")
    ap.add_argument("--focus-at", default=None, metavar="X,Y",
                    help="autofocus: focus on what pixel X,Y sees (with --aperture)")
    ap.add_argument("--unbiased", action="store_true",
                    help="count every sample in the history, the all-zero ones included: the image is the mean of "
                         "all samples, even if the config entry has no \"unbiased\": true")
    ap.add_argument("--roulette", nargs="?", type=int, const=True, default=None, metavar="DEPTH",
                    help="Russian roulette on diffuse and glossy bounces from DEPTH on (default 3), the survival "
                         "probability the bounce's albedo; switches --unbiased on, overrides the config entry's "
                         "\"roulette\"")
    ap.add_argument("--adaptive", nargs="?", type=float, const=True, default=None, metavar="THRESHOLD",
                    help="adaptive sampling: after the first frames only the 8x8 tiles whose half-buffer error "
                         "estimate is above THRESHOLD (default 0.02) go on, up to attempt+1 frames; switches "
                         "--unbiased on, overrides the config entry's \"adaptive\" threshold (one GPU only)")
    ap.add_argument("--adaptive-map", action="store_true",
                    help="with adaptive sampling also write <objname>_samples.hdr: each pixel's sample count over "
                         "the budget, as grey")
    return ap


def cli_estimator(a):
    """The command line's (unbiased, roulette) as App takes them: None leaves
    the entry's key; --roulette switches --unbiased on."""
    return (True if a.unbiased or a.roulette is not None else None), a.roulette


def cli_adaptive(a, cfg):
    """The command line's (adaptive, adaptive_map) as App takes them: None leaves the entry's key.
    --adaptive alone is the default threshold; --adaptive T over an entry with an "adaptive" object
    replaces its threshold and keeps the rest."""
    from . import config as C
    spec = None
    if a.adaptive is not None:
        spec = dict(cfg.ADAPTIVE() or {})
        spec["threshold"] = C.DEFAULT_ADAPTIVE_THRESHOLD if a.adaptive is True else a.adaptive
    return spec, (True if a.adaptive_map else None)


def cli_lens(a):
    """The command line's lens in the config key's form, or None: the entry's
    own.  --aperture needs exactly one of --focus and --focus-at, and either
    needs --aperture."""
    focus = a.focus is not None or a.focus_at is not None
    if a.aperture is None:
        if focus:
            raise ValueError("--focus and --focus-at need --aperture")
        return None
    if not focus:
        raise ValueError("--aperture needs --focus or --focus-at")
    if a.focus is not None and a.focus_at is not None:
        raise ValueError("--focus and --focus-at exclude each other")
    if a.focus is not None:
        return {"aperture": a.aperture, "focus": a.focus}
    try:
        at = [int(x) for x in a.focus_at.split(",")]
    except ValueError:
        at = []
    if len(at) != 2:
        raise ValueError("--focus-at: expected a pixel X,Y, got %r" % (a.focus_at,))
    return {"aperture": a.aperture, "focus_at": at}


def cli_bump(a, cfg):
    """The height-map scale a run maps with, or None: --bump [SCALE] if given, else the entry's "bump"."""
    from . import config as C
    return cfg.BUMP() if a.bump is None else C.parse_bump(a.bump)


def cli_cutouts(a, cfg):
    """The alpha threshold a run cuts with, or None: --cutouts [THRESHOLD] if given, else the entry's "cutouts"."""
    from . import config as C
    return cfg.CUTOUTS() if a.cutouts is None else C.parse_cutouts(a.cutouts)


def cli_smooth(a, cfg):
    """The crease angle a run shades with, or None: --smooth [DEG] if given, else the entry's "smooth"."""
    from . import config as C
    return cfg.SMOOTH() if a.smooth is None else C.parse_smooth(a.smooth)


def _numbers(text, what, counts):
    try:
        v = [float(x) for x in text.split(",")]
    except ValueError:
        v = []
    if len(v) not in counts:
        raise ValueError("%s: expected %s comma-separated numbers, got %r" % (what, " or ".join(map(str, counts)), text))
    return v


def cli_environment(a, cfg):
    """The command line's environment in the config key's form, or None: the
    entry's own.  --env and --env-map replace the entry's; --env-scale and
    --env-rotate alone adjust the entry's map."""
    if a.env is not None and a.env_map is not None:
        raise ValueError("--env and --env-map exclude each other")
    adjust = a.env_scale is not None or a.env_rotate is not None
    if a.env is not None:
        if adjust:
            raise ValueError("--env-scale and --env-rotate belong to a map, not to --env")
        return {"color": _numbers(a.env, "--env", (3,))}
    own = cfg.ENVIRONMENT()
    if a.env_map is not None:
        e = {"map": os.path.abspath(a.env_map)}
    elif not adjust:
        return None
    elif own is not None and own["map"] is not None:
        e = {"map": own["map"], "scale": list(own["scale"]), "rotate": own["rotate"]}
    else:
        raise ValueError("--env-scale and --env-rotate need --env-map or a config entry with an environment map")
    if a.env_scale is not None:
        v = _numbers(a.env_scale, "--env-scale", (1, 3))
        e["scale"] = v[0] if len(v) == 1 else v
    if a.env_rotate is not None:
        e["rotate"] = a.env_rotate
    return e


def main(argv=None):
    a = parser().parse_args(argv)
    from . import config as C
    cfg = C.Config(a.config, a.configid)
    if cfg.TESTALL() or cfg.TESTBVH():
        from . import bvhtest
        bvhtest.run(cfg, root=os.path.dirname(os.path.abspath(a.config)))
        return 0
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws > 1:
        return _main_dist(a)
    from .app import App
    unbiased, roulette = cli_estimator(a)
    adaptive, adaptive_map = cli_adaptive(a, cfg)
    if adaptive is not None:
        unbiased = True
    app = App(a.config, a.configid, out_dir=a.out, jitter=True if a.jitter else None,
              denoise=True if a.denoise else None, environment=cli_environment(a, cfg), smooth=a.smooth,
              textures=True if a.textures else None, lens=cli_lens(a), bump=a.bump, cutouts=a.cutouts,
              unbiased=unbiased, roulette=roulette, adaptive=adaptive, adaptive_map=adaptive_map)
    if app.lens_spec is not None:
        print("lens: jitter switched on (a lens needs a fresh primary ray every frame)")
    t0 = time.time()
    if a.frames and app.adaptive is not None:
        raise ValueError("--frames does not go with adaptive sampling: its budget is the entry's attempt + 1")
    if a.frames:
        app.update(a.frames)
        path = app.output_picture()
    else:
        path = app.run()
    print("wrote %s (%dx%d, %d frames, %.2f s)" % (path, app.w, app.h, app.attempt_count, time.time() - t0))
    if a.preview:
        from . import scene as S
        print("wrote", S.write_png(a.preview, app.preview()))
    return 0


def _main_dist(a):
    import torch
    import torch.distributed as dist

    from . import config as C
    from . import dist as D
    from . import render as R
    from . import scene as S
    from .app import apply_bump, apply_environment, apply_smooth, apply_textures, config_scene, resolve_lens
    # adaptive sampling is single-GPU: refused here, before any rank touches a GPU
    D.refuse_adaptive(a.adaptive is not None or a.adaptive_map or C.Config(a.config, a.configid).ADAPTIVE() is not None)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # MCPT_DIST_SHARED_GPU=1 rehearses the N-rank job on a one-GPU box: every
    # rank on device 0, gloo for the one reduce (tests/test_gpu_dist.py)
    shared = os.environ.get("MCPT_DIST_SHARED_GPU") == "1"
    if shared:
        local = 0
    torch.cuda.set_device(local)
    if shared:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    cfg = C.Config(a.config, a.configid)
    if not cfg.USEOPENCL():
        raise ValueError('config has "opencl": false — the reference throws "Not Implemented" here')
    root = os.path.dirname(os.path.abspath(a.config))
    # the same scene and tree as App.init: the GPU treelet pass over a fresh
    # HLBVH for every bvhtype (scenebuild.cpp:66-95)
    data = config_scene(cfg, root, local)
    rnd = R.Renderer(local)
    sc = rnd.upload(data)
    # every rank lights its own scene: its stripes' misses read the same environment
    env = cli_environment(a, cfg)
    apply_environment(rnd, sc, cfg.ENVIRONMENT() if env is None else C.parse_environment(env), cfg, root)
    apply_smooth(rnd, sc, cli_smooth(a, cfg), cfg, root)  # and shades with its own copy of the vertex normals
    textured = apply_textures(rnd, sc, a.textures or cfg.TEXTURES(), cfg, root, cli_cutouts(a, cfg))  # and of the textures, with their alpha
    apply_bump(rnd, sc, cli_bump(a, cfg), cfg, root)  # and of the bump and normal maps
    w, h = cfg.WIDTH(), cfg.HEIGHT()
    frames = a.frames or cfg.MAXATTEPMT() + 1
    spec = cli_lens(a)
    spec = cfg.LENS() if spec is None else C.parse_lens(spec)
    lens = resolve_lens(rnd, sc, S.parse_camera(cfg.GETCAMERA()), w, h, spec)  # every rank: the same lens
    unbiased, roulette = cli_estimator(a)
    roulette = cfg.ROULETTE() if roulette is None else C.parse_roulette(roulette)
    unbiased = bool(unbiased or cfg.UNBIASED() or roulette)  # every rank: the same estimator
    out = D.render_distributed(rnd, sc, S.parse_camera(cfg.GETCAMERA()), w, h, cfg.MAXDEPTH(), cfg.MAXATTEPMT(),
                               frames, R.default_seeds(w * h), jitter=a.jitter or cfg.JITTER(), lens=lens,
                               unbiased=unbiased, roulette=roulette)
    if dist.get_rank() == 0:
        path = os.path.join(a.out, cfg.GETOBJNAME() + ".hdr")
        S.write_hdr(path, out[0].reshape(h, w, 4), flip=True)
        print("wrote", path)
        if a.denoise or cfg.DENOISE():
            # the same filter on the reduced image: the whole image's first hits are one extra pass here
            from .app import App
            st = rnd.new_state(w, h, out[2])
            st.hist.copy_(torch.from_numpy(out[0]).view(-1, 4))
            st.count.copy_(torch.from_numpy(out[1]))
            hits = rnd.first_hits(sc, S.parse_camera(cfg.GETCAMERA()), w, h)
            albedo = rnd.first_hit_albedo(sc, hits) if textured else None
            den = rnd.denoise(sc, hits, st, albedo=albedo).cpu().numpy().reshape(h, w, 4)
            S.write_hdr(App.denoised_path(path), den, flip=True)
            print("wrote", App.denoised_path(path))
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
