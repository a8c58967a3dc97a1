"""Device-side driver over libmcpt_hip.so: the reference's OpenCL::init/update
frame loop (MCPT/OpenCLApp.cpp:36-82), RayGeneration (raygeneration.cpp),
SceneBuild/SceneCL (scenebuild.cpp) and ColorOut (colorout.cpp) on one GPU.

PyTorch only provides device memory and the stream; every kernel is the HIP
code in csrc/mcpt_device.hip.  Buffers are raw byte tensors holding the
reference's record layouts.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import adaptive as AD


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_bytes(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def default_seeds(n, variant="splitmix"):
    """Per-pixel 32-bit seeds.  The reference draws them with srand(time); rand()
    (scenebuild.cpp:113-120) — non-deterministic — so parity runs take seeds as
    an input.  'splitmix': splitmix64(0x5EED ^ i) & 0xFFFFFFFF;
    'msvc15' keeps 15 bits like MSVC's rand()."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(0x5EED) ^ i) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    s = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if variant == "msvc15":
        s &= np.uint32(0x7FFF)
    return s


def _lens_struct(lens):
    """(R, F) -> L.Lens, None -> None.  Values are checked by the library."""
    if lens is None:
        return None
    try:
        r, f = lens
        return L.Lens(float(r), float(f))
    except (TypeError, ValueError):
        raise ValueError("lens must be (radius, focus_distance), got %r" % (lens,))


def _roulette_depth(roulette):
    """render_frames' `roulette` -> mcpt_estimator.rr_depth: False / 0 off,
    True depth 3, else the depth (its range is checked by the library)."""
    if roulette is True:
        return 3
    if roulette is False or roulette is None:
        return 0
    if isinstance(roulette, (int, np.integer)):
        return int(roulette)
    raise ValueError("roulette must be a depth (an integer, 0: off) or a bool, got %r" % (roulette,))


def _estimator_struct(unbiased, roulette):
    """(unbiased, roulette) -> L.Estimator, or None for the default estimator.
    Roulette without the counted history is refused here, before any C call."""
    depth = _roulette_depth(roulette)
    if depth > 0 and not unbiased:
        raise ValueError("render_frames: roulette needs unbiased=True (a path it ends is a zero sample "
                         "that has to be counted)")
    if not unbiased and depth == 0:
        return None
    return L.Estimator(int(bool(unbiased)), depth)


def focus_from_hit(t, ray_direction, camera_direction):
    """The focus distance that puts a first hit in focus: F = t * dot(d, c^),
    the hit's distance `t` along the unit ray direction `d`, measured along the
    view axis c^ = camera_direction / |camera_direction| (float64, host)."""
    d = np.asarray(ray_direction, dtype=np.float64)[:3]
    c = np.asarray(camera_direction, dtype=np.float64)[:3]
    return float(t) * float(np.dot(d, c / np.linalg.norm(c)))


class DeviceScene:
    """SceneBuild::buildScene result living in HBM (child-box node layout).
    `data` is a host SceneData (mcpt_scene_upload), or a tuple (tris, nodes,
    mats) whose tris / nodes are device byte tensors (mcpt_scene_upload_device:
    everything built on the GPU, the same bytes)."""

    ARRAYS = ("near4", "near4q", "nodes4", "nodes", "tris", "triq", "near4x", "tri4", "nodes4x")

    def __init__(self, renderer, data):
        self.renderer = renderer
        self.data = data
        self.handle = ctypes.c_void_p()
        self.schedule = L.SCHED_PAIRED  # k_render leaf-test schedule: paired measured faster on C2-C5 (tune_schedule)
        if isinstance(data, tuple):
            t, nd, mats = data
            m = np.ascontiguousarray(mats)
            n = t.numel() // L.TRIANGLE.itemsize
            L.check(L.lib().mcpt_scene_upload_device(renderer.ctx, L.ptr(t), n, L.ptr(nd), nd.numel() // L.BVHNODE.itemsize,
                                                     L.ptr(m), len(m), _stream(), ctypes.byref(self.handle)))
            return
        t = np.ascontiguousarray(data.tris)
        nd = np.ascontiguousarray(data.nodes)
        m = np.ascontiguousarray(data.mats)
        L.check(L.lib().mcpt_scene_upload(renderer.ctx, L.ptr(t), len(t), L.ptr(nd), len(nd), L.ptr(m), len(m),
                                          ctypes.byref(self.handle)))

    def read(self, which):
        """One device array as bytes (mcpt_scene_read; which: a name of ARRAYS
        or "meta" -> int32 {stack_depth, stack_depth4, quantized, n_internal})."""
        k = 6 if which == "meta" else self.ARRAYS.index(which)
        k += 1 if which != "meta" and k >= 6 else 0  # near4x, tri4, nodes4x: codes 7-9, after the meta record's
        n = ctypes.c_int64()
        L.check(L.lib().mcpt_scene_read(self.handle, k, None, 0, ctypes.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        L.check(L.lib().mcpt_scene_read(self.handle, k, L.ptr(buf), n.value, ctypes.byref(n)))
        return buf.view(np.int32) if which == "meta" else buf

    def close(self):
        if self.handle:
            L.lib().mcpt_scene_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImageState:
    """Per-pixel state that persists across frames: seed chain (randBuffer),
    accumulated mean (frameBuffer) and sample count (sampleCount)."""

    def __init__(self, width, height, seeds, device):
        n = width * height
        self.width, self.height = width, height
        self.seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32)).to(device)
        self.hist = torch.zeros((n, 4), dtype=torch.float32, device=device)
        self.count = torch.zeros(n, dtype=torch.int32, device=device)
        self.frames_done = 0

    def image(self):
        """(H, W, 4) float32 accumulated image, row 0 = bottom (GL convention)."""
        return self.hist.cpu().numpy().reshape(self.height, self.width, 4)

    def seeds_np(self):
        return self.seeds.cpu().numpy().view(np.uint32)


class _HalfState:
    """One half history of an adaptive render: its own mean and count on the parent state's seed chain."""

    def __init__(self, state):
        self.width, self.height = state.width, state.height
        self.seeds = state.seeds
        self.hist = torch.zeros_like(state.hist)
        self.count = torch.zeros_like(state.count)
        self.frames_done = 0


class Renderer:
    """One GPU context (OpenCLBasic::init equivalent)."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise L.MCPTError("no GPU: the HIP path has no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.ctx = ctypes.c_void_p()
        L.check(L.lib().mcpt_ctx_create(device, ctypes.byref(self.ctx)))

    def close(self):
        if self.ctx:
            L.lib().mcpt_ctx_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, data):
        return DeviceScene(self, data)

    @staticmethod
    def set_sah_optimize(passes=3):
        """mcpt_set_sah_optimize: process-wide, for the scenes uploaded from
        here on.  passes > 0 (default 3) optimises the search tree of scenes of
        up to 131072 triangles by subtree reinsertion under the plain tree's
        stack need; 0 or False keeps the plain tree.  Cost only, never results."""
        L.check(L.lib().mcpt_set_sah_optimize(3 if passes is True else int(passes)))

    @staticmethod
    def sah_optimize():
        """The passes mcpt_set_sah_optimize set (0: the plain tree)."""
        p = ctypes.c_int32()
        L.check(L.lib().mcpt_get_sah_optimize(ctypes.byref(p)))
        return p.value

    def set_stats(self, on):
        L.check(L.lib().mcpt_set_stats(self.ctx, int(bool(on))))
        self._stats_on = bool(on)

    def stats(self):
        s = L.Stats()
        L.check(L.lib().mcpt_get_stats(self.ctx, ctypes.byref(s)))
        out = {f: getattr(s, f) for f, _ in L.Stats._fields_ if f not in ("pad", "pad1")}
        out["phase_ticks"] = list(out["phase_ticks"])
        if hasattr(L.lib(), "mcpt_get_node_format"):  # 0 128-B, 1 64-B quantized, 2 96-B exact nodes
            fmt = ctypes.c_int32()
            L.check(L.lib().mcpt_get_node_format(self.ctx, ctypes.byref(fmt)))
            out["node_format"] = fmt.value
        return out

    def set_pixel_segments(self, counts, iters=None):
        """mcpt_set_pixel_segments: with stats on, render calls add each pixel's
        segments into `counts` and its busy loop iterations into `iters` (int32
        CUDA tensors of width*height, zeroed by the caller; None: not
        collected)."""
        self._px_counts = (counts, iters)  # kept alive while the library holds the pointers
        n = min([t.numel() for t in (counts, iters) if t is not None], default=0)
        L.check(L.lib().mcpt_set_pixel_segments(self.ctx, None if counts is None else L.ptr(counts),
                                                None if iters is None else L.ptr(iters), n))

    def primary_cost(self):
        """mcpt_get_primary_cost: the cached view's per-pixel primary-ray
        traversal cost (uint32, width*height), or None without a cache."""
        n = ctypes.c_int64()
        L.check(L.lib().mcpt_get_primary_cost(self.ctx, None, 0, ctypes.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value, np.uint32)
        L.check(L.lib().mcpt_get_primary_cost(self.ctx, L.ptr(out), n.value, ctypes.byref(n)))
        return out

    def wave_log(self):
        """mcpt_get_wave_log (MCPT_PHASE_TIMING library only): per workgroup of
        the last launch an int64 row (start, first dry, end, last entry start
        [100 MHz ticks], iterations, entries started, lane-iterations waiting,
        XCD); an empty (0, 8) array on release builds."""
        n = ctypes.c_int64()
        L.check(L.lib().mcpt_get_wave_log(self.ctx, None, 0, ctypes.byref(n)))
        if n.value == 0:
            return np.zeros((0, 8), np.int64)
        buf = np.zeros((n.value, 8), np.uint64)
        L.check(L.lib().mcpt_get_wave_log(self.ctx, L.ptr(buf), n.value, ctypes.byref(n)))
        return buf[:, [0, 1, 2, 5, 3, 4, 6, 7]].astype(np.int64)

    def entry_log(self):
        """mcpt_get_entry_log (MCPT_PHASE_TIMING library only): (pixels, blocks, 3)
        uint32 claim / start / end times (100 MHz ticks, low 32 bits) of the
        last one-launch call's queue entries; None when nothing was logged."""
        n, b = ctypes.c_int64(), ctypes.c_int32()
        L.check(L.lib().mcpt_get_entry_log(self.ctx, None, 0, ctypes.byref(n), ctypes.byref(b)))
        if n.value == 0:
            return None
        buf = np.zeros((n.value, 3), np.uint32)
        L.check(L.lib().mcpt_get_entry_log(self.ctx, L.ptr(buf), n.value, ctypes.byref(n), ctypes.byref(b)))
        return buf.reshape(-1, b.value, 3)

    def set_tuning(self, **knobs):
        """mcpt_set_tuning: k_render launch-plan knobs (leaf_threshold,
        shade_threshold, queue_chunk, block_entries, max_block_frames,
        stack_window 0 auto / 1 window / 2 whole stack, lds_pad, queues, quantized 0 auto / 1
        the 64-B search-tree nodes / 2 the 128-B ones / 3 the 96-B exact ones); speed only,
        unnamed knobs take their defaults."""
        t = L.Tuning()
        for k, v in knobs.items():
            if k not in dict(L.Tuning._fields_):
                raise L.MCPTError("unknown tuning knob %r" % k)
            setattr(t, k, int(v))
        L.check(L.lib().mcpt_set_tuning(self.ctx, ctypes.byref(t)))

    def drop_caches(self):
        """mcpt_drop_caches: forget the primary-hit cache; the next render call
        recomputes (or traces) the primary hits itself."""
        L.check(L.lib().mcpt_drop_caches(self.ctx))

    def get_tuning(self):
        t = L.Tuning()
        L.check(L.lib().mcpt_get_tuning(self.ctx, ctypes.byref(t)))
        return {f: getattr(t, f) for f, _ in L.Tuning._fields_}

    def selfcheck_trig(self):
        """(angle, range) mismatch counts of the inline randomDirection sin/cos
        against the ocml calls (mcpt_selfcheck_trig); (0, 0) on a good build."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().mcpt_selfcheck_trig(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def selfcheck_pow(self, exponents):
        """Mismatches of the Phong lobe's pow restatement against ocml's
        pow_f32 over every float in (0, 1 + 2^-10] for each exponent
        (mcpt_selfcheck_pow); 0 on a good build."""
        ys = np.ascontiguousarray(exponents, np.float32)
        n = ctypes.c_int64()
        L.check(L.lib().mcpt_selfcheck_pow(self.ctx, L.ptr(ys), len(ys), ctypes.byref(n)))
        return n.value

    def measure_read_bw(self, nbytes=4 << 30):
        """Streaming HBM read bandwidth in GB/s (mcpt_measure_read_bw)."""
        g = ctypes.c_double()
        L.check(L.lib().mcpt_measure_read_bw(self.ctx, int(nbytes), ctypes.byref(g)))
        return g.value

    def gather_probe(self, record_bytes, table_bytes=1 << 31):
        """Device ms of mcpt_gather_probe (the FETCH_SIZE calibration kernel)."""
        g = ctypes.c_double()
        L.check(L.lib().mcpt_gather_probe(self.ctx, int(record_bytes), int(table_bytes), ctypes.byref(g)))
        return g.value

    def new_state(self, width, height, seeds=None):
        if seeds is None:
            seeds = default_seeds(width * height)
        return ImageState(width, height, seeds, self.device)

    # ---------------------------------------------------------- fused path
    def render_frames(self, scene, camera, state, max_depth, max_attempt, frames, frame_begin=None,
                      stripe_rows=16, stripe_index=0, stripe_count=1, mode=L.MODE_EXACT,
                      frames_per_launch=0, schedule=None, jitter=None, lens=None, unbiased=False, roulette=0,
                      tiles=None):
        """Frames [frame_begin, frame_begin+frames) for this GPU's row stripes
        (OpenCL::update x frames + ColorOut accumulation).  `schedule`
        (L.SCHED_*; default: the scene's, see tune_schedule) only changes speed.
        `jitter` (opt-in antialiasing; mcpt_render_params.jitter): every frame's
        primary ray goes through a point of the pixel's footprint drawn from
        the pixel's seed chain instead of its corner; such a call does without
        the primary-hit cache.  True / False or 0 / 1; another integer is the
        library's MCPT_ERR_ARG.  None (the default): on with a lens, else off.
        `lens` = (R, F) (opt-in depth of field; mcpt_render_frames_lens): a
        thin lens of radius R focused at distance F along the view axis, in
        scene units.  A lens needs a fresh primary ray every frame, so it
        switches `jitter` on; jitter=False given with a lens is a ValueError.
        R = 0 is no lens (the jittered call's bits).
        `unbiased` (opt-in; mcpt_estimator.count_all): the history counts every
        sample, the all-zero ones included, so a pixel is the mean of all its
        samples and `count` the frame count.  `roulette` (mcpt_estimator.rr_depth;
        0: off): Russian roulette on diffuse and glossy bounces from that depth
        on, the survival probability the bounce's albedo.  A path it ends is a
        zero sample that has to be counted: roulette > 0 with unbiased=False is
        a ValueError.
        `tiles` (opt-in; mcpt_render_frames_tiles): a mask with one entry per 8x8
        tile, row-major over ceil(W/8) x ceil(H/8); only the tiles with a nonzero
        entry are rendered, each of their pixels exactly as the whole-image call
        renders it, and no other pixel's state is read or written.  None: every
        tile.  Its length is checked by the library; it needs stripe_count = 1."""
        tiles_c = tile_mask = None
        if tiles is not None:
            tile_mask = np.ascontiguousarray(np.asarray(tiles).reshape(-1) != 0, np.uint8)
            tiles_c = L.TileSet(tile_mask.ctypes.data, len(tile_mask), 0)
        est_c = _estimator_struct(unbiased, roulette)
        lens_c = _lens_struct(lens)
        if lens_c is not None:
            if jitter is not None and not jitter:
                raise ValueError("render_frames: a lens needs jitter (leave `jitter` out, or pass True)")
            jitter = True
        elif jitter is None:
            jitter = False
        p = L.RenderParams()
        p.width, p.height = state.width, state.height
        p.max_depth, p.max_attempt = int(max_depth), int(max_attempt)
        p.frame_begin = state.frames_done if frame_begin is None else int(frame_begin)
        p.frames = int(frames)
        p.stripe_rows, p.stripe_index, p.stripe_count = int(stripe_rows), int(stripe_index), int(stripe_count)
        p.mode = int(mode)
        p.frames_per_launch = int(frames_per_launch)
        p.schedule = int(getattr(scene, "schedule", L.SCHED_PAIRED) if schedule is None else schedule)
        p.jitter = int(jitter)
        cam = np.ascontiguousarray(camera)
        if tiles_c is not None:
            L.check(L.lib().mcpt_render_frames_tiles(self.ctx, scene.handle, L.ptr(cam),
                                                     None if lens_c is None else ctypes.byref(lens_c),
                                                     None if est_c is None else ctypes.byref(est_c),
                                                     ctypes.byref(tiles_c), ctypes.byref(p), L.ptr(state.seeds),
                                                     L.ptr(state.hist), L.ptr(state.count), _stream()))
        elif est_c is not None:
            L.check(L.lib().mcpt_render_frames_est(self.ctx, scene.handle, L.ptr(cam),
                                                   None if lens_c is None else ctypes.byref(lens_c),
                                                   ctypes.byref(est_c), ctypes.byref(p), L.ptr(state.seeds),
                                                   L.ptr(state.hist), L.ptr(state.count), _stream()))
        elif lens_c is not None:
            L.check(L.lib().mcpt_render_frames_lens(self.ctx, scene.handle, L.ptr(cam), ctypes.byref(lens_c),
                                                    ctypes.byref(p), L.ptr(state.seeds), L.ptr(state.hist),
                                                    L.ptr(state.count), _stream()))
        else:
            L.check(L.lib().mcpt_render_frames(self.ctx, scene.handle, L.ptr(cam), ctypes.byref(p), L.ptr(state.seeds),
                                               L.ptr(state.hist), L.ptr(state.count), _stream()))
        state.frames_done = p.frame_begin + p.frames
        return state

    # ---------------------------------------------------------- adaptive sampling
    def tile_error(self, width, height, hist_a, count_a, hist_b, count_b, floor=1e-4):
        """mcpt_tile_error: the half-buffer error estimate of every 8x8 tile of
        two half histories (device tensors as ImageState keeps them), a float32
        device tensor of ceil(W/8) * ceil(H/8), row-major."""
        tx, ty = AD.tile_grid(width, height)
        err = torch.empty(tx * ty, dtype=torch.float32, device=self.device)
        L.check(L.lib().mcpt_tile_error(self.ctx, int(width), int(height), L.ptr(hist_a), L.ptr(count_a), L.ptr(hist_b),
                                        L.ptr(count_b), float(floor), L.ptr(err), _stream()))
        return err

    def merge_halves(self, hist_a, count_a, hist_b, count_b, hist_out=None, count_out=None):
        """mcpt_merge_halves: the count-weighted mean and the summed count of two
        half histories, into (hist_out, count_out) (new tensors when None)."""
        n = count_a.numel()
        if hist_out is None:
            hist_out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        if count_out is None:
            count_out = torch.empty(n, dtype=torch.int32, device=self.device)
        L.check(L.lib().mcpt_merge_halves(self.ctx, L.ptr(hist_a), L.ptr(count_a), L.ptr(hist_b), L.ptr(count_b), n,
                                          L.ptr(hist_out), L.ptr(count_out), _stream()))
        return hist_out, count_out

    def render_adaptive(self, scene, camera, state, max_depth, frames, threshold, min_frames=16, batch=8, floor=1e-4,
                        dilate=True, jitter=None, lens=None, roulette=0, mode=L.MODE_EXACT, schedule=None):
        """Adaptive sampling (opt-in, no reference counterpart): at most `frames`
        frames per pixel, spent where the image is noisy.  Frames go alternately
        into two half histories A and B that share `state`'s seed chain; round 0
        renders min_frames / 2 frames into A and then into B on every tile; each
        later round reads mcpt_tile_error of the halves, marks the tiles above
        `threshold` (adaptive.select_tiles; `dilate` adds their neighbours),
        stops when none is left or the budget is spent, and else renders
        min(batch, frames - issued) / 2 frames into A and then into B on those
        tiles alone (render_frames' `tiles`).  The history counts every sample
        (`unbiased` is always on).  At the end mcpt_merge_halves writes
        state.hist and state.count; state.frames_done is the frames issued.
        `state` must be fresh (frames_done == 0); frames, min_frames and batch
        are even with 2 <= min_frames <= frames; threshold >= 0 (inf: round 0
        alone; 0: every round whole-image while any tile's halves differ).  A
        ValueError otherwise, before any C call.  Returns an
        adaptive.AdaptiveReport.  Adaptive stopping is not exactly unbiased: a
        tile stops on a noisy estimate of its own error."""
        AD.check_arguments(frames, threshold, min_frames, batch, floor)
        if state.frames_done != 0:
            raise ValueError("render_adaptive: the state must be fresh (frames_done == 0), got %d" % state.frames_done)
        _roulette_depth(roulette)
        _lens_struct(lens)
        w, h = state.width, state.height
        halves = [_HalfState(state), _HalfState(state)]
        rep = AD.AdaptiveReport(w, h, int(frames))
        kw = dict(mode=mode, schedule=schedule, jitter=jitter, lens=lens, unbiased=True, roulette=roulette)

        def issue(n, mask):
            for half in halves:  # A, then B, on the one seed chain
                self.render_frames(scene, camera, half, max_depth, int(frames), n // 2, frame_begin=half.frames_done,
                                   tiles=mask, **kw)
            rep.round_frames.append(n)
            rep.frames_issued += n

        issue(int(min_frames), None)
        while True:
            n = AD.round_frames(rep.frames_issued, frames, batch)
            if n == 0:
                break
            a, b = halves
            err = self.tile_error(w, h, a.hist, a.count, b.hist, b.count, floor).cpu().numpy()
            mask = AD.select_tiles(err, threshold, rep.tiles_x, rep.tiles_y, dilate)
            rep.errors.append(err.reshape(rep.tiles_y, rep.tiles_x))
            rep.masks.append(mask.reshape(rep.tiles_y, rep.tiles_x))
            if not mask.any():
                break
            issue(n, mask)
        a, b = halves
        self.merge_halves(a.hist, a.count, b.hist, b.count, state.hist, state.count)
        state.frames_done = rep.frames_issued
        rep.samples = int(state.count.sum(dtype=torch.int64).item())
        rep.fraction = rep.samples / float(w * h * int(frames))
        return rep

    def tune_schedule(self, scene, camera, state, max_depth, max_attempt, frames=64, trials=1, **kw):
        """Pick the faster leaf-test schedule for this scene and view: render
        `frames` frames `trials` times with each schedule on a scratch copy
        of `state` (interleaved, device time of each call), keep the faster
        in scene.schedule.  Both schedules give bit-identical images, so this
        only moves speed.  Keywords (`jitter`, `lens`, `unbiased` and `roulette` among them) go to the scratch
        renders it times.  Returns (schedule, {schedule: best ms})."""
        sched, _, best = self.tune(scene, camera, state, max_depth, max_attempt, frames, trials, shade_thresholds=None,
                                   fetch_thresholds=None, tile_orders=None, **kw)
        return sched, {k[0]: v for k, v in best.items()}

    def tune(self, scene, camera, state, max_depth, max_attempt, frames=64, trials=1, shade_thresholds=(32, 40, 48),
             fetch_thresholds=(1, 8), block_entries=(8, 16), last_block=True, tile_orders=(0, 1, 2), fresh_view=False,
             **kw):
        """tune_schedule over the leaf-test schedule, the S-phase threshold
        (mcpt_tuning.shade_threshold) and then the fetch threshold
        (mcpt_tuning.fetch_threshold), then the block sizing
        (mcpt_tuning.block_entries) jointly with the tile order
        (mcpt_tuning.tile_order: dearest tiles first by their costliest or
        summed primary-ray cost, or image order), then a short last block
        against equal blocks (mcpt_tuning.last_block_frames -1, ceil(frames / 8)
        or ceil(frames / 4)) jointly with the block sizing again; ties keep the
        baseline value.  Their best values
        differ by scene (round 2, 3-frame blocks: veach_mis S 40, fetch 8;
        cbox S 32-40, fetch 8; the 10 M-triangle soup S 32, fetch 1; round 4:
        cbox gains 5-10 % from the dearest-first order, veach_mis loses 5 %).
        Every combination gives the same bits.  Each setting is judged by its
        median over the trials (a single timed call is what the pick has to
        predict; the minimum favoured lucky runs).  fresh_view: every trial
        call first drops the primary-hit cache, so it pays the primary-hit
        pass and the tile sort as a call of a new view does (bench.py's timed
        call).  Keywords of render_frames (mode, stripes, `jitter`, `lens`, `unbiased`, `roulette`) go to every
        scratch render, so a jittered or defocused render is tuned as it will run.  The winner goes to
        scene.schedule and the renderer's tuning.  Returns (schedule,
        shade_threshold, {(schedule, shade, fetch, entries, tile_order): median ms})."""
        if getattr(self, "_stats_on", False):
            raise L.MCPTError("tune: counters must be off (they change the kernel)")
        base = self.get_tuning()
        ths = list(shade_thresholds) if shade_thresholds else [base["shade_threshold"]]
        scratch = ImageState.__new__(ImageState)
        scratch.width, scratch.height, scratch.frames_done = state.width, state.height, state.frames_done
        best, samples = {}, {}

        def trial(sched, th, fe, be, to):
            self.set_tuning(**dict(base, shade_threshold=th, fetch_threshold=fe, block_entries=be, tile_order=to))
            scratch.seeds, scratch.hist, scratch.count = state.seeds.clone(), state.hist.clone(), state.count.clone()
            if fresh_view:
                self.drop_caches()
            self.render_frames(scene, camera, scratch, max_depth, max_attempt, frames,
                               frame_begin=state.frames_done, schedule=sched, **kw)
            ms = self.stats()["kernel_ms"]
            samples.setdefault((sched, th, fe, be, to), []).append(ms)
            best.clear()  # median per setting: a single timed call is what the pick predicts
            best.update({k: sorted(v)[len(v) // 2] for k, v in samples.items()})

        def pick():  # fastest median; ties to the smaller key
            return min(best, key=lambda k: (best[k], k))

        fe0 = base["fetch_threshold"] or 1  # 0 = the default, 1
        be0 = base["block_entries"] or 8    # 0 = the default, 8
        to0 = base["tile_order"]
        try:
            for _ in range(int(trials)):
                for th in ths:
                    for sched in (L.SCHED_SINGLE, L.SCHED_PAIRED):
                        trial(sched, th, fe0, be0, to0)
            sched, th, fe, be, to = pick()
            if shade_thresholds and fetch_thresholds:  # then the fetch threshold, with that pair
                for _ in range(int(trials)):
                    for f in fetch_thresholds:
                        if f != fe0:
                            trial(sched, th, f, be0, to0)
                sched, th, fe, be, to = pick()
            if shade_thresholds and (block_entries or tile_orders):  # then block sizing x tile order
                bes = list(block_entries) if block_entries else [be0]
                tos = list(tile_orders) if tile_orders else [to0]
                for _ in range(int(trials)):
                    for b in bes:
                        for o in tos:
                            if (b, o) != (be0, to0):
                                trial(sched, th, fe, b, o)
                sched, th, fe, be, to = pick()
                if (be, to) != (be0, to0):  # other blocks or orders move the best S threshold (C3: 48 -> 40)
                    for _ in range(int(trials)):
                        for t in ths:
                            if t != th:
                                trial(sched, t, fe, be, to)
                    sched, th, fe, be, to = pick()
            lb = base["last_block_frames"]
            if shade_thresholds and last_block:
                # then a short last block against equal blocks, jointly with the
                # block sizing: the best last block can belong to the sizing
                # that lost with equal blocks (C2, 20 frames: (15, 5) at 8
                # entries beats 5-frame blocks at 16, which beat (10, 10))
                lbs = {-1, (int(frames) + 7) // 8, (int(frames) + 3) // 4}
                bes = sorted(set(block_entries)) if block_entries else [be]
                lsamples = {(be, lb): list(samples[(sched, th, fe, be, to)])}
                for _ in range(int(trials)):
                    for b in bes:
                        for v in sorted(lbs | {lb}):
                            if (b, v) == (be, lb):
                                continue
                            self.set_tuning(**dict(base, shade_threshold=th, fetch_threshold=fe, block_entries=b,
                                                   tile_order=to, last_block_frames=v))
                            scratch.seeds, scratch.hist, scratch.count = (state.seeds.clone(), state.hist.clone(),
                                                                          state.count.clone())
                            if fresh_view:
                                self.drop_caches()
                            self.render_frames(scene, camera, scratch, max_depth, max_attempt, frames,
                                               frame_begin=state.frames_done, schedule=sched, **kw)
                            lsamples.setdefault((b, v), []).append(self.stats()["kernel_ms"])
                lbest = {k: sorted(v)[len(v) // 2] for k, v in lsamples.items()}
                # ties go to the baseline (the sizing picked above with the auto rule's value), then the smaller key
                be, lb = min(lbest, key=lambda k: (lbest[k], k != (be, base["last_block_frames"]), k))
        finally:
            self.set_tuning(**base)
        scene.schedule = sched
        if shade_thresholds:
            self.set_tuning(**dict(base, shade_threshold=th, fetch_threshold=fe, block_entries=be,
                                   last_block_frames=lb, tile_order=to))
        return sched, th, best

    # ------------------------------------------------ wavefront (drop-in)
    def generate_rays(self, camera, width, height):
        """rayGenerator.cl: W*H Ray records (device bytes)."""
        rays = _dev_bytes(width * height * L.RAY.itemsize, self.device)
        cam = np.ascontiguousarray(camera)
        L.check(L.lib().mcpt_generate_rays(self.ctx, L.ptr(cam), width, height, L.ptr(rays), _stream()))
        return rays

    def generate_rays_jittered(self, camera, width, height, seeds):
        """generate_rays with a jittered render's sub-pixel offsets
        (mcpt_generate_rays_jittered): each pixel's two draws come from, and
        advance, `seeds` (a W*H int32 CUDA tensor, in place)."""
        if seeds.numel() != width * height or seeds.element_size() != 4 or not seeds.is_cuda:
            raise L.MCPTError("generate_rays_jittered: seeds must be a CUDA tensor of width*height 32-bit words")
        rays = _dev_bytes(width * height * L.RAY.itemsize, self.device)
        cam = np.ascontiguousarray(camera)
        L.check(L.lib().mcpt_generate_rays_jittered(self.ctx, L.ptr(cam), width, height, L.ptr(seeds), L.ptr(rays),
                                                    _stream()))
        return rays

    def generate_rays_lens(self, camera, width, height, seeds, lens):
        """generate_rays_jittered plus the thin lens `lens` = (R, F) of
        render_frames (mcpt_generate_rays_lens): four draws a pixel, the two
        of the jitter and then the two of the lens sample.  None or R = 0: the
        jittered call, two draws."""
        if seeds.numel() != width * height or seeds.element_size() != 4 or not seeds.is_cuda:
            raise L.MCPTError("generate_rays_lens: seeds must be a CUDA tensor of width*height 32-bit words")
        rays = _dev_bytes(width * height * L.RAY.itemsize, self.device)
        cam = np.ascontiguousarray(camera)
        lens_c = _lens_struct(lens)
        L.check(L.lib().mcpt_generate_rays_lens(self.ctx, L.ptr(cam), None if lens_c is None else ctypes.byref(lens_c),
                                                width, height, L.ptr(seeds), L.ptr(rays), _stream()))
        return rays

    def intersect(self, scene, rays, hits=None, tmin=0.001, mode=L.MODE_EXACT):
        """intersect.cl on a ray buffer; returns the Hit buffer."""
        n = rays.numel() // L.RAY.itemsize
        if hits is None:
            hits = torch.zeros(n * L.HIT.itemsize, dtype=torch.uint8, device=self.device)
        L.check(L.lib().mcpt_intersect(self.ctx, scene.handle, L.ptr(rays), n, L.ptr(hits), float(tmin), int(mode),
                                       _stream()))
        return hits

    def shade(self, scene, rays, hits, color, seeds, max_depth, roulette=0):
        """shade.cl on (rays, hits, colour, seeds) in place.  `roulette` > 0:
        with render_frames' Russian roulette from that depth (mcpt_shade_est)."""
        n = rays.numel() // L.RAY.itemsize
        if roulette:
            L.check(L.lib().mcpt_shade_est(self.ctx, scene.handle, L.ptr(rays), L.ptr(hits), L.ptr(color), L.ptr(seeds),
                                           n, int(max_depth), _roulette_depth(roulette), _stream()))
            return
        L.check(L.lib().mcpt_shade(self.ctx, scene.handle, L.ptr(rays), L.ptr(hits), L.ptr(color), L.ptr(seeds), n,
                                   int(max_depth), _stream()))

    def accumulate(self, color, hist, count, max_attempt, count_all=False):
        """history.cl: running mean of non-zero samples; count_all: of every
        sample (render_frames' `unbiased`; mcpt_accumulate_all)."""
        n = count.numel()
        fn = L.lib().mcpt_accumulate_all if count_all else L.lib().mcpt_accumulate
        L.check(fn(self.ctx, L.ptr(color), L.ptr(hist), L.ptr(count), n, int(max_attempt), _stream()))

    def gamma_preview(self, color, out=None):
        """testkernel.cl func (ColorOut's GL display pass): float4 colours ->
        (pow(c, 1/2.2f) per channel, w = 0), a new float32 (n, 4) tensor unless
        `out` is given (may be `color` itself)."""
        if color.dtype != torch.float32 or not color.is_cuda or color.numel() % 4:
            raise L.MCPTError("gamma_preview: a float32 CUDA tensor of float4 colours")
        color = color.contiguous()
        if out is None:
            out = torch.empty_like(color)
        elif (out.dtype != torch.float32 or not out.is_cuda or out.device != color.device
              or not out.is_contiguous() or out.numel() != color.numel()):
            raise L.MCPTError("gamma_preview: out must be a contiguous float32 CUDA tensor the size of color")
        L.check(L.lib().mcpt_gamma_preview(self.ctx, L.ptr(color), L.ptr(out), color.numel() // 4, _stream()))
        return out.view(-1, 4)

    # ------------------------------------------- environment lighting (opt-in)
    def set_environment(self, scene, scale=(1.0, 1.0, 1.0), map=None, rotate=0.0):
        """mcpt_scene_set_environment: a ray that leaves `scene` picks up
        scale * map(direction) instead of black.  `scale`: a number or (r, g, b),
        finite and >= 0; `map`: None (a constant environment) or a lat-long
        image (height, width, 3) float32, row 0 the top (scene.read_hdr's
        layout), finite and >= 0; `rotate`: degrees about +Y.  Replaces a
        previous environment; the primary-hit cache stays valid."""
        s = np.broadcast_to(np.asarray(scale, np.float32), (3,)) if np.ndim(scale) == 0 else np.asarray(scale, np.float32)
        if s.shape != (3,):
            raise ValueError("set_environment: scale is a number or (r, g, b)")
        e = L.Environment()
        e.scale[0], e.scale[1], e.scale[2], e.scale[3] = float(s[0]), float(s[1]), float(s[2]), 0.0
        e.rotate_deg = float(rotate)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, np.float32)
            if m.ndim != 3 or m.shape[2] != 3 or m.size == 0:
                raise ValueError("set_environment: map is (height, width, 3), height and width at least 1")
            e.map_rgb = m.ctypes.data
            e.height, e.width = m.shape[0], m.shape[1]
        L.check(L.lib().mcpt_scene_set_environment(self.ctx, scene.handle, ctypes.byref(e)))

    def clear_environment(self, scene):
        """Back to the reference's black for rays that miss (the bits of a
        scene whose environment was never set)."""
        L.check(L.lib().mcpt_scene_set_environment(self.ctx, scene.handle, None))

    def env_eval(self, scene, rays):
        """mcpt_env_eval: the scene's environment radiance for every record of
        a Ray buffer (device bytes), a float32 (n, 4) device tensor (rgb, 0);
        zeros without an environment.  With generate_rays: a background plate."""
        n = rays.numel() * rays.element_size() // L.RAY.itemsize
        out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        L.check(L.lib().mcpt_env_eval(self.ctx, scene.handle, L.ptr(rays), n, L.ptr(out), _stream()))
        return out

    # ----------------------------------------------- smooth shading (opt-in)
    def set_vertex_normals(self, scene, vn):
        """mcpt_scene_set_vertex_normals: hits on `scene` are shaded with the
        normal interpolated from `vn`, (n_tris, 3, 3) float32 unit normals in
        the upload's triangle order (scene.vertex_normals, load_obj_normals or
        smooth_normals), instead of the face normal.  Replaces previous ones and
        drops the primary-hit cache."""
        v = np.ascontiguousarray(vn, np.float32)
        n = len(scene.data.tris) if hasattr(scene.data, "tris") else scene.data[0].numel() // L.TRIANGLE.itemsize
        if v.size != n * 9:
            raise ValueError("set_vertex_normals: %d triangles need (n, 3, 3) normals, got %r" % (n, v.shape))
        L.check(L.lib().mcpt_scene_set_vertex_normals(self.ctx, scene.handle, L.ptr(v)))

    def clear_vertex_normals(self, scene):
        """Back to the face normals (the bits of a scene that never had vertex normals)."""
        L.check(L.lib().mcpt_scene_set_vertex_normals(self.ctx, scene.handle, None))

    def shading_normals(self, scene, tri_ids, points, dirs):
        """mcpt_shading_normals: the shading normal of (triangle, hit point, ray
        direction) queries on a scene with vertex normals: a float32 (n, 4)
        device tensor.  tri_ids: n int32; points, dirs: (n, 3) or (n, 4)."""
        ids = torch.as_tensor(np.ascontiguousarray(tri_ids, np.int32)).to(self.device)
        n = ids.numel()

        def quad(a):
            a = np.asarray(a, np.float32).reshape(n, -1)
            q = np.zeros((n, 4), np.float32)
            q[:, :a.shape[1]] = a
            return torch.from_numpy(q).to(self.device)
        p, d = quad(points), quad(dirs)
        out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        L.check(L.lib().mcpt_shading_normals(self.ctx, scene.handle, L.ptr(ids), L.ptr(p), L.ptr(d), n, L.ptr(out),
                                             _stream()))
        torch.cuda.current_stream().synchronize()  # (the inputs above are temporaries)
        return out

    # ------------------------------------------------- texture maps (opt-in)
    def set_textures(self, scene, uv, tri_tex, images):
        """mcpt_scene_set_textures: the diffuse lobe's kd on `scene` is
        multiplied by the bilinear, repeating lookup of each hit's texture.
        uv: (n_tris, 3, 2) float32 in the upload's triangle order; tri_tex:
        n_tris int32 indices into `images`, -1: no texture; images: (h, w, 3)
        linear float32 arrays, row 0 the top (scene.load_textures returns the
        three).  Replaces previous ones and drops the primary-hit cache."""
        u = np.ascontiguousarray(uv, np.float32)
        t = np.ascontiguousarray(tri_tex, np.int32)
        n = len(scene.data.tris) if hasattr(scene.data, "tris") else scene.data[0].numel() // L.TRIANGLE.itemsize
        if u.size != n * 6 or t.size != n:
            raise ValueError("set_textures: %d triangles need (n, 3, 2) uvs and n indices, got %r and %r" %
                             (n, u.shape, t.shape))
        imgs = [np.ascontiguousarray(im, np.float32) for im in images]
        for k, im in enumerate(imgs):
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("set_textures: image %d must be (height, width, 3), got %r" % (k, im.shape))
        recs = (L.TextureImage * max(len(imgs), 1))()
        for k, im in enumerate(imgs):
            recs[k].rgb, recs[k].width, recs[k].height = L.ptr(im), im.shape[1], im.shape[0]
        tx = L.Textures(L.ptr(u), L.ptr(t), len(imgs), ctypes.cast(recs, ctypes.c_void_p))
        L.check(L.lib().mcpt_scene_set_textures(self.ctx, scene.handle, ctypes.byref(tx)))
        scene.cutouts = None  # (a new texture set has no alpha)

    def clear_textures(self, scene):
        """Back to the materials' kd (the bits of a scene that never had textures)."""
        L.check(L.lib().mcpt_scene_set_textures(self.ctx, scene.handle, None))
        scene.cutouts = None

    # ------------------------------------------------ alpha cutouts (opt-in)
    def set_texture_alpha(self, scene, alphas, threshold=0.5):
        """mcpt_scene_set_texture_alpha: a hit on `scene` whose texture's alpha
        is below `threshold` (in (0, 1]) is cut: the ray goes on through it.
        alphas: one (h, w) float32 image in [0, 1], row 0 the top, of its
        texture's size, or None (opaque), per image of set_textures
        (scene.load_cutouts returns them).  max_depth is at most 255 on such a
        scene.  Replaces a previous alpha and drops the primary-hit cache; a
        later set_textures or clear_textures drops the alpha."""
        imgs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in alphas]
        for k, a in enumerate(imgs):
            if a is not None and a.ndim != 2:
                raise ValueError("set_texture_alpha: alpha %d must be (height, width), got %r" % (k, a.shape))
        ptrs = (ctypes.c_void_p * max(len(imgs), 1))()
        for k, a in enumerate(imgs):
            ptrs[k] = None if a is None else a.ctypes.data
        ta = L.TextureAlpha(len(imgs), ctypes.cast(ptrs, ctypes.c_void_p), float(threshold), 0.0)
        L.check(L.lib().mcpt_scene_set_texture_alpha(self.ctx, scene.handle, ctypes.byref(ta)))
        scene.cutouts = float(np.float32(threshold))

    def clear_texture_alpha(self, scene):
        """Back to opaque textures (the bits of a textured scene that never had an alpha)."""
        L.check(L.lib().mcpt_scene_set_texture_alpha(self.ctx, scene.handle, None))
        scene.cutouts = None

    def texture_eval(self, scene, tri_ids, points):
        """mcpt_texture_eval: kd's factor at (triangle, hit point) queries on a
        textured scene: a float32 (n, 4) device tensor (w: the cutout alpha, 1
        without one; zeros for an
        index outside the scene).  tri_ids: n int32, host or device; points:
        (n, 3) or (n, 4), host or a device (n, 4) float32 tensor."""
        if torch.is_tensor(tri_ids):
            ids = tri_ids.to(self.device, torch.int32).contiguous()
        else:
            ids = torch.as_tensor(np.ascontiguousarray(tri_ids, np.int32)).to(self.device)
        n = ids.numel()
        if torch.is_tensor(points):
            p = points.to(self.device, torch.float32).reshape(n, 4).contiguous()
        else:
            a = np.asarray(points, np.float32).reshape(n, -1)
            q = np.zeros((n, 4), np.float32)
            q[:, :a.shape[1]] = a
            p = torch.from_numpy(q).to(self.device)
        out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        L.check(L.lib().mcpt_texture_eval(self.ctx, scene.handle, L.ptr(ids), L.ptr(p), n, L.ptr(out), _stream()))
        torch.cuda.current_stream().synchronize()  # (the inputs above are temporaries)
        return out

    # ------------------------------------------ bump and normal maps (opt-in)
    def set_normal_maps(self, scene, uv, tri_map, images):
        """mcpt_scene_set_normal_maps: every hit on `scene` is shaded with its
        normal perturbed by the bilinear, repeating lookup of the triangle's
        tangent-space normal map.  uv: (n_tris, 3, 2) float32 in the upload's
        triangle order; tri_map: n_tris int32 indices into `images`, -1:
        unmapped; images: (h, w, 3) float32 unit normals with z > 0, row 0 the
        top (scene.load_bump_maps returns the three).  Replaces previous ones
        and drops the primary-hit cache."""
        u = np.ascontiguousarray(uv, np.float32)
        t = np.ascontiguousarray(tri_map, np.int32)
        n = len(scene.data.tris) if hasattr(scene.data, "tris") else scene.data[0].numel() // L.TRIANGLE.itemsize
        if u.size != n * 6 or t.size != n:
            raise ValueError("set_normal_maps: %d triangles need (n, 3, 2) uvs and n indices, got %r and %r" %
                             (n, u.shape, t.shape))
        imgs = [np.ascontiguousarray(im, np.float32) for im in images]
        for k, im in enumerate(imgs):
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("set_normal_maps: image %d must be (height, width, 3), got %r" % (k, im.shape))
        recs = (L.NormalMapImage * max(len(imgs), 1))()
        for k, im in enumerate(imgs):
            recs[k].xyz, recs[k].width, recs[k].height = L.ptr(im), im.shape[1], im.shape[0]
        nm = L.NormalMaps(L.ptr(u), L.ptr(t), len(imgs), ctypes.cast(recs, ctypes.c_void_p))
        L.check(L.lib().mcpt_scene_set_normal_maps(self.ctx, scene.handle, ctypes.byref(nm)))

    def clear_normal_maps(self, scene):
        """Back to the unmapped normals (the bits of a scene that never had maps)."""
        L.check(L.lib().mcpt_scene_set_normal_maps(self.ctx, scene.handle, None))

    def bump_eval(self, scene, tri_ids, points, dirs, normals):
        """mcpt_bump_eval: the mapped shading normal at (triangle, hit point,
        ray direction, unmapped normal N) queries on a mapped scene: a float32
        (n, 4) device tensor (zeros for an index outside the scene).  tri_ids:
        n int32; points, dirs, normals: (n, 3) or (n, 4), host arrays or device
        (n, 4) float32 tensors."""
        if torch.is_tensor(tri_ids):
            ids = tri_ids.to(self.device, torch.int32).contiguous()
        else:
            ids = torch.as_tensor(np.ascontiguousarray(tri_ids, np.int32)).to(self.device)
        n = ids.numel()

        def dev4(x):
            if torch.is_tensor(x):
                return x.to(self.device, torch.float32).reshape(n, 4).contiguous()
            a = np.asarray(x, np.float32).reshape(n, -1)
            q = np.zeros((n, 4), np.float32)
            q[:, :a.shape[1]] = a
            return torch.from_numpy(q).to(self.device)

        p, d, nn = dev4(points), dev4(dirs), dev4(normals)
        out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        L.check(L.lib().mcpt_bump_eval(self.ctx, scene.handle, L.ptr(ids), L.ptr(p), L.ptr(d), L.ptr(nn), n,
                                       L.ptr(out), _stream()))
        torch.cuda.current_stream().synchronize()  # (the inputs above are temporaries)
        return out

    def first_hit_albedo(self, scene, hits):
        """Renderer.denoise's `albedo` for a textured scene: texture_eval at
        the first hits (first_hits' records), forced to 1 where the first hit
        is a miss or not MCPT_DIFFUSE / MCPT_GLOSSY, so that those pixels keep
        their bits.  A float32 (n, 4) device tensor."""
        h = records(hits, L.HIT)
        mats = scene.data.mats if hasattr(scene.data, "mats") else None
        hit = h["t"] < np.float32(3.0e38)
        ids = np.where(hit, h["triangle_id"].astype(np.int64), 0).astype(np.int32)
        a = self.texture_eval(scene, ids, h["point"]).cpu().numpy()
        keep = hit.copy()
        if mats is not None and len(mats):
            ty = np.asarray(mats["type"])[np.clip(h["material_id"].astype(np.int64), 0, len(mats) - 1)]
            keep &= (ty == L.MCPT_DIFFUSE) | (ty == L.MCPT_GLOSSY)
        a[~keep] = 1.0
        a[:, 3] = 1.0
        return torch.from_numpy(a).to(self.device)

    # ------------------------------------------------------ denoise (opt-in)
    def first_hits(self, scene, camera, width, height, mode=L.MODE_EXACT):
        """Every pixel's first hit (W*H Hit records, device bytes): generate_rays
        then intersect, the corner ray's also when the render is jittered.  On
        a scene with cutouts (set_texture_alpha): the first hit that is not
        cut, its t the distance along the pixel's ray."""
        return self._first_uncut(scene, self.generate_rays(camera, width, height), mode)

    def _first_uncut(self, scene, rays, mode):
        """intersect, and on a scene with cutouts the loop that follows the cut
        rays on from their hit points (intersect + texture_eval on those rays
        alone, at most 255 rounds: shading's pass-count cap)."""
        hits = self.intersect(scene, rays, mode=mode)
        a0 = getattr(scene, "cutouts", None)
        if a0 is None:
            return hits
        h = records(hits, L.HIT).copy()
        r = records(rays, L.RAY).copy()
        live = np.arange(len(h))
        t_before = np.zeros(len(h), np.float64)
        for _ in range(255):
            live = live[h["t"][live] < np.float32(3.0e38)]
            if len(live) == 0:
                break
            alpha = self.texture_eval(scene, h["triangle_id"][live].astype(np.int32), h["point"][live]).cpu().numpy()[:, 3]
            live = live[alpha < np.float32(a0)]
            if len(live) == 0:
                break
            t_before[live] += h["t"][live].astype(np.float64)
            sub = np.zeros(len(live), L.RAY)
            sub["origin"][:, :3] = h["point"][live][:, :3]
            sub["direction"] = r["direction"][live]
            hs = records(self.intersect(scene, to_device(sub, self.device), mode=mode), L.HIT)
            h[live] = hs
        found = h["t"] < np.float32(3.0e38)
        h["t"][found] = (t_before[found] + h["t"][found].astype(np.float64)).astype(np.float32)
        return to_device(h, self.device)

    def autofocus(self, scene, camera, width, height, px, py, mode=L.MODE_EXACT):
        """The lens focus distance F that puts what pixel (px, py) sees in
        focus: focus_from_hit of the pixel's corner ray's first hit
        (first_hits).  A ray that hits nothing there is a ValueError."""
        px, py = int(px), int(py)
        if not (0 <= px < width and 0 <= py < height):
            raise ValueError("autofocus: pixel (%d, %d) is outside the %d x %d image" % (px, py, width, height))
        rays = self.generate_rays(camera, width, height)
        hit = records(self._first_uncut(scene, rays, mode), L.HIT)[py * width + px]
        ray = records(rays, L.RAY)[py * width + px]
        if not float(hit["t"]) < 3.0e38:
            raise ValueError("autofocus: the ray of pixel (%d, %d) hits nothing to focus on" % (px, py))
        cam = np.ascontiguousarray(camera).view(L.CAMERA).reshape(-1)[0]
        return focus_from_hit(hit["t"], ray["direction"], cam["direction"])

    def denoise(self, scene, hits, state, iterations=None, sigma_normal=None, sigma_plane=None, sigma_color=None,
                albedo=None):
        """mcpt_denoise: the count-aware, geometry-guided a-trous filter of
        state.hist, guided by `hits` (first_hits of the same view), into a new
        float32 (n, 4) device tensor.  Reads the state, writes none of it.
        None takes the default of DENOISE_DEFAULTS (iterations 0..8, 0 copies
        hist; sigma_plane a fraction of the scene diagonal; sigma_color 0
        switches the colour term off).
        `albedo`: a float32 (n, 3) or (n, 4) array or device tensor, the
        texture factor at each pixel's first hit (first_hit_albedo): the filter
        then runs on hist / a' and a' is multiplied back, a' = max(a, 2^-8)
        per channel, so that a texture is not smeared across the pixels of one
        material and plane.  Exact for the diffuse lobe, approximate for glossy
        (whose specular lobe carries no texture).  mcpt_denoise itself is the
        same either way; a pixel whose a is 1 keeps the bits it has without."""
        n = state.width * state.height
        if not hits.is_cuda or hits.numel() * hits.element_size() != n * L.HIT.itemsize:
            raise L.MCPTError("denoise: hits must be the state's width*height Hit records on the GPU")
        given = dict(iterations=iterations, sigma_normal=sigma_normal, sigma_plane=sigma_plane,
                     sigma_color=sigma_color)
        v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
        p = L.DenoiseParams(int(v["iterations"]), float(v["sigma_normal"]), float(v["sigma_plane"]),
                            float(v["sigma_color"]))
        out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        hist, a = state.hist, None
        if albedo is not None:
            a = torch.as_tensor(albedo, dtype=torch.float32).to(self.device).reshape(n, -1)
            if a.shape[1] not in (3, 4):
                raise ValueError("denoise: albedo must be (n, 3) or (n, 4)")
            a4 = torch.ones((n, 4), dtype=torch.float32, device=self.device)
            a4[:, :3] = torch.clamp(a[:, :3], min=2.0 ** -8)
            a = a4
            hist = (state.hist.reshape(n, 4) / a).contiguous()
        L.check(L.lib().mcpt_denoise(self.ctx, scene.handle, L.ptr(hits), L.ptr(hist), L.ptr(state.count),
                                     state.width, state.height, ctypes.byref(p), L.ptr(out), _stream()))
        if a is not None:
            out = out * a
        return out


# Renderer.denoise's defaults: quality choices, not correctness.  The set with the least RMSE over
# the filtered pixels of C1 and of C2 at 512 x 512 after 20 frames, against 4096 frames from other seeds
# (tools/denoise_sweep.py, profiles/denoise_sigma_sweep.jsonl).
DENOISE_DEFAULTS = {"iterations": 3, "sigma_normal": 0.5, "sigma_plane": 0.005, "sigma_color": 0.0}


def records(buf, dtype):
    """View a device byte buffer as host numpy records."""
    return buf.cpu().numpy().view(dtype)


def to_device(arr, device):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(device)


def build_hlbvh_device(tris, device=0):
    """HLBVH<CPU> built on the GPU (mcpt_build_hlbvh_device): the same 2n-1
    BVHNode records as scene.build_hlbvh.  `tris` is a host TRIANGLE array or a
    device byte tensor of them; returns a device byte tensor of the nodes."""
    if isinstance(tris, np.ndarray):
        n = len(tris)
        tris = to_device(tris, device)
    else:
        n = tris.numel() // L.TRIANGLE.itemsize
    if n == 0:
        raise ValueError("empty scene")
    nodes = torch.empty((2 * n - 1) * L.BVHNODE.itemsize, dtype=torch.uint8, device=tris.device)
    L.check(L.lib().mcpt_build_hlbvh_device(L.ptr(tris), n, L.ptr(nodes), _stream()))
    return nodes


def build_hlbvh_host_nodes(tris, device=0):
    """HLBVH<CPU> nodes built on the GPU and returned as a host BVHNODE array
    (bit-identical to scene.build_hlbvh; a `build` for SceneData.from_arrays)."""
    return records(build_hlbvh_device(tris, device), L.BVHNODE).copy()


def treelet_device(nodes, device=0):
    """TreeletBVH<CPU> (MCPT/BVH/treeletBVH.cpp:343-372, "bvhtype": "treelet")
    run on the GPU by mcpt_treelet_device.  `nodes` is a host BVHNODE array
    (returns a restructured host copy) or a device byte tensor (restructured
    in place and returned)."""
    host = isinstance(nodes, np.ndarray)
    d = to_device(nodes, device) if host else nodes
    n = d.numel() // L.BVHNODE.itemsize
    L.check(L.lib().mcpt_treelet_device(L.ptr(d), n, _stream()))
    return records(d, L.BVHNODE).copy() if host else d


def treelet_gpu_device(nodes, device=0):
    """TreeletBVH<GPU> (MCPT/BVH/treeletBVH.cpp:413-438, kernels/treeletBVH.cl),
    the tree every reference render traverses (scenebuild.cpp:87-95), run by
    mcpt_treelet_gpu_device.  `nodes` is a host BVHNODE array in the HLBVH
    layout (returns a restructured host copy) or a device byte tensor
    (restructured in place and returned)."""
    host = isinstance(nodes, np.ndarray)
    d = to_device(nodes, device) if host else nodes
    n = d.numel() // L.BVHNODE.itemsize
    L.check(L.lib().mcpt_treelet_gpu_device(L.ptr(d), n, _stream()))
    return records(d, L.BVHNODE).copy() if host else d
