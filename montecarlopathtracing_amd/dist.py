"""Multi-GPU: image row stripes across one process per GPU.

Pixels are independent in the reference (per-pixel seed chain, history and
count; read-only scene), so rank r renders the 16-row stripes s with
s % world == r and no data moves during the frame loop.  At the end the
zero-elsewhere accumulators (mean, count, seed: 24 B per pixel) are packed
into one flat int32 buffer and summed onto rank 0 by ONE reduce (RCCL over
xGMI with the nccl backend; gloo on CPU in tests).  Each pixel has exactly
one non-zero contributor, so the integer sum of bit patterns is that
contributor's bits — exact for floats too, -0.0 included — giving the
single-GPU image for any GPU count.
"""
import numpy as np
import torch
import torch.distributed as dist


def owned_rows(height, stripe_rows, rank, world):
    """Rows of this rank, in the kernel's local-row order (k_render's global_row)."""
    rows = []
    lr = 0
    while True:
        s = lr // stripe_rows
        y = (s * world + rank) * stripe_rows + lr % stripe_rows
        if y >= height:
            break
        rows.append(y)
        lr += 1
    return np.asarray(rows, np.int64)


def owned_pixels(width, height, stripe_rows, rank, world):
    rows = owned_rows(height, stripe_rows, rank, world)
    return (rows[:, None] * width + np.arange(width)[None, :]).reshape(-1)


def ownership_mask(width, height, stripe_rows, rank, world):
    m = np.zeros(width * height, bool)
    m[owned_pixels(width, height, stripe_rows, rank, world)] = True
    return m


def reduce_image(hist, count, seeds, mask, group=None, dst=0):
    """Sum every rank's owned pixels onto rank `dst` with one collective.

    hist (N,4) float32, count (N,) int32, seeds (N,) int32 view of u32 — any
    device the process group's backend supports.  Non-owned pixels are zeroed,
    the three arrays packed as int32 bit patterns into one (N, 6) buffer and
    reduced with an integer SUM (one contributor per pixel: exact bits).
    Returns (hist float32 (N,4), count int32, seeds int64 holding the u32)."""
    if hist.is_cuda and dist.get_backend(group) == "gloo":  # gloo reduces host tensors
        hist, count, seeds = hist.cpu(), count.cpu(), seeds.cpu()
    m = torch.as_tensor(mask, device=hist.device)
    flat = torch.empty((hist.shape[0], 6), dtype=torch.int32, device=hist.device)
    flat[:, :4] = hist.contiguous().view(torch.int32)
    flat[:, 4] = count
    flat[:, 5] = seeds.view(torch.int32) if seeds.dtype == torch.int32 else seeds.to(torch.int32)
    flat.masked_fill_(~m[:, None], 0)
    dist.reduce(flat, dst=dst, op=dist.ReduceOp.SUM, group=group)
    h = flat[:, :4].contiguous().view(torch.float32)
    return h, flat[:, 4].contiguous(), flat[:, 5].to(torch.int64) & 0xFFFFFFFF


def refuse_adaptive(adaptive):
    """Adaptive sampling (Renderer.render_adaptive) is single-GPU: its tile subsets are not defined on a
    row-striped share.  ValueError for anything but None / False."""
    if adaptive is not None and adaptive is not False:
        raise ValueError("adaptive sampling is not available on the distributed path: a tile subset of a "
                         "row-striped share is not defined; render on one GPU, or drop \"adaptive\" / --adaptive")


def render_distributed(renderer, scene, camera, width, height, max_depth, max_attempt, frames, seeds,
                       stripe_rows=16, group=None, mode=0, jitter=False, vertex_normals=None, textures=None,
                       lens=None, bump=None, cutouts=None, unbiased=False, roulette=0, adaptive=None):
    """Render the whole image across the process group; rank 0 gets the image.
    `jitter`: Renderer.render_frames' sub-pixel jitter (per-pixel draws, so
    still the single-GPU image for any GPU count).  `vertex_normals`: smooth
    shading's (n_tris, 3, 3) normals, set on this rank's scene before it
    renders (Renderer.set_vertex_normals; None: the scene as it is), so every
    rank shades its stripes with the same ones.  `textures`: a (uv, tri_tex,
    images) triple (scene.load_textures'), set on this rank's scene likewise
    (Renderer.set_textures).  `lens`: Renderer.render_frames' thin lens (R, F)
    on every rank (per-pixel draws like the jitter's, which it switches on: no
    bit depends on the striping).  `bump`: a (uv, tri_map, images) triple
    (scene.load_bump_maps'), set on this rank's scene like the textures
    (Renderer.set_normal_maps).  `cutouts`: (alphas, threshold), set on this
    rank's scene after the textures (Renderer.set_texture_alpha).  `unbiased`,
    `roulette`: Renderer.render_frames' estimator on every rank (each pixel
    belongs to one rank and draws from its own chain, so striping changes no bit).
    `adaptive`: refused (ValueError) unless None or False: adaptive sampling renders
    subsets of whole-image tiles, which a striped share does not have.
    Returns (hist, count, seeds) as numpy on rank 0, None elsewhere."""
    refuse_adaptive(adaptive)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    if vertex_normals is not None:
        renderer.set_vertex_normals(scene, vertex_normals)
    if textures is not None:
        renderer.set_textures(scene, *textures)
    if cutouts is not None:
        renderer.set_texture_alpha(scene, *cutouts)
    if bump is not None:
        renderer.set_normal_maps(scene, *bump)
    st = renderer.new_state(width, height, seeds)
    kw = dict(stripe_rows=stripe_rows, stripe_index=rank, stripe_count=world, mode=mode,
              jitter=True if lens is not None else jitter, lens=lens, unbiased=unbiased, roulette=roulette)
    if frames >= 4096:  # long runs: each rank times the leaf schedules and S/fetch thresholds on one-block
        # 16-frame calls (same bits; neither block sizing nor tile order is tuned: long calls run
        # max_block_frames blocks, a regime one-block trials do not enter, App.update)
        renderer.tune(scene, camera, st, max_depth, max_attempt, frames=16, block_entries=None, last_block=False,
                      tile_orders=None, frames_per_launch=16, **kw)
    renderer.render_frames(scene, camera, st, max_depth, max_attempt, frames, **kw)
    torch.cuda.synchronize()
    mask = ownership_mask(width, height, stripe_rows, rank, world)
    h, c, s = reduce_image(st.hist, st.count, st.seeds, mask, group=group)
    if rank != 0:
        return None
    return h.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy().astype(np.uint32)
