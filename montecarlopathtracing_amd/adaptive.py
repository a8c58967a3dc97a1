"""Adaptive sampling's selection policy (Renderer.render_adaptive): which 8x8
tiles go on, and how many frames a round takes.  Pure numpy, no GPU: the driver
calls these and tests/adaptive_ref.py restates them.

Noise is estimated from two half histories A and B (Dammertz et al. 2010, "A
hierarchical automatic stopping condition for Monte Carlo global illumination"):
mcpt_tile_error gives each tile the mean over its pixels of
0.5 * |A - B|_1 / sqrt(floor + m.r + m.g + m.b), m the merged mean.
"""
import numpy as np


def tile_grid(width, height):
    """(tiles_x, tiles_y) of an image: 8x8 tiles, the last column and row cut by the image."""
    return (int(width) + 7) // 8, (int(height) + 7) // 8


def select_tiles(err, threshold, tiles_x, tiles_y, dilate=True):
    """The active mask of a round: uint8 (tiles_y * tiles_x,), 1 where the tile's
    error is above `threshold`.  "Above" is "not <= threshold", so +inf (a tile
    with a pixel one half has never sampled) and NaN are above every threshold.
    `dilate`: the set grows by its 8-neighbourhood inside the image, so a tile
    that goes on takes its neighbours along (no seam between neighbouring tiles
    with different sample counts)."""
    e = np.asarray(err, np.float32).reshape(tiles_y, tiles_x)
    with np.errstate(invalid="ignore"):
        on = ~(e <= np.float32(threshold))
    if dilate:
        p = np.zeros((tiles_y + 2, tiles_x + 2), bool)
        p[1:-1, 1:-1] = on
        grown = np.zeros_like(on)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= p[dy:dy + tiles_y, dx:dx + tiles_x]
        on = grown
    return on.astype(np.uint8).reshape(-1)


def round_frames(issued, frames, batch):
    """Frames of the next round after `issued` of a budget of `frames`: a batch,
    cut to what is left (0: the budget is spent).  All three are even, so each
    half takes half of it."""
    return max(0, min(int(batch), int(frames) - int(issued)))


def check_arguments(frames, threshold, min_frames, batch, floor):
    """render_adaptive's argument rules; ValueError before any C call."""
    for name, v in (("frames", frames), ("min_frames", min_frames), ("batch", batch)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 2 or v % 2:
            raise ValueError("render_adaptive: %s must be an even integer >= 2, got %r" % (name, v))
    if min_frames > frames:
        raise ValueError("render_adaptive: min_frames (%d) must not exceed frames (%d)" % (min_frames, frames))
    t = float(threshold)
    if np.isnan(t) or t < 0:
        raise ValueError("render_adaptive: threshold must be >= 0 (inf: stop after min_frames), got %r" % (threshold,))
    f = float(floor)
    if not (np.isfinite(f) and f > 0):
        raise ValueError("render_adaptive: floor must be finite and > 0, got %r" % (floor,))


class AdaptiveReport:
    """What render_adaptive did: per later round the tile error map it read
    (`errors`, float32 (tiles_y, tiles_x)) and the mask it chose (`masks`, uint8,
    same shape; the last one may be empty: the stop), the frames each round
    issued (`round_frames`, round 0 first), the per-pixel budget `frames`,
    `frames_issued`, the total `samples` and `fraction` = samples / (W * H * frames)."""

    def __init__(self, width, height, frames):
        self.width, self.height, self.frames = width, height, frames
        self.tiles_x, self.tiles_y = tile_grid(width, height)
        self.errors, self.masks, self.round_frames = [], [], []
        self.frames_issued = 0
        self.samples = 0
        self.fraction = 0.0
