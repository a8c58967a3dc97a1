// mcpt_plan.h — the launch plan of mcpt_render_frames: a call's frames cut into blocks
// and launches on a persistent grid.  Integer and double arithmetic, no HIP header: it
// is checked on the CPU (tests/native/plan_check.cpp, tests/golden/plan_cases.txt).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace mcpt {

constexpr int kDefaultBlockEntries = 8;  // mcpt_tuning.block_entries = 0
constexpr int kHandoffWords = 4;   // seed, mean.xyzw, count in four tagged 8-B granules (two 16-B stores)
constexpr int kMaxBlocksPerLaunch = 255;  // the hand-off tag's 8 bits of block index
constexpr uint32_t kHandoffMaxBytes = 0x7FFFFFFFu;  // images beyond it run without hand-offs

struct PlanIn {
  int32_t width, height, frames, frames_per_launch;  // frames_per_launch: frames per block; <= 0: auto
  int32_t stripe_rows, stripe_index, stripe_count;
  int32_t block_entries, max_block_frames, last_block_frames, pixel_spread;  // mcpt_tuning
  int64_t resident_wg;  // workgroups resident at once: max(per_cu, 1) * n_cu
  int32_t wg_waves;     // waves per workgroup
  // a tile-subset call (mcpt_render_frames_tiles): the tiles it renders, 0: all.  It takes the
  // tile count's place in the grid, the queue items, pixels per lane, block sizing and spread;
  // local_rows, tiles_x and tiles stay the whole view's (the primary-hit pass is whole-view)
  int64_t active_tiles = 0;
};

struct PlanOut {
  int32_t local_rows, tiles_x;  // rows owned by this stripe residue; 8-pixel columns
  int64_t tiles, grid_wg;       // 8x8 tiles (one per wave at a time); workgroups per launch
  int fpl, fpl_head;            // frames per block: the launch loop's stride; of the first nb_head blocks
  int32_t nb_head, fpl_tail;    // blocks from nb_head on have fpl_tail frames (INT32_MAX: every block fpl)
  int64_t max_blocks, n_blocks_all;  // blocks per launch at most; blocks of the call
  int n_launch;
  bool no_handoff;  // image past the hand-off area's range: one block per launch
  int32_t spread;   // RenderArgs::spread
};

inline PlanOut plan_launches(const PlanIn &in) {
  PlanOut o;
  int32_t full = in.height / (in.stripe_rows * in.stripe_count);
  int32_t rem = in.height - full * in.stripe_rows * in.stripe_count;
  int32_t extra = std::min(std::max(rem - in.stripe_index * in.stripe_rows, 0), in.stripe_rows);
  o.local_rows = full * in.stripe_rows + extra;
  o.tiles_x = (in.width + 7) / 8;
  o.tiles = (int64_t)o.tiles_x * ((o.local_rows + 7) / 8);
  const int64_t run_tiles = in.active_tiles > 0 ? in.active_tiles : o.tiles;  // the tiles the launches render
  // grid_wg workgroups of wg_waves waves: `grid` waves (a tile per wave at most)
  o.grid_wg = std::max<int64_t>(1, std::min<int64_t>((run_tiles + in.wg_waves - 1) / in.wg_waves, in.resident_wg));
  const int64_t grid = o.grid_wg * in.wg_waves;
  // frames_per_launch = frames per BLOCK: a lane runs one pixel for one block
  // of frames, then hands the pixel's state to whichever lane takes its next
  // block.  One launch runs many blocks of every pixel, block-major, so lanes
  // stay busy until the last block (no per-block drain of the GPU).
  // frames_per_launch <= 0: auto.  Blocks let the launch's tail shrink: the
  // fewest blocks (at least 2) that give every resident lane `block_entries`
  // queue entries (so the tail, where lanes run dry, is about
  // 1/block_entries of the launch), frames split evenly over them, at most
  // max_block_frames each.  Each block boundary costs a hand-off per pixel;
  // with the packed hand-off, 8 entries and 2-3 blocks per call measured best
  // (20-frame calls: C2 -2 %, C3 -11 %, C4 -1 %, C5 even against 32 entries;
  // one block loses 2-7 % to the tail; profiles/r03_blocks.txt).
  // That needs several entries per lane in each block (>= 4): a pixel's next
  // block is then claimed long after its previous one started.  With fewer
  // (small images, strong-scaled ranks: about one pixel per lane) every block
  // boundary becomes a wait for the slowest pixel of the previous block, so
  // blocks there keep at least 4 frames (measured on C2 and C4 shares of 2,
  // 4 and 8 ranks, tools/sweep.py --stripes).
  const uint32_t n_items = (uint32_t)run_tiles * 64u;
  const int cap = in.max_block_frames > 0 ? in.max_block_frames : 32;  // frames per block at most (auto plans)
  int fpl = in.frames_per_launch;
  bool tail_ok = false;  // auto plan with several entries per lane: a short last block may apply
  double slots_per_px = 0;  // pixels per resident lane (auto plans)
  const double px_per_lane = (double)n_items / ((double)in.resident_wg * 64 * in.wg_waves);  // vs resident lanes
  if (fpl <= 0) {
    const int frames = std::max(in.frames, 1);
    const double per_block = (double)n_items / (double)(grid * 64);  // entries per lane per block
    const int want = in.block_entries > 0 ? in.block_entries : kDefaultBlockEntries;
    int nb = std::max(2, (int)std::ceil(want / std::max(per_block, 1e-9)));
    nb = std::max(1, std::min(nb, frames));
    fpl = (frames + nb - 1) / nb;
    if (per_block < 4.0) fpl = std::max(fpl, 4);
    // at most a few pixels per lane (strong-scaled ranks): little left to
    // balance but the pixels' own chains, so one block per pixel below 0.75
    // pixels per lane and two up to 2.5 (C2 shares of 4 and 8 ranks, C4 of 8:
    // 1-12 % faster than 4-frame blocks; the C5 8-rank share, 2 pixels per
    // lane: 4 % faster than 5-frame blocks; tools/sweep.py --stripes --fpl)
    const double per_slot = px_per_lane;
    slots_per_px = per_slot;
    if (per_slot < 0.75)
      fpl = frames;
    else if (per_slot <= 2.5)
      fpl = std::max(fpl, (frames + 1) / 2);
    else
      tail_ok = true;
    fpl = std::max(1, std::min({fpl, cap, frames}));
  }
  // the hand-off area is addressed with 32-bit byte offsets below 2^31
  // (handoff_rsrc): a larger image runs ONE block per launch, at most `cap`
  // frames (no hand-off; launches chain through the state arrays, so every
  // launch stays bounded: ~67 M+ pixels x 32 frames)
  o.no_handoff = (int64_t)in.width * in.height * kHandoffWords * 8 > (int64_t)kHandoffMaxBytes;
  if (o.no_handoff)
    fpl = std::max(1, std::min(in.frames_per_launch > 0 ? in.frames_per_launch : std::max(in.frames, 1), cap));
  // blocks per launch: the hand-off tag holds 8 bits of block index, and
  // one launch covers at most ~4096 frames
  o.max_blocks = o.no_handoff ? 1 : std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)INT32_MAX / std::max<uint32_t>(n_items, 1), 4096 / fpl + 1,
                            (int64_t)kMaxBlocksPerLaunch}));
  o.n_blocks_all = (in.frames + fpl - 1) / fpl;
  o.n_launch = (int)((o.n_blocks_all + o.max_blocks - 1) / o.max_blocks);
  // a short last block (last_block_frames, auto plans of one launch with
  // several entries per lane): the first nb-1 blocks share frames - L evenly
  // and the last takes the remainder (<= L).  Entries are block-major, so the
  // last block's entries are the launch's tail; shorter ones leave lanes idle
  // for less time at its end.  Same blocks, same hand-offs, same bits.
  // Auto: ceil(frames / 8) from 6 pixels per lane; from 2.5, on a whole image (one
  // stripe set), ceil(frames / 4): C2 and C3 at 4 pixels per lane, 20 frames: 9.00 /
  // 2.98 ms against equal blocks' 9.34 / 3.08 (and (17, 3) 9.24 / 3.02); a strong-scaled
  // share keeps equal blocks (the C5 4-rank share: 43.1 ms with (15, 5), 40.4 equal;
  // profiles/r04_last_block_auto.jsonl; from 6: 20-frame C3 -2 %, 16-frame C4 -2 %,
  // 8-frame C5 -3 %); Renderer.tune tries equal blocks and both.
  o.fpl = fpl;
  o.fpl_head = fpl;
  o.nb_head = INT32_MAX;  // every block fpl frames
  o.fpl_tail = fpl;
  const bool tail_auto = in.last_block_frames == 0 && (slots_per_px >= 6.0 || in.stripe_count == 1);
  if (tail_ok && o.n_launch == 1 && o.n_blocks_all >= 2 && (in.last_block_frames > 0 || tail_auto)) {
    const int nb = (int)o.n_blocks_all;
    const int L = in.last_block_frames > 0 ? in.last_block_frames
                                           : (slots_per_px >= 6.0 ? (in.frames + 7) / 8 : (in.frames + 3) / 4);
    if (L < fpl) {
      const int head = (in.frames - L + nb - 2) / (nb - 1);
      const int last = in.frames - (nb - 1) * head;
      if (last >= 1 && last <= L && head <= cap) {  // the head blocks keep the block cap
        o.fpl_head = head;
        o.nb_head = nb - 1;
        o.fpl_tail = last;
      }
    }
  }
  // pixel_spread auto: spread slots up to 2.5 pixels per resident lane, where
  // each pixel's own chain sets the time (an N-rank share).  Tile-major slots
  // put one tile's dear pixels (C2: the pitcher's inside, ~29 loop iterations
  // per segment) in one wave, whose iterations then run the union of their
  // phases; spread, they share waves with cheap pixels that finish early.
  // Slowest share of 8 ranks: C2 5.83 -> 4.20 ms, C4 (64 frames) 58.1 -> 50.9;
  // 4 ranks: C2 6.51 -> 5.22, C4 76.7 -> 73.0; whole images even (C2, C3, C4,
  // C5 within 0.7 %; profiles/r04_spread.jsonl).
  o.spread = in.pixel_spread == 2 || (in.pixel_spread == 0 && px_per_lane <= 2.5) ? 1 : 0;
  return o;
}

}  // namespace mcpt
