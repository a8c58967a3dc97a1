// tile_subset_check: a tile-subset launch of k_render (mcpt_render_frames_tiles) walked
// on the CPU with the two headers alone (csrc/mcpt_queue.h, csrc/mcpt_plan.h): the list
// of active tiles as tile_order, its length as the geometry's tile count, exactly as the
// kernel overrides it.  Every image up to 3 x 3 tiles (with and without edge holes),
// every non-empty subset in ascending and descending list order, 1 / 2 / 8 queues,
// spread 0 / 1, 1-3 blocks.  A wrong count here is a hang on the GPU, not a wrong pixel.
// No input: prints "ok ..." and exits 0, or the first failing case and exits 1.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mcpt_plan.h"
#include "mcpt_queue.h"

using namespace mcpt;

[[noreturn]] static void fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
  std::exit(1);
}

// ------------------------------------------------------------ the queues of a subset
static long check_subsets() {
  static const int nqs[] = {1, 2, 8};
  long cases = 0;
  std::vector<int32_t> list, seen, where;
  std::vector<char> active;
  for (int tx = 1; tx <= 3; ++tx)
    for (int ty = 1; ty <= 3; ++ty)
      for (int hx = 0; hx < 2; ++hx)
        for (int hy = 0; hy < 2; ++hy) {
          const int W = 8 * tx - (hx ? 3 : 0), H = 8 * ty - (hy ? 7 : 0), n_all = tx * ty;
          for (uint32_t set = 1; set < (1u << n_all); ++set)
            for (int desc = 0; desc < 2; ++desc) {
              list.clear();
              for (int t = 0; t < n_all; ++t)
                if (set >> (desc ? n_all - 1 - t : t) & 1u) list.push_back(desc ? n_all - 1 - t : t);
              const uint32_t k = (uint32_t)list.size();
              active.assign((size_t)W * H, 0);
              long n_active_px = 0;
              for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                  if (set >> ((y / 8) * tx + x / 8) & 1u) active[(size_t)y * W + x] = 1, ++n_active_px;
              for (int nq : nqs)
                for (int spread = 0; spread < 2; ++spread)
                  for (int nb = 1; nb <= 3; ++nb) {
                    ++cases;
                    QueueGeometry G = queue_geometry(W, H, H, tx, 1, 0, 1, (uint32_t)nq, spread);
                    if (G.n_tiles != (uint32_t)n_all) fail("W %d H %d: %u tiles, expected %d", W, H, G.n_tiles, n_all);
                    G.n_tiles = k;  // k_render: if (A.active_tiles) geo.n_tiles = A.active_tiles
                    seen.assign((size_t)W * H * nb, 0);
                    where.assign((size_t)W * H * 2, -1);  // the pixel's queue and the entry of its latest block
                    long items_sum = 0, pixels = 0;
                    for (uint32_t qx = 0; qx < (uint32_t)nq; ++qx) {
                      const uint32_t items = queue_items(qx, k, (uint32_t)nq);
                      items_sum += items;
                      for (uint32_t q = 0; q < items * (uint32_t)nb; ++q) {
                        const QueueSlot s = entry_slot(q, qx, G);
#define WHERE "W %d H %d set 0x%x order %d nq %d spread %d blocks %d: queue %u entry %u", W, H, set, desc, nq, spread, nb, qx, q
                        if (s.tpos >= k || s.k >= 64u) fail("list position %u of %u, pixel %u: " WHERE, s.tpos, k, s.k);
                        const QueueEntry e = entry_pixel(q, qx, G, list.data());
                        if (e.block != q / items || e.block >= (uint32_t)nb) fail("block %u: " WHERE, e.block);
                        if (e.x < 0 || e.y < 0 || e.y > H) fail("range (%d, %d): " WHERE, e.x, e.y);
                        if (e.x >= W || e.y == H) continue;  // an edge-tile hole
                        const size_t p = (size_t)e.y * W + e.x;
                        if (!active[p]) fail("a pixel of an inactive tile (%d, %d): " WHERE, e.x, e.y);
                        if (seen[p * nb + e.block]++) fail("(%d, %d) block %u twice: " WHERE, e.x, e.y, e.block);
                        ++pixels;
                        if (e.block == 0) {
                          where[p * 2] = (int32_t)qx;
                        } else {
                          // the wait of block b is for block b - 1: the same queue, a lower entry
                          if (!seen[p * nb + e.block - 1]) fail("(%d, %d) block %u before block %u: " WHERE, e.x, e.y, e.block, e.block - 1);
                          if (where[p * 2] != (int32_t)qx || where[p * 2 + 1] >= (int32_t)q)
                            fail("(%d, %d) block %u not behind its block %u in one queue: " WHERE, e.x, e.y, e.block, e.block - 1);
                        }
                        where[p * 2 + 1] = (int32_t)q;
#undef WHERE
                      }
                    }
                    if (items_sum != 64l * k)
                      fail("W %d H %d set 0x%x nq %d: the queues hold %ld items, expected %ld", W, H, set, nq, items_sum, 64l * k);
                    if (pixels != n_active_px * nb)
                      fail("W %d H %d set 0x%x order %d nq %d spread %d blocks %d: %ld (pixel, block) entries, expected %ld", W, H,
                           set, desc, nq, spread, nb, pixels, n_active_px * nb);
                  }
            }
        }
  return cases;
}

// ------------------------------------------------------------ the plan of a subset
static bool same_plan(const PlanOut &a, const PlanOut &b) {
  return a.local_rows == b.local_rows && a.tiles_x == b.tiles_x && a.tiles == b.tiles && a.grid_wg == b.grid_wg &&
         a.fpl == b.fpl && a.fpl_head == b.fpl_head && a.nb_head == b.nb_head && a.fpl_tail == b.fpl_tail &&
         a.max_blocks == b.max_blocks && a.n_blocks_all == b.n_blocks_all && a.n_launch == b.n_launch &&
         a.no_handoff == b.no_handoff && a.spread == b.spread;
}

static long check_plans() {
  static const int Ws[] = {1, 8, 21, 24, 37, 64, 1024}, Hs[] = {1, 17, 24, 48, 1024}, fpls[] = {0, 1, 2, 3, 7};
  static const int wgs[] = {1, 8, 256, 2048}, waves[] = {1, 4, 8}, frames_[] = {1, 2, 3, 8, 20, 64, 300, 5000};
  static const int ents[] = {0, 4}, lasts[] = {-1, 0, 3}, spreads[] = {0, 1, 2};
  long cases = 0;
  for (int W : Ws)
    for (int H : Hs)
      for (int wg : wgs)
        for (int wv : waves)
          for (int be : ents)
            for (int last : lasts)
              for (int ps : spreads)
                for (int frames : frames_)
                  for (int fpl : fpls) {
                    // without the field, as every caller from before it builds a PlanIn
                    const PlanIn old{W, H, frames, fpl, 1, 0, 1, be, 0, last, ps, wg, wv};
                    const PlanOut P0 = plan_launches(old);
                    PlanIn in = old;
                    in.active_tiles = 0;
                    if (!same_plan(plan_launches(in), P0)) fail("W %d H %d frames %d: active_tiles 0 changes the plan", W, H, frames);
                    in.active_tiles = P0.tiles;  // every tile: the whole-image plan
                    if (!same_plan(plan_launches(in), P0)) fail("W %d H %d frames %d: every tile active changes the plan", W, H, frames);
                    const int64_t n = P0.tiles;
                    const int64_t ks[] = {1, 2, 3, n / 10, n / 2, n - 1};
                    for (int64_t k : ks) {
                      if (k < 1 || k >= n) continue;
                      ++cases;
                      in.active_tiles = k;
                      const PlanOut P = plan_launches(in);
                      if (P.tiles != P0.tiles || P.tiles_x != P0.tiles_x || P.local_rows != P0.local_rows)
                        fail("W %d H %d active %lld: the whole-view fields changed", W, H, (long long)k);
                      if (P.grid_wg < 1 || P.grid_wg > (k + wv - 1) / wv || P.grid_wg > wg)
                        fail("W %d H %d active %lld waves %d resident %d: grid of %lld workgroups", W, H, (long long)k, wv, wg,
                             (long long)P.grid_wg);
                      // the launches as launch_blocks walks them: every block at least one frame
                      int launches = 0;
                      int64_t f0 = 0;
                      while (f0 < frames) {
                        const LaunchFrames L = launch_frames(P, frames, f0);
                        if (L.frames < 1 || L.blocks < 1 || L.blocks > kMaxBlocksPerLaunch)
                          fail("W %d H %d active %lld frames %d: launch %d of %d frames in %d blocks", W, H, (long long)k, frames,
                               launches, L.frames, L.blocks);
                        if ((int64_t)L.blocks * k * 64 > (int64_t)INT32_MAX) fail("queue entries past 2^31");
                        int32_t next = 0;
                        for (int32_t b = 0; b < L.blocks; ++b) {
                          const BlockFrames B = block_frames(b, P.fpl_head, P.nb_head, P.fpl_tail, L.frames);
                          if (B.count < 1 || B.first != next)
                            fail("W %d H %d active %lld frames %d fpl %d: launch %d block %d: %d frames from %d (expected from %d)",
                                 W, H, (long long)k, frames, fpl, launches, b, B.count, B.first, next);
                          next = B.first + B.count;
                        }
                        if (next != L.frames) fail("launch %d: blocks end at %d of %d frames", launches, next, L.frames);
                        f0 += L.frames;
                        ++launches;
                      }
                      if (launches != P.n_launch) fail("%d launches, the plan says %d", launches, P.n_launch);
                    }
                  }
  return cases;
}

int main() {
  const long a = check_subsets();
  const long b = check_plans();
  std::printf("ok %ld subset walks, %ld subset plans\n", a, b);
  return 0;
}
