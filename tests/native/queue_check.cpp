// queue_check: k_render's queue and hand-off arithmetic (csrc/mcpt_queue.h) walked
// exhaustively at small shapes, with the launch plan (csrc/mcpt_plan.h) as the host
// makes it.  No input: prints "ok ..." and exits 0, or the first failing case and
// exits 1.  Every comparison is an equality or an order between integers.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcpt_plan.h"
#include "mcpt_queue.h"

using namespace mcpt;

static const PlanIn *g_plan = nullptr;  // the plan under check: named by fail()
[[noreturn]] static void fail(const char *fmt, ...) {
  if (g_plan)
    std::printf("W %d H %d frames %d frames_per_launch %d stripes %d block_entries %d max_block_frames %d "
                "last_block_frames %d resident_wg %lld: ", g_plan->width, g_plan->height, g_plan->frames,
                g_plan->frames_per_launch, g_plan->stripe_count, g_plan->block_entries, g_plan->max_block_frames,
                g_plan->last_block_frames, (long long)g_plan->resident_wg);
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
  std::exit(1);
}

// ------------------------------------------------------------ slot mapping
// Every entry of every queue of one launch geometry: each pixel of this rank's rows
// once per block and nothing else; a pixel's blocks in one queue at one slot, in
// entry order (what the kernel's no-deadlock argument rests on).
static long check_slots() {
  static const int Ws[] = {1, 7, 8, 9, 64, 65, 130, 523}, Hs[] = {1, 8, 9, 33, 70, 517};
  static const int rows[] = {1, 4, 16}, nqs[] = {1, 3, 8}, blocks[] = {1, 3};
  long cases = 0;
  std::vector<int32_t> order, seen, where;
  for (int W : Ws)
    for (int H : Hs)
      for (int sc = 1; sc <= 3; ++sc)
        for (int si = 0; si < sc; ++si)
          for (int sr : rows) {
            PlanIn in{};
            in.width = W, in.height = H, in.frames = 1, in.frames_per_launch = 1;
            in.stripe_rows = sr, in.stripe_index = si, in.stripe_count = sc;
            in.resident_wg = 256, in.wg_waves = 4;
            const PlanOut P = plan_launches(in);
            const uint32_t n_tiles = (uint32_t)P.tiles;
            // the image rows this rank owns
            std::vector<char> mine(H, 0);
            long n_mine = 0;
            for (int y = 0; y < H; ++y)
              if ((y / sr) % sc == si) mine[y] = 1, ++n_mine;
            if (n_mine != P.local_rows) fail("rows: W %d H %d stripes %d/%d x %d: %ld != %d", W, H, si, sc, sr, n_mine, P.local_rows);
            if (n_tiles == 0) continue;  // a rank without rows: the host launches nothing
            order.resize(n_tiles);
            for (uint32_t t = 0; t < n_tiles; ++t) order[t] = (int32_t)(n_tiles - 1u - t);
            for (int nq : nqs)
              for (int spread = 0; spread < 2; ++spread)
                for (int rev = 0; rev < 2; ++rev)
                  for (int nb : blocks) {
                    ++cases;
                    const QueueGeometry G = queue_geometry(W, H, P.local_rows, P.tiles_x, sr, si, sc, (uint32_t)nq, spread);
                    const int32_t *to = rev ? order.data() : nullptr;
                    if (G.n_tiles != n_tiles) fail("n_tiles %u != plan's %u", G.n_tiles, n_tiles);
                    seen.assign((size_t)W * H * nb, 0);
                    where.assign((size_t)W * H * 2, -1);  // the pixel's queue and slot
                    long entries = 0, pixels = 0, holes = 0;
                    for (uint32_t qx = 0; qx < (uint32_t)nq; ++qx) {
                      const uint32_t items = queue_items(qx, n_tiles, (uint32_t)nq);
                      for (uint32_t q = 0; q < items * (uint32_t)nb; ++q) {
                        ++entries;
                        const QueueSlot s = entry_slot(q, qx, G);  // where entry_pixel reads tile_order
                        if (s.tpos >= n_tiles || s.k >= 64u)
                          fail("W %d H %d nq %d spread %d: queue %u entry %u -> tile position %u of %u, pixel %u", W, H, nq,
                               spread, qx, q, s.tpos, n_tiles, s.k);
                        const QueueEntry e = entry_pixel(q, qx, G, to);
#define WHERE "W %d H %d stripes %d/%d x %d nq %d spread %d order %d blocks %d: queue %u entry %u -> block %u (%d, %d)", \
              W, H, si, sc, sr, nq, spread, rev, nb, qx, q, e.block, e.x, e.y
                        if (e.block != q / items) fail("block: " WHERE);
                        if (e.x < 0 || e.y < 0 || e.y > H) fail("range: " WHERE);
                        if (e.x >= W || e.y == H) {
                          ++holes;
                          continue;
                        }
                        if (!mine[e.y]) fail("another rank's row: " WHERE);
                        const size_t p = (size_t)e.y * W + e.x;
                        if (seen[p * nb + e.block]++) fail("produced twice: " WHERE);
                        ++pixels;
                        const int32_t slot = (int32_t)(q - e.block * items);
                        if (e.block == 0) {
                          where[p * 2] = (int32_t)qx, where[p * 2 + 1] = slot;
                        } else if (where[p * 2] != (int32_t)qx || where[p * 2 + 1] != slot) {
                          // entries ascend with the block at one slot: block b's entry
                          // b * items + slot lies below block b + 1's
                          fail("a later block in another queue or slot: " WHERE);
                        }
#undef WHERE
                      }
                    }
                    if (pixels != n_mine * W * nb)
                      fail("W %d H %d stripes %d/%d x %d nq %d spread %d order %d blocks %d: %ld pixels, expected %ld", W, H,
                           si, sc, sr, nq, spread, rev, nb, pixels, n_mine * W * nb);
                    if (holes != entries - pixels || entries != (long)n_tiles * 64 * nb)
                      fail("W %d H %d nq %d blocks %d: %ld entries, %ld pixels, %ld holes", W, H, nq, nb, entries, pixels, holes);
                  }
          }
  return cases;
}

// ------------------------------------------------------------ block ranges
// The launches of a plan walked as launch_blocks walks them, each launch's blocks as
// the S phase takes them: counts of at least 1 (a lane runs until its frame counter
// EQUALS the count), abutting, ending at the launch's frames; 1..255 blocks.
static long n_short = 0, n_multi = 0;
static void check_plan(const PlanIn &in) {
  const PlanOut P = plan_launches(in);
  g_plan = &in;
  int launches = 0;
  int64_t f0 = 0;
  while (f0 < in.frames) {
    const LaunchFrames L = launch_frames(P, in.frames, f0);
    if (L.frames < 1 || L.blocks < 1 || L.blocks > kMaxBlocksPerLaunch)
      fail("launch %d: %d frames in %d blocks", launches, L.frames, L.blocks);
    int32_t next = 0;
    for (int32_t b = 0; b < L.blocks; ++b) {
      const BlockFrames B = block_frames(b, P.fpl_head, P.nb_head, P.fpl_tail, L.frames);
      if (B.count < 1) fail("launch %d block %d: %d frames", launches, b, B.count);
      if (B.first != next) fail("launch %d block %d begins at %d, the one before ends at %d", launches, b, B.first, next);
      next = B.first + B.count;
    }
    if (next != L.frames) fail("launch %d: blocks end at %d of %d frames", launches, next, L.frames);
    f0 += L.frames;
    ++launches;
  }
  if (f0 != in.frames) fail("launches cover %lld frames", (long long)f0);
  if (launches != P.n_launch) fail("%d launches, the plan says %d", launches, P.n_launch);
  g_plan = nullptr;
  n_short += P.nb_head != INT32_MAX;
  n_multi += launches > 1;
}

static long check_blocks() {
  static const int Ws[] = {8, 64, 256, 1024}, Hs[] = {8, 64, 512}, fpls[] = {0, 1, 3, 7, 64}, scs[] = {1, 4};
  static const int ents[] = {0, 4, 64}, caps[] = {0, 1, 2}, lasts[] = {-1, 0, 1, 3}, wgs[] = {8, 256, 2048};
  static const int many[] = {255, 256, 300, 511, 600, 4097, 5000}, fpls2[] = {0, 1, 2, 20};
  long cases = 0;
  for (int W : Ws)
    for (int H : Hs)
      for (int sc : scs)
        for (int be : ents)
          for (int cap : caps)
            for (int last : lasts)
              for (int wg : wgs) {
                PlanIn in{};
                in.width = W, in.height = H;
                in.stripe_rows = 1, in.stripe_index = 0, in.stripe_count = sc;
                in.block_entries = be, in.max_block_frames = cap, in.last_block_frames = last;
                in.resident_wg = wg, in.wg_waves = 4;
                for (int frames = 1; frames <= 70; ++frames)
                  for (int fpl : fpls) {
                    in.frames = frames, in.frames_per_launch = fpl;
                    check_plan(in);
                    ++cases;
                  }
                for (int frames : many)
                  for (int fpl : fpls2) {
                    in.frames = frames, in.frames_per_launch = fpl;
                    check_plan(in);
                    ++cases;
                  }
              }
  return cases;
}

// ------------------------------------------------------------ hand-off
static long check_handoff() {
  static const uint32_t vals[] = {0u, 1u, 0xFFFFu, 0x10000u, 0x7FC00001u, 0x80000000u, 0xFFFFFFFFu, 0xDEADBEEFu};
  static const uint32_t tags[] = {1u, 0x0100u, 0xFFFFu};
  long cases = 0;
  for (uint32_t tag : tags)
    for (uint32_t seed : vals)
      for (uint32_t mx : vals)
        for (uint32_t my : vals)
          for (uint32_t mz : vals)
            for (uint32_t mw : vals)
              for (uint32_t count : vals) {
                ++cases;
                const HandoffGranules g = handoff_pack(seed, mx, my, mz, mw, count, tag);
                const HandoffState s = handoff_unpack(g.g[0], g.g[1], g.g[2], g.g[3], tag);
                if (!s.ready || s.seed != seed || s.mean[0] != mx || s.mean[1] != my || s.mean[2] != mz || s.mean[3] != mw ||
                    s.count != count)
                  fail("hand-off round trip: tag %x seed %x mean %x %x %x %x count %x -> ready %d %x %x %x %x %x %x", tag, seed, mx,
                       my, mz, mw, count, (int)s.ready, s.seed, s.mean[0], s.mean[1], s.mean[2], s.mean[3], s.count);
                if (seed != mx || my != mz || mw != count) continue;  // the tag checks: a subset of the payloads
                for (int k = 0; k < kHandoffWords; ++k) {  // one granule still carries another tag
                  uint64_t h[kHandoffWords] = {g.g[0], g.g[1], g.g[2], g.g[3]};
                  h[k] ^= (uint64_t)1 << (48 + (k * 5) % 16);
                  if (handoff_unpack(h[0], h[1], h[2], h[3], tag).ready) fail("hand-off ready with granule %d's tag changed (tag %x)", k, tag);
                  h[k] = g.g[k] & 0x0000FFFFFFFFFFFFull;  // a granule of the cleared area's tag
                  if (handoff_unpack(h[0], h[1], h[2], h[3], tag).ready) fail("hand-off ready with granule %d untagged (tag %x)", k, tag);
                }
              }
  for (uint32_t tag : tags)
    if (handoff_unpack(0, 0, 0, 0, tag).ready) fail("hand-off ready on a cleared area (tag %x)", tag);
  // tags: non-zero, 16 bits, one per (launch, block)
  std::vector<char> used(1 << 16, 0);
  for (uint32_t hi = 0; hi < 3; ++hi)  // the launch counter's upper bits do not matter
    for (uint32_t s = 1; s <= 255; ++s)
      for (uint32_t b = 0; b <= 255; ++b) {
        const uint32_t t = handoff_tag(handoff_tag_base(hi * 0x100u + s), b);
        if (t == 0 || t >= (1u << 16)) fail("tag of launch %u block %u: %x", s, b, t);
        if (hi == 0 && used[t]++) fail("tag %x of launch %u block %u names another (launch, block) too", t, s, b);
        if (hi != 0 && t != handoff_tag(handoff_tag_base(s), b)) fail("tag of launch %u depends on bits above 8", hi * 0x100u + s);
        ++cases;
      }
  return cases;
}

// ------------------------------------------------------------ queue state
static long check_queue_state() {
  long cases = 0;
  for (uint32_t nq = 1; nq <= 8; ++nq)
    for (uint32_t xcc = 0; xcc < 8; ++xcc) {
      ++cases;
      uint32_t qs = qs_init(xcc, nq);
      if (qs_claim_queue(qs) != xcc % nq || qs_pool_queue(qs) != xcc % nq || qs_dry_count(qs) != 0 || qs_dry(qs))
        fail("queue state: nq %u xcc %u starts as %x", nq, xcc, qs);
      uint32_t visited = 1u << qs_claim_queue(qs);
      for (uint32_t k = 0; k < nq; ++k) {
        if (qs_dry_count(qs) != k) fail("queue state: nq %u xcc %u: dry count %u before steal %u", nq, xcc, qs_dry_count(qs), k);
        qs = qs_set_pool_queue(qs, qs_claim_queue(qs));  // a claim: the pool is of the claim queue
        if (qs_pool_queue(qs) != qs_claim_queue(qs) || qs_dry_count(qs) != k) fail("queue state: set_pool_queue -> %x", qs);
        qs = qs_set_dry(qs);
        if (!qs_dry(qs) || qs_dry_count(qs) != k) fail("queue state: set_dry -> %x", qs);
        const uint32_t pool = qs_pool_queue(qs);
        qs = qs_steal(qs, nq);
        if (qs_dry(qs) || qs_pool_queue(qs) != pool || qs_claim_queue(qs) >= nq)
          fail("queue state: nq %u xcc %u: steal %u -> %x", nq, xcc, k, qs);
        if (k + 1 < nq) {
          if (visited >> qs_claim_queue(qs) & 1u) fail("queue state: nq %u xcc %u: queue %u visited twice", nq, xcc, qs_claim_queue(qs));
          visited |= 1u << qs_claim_queue(qs);
        }
      }
      if (visited != (1u << nq) - 1u) fail("queue state: nq %u xcc %u: visited %x", nq, xcc, visited);
      if (qs_dry_count(qs) != nq) fail("queue state: nq %u xcc %u: dry count %u after %u steals", nq, xcc, qs_dry_count(qs), nq);
    }
  return cases;
}

int main() {
  const long slots = check_slots();
  const long blocks = check_blocks();
  const long handoffs = check_handoff();
  const long states = check_queue_state();
  std::printf("ok %ld slot cases, %ld plans (%ld with a short last block, %ld of several launches), %ld hand-off cases, "
              "%ld queue states\n", slots, blocks, n_short, n_multi, handoffs, states);
  return 0;
}
