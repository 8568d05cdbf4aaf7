// enc_plan.h — the device encoder's GOP plan and its chunk / ring arithmetic
// (transcode_driver.cpp) as plain host C++: no HIP include, so
// that the CPU harness (tests/native/enc_plan_host.cpp) calls what the driver
// calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vts {

// One frame of a level as the kernels read it (an int4: transcode.h's ent).
// Search entry: (frame, ref slot or -1 = small[frame - 1], dst slot, w);
// write entry: (frame, GOP position j, IDR parity, index within the level).
struct PlanEntry {
  int32_t x, y, z, w;
};

// The GOPs (IDR at frame 0, at cuts, every keyint frames) and their levels:
// level j holds position j of every GOP that long, as search entries and
// write entries; level j's entries are [lvl_off[j], lvl_off[j + 1]).
struct GopPlan {
  std::vector<int64_t> gop_start;
  int64_t ngop = 0, maxlen = 0;  // GOPs; frames of the longest = levels
  std::vector<PlanEntry> sent, went;
  std::vector<int64_t> lvl_off;
};

// scores[f] > thr starts a GOP at f when idr_at_cuts; intra: level 1 predicts
// from the IDR picture's reconstruction, else from its source; rate != 0 (a
// rate-aware search): a search entry's w is the GOP's entry index in the
// previous level, else 0
inline GopPlan plan_gops(int64_t n, const std::vector<float> &scores, int64_t keyint, bool idr_at_cuts, float thr,
                         bool intra, int rate) {
  GopPlan g;
  for (int64_t f = 0; f < n; ++f)
    if (f == 0 || (idr_at_cuts && scores[f] > thr) || f - g.gop_start.back() >= keyint) g.gop_start.push_back(f);
  g.ngop = static_cast<int64_t>(g.gop_start.size());
  std::vector<int64_t> gop_len(static_cast<size_t>(g.ngop));
  for (int64_t k = 0; k < g.ngop; ++k) {
    gop_len[k] = (k + 1 < g.ngop ? g.gop_start[k + 1] : n) - g.gop_start[k];
    g.maxlen = std::max(g.maxlen, gop_len[k]);
  }
  g.lvl_off.assign(static_cast<size_t>(g.maxlen) + 1, 0);
  // with a rate-aware search, w of a search entry: the GOP's entry index in the previous level (GOPs of
  // different lengths: the indices differ between levels), where enc_search finds the previous picture's words
  std::vector<int> lvl_idx(static_cast<size_t>(g.ngop), 0);
  for (int64_t j = 0; j < g.maxlen; ++j) {
    g.lvl_off[j] = static_cast<int64_t>(g.went.size());
    for (int64_t k = 0; k < g.ngop; ++k) {
      if (gop_len[k] <= j) continue;
      const int f = static_cast<int>(g.gop_start[k] + j);
      const int prev_idx = rate ? lvl_idx[k] : 0;
      lvl_idx[k] = static_cast<int>(static_cast<int64_t>(g.went.size()) - g.lvl_off[j]);
      // level 1 predicts from the IDR picture: its source (all I_PCM) or, with intra, its reconstruction
      g.sent.push_back({f, j == 1 && !intra ? -1 : static_cast<int>(2 * k + ((j - 1) & 1)),
                        static_cast<int>(2 * k + (j & 1)), prev_idx});
      g.went.push_back({f, static_cast<int>(j), static_cast<int>(k & 1), lvl_idx[k]});
    }
  }
  g.lvl_off[g.maxlen] = static_cast<int64_t>(g.went.size());
  return g;
}

// The residual levels live in a ring of kRing levels: level j uses slot
// j % kRing, and the searches run at most kRing levels ahead of the slice
// writing that reads them.  The slices are written, gathered and drained in
// chunks of kChunkLevels levels: chunk c holds levels [c kChunkLevels,
// (c + 1) kChunkLevels) up to maxlen.
constexpr int64_t kRing = 32;
constexpr int64_t kChunkLevels = 16;
// The driver queues the searches kRing levels ahead, writes chunk c behind
// its last level's search, and then moves the searches on to the levels
// < chunk_end(c) + kRing: level j is queued right after chunk_freeing(j)'s
// write.  That needs kRing >= kChunkLevels (a chunk's last level is queued
// before the chunk waits for it); a whole number of chunks per ring keeps a
// chunk's levels in distinct ring slots that no later chunk shares in part.
static_assert(kRing % kChunkLevels == 0 && kRing >= kChunkLevels, "a ring slot is freed by an earlier chunk's write");

inline int64_t n_chunks(const GopPlan &g) { return (g.maxlen + kChunkLevels - 1) / kChunkLevels; }
inline int64_t chunk_first(int64_t c) { return c * kChunkLevels; }  // the chunk's levels [first, end)
inline int64_t chunk_end(const GopPlan &g, int64_t c) { return std::min(g.maxlen, (c + 1) * kChunkLevels); }
// level j >= kRing reuses the slot of level j - kRing: the chunk whose written slices free it
inline int64_t chunk_freeing(int64_t j) { return (j - kRing) / kChunkLevels; }
// entries of the largest chunk
inline int64_t max_chunk(const GopPlan &g) {
  int64_t m = 0;
  for (int64_t c = 0; c < n_chunks(g); ++c) m = std::max(m, g.lvl_off[chunk_end(g, c)] - g.lvl_off[chunk_first(c)]);
  return m;
}

}  // namespace vts
