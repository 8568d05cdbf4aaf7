// CPU harness over csrc/enc_plan.h: the device encoder's GOP plan and its
// chunk / ring arithmetic, exactly what csrc/transcode_driver.cpp calls, behind
// a C interface for tests/test_enc_plan_host.py (and enc_plan_main.cpp, the
// stand-alone sanitizer run).  TEST INFRASTRUCTURE.
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_plan.h"

extern "C" {

int64_t eph_ring() { return vts::kRing; }
int64_t eph_chunk_levels() { return vts::kChunkLevels; }
// level j >= kRing: the chunk whose written slices free its ring slot
int64_t eph_chunk_freeing(int64_t j) { return vts::chunk_freeing(j); }

// plan_gops(n, scores[n], ...) into the caller's arrays: sent / went [entries][4],
// lvl_off [maxlen + 1], gop_start [ngop], chunks [n_chunks][2] = (first level,
// end level).  dims = {entries, maxlen, ngop, n_chunks, max_chunk}.  Returns 0,
// or -1 when an array is too small (cap_entries entries, cap_levels levels and
// GOPs and chunks); dims is filled either way.
int eph_plan(int64_t n, const float *scores, int64_t keyint, int idr_at_cuts, float thr, int intra, int rate,
             int64_t cap_entries, int64_t cap_levels, int32_t *sent, int32_t *went, int64_t *lvl_off,
             int64_t *gop_start, int64_t *chunks, int64_t *dims) {
  const std::vector<float> sc(scores, scores + n);
  const vts::GopPlan g = vts::plan_gops(n, sc, keyint, idr_at_cuts != 0, thr, intra != 0, rate);
  const int64_t entries = static_cast<int64_t>(g.went.size()), nc = vts::n_chunks(g);
  dims[0] = entries;
  dims[1] = g.maxlen;
  dims[2] = g.ngop;
  dims[3] = nc;
  dims[4] = vts::max_chunk(g);
  if (static_cast<int64_t>(g.sent.size()) != entries || static_cast<int64_t>(g.lvl_off.size()) != g.maxlen + 1) return -2;
  if (entries > cap_entries || g.maxlen > cap_levels || g.ngop > cap_levels || nc > cap_levels) return -1;
  static_assert(sizeof(vts::PlanEntry) == 4 * sizeof(int32_t), "entries are four int32_t");
  std::memcpy(sent, g.sent.data(), g.sent.size() * sizeof(vts::PlanEntry));
  std::memcpy(went, g.went.data(), g.went.size() * sizeof(vts::PlanEntry));
  std::memcpy(lvl_off, g.lvl_off.data(), g.lvl_off.size() * sizeof(int64_t));
  std::memcpy(gop_start, g.gop_start.data(), g.gop_start.size() * sizeof(int64_t));
  for (int64_t c = 0; c < nc; ++c) {
    chunks[2 * c] = vts::chunk_first(c);
    chunks[2 * c + 1] = vts::chunk_end(g, c);
  }
  return 0;
}

}  // extern "C"
