// dbk_sched.h — the hand-off rules of the by-plane deblocking wavefront
// (decode_full.hip dp_plane / h264_deblock_plane), for the kernel, the host's
// shape guard (h264_sched.cpp general_shape_error) and the stand-alone model
// (tests/native/dbk_sched_main.cpp).  No filter arithmetic here: only who
// waits for whom.
//
// A workgroup of `waves` waves filters one plane of one picture.  A wave holds
// four macroblock rows in lockstep, row g of the wave dp_lag() macroblocks
// behind row g - 1; pass p (rows 4 p .. 4 p + 3) belongs to wave p % waves,
// so dp_rows_in_flight() rows are in flight.  A row hands the sample rows its
// successor's top edge needs to it through an LDS ring of dp_ring_cols()
// lines (ring[y % rows_in_flight][x % ring_cols]); prog[y] counts the
// macroblocks row y has finished (dp_publish).  Three waits, all on prog[]:
//   pass start  row y takes over the ring slot of row y - rows_in_flight,
//               whose reader, row dp_start_row(y), must have finished
//               (the whole wave waits for its four rows)
//   need_up     a wave's first row reads line x of the previous wave's last
//               row once that row has finished macroblock x + 1 (which
//               writes the line's last word)
//   need_dn     a wave's last row overwrites ring column x once the next
//               wave's first row has read column x - ring_cols
// The pass-start wait is for a whole row, so it can close a cycle with
// need_dn: a picture wide enough that the last wave must start before the
// first wave's first row can finish, and tall enough for a second pass,
// never finishes.  dp_shape_ok() says which shapes are free of that; the
// model decides it by running the rules, and tests/test_dbk_sched_host.py
// holds the two equal.  (A per-column pass-start wait would remove the limit.)
#pragma once

#if defined(__HIPCC__)
#define VTS_DBK_HD __host__ __device__
#else
#define VTS_DBK_HD
#endif

#ifndef VTS_DBK_THREADS
#define VTS_DBK_THREADS 1024
#endif

namespace vts {
namespace dbk {

constexpr int kThreads = VTS_DBK_THREADS;  // 1024: 16 waves, 64 macroblock rows in flight
constexpr int kWaves = kThreads / 64;
constexpr int kNoWait = -(1 << 30);        // a requirement every prog[] value meets
constexpr int kMaxMbHeight = 256;          // h264_derive: one lane per macroblock row, at most 4 waves

VTS_DBK_HD constexpr int dp_rows_in_flight(int waves) { return 4 * waves; }
VTS_DBK_HD constexpr int dp_ring_cols(int /*waves*/) { return 16; }
VTS_DBK_HD constexpr int dp_lag(int /*waves*/) { return 2; }

// prog[y] after row y has finished macroblock x; mbw + 1: row flushed
VTS_DBK_HD constexpr int dp_done(int mbw) { return mbw + 1; }
VTS_DBK_HD constexpr int dp_publish(int x, int mbw) { return x + 1 < mbw ? x + 1 : dp_done(mbw); }

// pass start: whether row y takes over a ring slot (not in the first pass),
// and then the row that must have published dp_done() before y may write it
VTS_DBK_HD constexpr bool dp_waits_at_start(int y, int waves) { return y - dp_rows_in_flight(waves) >= 0; }
VTS_DBK_HD constexpr int dp_start_row(int y, int waves) { return y - dp_rows_in_flight(waves) + 1; }

// row y = 4 p + g at macroblock x: what prog[y - 1] / prog[y + 1] must have reached
VTS_DBK_HD constexpr int dp_need_up(int g, int y, int x, int mbw) {
  return (g == 0 && y > 0) ? (x + 1 < mbw ? x + 2 : dp_done(mbw)) : kNoWait;
}
VTS_DBK_HD constexpr int dp_need_dn(int g, int y, int x, int mbh, int waves) {
  return (g == 3 && y + 1 < mbh) ? x - dp_ring_cols(waves) + 1 : kNoWait;
}

// First picture width, in macroblocks, at which the waits above deadlock.
// The last wave's last row runs at most ring_cols macroblocks ahead of the
// first wave's next pass, each wave ring_cols + 3 lag behind the one before
// it.  With a whole fifth row group (mbh >= rows_in_flight + 4) the first
// wave's second pass waits for the second wave's first row to finish, which
// needs the last wave under way: (ring_cols + 3 lag) (waves - 1) + 1.  With
// one to three more rows only need_dn holds the last wave back, ring_cols
// later.  One pass never waits.
VTS_DBK_HD constexpr int dp_first_bad_width(int mbh, int waves) {
  const int r = dp_rows_in_flight(waves);
  if (mbh <= r) return 1 << 30;
  const int t = (dp_ring_cols(waves) + 3 * dp_lag(waves)) * (waves - 1) + 1;
  return mbh >= r + 4 ? t : t + dp_ring_cols(waves);
}
VTS_DBK_HD constexpr bool dp_shape_ok(int mbw, int mbh, int waves) {
  return mbw >= 1 && mbh >= 1 && mbw < dp_first_bad_width(mbh, waves);
}

// known answers of the model (the 256-thread build's hang on 720p, the
// 512-thread build's limit below 4K)
static_assert(!dp_shape_ok(80, 45, 4) && dp_shape_ok(80, 45, 8) && dp_shape_ok(80, 45, 16), "720p");
static_assert(dp_shape_ok(120, 68, 16), "1080p");
// a build whose wave count would deadlock at 3840x2160 (240 x 135) must not compile
static_assert(kThreads % 64 == 0 && kThreads <= 1024 && dp_shape_ok(240, 135, kWaves),
              "deblocking workgroup size: the hand-off deadlocks at 3840x2160 (dbk_sched.h)");

}  // namespace dbk
}  // namespace vts
