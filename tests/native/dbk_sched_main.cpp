// dbk_sched_main.cpp — stand-alone model of the deblocking wavefront's
// hand-off (csrc/dbk_sched.h), run on the CPU by tests/test_dbk_sched_host.py.
//
// W waves of four lock-stepped macroblock rows are state machines over
// prog[], built from the header's functions only: a wave at a pass start
// waits for dp_start_row() of its four rows, then steps through
// it = 0 .. mbw + 3 lag - 1, row g at macroblock x = it - lag g, waiting for
// dp_need_up / dp_need_dn; a step reads the ring line of the row above,
// writes this row's line (and the last word of the line before it), then
// publishes dp_publish().  Every wait is `counter >= value` on counters that
// only grow, so whether the waves finish does not depend on the schedule: one
// greedy schedule decides deadlock.  The ring's data races do depend on it,
// so the ring is checked under several schedules:
//   - a read of line (y - 1, x) must find the tag (y - 1, x), with the last
//     word written (row y - 1's step x + 1, or its own step at x = mbw - 1);
//   - a write must not replace a line whose reader has not read it.
//
//   dbk_sched_main run MBW MBH WAVES [DU DD]   one shape under every schedule;
//                 DU / DD weaken need_up / need_dn by that many macroblocks
//   dbk_sched_main table WAVES                 the model against dp_shape_ok()
// Prints one result line; exit status 0 unless the arguments are wrong.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbk_sched.h"

namespace {
using namespace vts::dbk;

struct Line {
  int y = -1, x = -1;   // tag: whose macroblock the line holds
  bool last = false;    // its last word (the columns the next macroblock's left edge finishes)
  bool read = true;     // the row below has read it (or nobody will)
};

struct Wave {
  int p;            // pass
  int it = -1;      // -1: at the pass start
  bool done = false;
};

enum Sched { kRoundRobin, kReverse, kRunToBlock, kRandom, kSchedules };
const char *const kSchedName[kSchedules] = {"round-robin", "reverse", "run-to-block", "random"};

struct Result {
  bool deadlock = false;
  int64_t stale = 0, lost = 0;  // reads of a wrong / unfinished line, writes over an unread line
};

struct Model {
  int mbw, mbh, W, du, dd;
  bool ring_check;
  std::vector<int> prog;
  std::vector<Wave> waves;
  std::vector<Line> ring;
  Result res;

  Model(int mbw_, int mbh_, int W_, int du_, int dd_, bool ring_check_)
      : mbw(mbw_), mbh(mbh_), W(W_), du(du_), dd(dd_), ring_check(ring_check_), prog(static_cast<size_t>(mbh_), 0),
        waves(static_cast<size_t>(W_)) {
    for (int w = 0; w < W; ++w) {
      waves[static_cast<size_t>(w)].p = w;
      waves[static_cast<size_t>(w)].done = 4 * w >= mbh;
    }
    if (ring_check) ring.resize(static_cast<size_t>(dp_rows_in_flight(W) * dp_ring_cols(W)));
  }
  Line &line(int y, int x) {
    return ring[static_cast<size_t>((y % dp_rows_in_flight(W)) * dp_ring_cols(W) + (x & (dp_ring_cols(W) - 1)))];
  }
  int steps() const { return mbw + 3 * dp_lag(W); }

  bool can_step(const Wave &v) const {
    for (int g = 0; g < 4; ++g) {
      const int y = 4 * v.p + g;
      if (y >= mbh) continue;
      if (v.it < 0) {
        if (dp_waits_at_start(y, W) && prog[static_cast<size_t>(dp_start_row(y, W))] < dp_done(mbw)) return false;
        continue;
      }
      const int x = v.it - dp_lag(W) * g;
      if (x < 0 || x >= mbw) continue;
      const int up = dp_need_up(g, y, x, mbw), dn = dp_need_dn(g, y, x, mbh, W);
      if (up != kNoWait && prog[static_cast<size_t>(y - 1)] < up - du) return false;
      if (dn != kNoWait && prog[static_cast<size_t>(y + 1)] < dn - dd) return false;
    }
    return true;
  }

  void step(Wave &v) {
    if (v.it < 0) {
      v.it = 0;
      return;
    }
    // the wave's rows read, then write, then publish (the kernel's order in a step)
    for (int phase = 0; phase < 3; ++phase)
      for (int g = 0; g < 4; ++g) {
        const int y = 4 * v.p + g, x = v.it - dp_lag(W) * g;
        if (y >= mbh || x < 0 || x >= mbw) continue;
        if (phase == 0 && ring_check && y > 0) {
          Line &L = line(y - 1, x);
          if (L.y != y - 1 || L.x != x || !L.last) ++res.stale;
          else L.read = true;
        } else if (phase == 1 && ring_check && y + 1 < mbh) {
          Line &C = line(y, x);
          if (!C.read) ++res.lost;
          C = Line{y, x, x == mbw - 1, false};
          if (x > 0) {
            Line &P = line(y, x - 1);
            if (P.y == y && P.x == x - 1) P.last = true;
            else ++res.lost;
          }
        } else if (phase == 2) {
          prog[static_cast<size_t>(y)] = dp_publish(x, mbw);
        }
      }
    if (++v.it == steps()) {
      v.it = -1;
      v.p += W;
      v.done = 4 * v.p >= mbh;
    }
  }

  Result run(Sched sched, uint64_t seed) {
    uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    auto rnd = [&rng]() {
      rng ^= rng << 13;
      rng ^= rng >> 7;
      rng ^= rng << 17;
      return rng;
    };
    std::vector<int> order(static_cast<size_t>(W));
    for (;;) {
      for (int i = 0; i < W; ++i) order[static_cast<size_t>(i)] = sched == kReverse ? W - 1 - i : i;
      if (sched == kRandom)
        for (int i = W - 1; i > 0; --i) std::swap(order[static_cast<size_t>(i)], order[rnd() % static_cast<uint64_t>(i + 1)]);
      bool moved = false, all_done = true;
      for (int w : order) {
        Wave &v = waves[static_cast<size_t>(w)];
        // random: a wave takes a random number of steps (0..7) in its turn
        int budget = sched == kRunToBlock ? 1 << 30 : (sched == kRandom ? static_cast<int>(rnd() % 8) : 1);
        while (!v.done && budget-- > 0 && can_step(v)) {
          step(v);
          moved = true;
        }
        all_done = all_done && v.done;
      }
      if (all_done) return res;
      if (!moved) {
        bool any = false;
        for (const Wave &v : waves) any = any || (!v.done && can_step(v));
        if (!any) {
          res.deadlock = true;
          return res;
        }
      }
    }
  }
};

bool deadlocks(int mbw, int mbh, int W) { return Model(mbw, mbh, W, 0, 0, false).run(kRunToBlock, 0).deadlock; }

int run_one(int mbw, int mbh, int W, int du, int dd) {
  const bool dl = deadlocks(mbw, mbh, W) && du == 0 && dd == 0;
  int64_t stale = 0, lost = 0;
  int runs = 0;
  bool dl_any = dl, dl_all = true;
  for (int s = 0; s < kSchedules; ++s)
    for (uint64_t seed = 1; seed <= (s == kRandom ? 8u : 1u); ++seed) {
      const Result r = Model(mbw, mbh, W, du, dd, true).run(static_cast<Sched>(s), seed);
      stale += r.stale;
      lost += r.lost;
      dl_any = dl_any || r.deadlock;
      dl_all = dl_all && r.deadlock;
      ++runs;
    }
  // monotone waits: every schedule must agree on termination
  std::printf("run mbw=%d mbh=%d waves=%d du=%d dd=%d schedules=%d result=%s stale_reads=%lld lost_lines=%lld\n", mbw,
              mbh, W, du, dd, runs, dl_any != dl_all ? "inconsistent" : (dl_any ? "deadlock" : "complete"),
              static_cast<long long>(stale), static_cast<long long>(lost));
  return 0;
}

int table(int W) {
  static const int kH[] = {64, 65, 67, 68, 129, 256};
  int T = 0;  // the model's threshold: first deadlocking width of a tall picture
  for (int w = 1; w <= 1024 && !T; ++w)
    if (deadlocks(w, kMaxMbHeight, W)) T = w;
  int T3 = 0;  // ... of a picture with one to three rows in its second pass
  for (int w = 1; w <= 1024 && !T3; ++w)
    if (deadlocks(w, dp_rows_in_flight(W) + 1, W)) T3 = w;
  int64_t checked = 0, mismatches = 0;
  int bw = 0, bh = 0;
  auto check = [&](int mbw, int mbh) {
    ++checked;
    if (deadlocks(mbw, mbh, W) == dp_shape_ok(mbw, mbh, W)) {
      if (!mismatches++) bw = mbw, bh = mbh;
    }
  };
  for (int mbh : kH)
    for (int mbw = 1; mbw <= 1024; ++mbw) check(mbw, mbh);
  const int kW[] = {1, 16, 17, T - 1, T, 1024};
  for (int mbw : kW)
    for (int mbh = 1; mbh <= kMaxMbHeight && mbw >= 1; ++mbh) check(mbw, mbh);
  std::printf("table waves=%d T=%d T_short=%d checked=%lld mismatches=%lld first_mismatch=%dx%d\n", W, T, T3,
              static_cast<long long>(checked), static_cast<long long>(mismatches), bw, bh);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 5 && !std::strcmp(argv[1], "run")) {
    const int mbw = std::atoi(argv[2]), mbh = std::atoi(argv[3]), W = std::atoi(argv[4]);
    const int du = argc > 5 ? std::atoi(argv[5]) : 0, dd = argc > 6 ? std::atoi(argv[6]) : 0;
    if (mbw >= 1 && mbw <= 1024 && mbh >= 1 && mbh <= 1024 && W >= 1 && W <= 16) return run_one(mbw, mbh, W, du, dd);
  } else if (argc == 3 && !std::strcmp(argv[1], "table")) {
    const int W = std::atoi(argv[2]);
    if (W >= 1 && W <= 16) return table(W);
  }
  std::fprintf(stderr, "usage: %s run MBW MBH WAVES [DU DD] | table WAVES\n", argv[0]);
  return 2;
}
