// Stand-alone driver of the rate control harness for an AddressSanitizer +
// UndefinedBehaviorSanitizer run (built with -fsanitize=address,undefined and
// run as a program; tests/test_enc_ratectl_host.py does so when the compiler
// has the runtimes).  The law over seeded measures in exactly sized arrays,
// GOPs of 1, 2, 3 and 250 pictures, budgets from 0 to the largest the ABI
// admits and measures up to 2^32 - 1: every product stays inside int64 (the
// undefined-behaviour sanitizer traps a signed overflow).  TEST INFRASTRUCTURE.
#include <cstdio>
#include <vector>

#include "enc_ratectl_host.cpp"

namespace {
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 33);
  }
  int below(int n) { return static_cast<int>(next() % static_cast<uint32_t>(n)); }
};

int check(bool ok, const char *what) {
  if (!ok) std::fprintf(stderr, "enc_ratectl_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  Rng r{4242};
  // one frame a second at the top bitrate: the largest B; and a frame of 1 / 240 s at 1 kbps: nearly the least
  const int64_t budgets[] = {0, erch_frame_budget(1, 1, 240), erch_frame_budget(500, 1000, 30000),
                             erch_frame_budget(erc::kMaxKbps, 1, 1)};
  bad += check(budgets[1] == 4 && budgets[2] == 16666 && budgets[3] == 1000000000ll, "frame_budget");
  for (int64_t B : budgets)
    for (int L : {1, 2, 3, 250})
      for (int round = 0; round < 200; ++round) {
        const int lo = 1 + r.below(51), hi = lo + r.below(52 - lo), qp = 1 + r.below(51);
        std::vector<uint32_t> bits(static_cast<size_t>(L));  // exactly the GOP: a read past it is caught
        std::vector<uint8_t> qps(static_cast<size_t>(L));
        const int kind = round % 4;
        for (auto &b : bits)
          b = kind == 0 ? 0xffffffffu - static_cast<uint32_t>(r.below(3))
                        : (kind == 1 ? static_cast<uint32_t>(r.below(3)) : (r.next() >> r.below(31)));
        erch_replay(B, L, qp, lo, hi, bits.data(), qps.data());
        for (int j = 0; j < L; ++j) {
          bad += check(qps[j] >= lo && qps[j] <= hi, "a QP outside [qp_min, qp_max]");
          if (j > 0) bad += check(qps[j] - qps[j - 1] <= 4 && qps[j - 1] - qps[j] <= 4, "a step beyond 4");
        }
      }
  if (bad) return 1;
  std::puts("enc_ratectl_main: ok");
  return 0;
}
