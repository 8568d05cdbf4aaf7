// Stand-alone driver of the adaptive quantisation harness for an
// AddressSanitizer + UndefinedBehaviorSanitizer run (built with
// -fsanitize=address,undefined and run as a program; tests/test_enc_aq_host.py
// does so when the compiler has the runtimes).  The law over the extreme
// sums 8-bit samples give (the undefined-behaviour sanitizer traps a signed
// overflow and a shift out of range), seeded pictures in exactly sized arrays,
// and the running-QP rule over seeded rows.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <vector>

#include "enc_aq_host.cpp"

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
  if (!ok) std::fprintf(stderr, "enc_aq_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  Rng r{77};
  // the law at its corners: no energy, the largest (half the samples 0, half 255, in every plane), all 255
  bad += check(eaqh_energy(0, 0, 0, 0, 0, 0) == 0, "E of black");
  bad += check(eaqh_energy(256 * 255, 256 * 65025, 64 * 255, 64 * 65025, 64 * 255, 64 * 65025) == 0, "E of white");
  const uint32_t emax = eaqh_energy(128 * 255, 128 * 65025, 32 * 255, 32 * 65025, 32 * 255, 32 * 65025);
  bad += check(emax == 4161600u + 2 * 1040400u, "the largest E");
  for (uint32_t e = 0; e <= emax + 1; e = e < 70000 ? e + 1 : e + 997)
    for (int s : {1, 256, 768})
      for (int m : {1, 8, 10}) {
        const int off = eaqh_offset(e, s, m);
        bad += check(off >= -m && off <= m, "an offset outside aq_max");
        if (s == 1) bad += check(off == 0, "strength_q8 1 moved a macroblock");
      }
  bad += check(eaqh_offset(0, 256, 8) == -8 && eaqh_offset(1, 256, 10) == -10, "a constant macroblock");
  // pictures: 1 x 1 and 5 x 3 macroblocks
  for (int round = 0; round < 40; ++round) {
    const int mbw = round & 1 ? 5 : 1, mbh = round & 1 ? 3 : 1, cw = 16 * mbw, ch = 16 * mbh;
    std::vector<uint8_t> pic(static_cast<size_t>(cw) * ch * 3 / 2);
    const int amp = 1 + r.below(255);
    for (auto &b : pic) b = static_cast<uint8_t>(r.below(amp + 1));
    std::vector<int8_t> off(static_cast<size_t>(mbw) * mbh);
    eaqh_picture(pic.data(), cw, ch, 1 + r.below(768), 1 + r.below(10), off.data());
    for (int8_t o : off) bad += check(o >= -10 && o <= 10, "a picture's offset");
  }
  // rows: the deltas add up to the QPs, and stay inside mb_qp_delta's range
  for (int round = 0; round < 400; ++round) {
    const int n = 1 + r.below(12), sq = 1 + r.below(51);
    std::vector<uint8_t> kind(static_cast<size_t>(n)), cbp(kind.size()), qp(kind.size()), sent(kind.size()), inc(kind.size());
    std::vector<int32_t> delta(kind.size()), qpy(kind.size());
    for (int i = 0; i < n; ++i) {
      kind[i] = static_cast<uint8_t>(r.below(3));
      cbp[i] = static_cast<uint8_t>(r.below(2) ? r.below(48) : 0);
      const int q = sq + r.below(21) - 10;
      qp[i] = static_cast<uint8_t>(q < 1 ? 1 : (q > 51 ? 51 : q));
    }
    eaqh_row(n, sq, kind.data(), cbp.data(), qp.data(), delta.data(), sent.data(), inc.data(), qpy.data());
    int run = sq;
    for (int i = 0; i < n; ++i) {
      run += delta[i];
      bad += check(delta[i] >= -26 && delta[i] <= 25, "mb_qp_delta out of range");
      if (sent[i]) bad += check(run == qp[i], "the deltas do not add up to the macroblock's QP");
      else bad += check(delta[i] == 0, "a delta where none is sent");
      bad += check(qpy[i] == (kind[i] == 0 ? 0 : run), "QP_Y");
    }
  }
  if (bad) return 1;
  std::puts("enc_aq_main: ok");
  return 0;
}
