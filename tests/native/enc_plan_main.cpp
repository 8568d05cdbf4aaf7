// Stand-alone driver of the GOP plan harness for an AddressSanitizer +
// UndefinedBehaviorSanitizer run (built with -fsanitize=address,undefined and
// run as a program; tests/test_enc_plan_host.py does so when the compiler has
// the runtimes).  The inputs of that test (every n, keyint, score vector and
// flag) into exactly sized arrays, with the counting properties checked here
// too: every frame once among the write and the search entries, lvl_off ending
// at the entry count, the chunks tiling the levels.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstdlib>

#include "enc_plan_host.cpp"

namespace {
int check(bool ok, const char *what) {
  if (!ok) std::fprintf(stderr, "enc_plan_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  const float thr = 0.08f;
  for (int64_t n : {1, 2, 3, 17, 33, 49, 50, 70})
    for (int64_t keyint : {1, 2, 16, 33, 250})
      for (int cuts = 0; cuts < 4; ++cuts) {  // none; frame 1; frame n - 1; several, both ends among them
        std::vector<float> sc(static_cast<size_t>(n), 0.0f);
        if (cuts == 1 && n > 1) sc[1] = 1;
        if (cuts == 2) sc[static_cast<size_t>(n - 1)] = 1;
        if (cuts == 3)
          for (int64_t f : {int64_t{1}, int64_t{5}, n / 2, n - 1})
            if (f < n) sc[static_cast<size_t>(f)] = 1;
        for (int flags = 0; flags < 8; ++flags) {
          const int idr_at_cuts = flags & 1, intra = (flags >> 1) & 1, rate = (flags & 4) ? 3 : 0;
          int64_t dims[5];
          bad += check(eph_plan(n, sc.data(), keyint, idr_at_cuts, thr, intra, rate, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                nullptr, dims) == -1, "arrays of no size were accepted");
          bad += check(dims[0] == n, "not one entry per frame");
          const int64_t cap_levels = std::max({dims[1], dims[2], dims[3]});
          std::vector<int32_t> sent(static_cast<size_t>(4 * dims[0])), went(sent.size());
          std::vector<int64_t> lvl_off(static_cast<size_t>(cap_levels + 1)), gop_start(static_cast<size_t>(cap_levels)),
              chunks(static_cast<size_t>(2 * cap_levels));
          bad += check(eph_plan(n, sc.data(), keyint, idr_at_cuts, thr, intra, rate, dims[0], cap_levels, sent.data(),
                                went.data(), lvl_off.data(), gop_start.data(), chunks.data(), dims) == 0, "eph_plan failed");
          std::vector<int> seen_w(static_cast<size_t>(n), 0), seen_s(static_cast<size_t>(n), 0);
          for (int64_t e = 0; e < dims[0]; ++e) {
            const int32_t fw = went[static_cast<size_t>(4 * e)], fs = sent[static_cast<size_t>(4 * e)];
            if (fw < 0 || fw >= n || fs < 0 || fs >= n) {
              bad += check(false, "a frame outside the video");
              continue;
            }
            ++seen_w[static_cast<size_t>(fw)];
            ++seen_s[static_cast<size_t>(fs)];
          }
          for (int64_t f = 0; f < n; ++f)
            bad += check(seen_w[static_cast<size_t>(f)] == 1 && seen_s[static_cast<size_t>(f)] == 1, "a frame not exactly once");
          bad += check(lvl_off[0] == 0 && lvl_off[static_cast<size_t>(dims[1])] == dims[0], "lvl_off does not span the entries");
          int64_t at = 0, largest = 0;
          for (int64_t c = 0; c < dims[3]; ++c) {
            bad += check(chunks[static_cast<size_t>(2 * c)] == at && chunks[static_cast<size_t>(2 * c + 1)] > at,
                         "the chunks do not tile the levels");
            at = chunks[static_cast<size_t>(2 * c + 1)];
            largest = std::max(largest, lvl_off[static_cast<size_t>(at)] - lvl_off[static_cast<size_t>(chunks[static_cast<size_t>(2 * c)])]);
          }
          bad += check(at == dims[1] && largest == dims[4], "the chunks' end or max_chunk");
        }
      }
  if (bad) return 1;
  std::puts("enc_plan_main: ok");
  return 0;
}
