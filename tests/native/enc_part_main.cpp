// Stand-alone driver of the inter-partition harness for an AddressSanitizer +
// UndefinedBehaviorSanitizer run (built with -fsanitize=address,undefined and
// run as a program; tests/test_enc_part_host.py does so when the compiler has
// the runtimes).  The predictors and the shape decision over seeded inputs, bS
// over seeded vector sets, and seeded macroblock rows of 1, 2 and 9 macroblocks
// of every kind and shape with vectors past every picture edge, at qp 1, 28
// and 51, with and without the filter, through the encoder and all three
// writers into exactly sized buffers.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstdlib>

#define EI4H_NO_SPS_PPS  // make_sps_pps lives in the stream writer; this program is the one file
#include "enc_part_host.cpp"

namespace {
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 33);
  }
  int below(int n) { return static_cast<int>(next() % static_cast<uint32_t>(n)); }
  int around(int n) { return below(2 * n + 1) - n; }
};

int check(bool ok, const char *what) {
  if (!ok) std::fprintf(stderr, "enc_part_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  Rng r{777};
  for (int round = 0; round < 2000; ++round) {
    int32_t q8[8], l4[4], out[2];
    for (int &v : q8) v = r.around(300);
    for (int &v : l4) v = r.around(300);
    for (int shape = 0; shape < 4; ++shape)
      for (int part = 0; part < epart::shape_blocks(shape); ++part) {
        eph_pred(shape, part, q8, r.below(2), l4, out);
        bad += check(out[0] >= -300 && out[0] <= 300 && out[1] >= -300 && out[1] <= 300, "a predictor outside its inputs");
      }
    const int ncand = 1 + r.below(30);
    std::vector<uint32_t> quads(static_cast<size_t>(ncand) * 4);  // exactly the candidates: a read past them is caught
    std::vector<int32_t> vec(static_cast<size_t>(ncand) * 2);
    for (auto &v : quads) v = static_cast<uint32_t>(r.below(16321));
    for (auto &v : vec) v = 4 * r.around(16);
    uint32_t cost9[9], sad9[9];
    int32_t idx9[9];
    const int shape = eph_pick(ncand, quads.data(), vec.data(), 1 + r.below(1335), r.around(8), r.around(8), cost9, idx9, sad9);
    bad += check(shape >= 0 && shape <= 3, "a shape out of range");
    uint32_t w[2][4];
    for (auto &m : w)
      for (auto &v : m) v = epart::mv_word(r.around(6), r.around(6));
    const int sp = eph_canonical(w[0]), sq = eph_canonical(w[1]);
    for (int dir = 0; dir < 2; ++dir)
      for (int e = dir; e < 4; ++e)
        for (int k = 0; k < 16; ++k) {
          const int bs = eph_bs(sp ? epart::part_cmd(sp) : w[0][0], static_cast<uint32_t>(r.below(4) ? 0 : r.below(65536)), w[0],
                                sq ? epart::part_cmd(sq) : w[1][0], 0, w[1], dir, e, k);
          bad += check(bs >= 0 && bs <= 2, "bS of two inter macroblocks out of range");
        }
  }
  for (int mbw : {1, 2, 9})
    for (int qp : {1, 28, 51})
      for (int dbk = 0; dbk < 2; ++dbk) {
        const int npic = 3, mbh = 2, nmb = npic * mbh * mbw;
        const size_t fsz = static_cast<size_t>(16 * mbw) * 16 * mbh * 3 / 2;
        std::vector<uint8_t> src(fsz * npic), rec(fsz * npic), kind(static_cast<size_t>(nmb)), cbp(static_cast<size_t>(nmb));
        for (size_t i = 0; i < src.size(); ++i)
          src[i] = static_cast<uint8_t>(i >= fsz && r.below(3) ? std::min(255, std::max(1, src[i - fsz] + r.below(5) - 2))
                                                                : 1 + r.below(255));
        std::vector<int32_t> vec(static_cast<size_t>(nmb) * 8);
        for (int a = 0; a < nmb; ++a) {
          kind[a] = static_cast<uint8_t>(a < mbh * mbw ? r.below(3) : r.below(5));
          const int shape = r.below(4);  // the canonical shape of the vectors
          for (int i = 0; i < 4; ++i) {
            const int from = shape == 0 ? 0 : (shape == 1 ? (i & 2) : (shape == 2 ? (i & 1) : i));
            for (int c = 0; c < 2; ++c) vec[8 * a + 2 * i + c] = from < i ? vec[8 * a + 2 * from + c] : r.around(r.below(2) ? 9 : 320);
          }
        }
        std::vector<uint32_t> cmd(static_cast<size_t>(nmb)), mv4(static_cast<size_t>(nmb) * 4);
        std::vector<int16_t> coef(static_cast<size_t>(nmb) * kCoefPerMb);
        std::vector<uint64_t> modes(static_cast<size_t>(nmb));
        eph_encode(mbw, mbh, npic, qp, dbk, src.data(), kind.data(), vec.data(), cmd.data(), cbp.data(), coef.data(),
                   modes.data(), mv4.data(), rec.data());
        int64_t len[3];
        for (int cabac = 0; cabac < 3; ++cabac) {
          std::vector<uint8_t> out(static_cast<size_t>(nmb) * ecab::kMbBytes + 1024);
          int64_t sizes[3];
          len[cabac] = eph_write(mbw, mbh, npic, qp, dbk, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                 mv4.data(), out.data(), static_cast<int64_t>(out.size()), sizes);
          bad += check(len[cabac] > 0 && sizes[0] + sizes[1] + sizes[2] == len[cabac], "eph_write failed");
          std::vector<uint8_t> exact(static_cast<size_t>(len[cabac] > 0 ? len[cabac] : 1));
          bad += check(eph_write(mbw, mbh, npic, qp, dbk, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                 mv4.data(), exact.data(), len[cabac], sizes) == len[cabac], "an exactly sized buffer overflowed");
          bad += check(eph_write(mbw, mbh, npic, qp, dbk, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                 mv4.data(), exact.data(), len[cabac] - 1, sizes) == -1,
                       "a short buffer did not report the overflow");
        }
        bad += check(len[1] == len[2], "BinRing and the direct coder differ in length");
      }
  if (bad) return 1;
  std::puts("enc_part_main: ok");
  return 0;
}
