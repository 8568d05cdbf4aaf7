// Stand-alone driver of the Intra_4x4 harness for an AddressSanitizer +
// UndefinedBehaviorSanitizer run (built with -fsanitize=address,undefined and
// run as a program; tests/test_enc_intra4_host.py does so when the compiler
// has the runtimes).  Every block over seeded tiles, and seeded macroblock
// rows of 1, 2 and 10 macroblocks of every kind, in I and P slices, at qp 1,
// 28 and 51, through the encoder and all three writers into exactly sized
// buffers.  TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstdlib>

#define EI4H_NO_SPS_PPS  // make_sps_pps lives in the stream writer; this program is the one file
#include "enc_intra4_host.cpp"

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
  if (!ok) std::fprintf(stderr, "enc_intra4_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  Rng r{4242};
  for (int round = 0; round < 50; ++round)
    for (int k = 0; k < 16; ++k)
      for (int mb_left = 0; mb_left < 2; ++mb_left) {
        std::vector<uint8_t> tile(16 * ei4::kTilePitch);  // exactly the tile: a read past it is caught
        for (auto &v : tile) v = static_cast<uint8_t>(r.below(4) == 0 ? (r.below(2) ? 255 : 0) : r.below(256));
        std::vector<uint8_t> avail(4), pred(9 * 16);
        const uint32_t allowed = ei4h_block(k, mb_left, tile.data(), avail.data(), pred.data());
        bad += check((allowed >> 2) & 1u, "DC is not allowed");
        uint64_t cur = 0, left = 0;
        for (int j = 0; j < 16; ++j) {
          cur |= static_cast<uint64_t>(r.below(9)) << (4 * j);
          left |= static_cast<uint64_t>(r.below(9)) << (4 * j);
        }
        const int pm = ei4h_pred_mode(k, cur, mb_left, r.below(2) ? left : ei4::kNoModes);
        bad += check(pm >= 0 && pm <= 8, "predicted mode out of range");
      }
  for (int mbw : {1, 2, 10})
    for (int qp : {1, 28, 51})
      for (int round = 0; round < 2; ++round) {
        const int npic = 3, mbh = 2, nmb = npic * mbh * mbw;
        const size_t fsz = static_cast<size_t>(16 * mbw) * 16 * mbh * 3 / 2;
        std::vector<uint8_t> src(fsz * npic), rec(fsz * npic), kind(static_cast<size_t>(nmb)), cbp(static_cast<size_t>(nmb));
        for (size_t i = 0; i < src.size(); ++i)
          src[i] = static_cast<uint8_t>(i >= fsz && r.below(3) ? std::min(255, std::max(1, src[i - fsz] + r.below(5) - 2))
                                                                : 1 + r.below(255));
        for (int a = 0; a < nmb; ++a) {
          const int idr_kinds[4] = {0, 1, 2, 5};
          kind[a] = static_cast<uint8_t>(a < mbh * mbw ? idr_kinds[r.below(4)] : r.below(6));
        }
        std::vector<uint32_t> cmd(static_cast<size_t>(nmb));
        std::vector<int16_t> coef(static_cast<size_t>(nmb) * kCoefPerMb);
        std::vector<uint64_t> modes(static_cast<size_t>(nmb));
        std::vector<int32_t> bits(static_cast<size_t>(nmb) * 2);
        ei4h_encode(mbw, mbh, npic, qp, src.data(), kind.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                    bits.data(), rec.data());
        int64_t len[3];
        for (int cabac = 0; cabac < 3; ++cabac) {
          std::vector<uint8_t> out(static_cast<size_t>(nmb) * ecab::kMbBytes + 1024);
          int64_t sizes[3];
          len[cabac] = ei4h_write(mbw, mbh, npic, qp, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                  out.data(), static_cast<int64_t>(out.size()), sizes);
          bad += check(len[cabac] > 0 && sizes[0] + sizes[1] + sizes[2] == len[cabac], "ei4h_write failed");
          std::vector<uint8_t> exact(static_cast<size_t>(len[cabac] > 0 ? len[cabac] : 1));
          bad += check(ei4h_write(mbw, mbh, npic, qp, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                  exact.data(), len[cabac], sizes) == len[cabac], "an exactly sized buffer overflowed");
          bad += check(ei4h_write(mbw, mbh, npic, qp, cabac, src.data(), cmd.data(), cbp.data(), coef.data(), modes.data(),
                                  exact.data(), len[cabac] - 1, sizes) == -1, "a short buffer did not report the overflow");
        }
        bad += check(len[1] == len[2], "BinRing and the direct coder differ in length");
      }
  if (bad) return 1;
  std::puts("enc_intra4_main: ok");
  return 0;
}
