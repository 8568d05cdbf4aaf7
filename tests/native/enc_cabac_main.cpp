// Stand-alone driver of the CABAC harness for an AddressSanitizer +
// UndefinedBehaviorSanitizer run (built with -fsanitize=address,undefined and
// run as a program; tests/test_enc_cabac_host.py does so when the compiler has
// the runtimes).  Seeded bin sequences through the engine, the context
// tables at every QP, and macroblock rows of every kind through both writers,
// into exactly sized buffers; a slot one byte short must report the overflow
// and store nothing past it; CAVLC rows through the byte sink and the kernel's
// dword sink into exactly sized buffers, generous and 1 .. 5 bytes short.
// TEST INFRASTRUCTURE.
#include <cstdio>
#include <cstdlib>

#define ECH_NO_SPS_PPS  // make_sps_pps lives in the stream writer; this program is the one file
#include "enc_cabac_host.cpp"

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
  if (!ok) std::fprintf(stderr, "enc_cabac_main: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  Rng r{12345};
  // the engine: long runs of one context (outstanding bits), bypass, a flush with raw bytes and a restart
  for (int round = 0; round < 20; ++round) {
    std::vector<int32_t> ops;
    const int n = 200 + r.below(3000);
    for (int i = 0; i < n; ++i) {
      const int k = r.below(20);
      if (k < 14) ops.insert(ops.end(), {0, r.below(3) ? 100 + r.below(4) : r.below(ecab::kNumCtx - 1), r.below(8) == 0});
      else if (k < 19) ops.insert(ops.end(), {1, 0, r.below(2)});
      else ops.insert(ops.end(), {2, 0, 0});
      if (r.below(500) == 0) {
        ops.insert(ops.end(), {2, 0, 1, 4, 0, 0});
        for (int b = 0; b < 16; ++b) ops.insert(ops.end(), {3, 1 + r.below(255), 0});
        ops.insert(ops.end(), {5, 0, 0});
      }
    }
    ops.insert(ops.end(), {2, 0, 1});
    std::vector<uint8_t> big(ops.size() * 2 + 64);
    const int qp = r.below(52);
    const int64_t len = ech_engine(ops.data(), static_cast<int64_t>(ops.size() / 3), round & 1, qp, big.data(),
                                   static_cast<int64_t>(big.size()));
    bad += check(len > 0, "engine overflowed a generous buffer");
    std::vector<uint8_t> exact(static_cast<size_t>(len > 0 ? len : 1));
    bad += check(ech_engine(ops.data(), static_cast<int64_t>(ops.size() / 3), round & 1, qp, exact.data(), len - 1) == -1 ||
                     len <= 1, "a short buffer did not report the overflow");
  }
  for (int qp = 0; qp <= 51; ++qp) {
    uint8_t st[ecab::kNumCtx];
    ech_contexts(qp & 1, qp, st);
    for (int i = 0; i < ecab::kNumCtx; ++i) bad += check((st[i] >> 1) <= 62, "pStateIdx > 62");
  }
  // macroblock rows of every kind
  for (int mbw : {1, 2, 10})
    for (int round = 0; round < 6; ++round) {
      const int npic = 3, mbh = 2, nmb = npic * mbh * mbw;
      std::vector<uint32_t> cmd(static_cast<size_t>(nmb));
      std::vector<uint8_t> cbp(static_cast<size_t>(nmb)), pcm(static_cast<size_t>(nmb) * 384);
      std::vector<int16_t> coef(static_cast<size_t>(nmb) * kCoefPerMb);
      for (auto &v : pcm) v = static_cast<uint8_t>(1 + r.below(255));
      for (auto &v : coef) {
        const int k = r.below(40);
        v = static_cast<int16_t>(k < 28 ? 0 : (k < 36 ? r.below(3) - 1 : (k < 39 ? r.below(41) - 20 : r.below(3001) - 1500)));
      }
      for (int a = 0; a < nmb; ++a) {
        const bool idr = a < mbh * mbw;
        const int kind = idr ? r.below(2) : r.below(6);
        if (kind == 0) {
          cmd[a] = edb::kPcmCmd;
        } else if (kind == 1) {
          const int cc = r.below(3), l15 = r.below(2) ? 15 : 0;
          cmd[a] = edb::kIntraCmd | static_cast<uint32_t>(1 + r.below(2)) | (static_cast<uint32_t>(r.below(2)) << 2) |
                   (static_cast<uint32_t>(l15 | (cc << 4)) << 4);
        } else if (kind == 2) {
          cmd[a] = 0;
        } else {
          const int mvx = r.below(135) - 67, mvy = r.below(135) - 67;
          cmd[a] = (static_cast<uint32_t>(mvx) & 0xffffu) | (static_cast<uint32_t>(mvy) << 16);
          cbp[a] = kind >= 4 ? static_cast<uint8_t>(1 + r.below(47)) : 0;
        }
      }
      for (int cabac = 0; cabac < 3; ++cabac) {
        std::vector<uint8_t> out(static_cast<size_t>(nmb) * ecab::kMbBytes + 1024);
        int64_t sizes[3];
        const int64_t len = ech_pictures(mbw, mbh, npic, 20 + r.below(20), round & 1, cabac, cmd.data(), cbp.data(),
                                         coef.data(), pcm.data(), out.data(), static_cast<int64_t>(out.size()), sizes);
        bad += check(len > 0 && sizes[0] + sizes[1] + sizes[2] == len, "ech_pictures failed");
      }
      // both sinks over an I and a P row (zeros among the samples: emulation prevention), into buffers of
      // exactly `cap` bytes and cap / 4 words: a generous cap, then 1 .. 5 bytes short of the slice
      for (size_t i = 0; i < pcm.size(); i += 1 + static_cast<size_t>(r.below(3))) pcm[i] = 0;
      for (int p = 0; p < 2; ++p) {
        const size_t at = static_cast<size_t>(p) * mbh * mbw;
        int64_t full[4] = {0, 0, 0, 0};
        for (int shortby = 0; shortby <= 5; ++shortby) {
          const int64_t cap = shortby ? full[0] - shortby : static_cast<int64_t>(mbw) * ecab::kMbBytes + 64;
          std::vector<uint8_t> bytes(static_cast<size_t>(cap));
          std::vector<uint32_t> words(static_cast<size_t>(cap / 4));
          int64_t res[4];
          ech_sinks(p == 0, mbw, 20 + round, round & 1, cmd.data() + at, cbp.data() + at, coef.data() + at * kCoefPerMb,
                    pcm.data() + at * 384, cap, bytes.data(), words.data(), res);
          if (!shortby) {
            std::memcpy(full, res, sizeof full);
            bad += check(!res[1] && !res[3] && res[0] == res[2] && res[0] > 0 &&
                             !std::memcmp(bytes.data(), words.data(), static_cast<size_t>(res[0])),
                         "the two sinks differ");
          } else {
            bad += check(res[1] && res[3] && res[0] == full[0] && res[2] == full[0], "a short sink did not report the overflow");
          }
        }
      }
    }
  if (bad) return 1;
  std::puts("enc_cabac_main: ok");
  return 0;
}
