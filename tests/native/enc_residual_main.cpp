// Stand-alone driver of the residual harness for sanitizer runs (not part of
// the pytest suite): the inputs of tests/test_enc_residual_host.py — fixed and
// seeded random blocks in [-255, 255] at every QP — through every entry point.
//   g++ -std=c++20 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-unknown-pragmas \
//       -Ivideo-transformer_amd/csrc -Iinclude tests/native/enc_residual_host.cpp tests/native/enc_residual_main.cpp
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" {
void ersh_fwd4(int, const int *, int *);
void ersh_code_blocks(int, const int *, int, int, int *, int *, int *, int *);
void ersh_chroma_dc(int, const int *, int, int *, int *);
void ersh_i16_dc(int, const int *, int, int *);
void ersh_all_zero(int, const int *, int, int, int *, int *);
void ersh_all_zero_chroma_dc(int, const int *, int, int *);
void ersh_diff(int, const uint8_t *, const uint8_t *, int *);
void ersh_recon_inter(int, const int *, int, const uint8_t *, uint8_t *);
void ersh_recon_chroma(int, const int *, const int *, int, int, const uint8_t *, uint8_t *);
void ersh_recon_i16(int, const int *, const int *, int, int, const uint8_t *, uint8_t *);
}

int main() {
  const int n = 2048;  // whole macroblocks of 16
  std::mt19937 rng(20260);
  std::vector<int> x(16 * n), w(16 * n), z(16 * n), lv(16 * n), dc(n), nz(n), zero(n), dl(16 * n);
  std::vector<uint8_t> pred(16 * n), out(16 * n);
  for (int i = 0; i < 16 * n; ++i) {
    const int b = i / 16, amp = b < 4 ? 255 : (b & 1 ? 255 : 1 + b % 24);
    x[i] = b == 0 ? 255 : b == 1 ? -255 : b == 2 ? ((i / 4 + i) & 1 ? -255 : 255) : b == 3 ? 0
                                                   : static_cast<int>(rng() % (2 * amp + 1)) - amp;
    pred[i] = static_cast<uint8_t>(b < 4 ? 255 * (b & 1) : rng());
  }
  long mismatches = 0;
  ersh_fwd4(n, x.data(), w.data());
  for (int qp = 0; qp < 52; ++qp)
    for (int dc_out = 0; dc_out < 2; ++dc_out) {
      ersh_code_blocks(n, x.data(), qp, dc_out, z.data(), lv.data(), dc.data(), nz.data());
      ersh_all_zero(n, x.data(), qp, dc_out, zero.data(), dc.data());
      for (int b = 0; b < n; ++b) mismatches += zero[b] == nz[b];
      ersh_recon_inter(n, z.data(), qp, pred.data(), out.data());
      if (!dc_out) continue;
      ersh_chroma_dc(n / 4, dc.data(), qp, dl.data(), nz.data());
      ersh_all_zero_chroma_dc(n / 4, dc.data(), qp, zero.data());
      for (int b = 0; b < n / 4; ++b) mismatches += zero[b] == nz[b];
      for (int ac = 0; ac < 2; ++ac) ersh_recon_chroma(n / 4, dl.data(), z.data(), ac, qp, pred.data(), out.data());
      ersh_i16_dc(n / 16, dc.data(), qp, dl.data());
      for (int ac = 0; ac < 2; ++ac) ersh_recon_i16(n / 16, dl.data(), z.data(), ac, qp, pred.data(), out.data());
    }
  ersh_diff(n, out.data(), pred.data(), w.data());
  std::printf("enc_residual: %d blocks x 52 qp, predicate/quantiser mismatches %ld\n", n, mismatches);
  return mismatches != 0;
}
