// ingest_clamp_main.cpp — the ingest kernel's dword clamp (csrc/pixel_clamp.h,
// the same header downscale.hip compiles) on the host, stand-alone:
//
//   ingest_clamp_main OUT
//
// writes vts::clamp_min1_x4 of every test dword to OUT as native uint32, in
// this order: the 6^4 dwords whose bytes (byte 3 slowest) come from
// {0, 1, 2, 0x7f, 0x80, 0xff}; then, for each of the 36 high halves made of
// two such bytes (byte 3 slower), every 16-bit low half in ascending order.
// It also checks each against the per-byte max(b, 1) itself and exits 1,
// naming the first dword that differs.  tests/test_ingest_clamp_host.py
// rebuilds the inputs and compares OUT with its own per-byte result.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pixel_clamp.h"

namespace {
uint32_t per_byte(uint32_t v) {
  uint32_t r = 0;
  for (int b = 0; b < 4; ++b) {
    const uint32_t x = (v >> (8 * b)) & 255u;
    r |= (x < 1 ? 1u : x) << (8 * b);
  }
  return r;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 2;
  }
  static const uint32_t kSet[6] = {0, 1, 2, 0x7f, 0x80, 0xff};
  std::vector<uint32_t> in;
  for (uint32_t b3 : kSet)
    for (uint32_t b2 : kSet)
      for (uint32_t b1 : kSet)
        for (uint32_t b0 : kSet) in.push_back(b3 << 24 | b2 << 16 | b1 << 8 | b0);
  for (uint32_t b3 : kSet)
    for (uint32_t b2 : kSet)
      for (uint32_t lo = 0; lo < 65536; ++lo) in.push_back(b3 << 24 | b2 << 16 | lo);
  std::vector<uint32_t> out(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    out[i] = vts::clamp_min1_x4(in[i]);
    if (out[i] != per_byte(in[i])) {
      std::fprintf(stderr, "clamp_min1_x4(0x%08x) = 0x%08x, per byte 0x%08x\n", in[i], out[i], per_byte(in[i]));
      return 1;
    }
  }
  std::FILE *f = std::fopen(argv[1], "wb");
  if (!f || std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 2;
  }
  std::printf("%zu dwords\n", in.size());
  return 0;
}
