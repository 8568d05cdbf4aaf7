// pixel_clamp.h — packed-byte sample arithmetic shared by the ingest kernel
// (downscale.hip) and its CPU harness (tests/native/ingest_clamp_main.cpp);
// plain C++ on the host (pixel.h holds the device-only helpers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTS_PIXEL_FN __host__ __device__ __forceinline__
#else
#define VTS_PIXEL_FN inline
#endif

namespace vts {

// max(b, 1) of each of the four bytes of v (the small store holds no 0
// sample).  Exact per byte: the low seven bits of a byte plus 0x7f never
// carry out of the byte, so bit 7 of `nz` says "this byte is not 0" on its
// own.  The shorter (v - 0x01010101) & ~v & 0x80808080 test borrows across
// bytes and marks a 0x01 byte above a zero byte.
VTS_PIXEL_FN uint32_t clamp_min1_x4(uint32_t v) {
  const uint32_t nz = ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v;
  return v | ((~nz & 0x80808080u) >> 7);
}

}  // namespace vts
