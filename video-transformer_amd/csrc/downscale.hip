// downscale.hip — the small store: every decoded frame of the transcoded
// range (the whole video by default) downscaled (area filter, NV12 -> NV12 at
// (w, height), coded 16-aligned; at ratio 1 copied by ingest_nv12) into one
// store while it sits in the decode ring.  The decode sessions call
// setup_small and small_window (session.h); the device encoder
// (transcode.hip, transcode_driver.cpp) reads the store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pixel_clamp.h"
#include "session.h"

namespace vts {
namespace {

constexpr int kMaxTaps = 16;

// ----------------------------------------------------------- downscale
// Area filter, per axis: destination o covers source footprint [o n, (o+1) n)
// in units of 1/m; source i covers [i m, (i+1) m).  Tap table entry o =
// [i0, w_0 .. w_{K-1}] (weights / gcd(n, m)); outputs past the display size
// (coded padding) repeat the last display entry.
struct DsArgs {
  const uint8_t *src;      // ring surface of the window's first frame
  int64_t src_stride;
  int32_t pitch, uv_rows;  // UV plane at pitch * uv_rows
  int32_t sw, sh;          // source display size
  uint8_t *dst;            // small store, the window's first frame
  int64_t dst_stride;
  int32_t cw, ch;          // destination coded size
  const int32_t *tx, *ty, *tcx, *tcy;
  int32_t kx, ky, kcx, kcy;
  int32_t tl, tc;          // normalisers (product of the axes' n / gcd)
  int64_t n_frames;
};

__device__ __forceinline__ uint32_t area_px(const uint8_t *p, int pitch, int step, const int32_t *ex,
                                            int kx, const int32_t *ey, int ky, int nx, int ny, int t) {
  uint32_t sum = 0;
  const int x0 = ex[0], y0 = ey[0];
  for (int j = 0; j < ky; ++j) {
    const uint32_t wy = static_cast<uint32_t>(ey[1 + j]);
    if (!wy) continue;
    const uint8_t *row = p + static_cast<int64_t>(min(y0 + j, ny - 1)) * pitch;
    uint32_t s = 0;
    for (int i = 0; i < kx; ++i) s += static_cast<uint32_t>(ex[1 + i]) * row[min(x0 + i, nx - 1) * step];
    sum += wy * s;
  }
  const uint32_t v = (sum + static_cast<uint32_t>(t) / 2) / static_cast<uint32_t>(t);
  return v < 1 ? 1u : v;
}

// Integer ratio K on both axes (720p -> 360p: 2, 1080p -> 360p: 3): four
// outputs from K rows of 4K contiguous bytes, dword loads; luma and NV12
// chroma (4 bytes U0 V0 U1 V1 from 2K source pairs) share the addressing.
template <int K>
__device__ __forceinline__ uint32_t box4(const uint8_t *p, int pitch, bool chroma) {
  uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t *r = reinterpret_cast<const uint32_t *>(p + static_cast<int64_t>(j) * pitch);
#pragma unroll
    for (int w = 0; w < K; ++w) {
      const uint32_t v = r[w];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int byte = 4 * w + b;  // 0 .. 4K-1
        // luma: output byte / K; chroma: pair byte / 2 -> output pair (pair / K), plane byte & 1
        const int q = chroma ? 2 * ((byte >> 1) / K) + (byte & 1) : byte / K;
        acc[q] += (v >> (8 * b)) & 255u;
      }
    }
  }
  uint32_t out = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t m = (acc[q] + K * K / 2) / (K * K);
    out |= (m < 1 ? 1u : m) << (8 * q);
  }
  return out;
}

template <int K>
__global__ void __launch_bounds__(256) downscale_nv12(DsArgs a) {
  const int groups = a.cw / 4;
  const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  const int rows = a.ch + a.ch / 2;
  if (t >= static_cast<int64_t>(groups) * rows) return;
  const int64_t f = blockIdx.y;
  const int g = static_cast<int>(t % groups), row = static_cast<int>(t / groups);
  const uint8_t *src = a.src + f * a.src_stride;
  uint8_t *dst = a.dst + f * a.dst_stride;
  if constexpr (K > 0) {
    const int dw = a.sw / K, dh = a.sh / K;  // output display size
    if (row < dh && 4 * g + 3 < dw) {
      *reinterpret_cast<uint32_t *>(dst + static_cast<int64_t>(row) * a.cw + 4 * g) =
          box4<K>(src + static_cast<int64_t>(K * row) * a.pitch + 4 * K * g, a.pitch, false);
      return;
    }
    if (row >= a.ch && row - a.ch < dh / 2 && 4 * g + 3 < dw) {
      const int cy = row - a.ch;
      const uint8_t *uv = src + static_cast<int64_t>(a.pitch) * a.uv_rows;
      *reinterpret_cast<uint32_t *>(dst + static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(cy) * a.cw +
                                    4 * g) = box4<K>(uv + static_cast<int64_t>(K * cy) * a.pitch + 4 * K * g, a.pitch, true);
      return;
    }
  }
  uint32_t out = 0;
  if (row < a.ch) {
    const int32_t *ey = a.ty + static_cast<int64_t>(row) * (1 + a.ky);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int32_t *ex = a.tx + static_cast<int64_t>(4 * g + q) * (1 + a.kx);
      out |= area_px(src, a.pitch, 1, ex, a.kx, ey, a.ky, a.sw, a.sh, a.tl) << (8 * q);
    }
    *reinterpret_cast<uint32_t *>(dst + static_cast<int64_t>(row) * a.cw + 4 * g) = out;
  } else {
    const int cy = row - a.ch;
    const uint8_t *uv = src + static_cast<int64_t>(a.pitch) * a.uv_rows;
    const int32_t *ey = a.tcy + static_cast<int64_t>(cy) * (1 + a.kcy);
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // bytes U0 V0 U1 V1 of chroma columns 2g, 2g+1
      const int32_t *ex = a.tcx + static_cast<int64_t>(2 * g + (q >> 1)) * (1 + a.kcx);
      out |= area_px(uv + (q & 1), a.pitch, 2, ex, a.kcx, ey, a.kcy, a.sw / 2, a.sh / 2, a.tc) << (8 * q);
    }
    *reinterpret_cast<uint32_t *>(dst + static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(cy) * a.cw +
                                  4 * g) = out;
  }
}

// ------------------------------------------------------------- ingest
// Ratio 1 (output size = source display size): the store's frame is the
// source's with every sample max(s, 1) and the coded padding rebuilt from the
// display edge (the surface's own padding holds whatever the stream coded in
// the cropped area).  One lane makes 16 bytes of one row, luma rows then the
// NV12 chroma rows: one 16-byte load and one 16-byte store where the group
// lies inside the display, the edge rule byte by byte where it crosses the
// display width or the row is a padded one.  small_window checks the 16-byte
// alignment of both sides.
struct IngestArgs {
  const uint8_t *src;  // ring surface of the first frame
  int64_t src_stride;
  int32_t pitch, uv_rows;
  int32_t sw, sh;      // display size (even)
  uint8_t *dst;        // small store, the first frame's slot
  int64_t dst_stride;
  int32_t cw, ch;      // coded size
};

__global__ void __launch_bounds__(256) ingest_nv12(IngestArgs a) {
  const int groups = a.cw / 16;
  const int rows = a.ch + a.ch / 2;
  const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (t >= static_cast<int64_t>(groups) * rows) return;
  const int64_t f = blockIdx.y;
  const int g = static_cast<int>(t % groups), row = static_cast<int>(t / groups);
  const bool chroma = row >= a.ch;
  const int y = chroma ? row - a.ch : row;        // row of its plane
  const int ny = chroma ? a.sh / 2 : a.sh;        // display rows of the plane
  const uint8_t *plane = a.src + f * a.src_stride + (chroma ? static_cast<int64_t>(a.pitch) * a.uv_rows : 0);
  uint4 *out = reinterpret_cast<uint4 *>(a.dst + f * a.dst_stride + static_cast<int64_t>(row) * a.cw + 16 * g);
  uint4 v;
  if (y < ny && 16 * g + 16 <= a.sw) {
    v = *reinterpret_cast<const uint4 *>(plane + static_cast<int64_t>(y) * a.pitch + 16 * g);
  } else {
    // columns >= sw repeat the last display column (chroma: the last U, V pair), rows >= ny the last display row
    const uint8_t *r = plane + static_cast<int64_t>(min(y, ny - 1)) * a.pitch;
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t d = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int x = 16 * g + 4 * q + b;
        const int sx = chroma ? 2 * min(x >> 1, a.sw / 2 - 1) + (x & 1) : min(x, a.sw - 1);
        d |= static_cast<uint32_t>(r[sx]) << (8 * b);
      }
      w[q] = d;
    }
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  v.x = clamp_min1_x4(v.x);
  v.y = clamp_min1_x4(v.y);
  v.z = clamp_min1_x4(v.z);
  v.w = clamp_min1_x4(v.w);
  *out = v;
}

// ------------------------------------------------------------ host
int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// tap table for n source -> m destination samples over `coded` outputs
std::vector<int32_t> area_taps(int64_t n, int64_t m, int coded, int *k_out, int32_t *t_out) {
  const int64_t g = gcd64(n, m);
  int k = 1;
  for (int64_t o = 0; o < m; ++o) {
    const int64_t i0 = o * n / m, i1 = ((o + 1) * n + m - 1) / m;
    k = std::max<int>(k, static_cast<int>(i1 - i0));
  }
  std::vector<int32_t> t(static_cast<size_t>(coded) * (1 + k), 0);
  for (int x = 0; x < coded; ++x) {
    const int64_t o = std::min<int64_t>(x, m - 1);
    const int64_t i0 = o * n / m;
    int32_t *e = &t[static_cast<size_t>(x) * (1 + k)];
    e[0] = static_cast<int32_t>(i0);
    for (int i = 0; i < k; ++i) {
      const int64_t si = i0 + i;
      const int64_t lo = std::max(o * n, si * m), hi = std::min((o + 1) * n, (si + 1) * m);
      e[1 + i] = (si < n && hi > lo) ? static_cast<int32_t>((hi - lo) / g) : 0;
    }
  }
  *k_out = k;
  *t_out = static_cast<int32_t>(n / g);
  return t;
}

}  // namespace

int setup_small(vts_ctx *c, int sh, int64_t f0, int64_t f1) {
  SmallStore &S = c->small;
  const int W = c->width, H = c->height;
  const int sw = static_cast<int>((static_cast<int64_t>(sh) * W + H) / (2 * static_cast<int64_t>(H))) * 2;
  if (sw < 2) return fail(VTS_E_INVALID, "output width %d from %dx%d at height %d", sw, W, H, sh);
  if (S.d && S.w == sw && S.h == sh && S.cap >= f1 - f0) {  // the same geometry and room for the range
    S.f0 = f0;
    S.f1 = f1;
    return VTS_OK;
  }
  if (S.d) vts::dfree(S.d);
  if (S.d_taps) vts::dfree(S.d_taps);
  S = SmallStore{};
  S.w = sw;
  S.h = sh;
  S.f0 = f0;
  S.f1 = f1;
  S.cw = (sw + 15) & ~15;
  S.ch = (sh + 15) & ~15;
  S.stride = (static_cast<int64_t>(S.cw) * S.ch * 3 / 2 + 255) & ~int64_t(255);
  int32_t tl_x, tl_y, tc_x, tc_y;
  const auto tx = area_taps(W, sw, S.cw, &S.taps_x, &tl_x);
  const auto ty = area_taps(H, sh, S.ch, &S.taps_y, &tl_y);
  const auto tcx = area_taps(W / 2, sw / 2, S.cw / 2, &S.taps_cx, &tc_x);
  const auto tcy = area_taps(H / 2, sh / 2, S.ch / 2, &S.taps_cy, &tc_y);
  if (std::max({S.taps_x, S.taps_y, S.taps_cx, S.taps_cy}) > kMaxTaps)
    return fail(VTS_E_UNSUPPORTED, "downscale ratio %dx%d -> %dx%d needs more than %d taps", W, H, sw, sh,
                kMaxTaps);
  if (static_cast<int64_t>(tl_x) * tl_y * 255 > 0x7fffffffll || static_cast<int64_t>(tc_x) * tc_y * 255 > 0x7fffffffll)
    return fail(VTS_E_UNSUPPORTED, "downscale ratio %dx%d -> %dx%d overflows 32-bit sums", W, H, sw, sh);
  S.tl = tl_x * tl_y;
  S.tc = tc_x * tc_y;
  std::vector<int32_t> all;
  S.off[0] = 0;
  for (const auto *v : {&tx, &ty, &tcx, &tcy}) {
    all.insert(all.end(), v->begin(), v->end());
  }
  S.off[1] = static_cast<int64_t>(tx.size());
  S.off[2] = S.off[1] + static_cast<int64_t>(ty.size());
  S.off[3] = S.off[2] + static_cast<int64_t>(tcx.size());
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(vts::dmalloc(&S.d_taps, all.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(S.d_taps, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const size_t bytes = static_cast<size_t>(S.stride * (f1 - f0) + 256);
  if (vts::dmalloc(&S.d, bytes) != hipSuccess) {
    (void)hipGetLastError();
    S.d = nullptr;
    return fail(VTS_E_HIP, "cannot allocate %.1f GiB for the %dx%d frames", bytes / 1073741824.0, sw, sh);
  }
  S.cap = f1 - f0;
  return VTS_OK;
}

int small_window(vts_ctx *c, int ring, int64_t wf0, int64_t wf1, hipStream_t s) {
  const SmallStore &S = c->small;
  // the window's frames the store holds (none: nothing to do); frame f of the
  // window is ring surface f - wf0 and goes to the store's slot f - S.f0
  const int64_t f0 = std::max(wf0, S.f0), f1 = std::min(wf1, S.f1);
  if (f1 <= f0) return VTS_OK;
  if (f0 < S.f0 || f1 - S.f0 > S.cap)  // never: setup_small gave the range its slots
    return fail(VTS_E_HIP, "small store of %lld slots from frame %lld: frames %lld .. %lld", static_cast<long long>(S.cap),
                static_cast<long long>(S.f0), static_cast<long long>(f0), static_cast<long long>(f1 - 1));
  DsArgs a{};
  a.src = c->d_surf[ring] + (f0 - wf0) * c->frame_stride;
  a.src_stride = c->frame_stride;
  a.pitch = c->pitch;
  a.uv_rows = c->coded_h;
  a.sw = c->width;
  a.sh = c->height;
  a.dst = S.d + (f0 - S.f0) * S.stride;
  a.dst_stride = S.stride;
  a.cw = S.cw;
  a.ch = S.ch;
  a.tx = S.d_taps + S.off[0];
  a.ty = S.d_taps + S.off[1];
  a.tcx = S.d_taps + S.off[2];
  a.tcy = S.d_taps + S.off[3];
  a.kx = S.taps_x;
  a.ky = S.taps_y;
  a.kcx = S.taps_cx;
  a.kcy = S.taps_cy;
  a.tl = S.tl;
  a.tc = S.tc;
  a.n_frames = f1 - f0;
  const int64_t threads = static_cast<int64_t>(S.cw / 4) * (S.ch + S.ch / 2);
  // integer ratio on both axes (equal): the dword box path; else the tap tables
  const int W = c->width, H = c->height;
  const int k = (W % S.w == 0 && H % S.h == 0 && W / S.w == H / S.h) ? W / S.w : 0;
  // ratio 1: 16-byte groups, when both sides are 16-byte aligned (they are: the pitch is the coded width,
  // frame_stride and stride are multiples of 256 and the allocations' bases of more; else the tap tables)
  const auto al16 = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool ingest = k == 1 && al16(a.src) && al16(a.dst) && a.pitch % 16 == 0 && a.src_stride % 16 == 0 &&
                      a.cw % 16 == 0 && a.dst_stride % 16 == 0 &&
                      (static_cast<int64_t>(a.pitch) * a.uv_rows) % 16 == 0;
  const int64_t groups16 = static_cast<int64_t>(S.cw / 16) * (S.ch + S.ch / 2);
  for (int64_t g0 = 0; g0 < f1 - f0; g0 += 65535) {  // grid.y <= 65535 frames per launch
    DsArgs b = a;
    b.src = a.src + g0 * a.src_stride;
    b.dst = a.dst + g0 * a.dst_stride;
    b.n_frames = std::min<int64_t>(65535, f1 - f0 - g0);
    if (ingest) {
      const IngestArgs ia{b.src, b.src_stride, b.pitch, b.uv_rows, b.sw, b.sh, b.dst, b.dst_stride, b.cw, b.ch};
      hipLaunchKernelGGL(ingest_nv12, dim3(static_cast<unsigned>((groups16 + 255) / 256), static_cast<unsigned>(b.n_frames)),
                         dim3(256), 0, s, ia);
      continue;
    }
    const dim3 grid(static_cast<unsigned>((threads + 255) / 256), static_cast<unsigned>(b.n_frames));
    switch (k) {
      case 2: hipLaunchKernelGGL(downscale_nv12<2>, grid, dim3(256), 0, s, b); break;
      case 3: hipLaunchKernelGGL(downscale_nv12<3>, grid, dim3(256), 0, s, b); break;
      case 4: hipLaunchKernelGGL(downscale_nv12<4>, grid, dim3(256), 0, s, b); break;
      default: hipLaunchKernelGGL(downscale_nv12<0>, grid, dim3(256), 0, s, b); break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(VTS_E_HIP, "downscale_nv12 launch: %s", hipGetErrorString(e));
  return VTS_OK;
}

}  // namespace vts
