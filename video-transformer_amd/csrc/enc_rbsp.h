// enc_rbsp.h — the bit writer under both of the device encoder's entropy
// coders (enc_cavlc.h, enc_cabac.h), written once for the
// kernels and for the CPU harnesses.
//
//   Rbsp<Store>   RBSP bits -> EBSP bytes (7.4.1.1 emulation prevention):
//                 byte, bits, ue, se, align over the Store's put();
//   ByteStore     bytes into a bounded buffer (the harnesses);
//   WordStore     four bytes per aligned dword store into a staging slot (the
//                 kernels; plain C++, so the harness runs it too);
//                 both set `over` instead of storing past `cap`;
//   BitCount      the same interface counting the RBSP bits, nothing stored;
//   slice_header  the slice header of the encoder's slices (7.3.3) in either
//                 entropy coding mode.
#pragma once
#include <cstdint>

#include "parse_slice.h"  // VTS_HD, VTS_INLINE

namespace vts {
namespace full {
namespace erbsp {

struct ByteStore {
  uint8_t *p;
  int64_t cap, n;  // bytes
  bool over;
  VTS_HD void put(uint32_t b) {
    if (n < cap) p[n] = static_cast<uint8_t>(b);
    else over = true;
    ++n;
  }
  VTS_HD void flush() {}
};

struct WordStore {
  uint32_t *w;      // 4-byte aligned
  int64_t cap, n;   // bytes
  uint32_t cur;     // the bytes of the word being filled
  bool over;
  VTS_HD void put(uint32_t b) {
    cur |= b << (8 * (n & 3));
    if (!(++n & 3)) {
      if (n <= cap) w[(n >> 2) - 1] = cur;
      else over = true;
      cur = 0;
    }
  }
  VTS_HD void flush() {  // the partial word (its tail bytes are don't-care)
    if (n & 3) {
      if (n <= cap) w[n >> 2] = cur;
      else over = true;
    }
  }
};

template <class Store>
struct Rbsp : Store {
  uint64_t acc;
  int nacc, zeros;
  VTS_HD void byte(uint32_t b) {
    if (zeros >= 2 && b <= 3) {
      this->put(3);
      zeros = 0;
    }
    this->put(b);
    zeros = b ? 0 : zeros + 1;
  }
  VTS_HD void bits(int k, uint32_t v) {  // k <= 32
    acc = (acc << k) | v;
    nacc += k;
    while (nacc >= 8) {
      nacc -= 8;
      byte(static_cast<uint32_t>(acc >> nacc) & 0xffu);
    }
  }
  VTS_HD void ue(uint32_t v) {
    const uint32_t x = v + 1;
    const int len = 31 - __builtin_clz(x);
    if (len) bits(len, 0);
    bits(len + 1, x);
  }
  VTS_HD void se(int v) { ue(v > 0 ? static_cast<uint32_t>(2 * v - 1) : static_cast<uint32_t>(-2 * v)); }
  VTS_HD void align() {
    if (nacc) bits(8 - nacc, 0);
  }
};
// The byte sink is made as ByteSink{p, cap}; the further arguments are the
// members in the order its callers have always been able to list them.
struct ByteSink : Rbsp<ByteStore> {
  VTS_HD ByteSink(uint8_t *p, int64_t cap, int64_t n = 0, uint64_t acc = 0, int nacc = 0, int zeros = 0, bool over = false)
      : Rbsp<ByteStore>{{p, cap, n, over}, acc, nacc, zeros} {}
};
using WordSink = Rbsp<WordStore>;
VTS_HD VTS_INLINE WordSink word_sink(uint32_t *w, int64_t cap) { return WordSink{{w, cap, 0, 0, false}, 0, 0, 0}; }

VTS_HD VTS_INLINE int ue_bits(uint32_t v) { return 2 * (31 - __builtin_clz(v + 1)) + 1; }

struct BitCount {
  int64_t n = 0;
  VTS_HD void bits(int k, uint32_t) { n += k; }
  VTS_HD void ue(uint32_t v) { n += ue_bits(v); }
  VTS_HD void se(int v) { ue(v > 0 ? static_cast<uint32_t>(2 * v - 1) : static_cast<uint32_t>(-2 * v)); }
};

// 7.3.3 for one slice per macroblock row of a picture that is a reference
// with one reference picture.  cabac: cabac_init_idc 0 in its place in P
// slices, and cabac_alignment_one_bits (7.3.4) behind the header.  dbk: the
// slice asks for the filter inside the slice with the two offsets.
template <class Sink>
VTS_HD inline void slice_header(Sink &o, bool cabac, bool idr, int first_mb, int frame_num, int idr_pic_id,
                                int slice_qp_delta, bool dbk, int dbk_alpha, int dbk_beta) {
  o.put(idr ? 0x65 : 0x41);  // nal_ref_idc 3 IDR / 2 non-IDR
  o.ue(static_cast<uint32_t>(first_mb));
  o.ue(idr ? 7 : 5);  // slice_type I / P (all slices of the picture)
  o.ue(0);            // pic_parameter_set_id
  o.bits(16, static_cast<uint32_t>(frame_num) & 0xffffu);
  if (idr) {
    o.ue(static_cast<uint32_t>(idr_pic_id));
    o.bits(2, 0);  // no_output_of_prior_pics, long_term_reference
  } else {
    o.bits(3, 0);  // num_ref_idx_active_override, ref_pic_list_modification_l0, adaptive_ref_pic_marking
    if (cabac) o.ue(0);  // cabac_init_idc
  }
  o.se(slice_qp_delta);  // pic_init_qp 26
  if (dbk) {
    o.ue(2);  // disable_deblocking_filter_idc: filtered, but not across slice boundaries
    o.se(dbk_alpha);
    o.se(dbk_beta);
  } else {
    o.ue(1);
  }
  if (cabac && o.nacc) o.bits(8 - o.nacc, (1u << (8 - o.nacc)) - 1u);  // cabac_alignment_one_bit
}

}  // namespace erbsp
}  // namespace full
}  // namespace vts
