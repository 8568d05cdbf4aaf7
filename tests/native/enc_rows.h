// What the encoder harnesses (enc_cabac_host.cpp, enc_intra4_host.cpp) share:
// a macroblock row (command words, coded_block_pattern, levels, mode words,
// I_PCM samples: what a level of transcode.hip holds) written as one slice by
// the headers the kernels call, walked in the kernels' order: enc_cavlc.h as
// enc_write does, enc_cabac.h as enc_write_cabac does.  TEST INFRASTRUCTURE.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_cabac.h"
#include "enc_cavlc.h"

namespace ecab = vts::full::ecab;
namespace ecav = vts::full::ecav;
namespace edb = vts::full::edb;
namespace ei4 = vts::full::ei4;
namespace erbsp = vts::full::erbsp;

namespace {
constexpr int kCoefPerMb = 384;  // transcode.hip's level layout

using Sink = erbsp::ByteSink;

struct RowData {
  const uint32_t *cmd;
  const uint8_t *cbp;
  const int16_t *coef;    // [mx][384]
  const uint64_t *modes;  // read for I_NxN macroblocks only
  const uint8_t *pcm;     // [mx][384]
};

// the I_PCM samples behind mb_type: pcm_alignment_zero_bits and the 384 bytes
template <class S>
void pcm_samples(S &o, const uint8_t *pcm) {
  o.align();
  for (int i = 0; i < 384; ++i) o.byte(pcm[i]);
}

// macroblock mx of the row through enc_cavlc.h: enc_write's dispatch
template <class S>
void cavlc_mb(S &o, bool idr, ecav::Row &z, const RowData &d, int mx) {
  const uint32_t c = d.cmd[mx];
  const int16_t *cp = d.coef + static_cast<int64_t>(mx) * kCoefPerMb;
  if (c == edb::kPcmCmd) ecav::mb_pcm_head(o, idr, z);  // the caller supplies the samples
  else if (ei4::is_i4_cmd(c)) ecav::mb_intra4(o, idr, z, c, d.modes[mx], cp);
  else if (edb::is_intra_cmd(c)) ecav::mb_intra16(o, idr, z, c, cp);
  else if (c == 0 && d.cbp[mx] == 0) ecav::mb_skip(z);
  else ecav::mb_inter(o, z, c, d.cbp[mx], cp);
}
// one slice as CAVLC; S: the byte or the dword sink
template <class S>
void cavlc_row(S &o, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const RowData &d) {
  erbsp::slice_header(o, false, idr, row * mbw, frame_num, 0, qp - 26, dbk, 0, 0);
  ecav::Row z;
  z.start();
  for (int mx = 0; mx < mbw; ++mx) {
    cavlc_mb(o, idr, z, d, mx);
    if (d.cmd[mx] == edb::kPcmCmd) pcm_samples(o, d.pcm + 384 * mx);
  }
  ecav::slice_end(o, z);
}

// the same slice as CABAC; E: the Encoder itself, or the kernel's BinRing in front of it
template <class E>
void cabac_mbs(E &e, Sink &o, bool idr, int mbw, const RowData &d) {
  ecab::Left l = ecab::left_none();
  bool a_ok = false;
  int amx = 0, amy = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = d.cmd[mx];
    const int16_t *cp = d.coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const bool last = mx == mbw - 1;
    if (c == edb::kPcmCmd) {
      ecab::mb_pcm_begin(e, idr, l);
      pcm_samples(o, d.pcm + 384 * mx);
      ecab::mb_pcm_end(e, l, last);
      a_ok = false;
    } else if (ei4::is_i4_cmd(c)) {
      ecab::mb_intra4(e, idr, l, c, d.modes[mx], cp, last);
      a_ok = false;
    } else if (edb::is_intra_cmd(c)) {
      ecab::mb_intra16(e, idr, l, c, cp, last);
      a_ok = false;
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16), cbp = d.cbp[mx];
      if (mvx == 0 && mvy == 0 && cbp == 0) ecab::mb_skip(e, l, last);
      else ecab::mb_inter(e, l, mvx - (a_ok ? amx : 0), mvy - (a_ok ? amy : 0), cbp, cp, last);
      a_ok = true;
      amx = mvx;
      amy = mvy;
    }
  }
  e.sync();
}
void cabac_row(Sink &o, bool ring, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const RowData &d) {
  ecab::slice_header(o, idr, row * mbw, frame_num, 0, qp, dbk, 0, 0);
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, idr, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  if (ring) {
    std::vector<uint16_t> bins(ecab::kRingBins);
    ecab::BinRing<Sink> r{&e, bins.data(), 0};
    cabac_mbs(r, o, idr, mbw, d);
  } else {
    cabac_mbs(e, o, idr, mbw, d);
  }
  o.align();  // the flush ended in rbsp_stop_one_bit
}

// npic pictures of mbh rows (picture 0 IDR, the others P; frame_num = the index) as AVCC samples (4-byte
// lengths, one NAL unit per row) into out, their sizes into sizes.  cabac: 0 CAVLC, 1 the bins coded as they
// come, 2 through the kernel's BinRing.  row_data(p, row): the row's data.  Returns the bytes, -1 on overflow.
template <class F>
int64_t write_pictures(int mbw, int mbh, int npic, int qp, bool dbk, int cabac, F row_data, uint8_t *out, int64_t cap,
                       int64_t *sizes) {
  int64_t at = 0;
  const int64_t slot = 64 + static_cast<int64_t>(mbw) * ecab::kMbBytes;
  std::vector<uint8_t> buf(static_cast<size_t>(slot));
  for (int p = 0; p < npic; ++p) {
    const int64_t at0 = at;
    for (int row = 0; row < mbh; ++row) {
      const RowData d = row_data(p, row);
      Sink o{buf.data(), slot};
      if (cabac) cabac_row(o, cabac == 2, p == 0, row, mbw, p, qp, dbk, d);
      else cavlc_row(o, p == 0, row, mbw, p, qp, dbk, d);
      if (o.over || at + 4 + o.n > cap) return -1;
      out[at] = static_cast<uint8_t>(o.n >> 24);
      out[at + 1] = static_cast<uint8_t>(o.n >> 16);
      out[at + 2] = static_cast<uint8_t>(o.n >> 8);
      out[at + 3] = static_cast<uint8_t>(o.n);
      std::memcpy(out + at + 4, buf.data(), static_cast<size_t>(o.n));
      at += 4 + o.n;
    }
    sizes[p] = at - at0;
  }
  return at;
}
}  // namespace
