// CPU harness of the device encoder's CABAC writer (enc_cabac.h, the header
// the enc_write_cabac kernel calls):
//   ech_engine:    a sequence of decisions, bypass and terminate bins, raw
//                  bytes and restarts through ecab::Encoder into a ByteSink;
//   ech_contexts:  the 277 context variables of 9.3.1.1;
//   ech_sps_pps:   make_sps_pps (synth.cpp) with and without CABAC;
//   ech_pictures:  macroblock rows (command words, coded_block_pattern,
//                  levels, I_PCM samples: what a level of transcode.hip holds)
//                  written as slices, one per row, through enc_cabac.h's
//                  mb_* functions or, as CAVLC, through enc_cavlc.h's: the
//                  code the enc_write kernel calls, walked in its order
//                  (enc_rows.h);
//   ech_sinks:     one CAVLC slice through the byte sink and through the
//                  kernel's dword sink (enc_rbsp.h) into bounded buffers.
// TEST INFRASTRUCTURE (tests/test_enc_cabac_host.py; enc_cabac_main.cpp runs
// the same functions under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_rows.h"
#include "h264.h"

using namespace vts;

// ops: n triples (kind, a, b): 0 decision(ctx a, bin b), 1 bypass(b), 2 terminate(b), 3 raw byte a,
// 4 alignment zero bits, 5 restart (InitEncoder; the contexts stay).  Returns the bytes, -1 on overflow.
extern "C" int64_t ech_engine(const int32_t *ops, int64_t n, int islice, int qp, uint8_t *out, int64_t cap) {
  Sink o{out, cap};
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, islice != 0, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  for (int64_t i = 0; i < n; ++i) {
    const int k = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
    if (k == 0) e.decision(a, b);
    else if (k == 1) e.bypass(b);
    else if (k == 2) e.terminate(b);
    else if (k == 3) o.byte(static_cast<uint32_t>(a));
    else if (k == 4) o.align();
    else e.start();
  }
  o.align();
  return o.over ? -1 : o.n;
}

extern "C" void ech_contexts(int islice, int qp, uint8_t *st) { ecab::init_contexts(st, islice != 0, qp); }

#ifndef ECH_NO_SPS_PPS  // enc_cabac_main.cpp links no stream writer
// SPS / PPS NAL units (each at most 64 bytes) of an mbw x mbh picture; sizes in n[0], n[1]
extern "C" void ech_sps_pps(int mbw, int mbh, int cabac, uint8_t *sps, uint8_t *pps, int32_t *n) {
  std::vector<uint8_t> s, p;
  make_sps_pps(mbw, mbh, 0, 0, 30, &s, &p, 0, cabac != 0);
  std::memcpy(sps, s.data(), s.size());
  std::memcpy(pps, p.data(), p.size());
  n[0] = static_cast<int32_t>(s.size());
  n[1] = static_cast<int32_t>(p.size());
}
#endif

// npic pictures of mbh rows of mbw macroblocks (picture 0 IDR, the others P; frame_num = the index): one
// AVCC sample each (4-byte lengths, one NAL unit per row) into out, their sizes into sizes.  cabac: 0 CAVLC,
// 1 the bins coded as they come, 2 through the kernel's BinRing.  cmd / cbp:
// [pic][row][mx], coef: ... [384], pcm: ... [384] samples >= 1.  Returns the bytes, -1 on overflow.
extern "C" int64_t ech_pictures(int mbw, int mbh, int npic, int qp, int dbk, int cabac, const uint32_t *cmd,
                                const uint8_t *cbp, const int16_t *coef, const uint8_t *pcm, uint8_t *out,
                                int64_t cap, int64_t *sizes) {
  auto row_data = [&](int p, int row) {
    const int64_t r = (static_cast<int64_t>(p) * mbh + row) * mbw;
    return RowData{cmd + r, cbp + r, coef + r * kCoefPerMb, nullptr, pcm + r * 384};
  };
  return write_pictures(mbw, mbh, npic, qp, dbk != 0, cabac, row_data, out, cap, sizes);
}

// One CAVLC slice of mbw macroblocks through the byte sink into bytes[0, cap) and through the kernel's dword
// sink into words[0, cap / 4) (cap: a multiple of 4, or short of the slice, as in the kernel, where the last
// partial word is stored whole).  res: the byte sink's length and overflow flag, then the dword sink's.  pcm
// may hold any bytes, zeros included: they pass through emulation prevention like the rest.
extern "C" void ech_sinks(int idr, int mbw, int qp, int dbk, const uint32_t *cmd, const uint8_t *cbp,
                          const int16_t *coef, const uint8_t *pcm, int64_t cap, uint8_t *bytes, uint32_t *words,
                          int64_t *res) {
  const RowData d{cmd, cbp, coef, nullptr, pcm};
  Sink b{bytes, cap};
  cavlc_row(b, idr != 0, 3, mbw, idr ? 0 : 5, qp, dbk != 0, d);
  b.flush();
  erbsp::WordSink w = erbsp::word_sink(words, cap);
  cavlc_row(w, idr != 0, 3, mbw, idr ? 0 : 5, qp, dbk != 0, d);
  w.flush();
  res[0] = b.n;
  res[1] = b.over;
  res[2] = w.n;
  res[3] = w.over;
}
