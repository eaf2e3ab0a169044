// One step of the Viterbi traceback, stated once for host and device: the node record's layout, and the candidates of a
// walk standing on (state, pos, mut) in the reference's order (viterbi.cpp:217-228,247-301):
//   from an S cell            emit in-edges, null in-edges, own D, own T1, the local start
//   from a D cell             per emit in-edge D then S, then the null in-edges' D
//   from duplication lane k   T(k+1) one column back, then S
// and the first strictly greater candidate wins -- that part is the drivers' (viterbi_kernels.hip).  The kernels and
// tools/traceback_host_check.cpp (a sanitizer build on the CPU) compile this text.
#pragma once
#include <stdint.h>

#include "device_model.h"

#if defined(__HIP__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif
#define DNAS_TB_FN DNAS_HD inline __attribute__((always_inline))

// Everything a step needs to know about a state in one 64-byte line (DevModel::rec).
//   word 0         emit in-edges (bits 0-3), null in-edges (bits 4-7) -- kNotInline: more than the record holds, step through
//                  the CSR arrays --, mdl (bits 8-11), the left context's bases (bits 12-19, 2 each)
//   word 1         the state's lattice slot
//   words 2+3e ..  in-edge e (0 .. kRecEmit-1 emitting, kNullEdge the null one): source state, its lattice slot,
//                  input symbol | emitted base << 8 | score index << 16, the score being DevModel::recScore[index]
// No accessor indexes w[] by a run-time value: edge(e, f) selects among constants, and folds where e is one.
struct alignas(16) NodeRecord {
  static constexpr unsigned kNotInline = 15;
  static constexpr int kNullEdge = kRecEmit;
  uint32_t w[16];

  DNAS_TB_FN unsigned emitCount() const { return w[0] & 15u; }
  DNAS_TB_FN unsigned nullCount() const { return (w[0] >> 4) & 15u; }
  DNAS_TB_FN bool isInline() const { return emitCount() != kNotInline && nullCount() != kNotInline; }
  DNAS_TB_FN int mdl() const { return (int)((w[0] >> 8) & 15u); }
  DNAS_TB_FN unsigned ctxBits() const { return (w[0] >> 12) & 0xffu; }
  DNAS_TB_FN int ctx(int q) const { return (int)((ctxBits() >> (2 * q)) & 3u); }
  DNAS_TB_FN int ownSlot() const { return (int)w[1]; }
  DNAS_TB_FN uint32_t edge(int e, int f) const { return e == 0 ? w[2 + f] : e == 1 ? w[5 + f] : e == 2 ? w[8 + f] : w[11 + f]; }
  DNAS_TB_FN int src(int e) const { return (int)edge(e, 0); }
  DNAS_TB_FN int slot(int e) const { return (int)edge(e, 1); }
  DNAS_TB_FN uint8_t in(int e) const { return (uint8_t)(edge(e, 2) & 255u); }
  DNAS_TB_FN uint8_t base(int e) const { return (uint8_t)((edge(e, 2) >> 8) & 255u); }
  DNAS_TB_FN unsigned scoreIndex(int e) const { return (edge(e, 2) >> 16) & 255u; }

  // Host: the record of state j of a model whose pointers (einSlot, ninSlot, slotOf included) are host memory.
  // scoreIndex(v) names an edge score by a byte; below 0 it cannot, and the model gets no records: false.
  template <class ScoreIndex>
  static bool pack(const DevModel& h, int j, ScoreIndex&& scoreIndex, NodeRecord& r) {
    const int e0 = h.einPtr[j], ne = h.einPtr[j + 1] - e0, n0 = h.ninPtr[j], nn = h.ninPtr[j + 1] - n0;
    uint32_t ctxBits = 0;
    for (int q = 0; q < h.D; ++q) ctxBits |= (uint32_t)(h.ctx[(size_t)j * h.D + q] & 3u) << (2 * q);
    for (uint32_t& x : r.w) x = 0;
    r.w[0] = (uint32_t)(ne > kRecEmit ? kNotInline : ne) | (uint32_t)(nn > kRecNull ? kNotInline : nn) << 4 | (uint32_t)h.mdl[j] << 8 | ctxBits << 12;
    r.w[1] = (uint32_t)(h.slotOf ? h.slotOf[j] : j);
    for (int i = 0; i < ne && ne <= kRecEmit; ++i) {
      const int k = scoreIndex(h.einScore[e0 + i]);
      if (k < 0) return false;
      uint32_t* const w = r.w + 2 + 3 * i;
      w[0] = (uint32_t)h.einSrc[e0 + i];
      w[1] = (uint32_t)h.einSlot[e0 + i];
      w[2] = (uint32_t)h.einIn[e0 + i] | (uint32_t)h.einBase[e0 + i] << 8 | (uint32_t)k << 16;
    }
    for (int i = 0; i < nn && nn <= kRecNull; ++i) {
      const int k = scoreIndex(h.ninScore[n0 + i]);
      if (k < 0) return false;
      uint32_t* const w = r.w + 2 + 3 * (kNullEdge + i);
      w[0] = (uint32_t)h.ninSrc[n0 + i];
      w[1] = (uint32_t)h.ninSlot[n0 + i];
      w[2] = (uint32_t)h.ninIn[n0 + i] | (uint32_t)k << 16;
    }
    return true;
  }
};
static_assert(sizeof(NodeRecord) == 64 && kRecEmit == 3 && kRecNull == 1, "edge(e, f) spells the record's four in-edges out");

// A candidate of a step: the lattice cell it reads, and what the walk takes along if it wins.
struct TbCand {
  int state, slot, pos, lane;   // cell (pos, lane) of `state`, which lives in lattice slot `slot`
  double trans;                 // transition score: the candidate's value is cell + trans
  uint8_t in;                   // input symbol decoded on the way (0: none)
  uint8_t emit;                 // 1 + the base an emit in-edge emitted, else 0
  bool other;                   // an in-edge's source: another state than the one the walk stands on
};

// An in-edge as a source of candidates reads it.
struct TbEdge {
  int src, slot;
  double score;
  uint8_t in, base;
};

// The in-edges of a state from its node record.  The walk declines mut == 0 && pos == 0 in a local model beforehand
// (the local start is no candidate here), and states whose record is not inline.
struct TbRecordEdges {
  static constexpr bool kFull = false;   // neither the local start nor TbCand::emit (nothing logs events on this path)
  const NodeRecord& r;
  const double* recScore;
  DNAS_TB_FN int emitCount() const { return (int)r.emitCount(); }
  DNAS_TB_FN int nullCount() const { return (int)r.nullCount(); }
  DNAS_TB_FN int mdl() const { return r.mdl(); }
  DNAS_TB_FN int ownSlot() const { return r.ownSlot(); }
  DNAS_TB_FN int ctx(int q) const { return r.ctx(q); }
  DNAS_TB_FN TbEdge emitEdge(int i) const { return TbEdge{r.src(i), r.slot(i), recScore[r.scoreIndex(i)], r.in(i), r.base(i)}; }
  DNAS_TB_FN TbEdge nullEdge(int) const {
    constexpr int e = NodeRecord::kNullEdge;
    return TbEdge{r.src(e), r.slot(e), recScore[r.scoreIndex(e)], r.in(e), 0};
  }
};

// The same through the CSR arrays: the state's row pointers, mdl and lattice slot as the caller fetched them, and
// ctxAt(q), the context's base q (the thread-per-read walk reads m.ctx, the wave-per-read walk a lane of its wave).
template <class Ctx>
struct TbCsrEdges {
  static constexpr bool kFull = true;
  const DevModel& m;
  int e0, e1, n0, n1, mdl_, slot_;
  Ctx ctxAt;
  DNAS_TB_FN int emitCount() const { return e1 - e0; }
  DNAS_TB_FN int nullCount() const { return n1 - n0; }
  DNAS_TB_FN int mdl() const { return mdl_; }
  DNAS_TB_FN int ownSlot() const { return slot_; }
  DNAS_TB_FN int ctx(int q) const { return ctxAt(q); }
  DNAS_TB_FN TbEdge emitEdge(int i) const {
    const int e = e0 + i;
    return TbEdge{m.einSrc[e], m.einSlot[e], m.einScore[e], m.einIn[e], m.einBase[e]};
  }
  DNAS_TB_FN TbEdge nullEdge(int i) const {
    const int e = n0 + i;
    return TbEdge{m.ninSrc[e], m.ninSlot[e], m.ninScore[e], m.ninIn[e], 0};
  }
};

// The candidates of the walk standing on (state, pos, mut), count() of them, at(c) in the reference's order.
// sub, len: the model's tables wherever the caller keeps them (the kernels: LDS).  x: the read's base before column
// pos.  The one context base a step can need is read when the step is built -- by every lane of a wave alike.
template <class Edges>
struct TbStep {
  const DevModel& m;
  const double *sub, *len;
  Edges ed;
  int state, pos, mut, x;
  int nE, nN, slot, ctxBase;
  bool hasT1, deeper, start;

  DNAS_TB_FN TbStep(const DevModel& m_, const double* sub_, const double* len_, const Edges& ed_, int state_, int pos_, int mut_, int x_)
      : m(m_), sub(sub_), len(len_), ed(ed_), state(state_), pos(pos_), mut(mut_), x(x_) {
    nE = mut == 0 ? (pos > 0 ? ed.emitCount() : 0) : mut == 1 ? ed.emitCount() : 0;   // no column before the first
    nN = mut < 2 ? ed.nullCount() : 0;
    slot = ed.ownSlot();
    hasT1 = mut == 0 && ed.mdl() > 0 && pos > 0;
    deeper = mut >= 2 && mut - 2 < ed.mdl() - 1;
    start = Edges::kFull && mut == 0 && pos == 0 && m.local;
    ctxBase = hasT1 ? ed.ctx(0) : deeper ? ed.ctx(mut - 1) : 0;
  }

  // The list below as runs of like candidates, f(first, n) for each in turn: a driver that gathers one kind at a time
  // (a thread per read) asks at() for first .. first + n - 1.
  template <class F>
  DNAS_TB_FN void runs(F&& f) const {
    if (mut == 0) {
      f(0, nE);
      f(nE, nN);
      f(nE + nN, 1 + (hasT1 ? 1 : 0) + (start ? 1 : 0));
    } else if (mut == 1) {
      f(0, 2 * nE);
      f(2 * nE, nN);
    } else {
      f(0, deeper ? 2 : 1);
    }
  }
  DNAS_TB_FN int count() const {
    int total = 0;
    runs([&](int, int n) { total += n; });
    return total;
  }

  DNAS_TB_FN TbCand own(int ps, int lane, double trans) const { return TbCand{state, slot, ps, lane, trans, 0, 0, false}; }
  DNAS_TB_FN static uint8_t emitOf(const TbEdge& e) { return Edges::kFull ? (uint8_t)(1 + e.base) : 0; }

  DNAS_TB_FN TbCand at(int c) const {
    if (mut == 0) {
      if (c < nE) {
        const TbEdge e = ed.emitEdge(c);
        return TbCand{e.src, e.slot, pos - 1, 0, (e.score + m.noGap) + sub[e.base * 4 + x], e.in, emitOf(e), true};
      }
      c -= nE;
      if (c < nN) {
        const TbEdge e = ed.nullEdge(c);
        return TbCand{e.src, e.slot, pos, 0, e.score, e.in, 0, true};
      }
      c -= nN;
      if (c == 0) return own(pos, 1, m.delEnd);
      if (c == 1 && hasT1) return own(pos - 1, 2, sub[ctxBase * 4 + x]);
      return TbCand{0, m.slotOf ? m.slotOf[0] : 0, 0, 0, 0., 0, 0, true};   // the local start
    }
    if (mut == 1) {
      if (c < 2 * nE) {
        const TbEdge e = ed.emitEdge(c >> 1);
        const bool fromD = (c & 1) == 0;
        return TbCand{e.src, e.slot, pos, fromD ? 1 : 0, e.score + (fromD ? m.delExtend : m.delOpen), e.in, emitOf(e), true};
      }
      const TbEdge e = ed.nullEdge(c - 2 * nE);
      return TbCand{e.src, e.slot, pos, 1, e.score, e.in, 0, true};
    }
    if (deeper && c == 0) return own(pos - 1, mut + 1, sub[ctxBase * 4 + x]);
    return own(pos, 0, m.tanDup + len[mut - 2]);
  }
};

using TbRecordStep = TbStep<TbRecordEdges>;
template <class Ctx>
using TbCsrStep = TbStep<TbCsrEdges<Ctx>>;

DNAS_TB_FN TbRecordStep tbRecordStep(const DevModel& m, const double* sub, const double* len, const NodeRecord& r, int state, int pos, int mut, int x) {
  return TbRecordStep(m, sub, len, TbRecordEdges{r, m.recScore}, state, pos, mut, x);
}
template <class Ctx>
DNAS_TB_FN TbCsrStep<Ctx> tbCsrStep(const DevModel& m, const double* sub, const double* len, int e0, int e1, int n0, int n1, int mdl, int slot,
                                    const Ctx& ctxAt, int state, int pos, int mut, int x) {
  return TbCsrStep<Ctx>(m, sub, len, TbCsrEdges<Ctx>{m, e0, e1, n0, n1, mdl, slot, ctxAt}, state, pos, mut, x);
}
