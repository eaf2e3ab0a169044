// The wavefront of the pair-HMM Viterbi recurrence (host/pairalign.hpp), stated once for the kernels that walk it:
// pair_align_fill_kernel (pair_align_kernels.hip), which files a choice word per cell for the traceback, and
// assign_score_kernel (assign_kernels.hip), which keeps S(I,O) only.  Both are bit-identical to alignPairHost.
//
// A wave owns a pair.  The rows of the matrix are taken in stripes of 64: lane l owns row 64 s + l and is skewed one column
// per lane, at step t it stands on column c0 + t - l (c0: the first column of the stripe's band).  S and D of the row above
// are what lane l - 1 computed one step earlier (lane shuffle), the diagonal S what it computed two steps earlier (the value
// shuffled at the step before, kept); the duplication lanes T_0 .. T_{P-1} of (ip, op - 1) never leave the lane's registers,
// the output base travels down the lanes with the scores.  Lane 63's S and D go to a boundary row of O + 1 columns -- in LDS
// while that fits, else in the wave's scratch in HBM -- from which lane 0 of the next stripe reads them: any band width and
// the full matrix are served.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "errors.hpp"
#include "host/pairalign.hpp"

namespace {

constexpr int kPaWavesPerBlock = 4;
constexpr int kPaLdsDoubles = 2048;                      // per wave: 16 substitution scores, then the boundary row
constexpr int kPaLdsCols = (kPaLdsDoubles - 16) / 2;     // columns (O + 1) a boundary row in LDS holds at most

struct PaScores {
  double delOpen, tanDup, noGap, delExtend, delEnd;
  double len[dnas::kAlignMaxLen];
  int P;
  static PaScores from(const dnas::PairScores& hs) {
    PaScores sc{};
    sc.delOpen = hs.delOpen; sc.tanDup = hs.tanDup; sc.noGap = hs.noGap; sc.delExtend = hs.delExtend; sc.delEnd = hs.delEnd;
    for (int k = 0; k < dnas::kAlignMaxLen; ++k) sc.len[k] = hs.len[k];
    sc.P = hs.P;
    return sc;
  }
};

// What fill and traceback agree on: the band as host/pairalign.hpp defines it, and where a cell's choice word lies.
struct PaGeom {
  int lo, hi, stepsMax, stripes;
  __host__ __device__ PaGeom(int I, int O, int band) {
    const int b = band < 0 || band > I + O + 1 ? I + O + 1 : band;
    lo = (O < I ? O - I : 0) - b;
    hi = (O > I ? O - I : 0) + b;
    // a stripe of rows r0 .. r0 + 63 runs from column c0 = rowLo(r0) to rowHi(r0 + 63), lane 63 another 63 steps behind
    const long w = (long)hi - lo + 1 + 126, f = (long)O + 64;
    stepsMax = (int)(w < f ? w : f);
    stripes = I / 64 + 1;
  }
  __host__ __device__ int rowLo(int ip) const { return ip + lo > 0 ? ip + lo : 0; }
  __host__ __device__ int rowHi(int ip, int O) const { return ip + hi < O ? ip + hi : O; }
  __host__ __device__ size_t words() const { return (size_t)stripes * (size_t)stepsMax * 64; }
  __host__ __device__ size_t wordAt(int ip, int op) const {
    const int s = ip >> 6, l = ip & 63;
    return ((size_t)s * (size_t)stepsMax + (size_t)(op - rowLo(s << 6) + l)) * 64 + (size_t)l;
  }
};

__device__ inline double paNegInf() { return -__builtin_huge_val(); }

// One pair, by the 64 lanes of one wave: a[0..I) against b[0..O), or with rev against the reverse complement of b, read in
// place (base j of it is 3 - b[O-1-j]).  sub: the wave's 16 substitution scores in LDS; bndLds: its boundary row there, of
// ldsCols columns; bndMem: the one in HBM, used when O + 1 > ldsCols.  RECORD: one 16-bit choice word per cell goes to rec
// (bits 0-1: S took s0 / s1 / s2, bit 2: D took d1, bit 3 + k: T_k took t1), filed under (stripe, step, lane): a wave's store
// is 128 consecutive bytes.  The lane that stands on (I, O) writes S(I,O) to *scoreOut; that is every pair's last store.
template <int KP, bool RECORD>
__device__ __forceinline__ void paFillPair(const PaScores& sc, const double* sub, double* bndLds, int ldsCols, double* bndMem,
                                           int lane, int band, const int8_t* a, int I, const int8_t* b,
                                           int O, bool rev, uint16_t* rec, double* scoreOut) {
  const double NEG = paNegInf();
  const int P = sc.P;
  const PaGeom g(I, O, band);
  const bool useLds = O + 1 <= ldsCols;

  for (int s = 0; s < g.stripes; ++s) {
    const int r0 = s << 6, r = r0 + lane;
    const bool row = r <= I;
    const int rlo = row ? g.rowLo(r) : 1, rhi = row ? g.rowHi(r, O) : 0;
    const int c0 = g.rowLo(r0);
    const int last = I - r0 < 63 ? I - r0 : 63;
    const int tmax = g.rowHi(r0 + last, O) - c0 + last;
    const int ulo = g.rowLo(r0 - 1), uhi = g.rowHi(r0 - 1, O);     // the row above the stripe (s > 0)
    const int kmax = row ? (r < P ? r : P) : 0;
    unsigned ctx = 0;                                              // in[r-1-k] at bits 2k: the bases this row compares with
#pragma unroll
    for (int k = 0; k <= KP; ++k)
      if (row && r - 1 - k >= 0) ctx |= ((unsigned)a[r - 1 - k] & 3u) << (2 * k);
    double T[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) T[k] = NEG;
    double Sdiag = NEG, pubS = NEG, pubD = NEG;
    int ypub = 0, ychunk = 0;
    if (lane == 0 && s > 0 && c0 >= 1)
      Sdiag = useLds ? bndLds[2 * (c0 - 1)]
                     : __hip_atomic_load(bndMem + 2 * (size_t)(c0 - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint16_t* recStripe = nullptr;
    if (RECORD) recStripe = rec + (size_t)s * (size_t)g.stepsMax * 64 + lane;

    for (int t = 0; t <= tmax; ++t) {
      if ((t & 63) == 0) {                                         // the next 64 output bases lane 0 will hand down
        const int j = c0 + t - 1 + lane;
        ychunk = j >= 0 && j < O ? (rev ? 3 - ((int)b[O - 1 - j] & 3) : (int)b[j] & 3) : 0;
      }
      double Sup = __shfl_up(pubS, 1), Dup = __shfl_up(pubD, 1);
      int y = __shfl_up(ypub, 1);
      const int y0 = __shfl(ychunk, t & 63);
      const int op = c0 + t - lane;
      if (lane == 0) {
        y = y0;
        Sup = Dup = NEG;
        if (s > 0 && op >= ulo && op <= uhi) {
          if (useLds) {
            Sup = bndLds[2 * op];
            Dup = bndLds[2 * op + 1];
          } else {
            Sup = __hip_atomic_load(bndMem + 2 * (size_t)op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            Dup = __hip_atomic_load(bndMem + 2 * (size_t)op + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      const bool active = op >= rlo && op <= rhi;
      double S = NEG, D = NEG;
      if (active) {
        unsigned word = 0;
        double c;
        c = Sup + sc.delOpen;
        if (c > D) D = c;
        c = Dup + sc.delExtend;
        if (c > D) { D = c; word = 4u; }
        if (r == 0 && op == 0) {
          S = 0;
        } else {
          const double sub0 = sub[(ctx & 3u) * 4 + y];
          c = Sdiag + sc.noGap + sub0;
          if (c > S) S = c;
          c = T[0] + sub0;
          if (c > S) { S = c; word = (word & ~3u) | 1u; }
          c = D + sc.delEnd;
          if (c > S) { S = c; word = (word & ~3u) | 2u; }
        }
        const double open = S + sc.tanDup;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          double best = NEG;
          if (k + 1 < KP) {
            c = T[k + 1] + sub[((ctx >> (2 * k + 2)) & 3u) * 4 + y];
            if (c > best) best = c;
          }
          c = open + sc.len[k];
          if (c > best) { best = c; word |= 8u << k; }
          T[k] = k < kmax ? best : NEG;
        }
        if (RECORD) recStripe[(size_t)t * 64] = (uint16_t)word;
        if (lane == 63) {
          if (useLds) {
            bndLds[2 * op] = S;
            bndLds[2 * op + 1] = D;
          } else {
            __hip_atomic_store(bndMem + 2 * (size_t)op, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(bndMem + 2 * (size_t)op + 1, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        if (r == I && op == O) *scoreOut = S;
      }
      Sdiag = Sup;
      pubS = S;
      pubD = D;
      ypub = y;
    }
    // the next stripe's lane 0 reads what this stripe's lane 63 wrote
    if (useLds) __builtin_amdgcn_wave_barrier();
    else __threadfence();
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct PaBuffers {
  std::vector<void*> mem;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~PaBuffers() {
    for (void* q : mem) (void)hipFree(q);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

#define PA_TRY(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return dnas::fail(DNAS_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
int paAlloc(PaBuffers& bufs, T** out, size_t n) {
  void* q = nullptr;
  PA_TRY(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  bufs.mem.push_back(q);
  *out = (T*)q;
  return DNAS_OK;
}

template <class T>
int paUpload(PaBuffers& bufs, T** out, const T* src, size_t n) {
  if (const int rc = paAlloc(bufs, out, n)) return rc;
  if (n) PA_TRY(hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice));
  return DNAS_OK;
}

}  // namespace
