// The sum-product cell of the forward walk (paWalkForward, pair_align_device.h): the forward score of host/pairforward.hpp on
// the wavefront of that file.  PaGeom, the walk, the launch plan, the chunk loop and the buffers are the shared ones; only the
// cell differs: where the Viterbi cell compares, this one calls lse, the reference's table function (host/lsetable.hpp),
// bit-identical to forwardPairHost in table mode.
// The two-pass kernels run that cell (pair_counts_device.h); the two forward score kernels run paForwardScorePair, the walk and
// the cell kept by hand in one function at the end of this file, for the reason given there.
//
// The table (800 KB, L2 resident) comes in as a const double* __restrict__ and is read through a buffer descriptor made of it.
// A cell carries a chain of three dependent look-ups (D, then the two of S); the KP look-ups of the T_k behind them do not
// depend on each other: their indices are all formed first, then the loads are issued together, then the interpolations finish.
// A lane whose difference is 10 or more (or whose operands are both -inf) takes no load: its offset lies beyond the
// descriptor's bounds.
#pragma once
#include "host/lsetable.hpp"
#include "pair_align_device.h"

namespace {

// x / .0001 correctly rounded without the division sequence (Markstein: q0 = x * r, the residual x - c * q0 is exact in one
// fma, q = q0 + e * r with r the correctly rounded reciprocal), as fwdback_onchip.hip has it.  For a residual that underflows
// (x below 1e-280) q may differ from the quotient in its last bits, which neither use below sees: (int) of it is 0, and
// f0 + df * q with f0 >= 4.5e-5 and df * q < 1e-280 is f0.
__device__ __forceinline__ double pfDivStep(double x) {
  constexpr double c = .0001, r = 1.0 / .0001;
  const double q0 = x * r;
  const double e = __builtin_fma(-c, q0, x);
  return __builtin_fma(e, r, q0);
}

// lse(a, b) = max + f(max - min) in three parts, so that several can be in flight: the index, the load, the finish.
// max - min is NaN for two -inf and +inf for one: both are "no look-up, f = 0", like every difference from 10 on.  The table is
// read the buffer way, as fwdback_onchip.hip reads it: its base in scalar registers, one 16-byte load for the two neighbouring
// entries, no 64-bit address arithmetic per look-up; a lane without a look-up gives an offset beyond the table, for which the
// hardware returns zeros without touching memory -- f0 + (f1 - f0) * q is then the 0 the function asks for.
typedef __amdgpu_buffer_rsrc_t pf_rsrc_t;
typedef double pf_dbl2 __attribute__((ext_vector_type(2)));
constexpr int kPfNoLookup = -16;             // as an unsigned byte offset: beyond any table

__device__ __forceinline__ pf_rsrc_t pfTable(const double* __restrict__ tab) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(tab), 0, dnas::kLseTableSize * 8, 0x00020000);
}

struct PfLse {
  double mx, dx;
  pf_dbl2 f;
  int off;
  __device__ __forceinline__ void index(double a, double b) {
    double mn;       // (the instructions themselves: no NaN comes in, so the canonicalising copies around fmax / fmin are waste)
    asm("v_max_f64 %0, %1, %2" : "=v"(mx) : "v"(a), "v"(b));
    asm("v_min_f64 %0, %1, %2" : "=v"(mn) : "v"(a), "v"(b));
    const double x = mx - mn;
    const bool in = x < 10.;
    const double xs = in ? x : 0.;
    const int n = (int)pfDivStep(xs);          // (int)(x / .0001), at most 99 999: entries n and n + 1 exist
    dx = xs - (n * .0001);
    off = in ? n * 8 : kPfNoLookup;
  }
  __device__ __forceinline__ void load(pf_rsrc_t tab) {
    f = __builtin_bit_cast(pf_dbl2, __builtin_amdgcn_raw_buffer_load_b128(tab, off, 0, 0));   // tab[n], tab[n + 1]
  }
  __device__ __forceinline__ double finish() const {
    const double df = f.y - f.x;
    return mx + (f.x + df * pfDivStep(dx));    // f0 + df * (dx / .0001)
  }
};

__device__ __forceinline__ double pfLse(pf_rsrc_t tab, double a, double b) {
  PfLse q;
  q.index(a, b);
  q.load(tab);
  return q.finish();
}

// What the sum-product cell does with a finished cell besides handing it on: nothing here, which leaves the score kernels the
// instances they are; pair_counts_device.h parks the cell for its backward pass.
struct PfNoPark {
  template <int KP>
  __device__ __forceinline__ void cell(int, int, int, int, int, double, double, const double (&)[KP]) {}
};

// The sum-product cell of paWalkForward: where the Viterbi cell compares, this one calls lse.  A lane the row does not have
// (k >= kmax) takes no look-up and leaves T_k = -inf.  park.cell<KP>(stripe, step, r, op, kmax, S, D, T) is called with the
// finished cell.
template <class Park = PfNoPark>
struct PaForwardCell {
  pf_rsrc_t tab;
  Park park;
  template <int KP>
  __device__ __forceinline__ void update(const PaScores& sc, const double* sub, double Sup, double Dup, double Sdiag, double (&T)[KP],
                                         unsigned ctx, int y, int kmax, bool origin, int s, int t, int r, int op, double& S,
                                         double& D) {
    const double NEG = paNegInf();
    D = pfLse(tab, Sup + sc.delOpen, Dup + sc.delExtend);
    if (origin) {
      S = 0;
    } else {
      const double sub0 = sub[(ctx & 3u) * 4 + y];
      S = pfLse(tab, pfLse(tab, Sdiag + sc.noGap + sub0, T[0] + sub0), D + sc.delEnd);
    }
    const double open = S + sc.tanDup;
    PfLse q[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const double t0 = k + 1 < KP ? T[k + 1] + sub[((ctx >> (2 * k + 2)) & 3u) * 4 + y] : NEG;
      q[k].index(t0, open + sc.len[k]);
      if (!(k < kmax)) q[k].off = kPfNoLookup;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) q[k].load(tab);
#pragma unroll
    for (int k = 0; k < KP; ++k) T[k] = k < kmax ? q[k].finish() : NEG;
    park.template cell<KP>(s, t, r, op, kmax, S, D, T);
  }
};

// The forward score kernels' pair, on a hand-kept body: pair_forward_score_kernel and consensus_forward_kernel.  Under
// paWalkForward with PaForwardCell<> their step loops have the same instructions but for three (one address add folded away, the
// boundary row's LDS offset, the (0,0) test) in another order, and at KP = 2 and 13 they measured 0.4 % slower than this text,
// which is beyond its own spread of 0.3 % (profiles/EXPERIMENTS.md).  This is the walk of paWalkForward and the cell of
// PaForwardCell written out in one function, (stripe, step, lane) as PaStripe has them; it compiles to the instructions these
// kernels had before the walk was shared.  The two-pass kernels (pair_counts_device.h) are on the shared walk.
struct PaForwardScoreCell {
  const double* __restrict__ tab;
};

template <int KP>
__device__ __forceinline__ void paForwardScorePair(const PaScores& sc, const double* __restrict__ lseTab, const double* sub, double* bndLds,
                                              int ldsCols, double* bndMem, int lane, int band, const int8_t* a, int I,
                                              const int8_t* b, int O, bool rev, double* scoreOut) {
  const double NEG = paNegInf();
  const int P = sc.P;
  const PaGeom g(I, O, band);
  const bool useLds = O + 1 <= ldsCols;
  const pf_rsrc_t tab = pfTable(lseTab);

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
        D = pfLse(tab, Sup + sc.delOpen, Dup + sc.delExtend);
        if (r == 0 && op == 0) {
          S = 0;
        } else {
          const double sub0 = sub[(ctx & 3u) * 4 + y];
          S = pfLse(tab, pfLse(tab, Sdiag + sc.noGap + sub0, T[0] + sub0), D + sc.delEnd);
        }
        const double open = S + sc.tanDup;
        PfLse q[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const double t0 = k + 1 < KP ? T[k + 1] + sub[((ctx >> (2 * k + 2)) & 3u) * 4 + y] : NEG;
          q[k].index(t0, open + sc.len[k]);
          if (!(k < kmax)) q[k].off = kPfNoLookup;                   // a lane the row does not have: no look-up, T_k = -inf below
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) q[k].load(tab);
#pragma unroll
        for (int k = 0; k < KP; ++k) T[k] = k < kmax ? q[k].finish() : NEG;
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

// paScoreChunk's pair under PaForwardScoreCell: the hand-kept body instead of the shared walk.
template <int KP>
__device__ __forceinline__ void paScorePair(const PaScores& sc, double* sub, int ldsCols, double* bndMem, int lane, int band,
                                            const PaItem& it, double* scoreOut, PaForwardScoreCell& cell) {
  paForwardScorePair<KP>(sc, cell.tab, sub, sub + 16, ldsCols, bndMem, lane, band, it.a, it.I, it.b, it.O, it.rev, scoreOut);
}

}  // namespace
