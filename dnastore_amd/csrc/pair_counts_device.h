// Posterior move counts of a pair over its whole band (host/paircounts.hpp), by the 64 lanes of one wave in two passes over the
// wavefront of pair_align_device.h.
//
// Pass 1 is paWalkForward under the sum-product cell with a park policy: every finished cell's S, D and T_0 .. T_{P-1} go to
// the wave's scratch in HBM, filed by (stripe, step, lane) as PaGeom::wordAt files a choice word, one plane of PaGeom::words()
// doubles per value: a wave's store of one value is 512 consecutive bytes.  The lane on (I,O) keeps Z in a register.
//
// Pass 2 is the mirror image: stripes last to first, steps tmax down to 0, each lane on the cell it stood on in pass 1 at that
// (stripe, step), so it meets its own parked cell.  B_S and B_D of the row below are what lane l + 1 computed one step earlier
// (__shfl_down), the diagonal B_S what it computed two steps earlier (kept), B_S and the B_T lanes of (ip, op + 1) never leave
// the lane's registers.  Lane 0's B_S and B_D go to the boundary row (LDS while O + 1 <= ldsCols, else the wave's HBM row), from
// which the last lane of the stripe above reads them.  The output base out[op] is handed up the lanes from the stripe's last
// row.  B_S is a tree of KP + 2 leaves (-inf for the lanes a row does not have: not a bit changes, paircounts.hpp), each level's
// look-ups issued together.  The lane then forms the 4 + 2 KP posteriors of the moves out of its cell.
//
// Accumulators are private to a lane: 5 + KP in registers, the 16 data-indexed substitution counters in LDS slots [16][64].  At
// the end of a pair the lanes are summed in a fixed tree (l takes l + 32, 16, 8, 4, 2, 1) and lane 0 writes the pair's slot:
// 21 + P counts, Z, B_S(0,0).  No atomics.
//
// What pass 2 does with the posteriors is a policy: PcTotals is the paragraph above (pair_counts_kernel), PcProfile files them
// per row of the original instead (pair_profile_kernel, csrc/pair_profile_kernels.hip).
#pragma once
#include "pair_forward_device.h"

namespace {

constexpr int kPcSubSlots = 16 * 64;                                  // per wave: nSub[16] per lane
constexpr int kPcLdsCols = (kPaLdsDoubles - 16 - kPcSubSlots) / 2;    // a block of 4 waves stays within 64 KiB of LDS
constexpr int kPpMatchSlots = 4 * 64;                                 // per wave, the profile kernel: match by y per lane
constexpr int kPpLdsCols = (kPaLdsDoubles - 16 - kPpMatchSlots) / 2;  // the same 64 KiB: its boundary row stays in LDS longer

// Pass 1's policy: park the cell, keep Z.
struct PcPark {
  double* scr;          // this lane's column of the wave's scratch
  size_t words;
  int stepsMax, P, I, O;
  double z;
  template <int KP>
  __device__ __forceinline__ void cell(int s, int t, int r, int op, int, double S, double D, const double (&T)[KP]) {
    double* p = scr + ((size_t)s * (size_t)stepsMax + (size_t)t) * 64;
    p[0] = S;
    p[words] = D;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < P) p[(size_t)(2 + k) * words] = T[k];
    if (r == I && op == O) z = S;
  }
};

// tree(v_0 .. v_{N-1}): neighbours combined level by level, an odd last element carried up.
template <int N>
__device__ __forceinline__ double pcTree(pf_rsrc_t tab, const double (&v)[N]) {
  if constexpr (N == 1) {
    return v[0];
  } else {
    constexpr int H = N / 2, M = (N + 1) / 2;
    PfLse q[H];
#pragma unroll
    for (int i = 0; i < H; ++i) q[i].index(v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < H; ++i) q[i].load(tab);
    double w[M];
#pragma unroll
    for (int i = 0; i < H; ++i) w[i] = q[i].finish();
    if constexpr ((N & 1) != 0) w[M - 1] = v[N - 1];
    return pcTree<M>(tab, w);
  }
}

__device__ __forceinline__ double pcLaneSum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  return v;                                                            // lane 0 holds the tree's root
}

// What pass 2 does with the posteriors of a cell's moves is a policy.  Its register accumulators acc[kRegs + KP] are the caller's
// array, handed down as an argument (not held by the policy: an array whose address is stored is no longer the one vector of
// registers the compiler makes of it).  moves() gets, for the cell (ip,op) with y = out[op]: the parked forward values fs, fd,
// ft[k]; B_S(ip+1,op+1), B_D(ip+1,op) and B_S(ip,op) as Sdiag, Ddn and S; BT[k] = B_Tk(ip,op) and tgt[k], what T_k's emission
// leads to at (ip,op+1); sub0 = sub[in[ip]][y] and subk[k] = sub[in[ip-1-k]][y] with their table indices idx0 and idx[k].  What
// a policy does not use is not formed: the look-ups behind it have no other reader, and ft[k] is read from the scratch only under
// kEmissions (a policy without it has no such planes parked).  stripeEnd(acc, r, row) is called by every lane when its stripe is
// done.

// The default: every move's posterior summed over the whole matrix.  acc[5 + KP]: nDelOpen, nTanDup, nNoGap, nDelExtend,
// nDelEnd, nLen[k]; accSub: the wave's [16][64] LDS slots.
struct PcTotals {
  static constexpr int kRegs = 5;
  static constexpr bool kEmissions = true;     // meets the parked T lanes again
  double* accSub;
  template <int KP>
  __device__ __forceinline__ void moves(double (&acc)[5 + KP], const PaScores& sc, double Z, double fs, double fd,
                                        const double (&ft)[KP], double Sdiag, double Ddn, double S, const double (&BT)[KP],
                                        const double (&tgt)[KP], double sub0, const double (&subk)[KP], int idx0,
                                        const int (&idx)[KP], int) const {
    double e = exp(fs + sc.noGap + sub0 + Sdiag - Z);
    acc[2] += e;
    accSub[idx0 * 64] += e;
    acc[0] += exp(fs + sc.delOpen + Ddn - Z);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      e = exp(fs + sc.tanDup + sc.len[k] + BT[k] - Z);
      acc[1] += e;
      acc[5 + k] += e;
    }
    acc[3] += exp(fd + sc.delExtend + Ddn - Z);
    acc[4] += exp(fd + sc.delEnd + S - Z);
#pragma unroll
    for (int k = 0; k < KP; ++k) accSub[idx[k] * 64] += exp(ft[k] + subk[k] + tgt[k] - Z);
  }
  template <int N>
  __device__ __forceinline__ void stripeEnd(double (&)[N], int, bool) const {}
};

// The profile policy (include/dnastore_amd.h, dnas_pair_profiles): the moves that consume in[r] or insert in front of it, kept
// per row.  A lane stands on row r for a whole stripe, so its accumulators at the end of the stripe are row r's planes: acc[2 +
// KP] -- delOpen, delExtend, the duplications by k -- in registers, the match by y in the wave's [4][64] LDS slots.  Every lane
// with a row stores them to the pair's block, plane j at block + j * rows + r -- consecutive lanes write consecutive doubles --
// and clears them.  Neither delEnd nor the T_k emissions are formed.  Planes from 6 + P on are not stored: the block does not
// have them.
struct PcProfile {
  static constexpr int kRegs = 2;
  static constexpr bool kEmissions = false;    // never reads a parked T lane: pass 1 parks S and D only, two planes of scratch
  double* accY;                      // this lane's column of the [4][64] slots
  double* block;
  int rows, P;                       // rows = I + 1
  template <int N>
  __device__ __forceinline__ void clear(double (&acc)[N]) const {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0;
#pragma unroll
    for (int y = 0; y < 4; ++y) accY[y * 64] = 0;
  }
  template <int KP>
  __device__ __forceinline__ void moves(double (&acc)[2 + KP], const PaScores& sc, double Z, double fs, double fd,
                                        const double (&)[KP], double Sdiag, double Ddn, double, const double (&BT)[KP],
                                        const double (&)[KP], double sub0, const double (&)[KP], int, const int (&)[KP],
                                        int y) const {
    accY[y * 64] += exp(fs + sc.noGap + sub0 + Sdiag - Z);
    acc[0] += exp(fs + sc.delOpen + Ddn - Z);
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[2 + k] += exp(fs + sc.tanDup + sc.len[k] + BT[k] - Z);
    acc[1] += exp(fd + sc.delExtend + Ddn - Z);
  }
  template <int N>
  __device__ __forceinline__ void stripeEnd(double (&acc)[N], int r, bool row) const {
    if (row) {
      double* const p = block + r;
#pragma unroll
      for (int y = 0; y < 4; ++y) p[(size_t)(DNAS_PROFILE_MATCH + y) * (size_t)rows] = accY[y * 64];
      p[(size_t)DNAS_PROFILE_DEL_OPEN * (size_t)rows] = acc[0];
      p[(size_t)DNAS_PROFILE_DEL_EXTEND * (size_t)rows] = acc[1];
#pragma unroll
      for (int k = 0; k < N - 2; ++k)
        if (k < P) p[(size_t)(DNAS_PROFILE_DUP + k) * (size_t)rows] = acc[2 + k];
    }
    clear(acc);
  }
};


// Pass 2, a walk of its own over PaStripe, PaBoundary and PaBases with the lane roles mirrored.  policy.moves() is handed every
// cell inside the band by the lane that stands on it, policy.stripeEnd(r, row) is called by every lane when its stripe is done;
// -> B_S(0,0) in every lane.  scr: this lane's column of the parked planes.
template <int KP, class Policy>
__device__ __forceinline__ double pcBackwardPair(const PaScores& sc, pf_rsrc_t tab, const double* sub, const PaBoundary& bnd,
                                                 const double* scr, int lane, int band, const PaItem& it, double Z,
                                                 const Policy& policy, double (&acc)[Policy::kRegs + KP]) {
  const double NEG = paNegInf();
  const int P = sc.P, I = it.I, O = it.O;
  const PaGeom g(I, O, band);
  const size_t words = g.words();
  double b00 = NEG;

  for (int s = g.stripes - 1; s >= 0; --s) {
    const PaStripe st(g, I, O, P, s, lane);
    const int r = st.r, last = st.last, tmax = st.tmax, kmax = st.kmax;
    const bool below = s < g.stripes - 1;                              // then last == 63
    const PaSpan dn = st.below(g, O);
    const unsigned ctx = paContext<KP>(it, st.row, r);                 // in[r] for the match, in[r-1-k] for T_k
    double BT[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) BT[k] = NEG;
    double Sdiag = NEG, pubS = NEG, pubD = NEG;
    int ypub = 0;
    PaBases bases;
    if (lane == last && below) {
      const int opf = st.op(tmax) + 1;
      if (dn.has(opf)) Sdiag = bnd.loadS(opf);
    }
    const double* const scrStripe = scr + (size_t)s * (size_t)g.stepsMax * 64;

    for (int t = tmax; t >= 0; --t) {
      bases.fetch(it, tmax - t, st.c0 + t - last, -1, lane);                   // the last row hands the bases up
      double Sdn = __shfl_down(pubS, 1), Ddn = __shfl_down(pubD, 1);
      int y = __shfl_down(ypub, 1);
      const int ysrc = bases.get(tmax - t);
      const int op = st.op(t);
      if (lane == last) {
        y = ysrc;
        Sdn = Ddn = NEG;
        if (below && dn.has(op)) bnd.load(op, Sdn, Ddn);
      }
      double S = NEG, D = NEG;
      if (st.active(op)) {
        // the parked forward cell: issued first, needed last
        const double* const p = scrStripe + (size_t)t * 64;
        const double fs = p[0], fd = p[words];
        double ft[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) ft[k] = Policy::kEmissions && k < P ? p[(size_t)(2 + k) * words] : NEG;

        // T_k, then S, then D
        double tgt[KP], subk[KP], v[KP + 2];
        int idx[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          tgt[k] = k > 0 ? BT[k - 1] : pubS;                           // B_T{k-1}(ip,op+1), or B_S(ip,op+1): this lane's last step
          idx[k] = (int)((ctx >> (2 * k + 2)) & 3u) * 4 + y;
          subk[k] = sub[idx[k]];
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) BT[k] = k < kmax ? subk[k] + tgt[k] : NEG;
        const int idx0 = (int)(ctx & 3u) * 4 + y;
        const double sub0 = sub[idx0];
        v[0] = (sc.noGap + sub0) + Sdiag;
        v[1] = sc.delOpen + Ddn;
#pragma unroll
        for (int k = 0; k < KP; ++k) v[2 + k] = (sc.tanDup + sc.len[k]) + BT[k];
        S = r == I && op == O ? 0. : pcTree<KP + 2>(tab, v);
        D = pfLse(tab, sc.delExtend + Ddn, sc.delEnd + S);
        if (lane == 0) bnd.store(op, S, D);

        // the moves out of this cell
        policy.template moves<KP>(acc, sc, Z, fs, fd, ft, Sdiag, Ddn, S, BT, tgt, sub0, subk, idx0, idx, y);
        if (r == 0 && op == 0) b00 = S;
      }
      Sdiag = Sdn;
      pubS = S;
      pubD = D;
      ypub = y;
    }
    policy.stripeEnd(acc, r, st.row);
    bnd.handOver();      // the stripe above reads in its last lane what this stripe's lane 0 wrote
  }
  return __shfl(b00, 0);
}

// One pair: both passes, the lanes summed, the slot written.  slot: nc = 21 + P counts, Z, B_S(0,0).  wave: this wave's LDS --
// 16 substitution scores, 2 ldsCols boundary doubles, then the [16][64] counters.
template <int KP>
__device__ __forceinline__ void pcCountsPair(const PaScores& sc, const double* __restrict__ lseTab, double* wave, int ldsCols,
                                             double* bndMem, double* scr, int lane, int band, const PaItem& it, double* slot) {
  const int P = sc.P, nc = 21 + P;
  const PaGeom g(it.I, it.O, band);
  double* const sub = wave;
  const PaBoundary bnd(wave + 16, ldsCols, bndMem, it.O);
  double* const accSub = wave + 16 + 2 * ldsCols + lane;
  PaForwardCell<PcPark> fwd{pfTable(lseTab), PcPark{scr + lane, g.words(), g.stepsMax, P, it.I, it.O, paNegInf()}};
  paWalkForward<KP>(sc, sub, bnd, lane, band, it, slot + nc, fwd);
  const double Z = __shfl(fwd.park.z, it.I & 63);

  double acc[5 + KP];
#pragma unroll
  for (int k = 0; k < 5 + KP; ++k) acc[k] = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) accSub[i * 64] = 0;
  double b00 = paNegInf();
  if (Z > paNegInf())
    b00 = pcBackwardPair<KP>(sc, fwd.tab, sub, bnd, scr + lane, lane, band, it, Z, PcTotals{accSub}, acc);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double tot = pcLaneSum(acc[k]);
    if (lane == 0) slot[k] = tot;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const double tot = pcLaneSum(accSub[i * 64]);
    if (lane == 0) slot[5 + i] = tot;
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const double tot = pcLaneSum(acc[5 + k]);
    if (lane == 0 && k < P) slot[21 + k] = tot;
  }
  if (lane == 0) slot[nc + 1] = b00;
}

// One pair's profile: both passes under PcProfile.  block: the pair's (6 + P) x (I + 1) doubles, every one of them written
// unless Z = -inf (then none is: the host does not read it); *zOut = Z.  wave: this wave's LDS -- 16 substitution scores, 2 ldsCols boundary doubles, then
// the [4][64] match counters.
template <int KP>
__device__ __forceinline__ void pcProfilePair(const PaScores& sc, const double* __restrict__ lseTab, double* wave, int ldsCols,
                                              double* bndMem, double* scr, int lane, int band, const PaItem& it, double* block,
                                              double* zOut) {
  const PaGeom g(it.I, it.O, band);
  double* const sub = wave;
  const PaBoundary bnd(wave + 16, ldsCols, bndMem, it.O);
  PaForwardCell<PcPark> fwd{pfTable(lseTab), PcPark{scr + lane, g.words(), g.stepsMax, /* T lanes parked */ 0, it.I, it.O, paNegInf()}};
  paWalkForward<KP>(sc, sub, bnd, lane, band, it, zOut, fwd);
  const double Z = __shfl(fwd.park.z, it.I & 63);
  if (Z > paNegInf()) {
    const PcProfile profile{wave + 16 + 2 * ldsCols + lane, block, it.I + 1, sc.P};
    double acc[2 + KP];
    profile.clear(acc);
    pcBackwardPair<KP>(sc, fwd.tab, sub, bnd, scr + lane, lane, band, it, Z, profile, acc);
  }
}

}  // namespace
