// Posterior expected counts of every move of the mutator pair HMM over the whole band of an (original, read) pair: the backward
// pass to host/pairforward.hpp and the E-step built on the two (include/dnastore_amd.h, dnas_pair_counts).  F_S, F_D, F_Tk are
// the forward values of host/pairforward.hpp bit for bit, Z = F_S(I,O).  With ip, op the bases consumed, x = in[..], y = out[..]:
//
//   B_S(I,O)    = 0
//   B_Tk(ip,op) = sub[in[ip-1-k]][out[op]] + (k > 0 ? B_T{k-1}(ip,op+1) : B_S(ip,op+1))                  (k < min(ip,P), op < O)
//   B_S(ip,op)  = tree( (noGap + sub[in[ip]][out[op]]) + B_S(ip+1,op+1) ,  delOpen + B_D(ip+1,op) ,
//                       (tanDup + len[0]) + B_T0(ip,op) , ... , (tanDup + len[n-1]) + B_T{n-1}(ip,op) )  n = min(ip,P)
//   B_D(ip,op)  = lse( delExtend + B_D(ip+1,op) ,  delEnd + B_S(ip,op) )
//
// A term that reads a cell outside the band or the matrix is -inf; inside a cell the order is T_k, S, D.  tree(v_0 .. v_{m-1})
// combines neighbours level by level: v_i <- lse(v_2i, v_2i+1), an odd last element carried up unchanged, until one is left
// (depth ceil(log2(n + 2))).  Because lse(x, -inf) = x and lse(-inf, -inf) = -inf exactly, padding the list with -inf does not
// change a bit, which is how the kernel (pair_counts_device.h) runs one tree of KP + 2 leaves for every row.
//
// The posterior of a move n -> n' of weight w is exp(F(n) + w + B(n') - Z), the exponent summed left to right with w's own parts
// in the order of the table below, and is added to each of the move's counts (MutatorCounts order, [21 + P]):
//
//   S(ip,op)  -> S(ip+1,op+1)   F_S + noGap + sub[x][y] + B_S(ip+1,op+1) - Z       nNoGap, nSub[x][y]      x = in[ip], y = out[op]
//   S(ip,op)  -> D(ip+1,op)     F_S + delOpen + B_D(ip+1,op) - Z                   nDelOpen
//   S(ip,op)  -> T_k(ip,op)     F_S + tanDup + len[k] + B_Tk(ip,op) - Z            nTanDup, nLen[k]
//   D(ip,op)  -> D(ip+1,op)     F_D + delExtend + B_D(ip+1,op) - Z                 nDelExtend
//   D(ip,op)  -> S(ip,op)       F_D + delEnd + B_S(ip,op) - Z                      nDelEnd
//   T_k(ip,op)-> T_{k-1} or S   F_Tk + sub[x][y] + B(target at (ip,op+1)) - Z      nSub[x][y]              x = in[ip-1-k], y = out[op]
//
// Z = -inf: no path; the counts are zero and B_S(0,0) is reported as -inf.
#pragma once
#include <cstdint>

#include "pairalign.hpp"

namespace dnas {

// One thread; every forward cell of the band is kept (S, D and the T lanes), the backward values roll.  counts[21 + sc.P] is
// overwritten, its additions made in cell order: rows last to first, columns right to left, per cell match, delOpen, the
// duplications k = 0 .., delExtend, delEnd, the T_k emissions k = 0 ...  *ll = Z, the bits of forwardPairHost; *llBackward =
// B_S(0,0) (may be null).  rev, exactLse: as forwardPairHost.  -> false when Z = -inf.
bool pairCountsHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                    bool exactLse, double* counts, double* ll, double* llBackward);

// The same two passes -- one recurrence body serves both -- with the posteriors of the moves that consume in[ip] or insert in
// front of it filed by row instead of summed over the matrix (include/dnastore_amd.h, dnas_pair_profiles): profile[W x (I + 1)],
// W = 6 + sc.P, plane-major, is overwritten, each value the sum over its row's columns right to left.  delEnd and the T_k
// emissions are not formed.  *ll = Z.  -> false when Z = -inf (the profile is zero).
bool pairProfileHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                     bool exactLse, double* profile, double* ll);

// The aggregate of dnas_pair_profiles: add() is called with the blocks of the OK pairs in pair order, which is what makes the
// result independent of grid, chunking and device count.  profile[(5 + P) x nPositions] and coverage[nPositions] are zeroed by
// the constructor.
class ProfileSum {
 public:
  ProfileSum(int P, int anchor, int64_t nPositions, double* profile, int64_t* coverage);
  void add(const int8_t* in, int64_t I, const double* block);

 private:
  int P_, anchor_;
  int64_t n_;
  double* profile_;
  int64_t* coverage_;
};

// dnas_pair_profiles_host over a list of pairs, one thread; out_pair_profiles may be null.
void pairProfilesHostAll(const PairScores& sc, int64_t band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                         const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev, bool exactLse, ProfileSum* sum,
                         double* out_pair_profiles, double* out_pair_ll, uint8_t* out_status);

// The argument checks of dnas_pair_profiles and dnas_pair_profiles_host: checkForwardArgs plus the anchor and the outputs.
int checkProfileArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                     const int8_t* out_seqs, const int64_t* out_off, int32_t anchor, int64_t n_positions, const double* out_profile,
                     const int64_t* out_coverage, const double* out_pair_ll, const uint8_t* out_status);

// dnas_pair_counts_host over a list of pairs, one thread; out_pair_counts and out_pair_ll_backward may be null.
void pairCountsHostAll(const PairScores& sc, int64_t band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                       const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev, bool exactLse, double* out_counts,
                       double* out_ll, double* out_pair_counts, double* out_pair_ll, double* out_pair_ll_backward,
                       uint8_t* out_status);

// The call's totals from the per-pair values, in pair order over the pairs with status OK: what makes out_counts and out_ll
// independent of grid, chunking and device count.  pairCounts: n x nc.
void pairCountsTotals(int64_t n, int nc, const double* pairCounts, const double* pairLl, const uint8_t* status, double* out_counts,
                      double* out_ll);

// The argument checks of dnas_pair_counts and dnas_pair_counts_host: checkForwardArgs plus the outputs.
int checkCountsArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                    const int8_t* out_seqs, const int64_t* out_off, const double* out_counts, const double* out_ll,
                    const double* out_pair_ll, const uint8_t* out_status);

}  // namespace dnas
