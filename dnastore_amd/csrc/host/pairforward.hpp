// The forward score of an (original, read) pair under the mutator pair HMM: log P(read | original) summed over every alignment
// inside the band, where host/pairalign.hpp keeps the single best one.  The same lattice, band and start; "best of" becomes
// log-sum-exp:
//
//   D(ip,op)   = lse( S(ip-1,op) + delOpen ,  D(ip-1,op) + delExtend )                                   (ip > 0)
//   S(ip,op)   = lse( lse( S(ip-1,op-1) + noGap + sub[in[ip-1]][out[op-1]] ,
//                          T_0(ip,op-1) + sub[in[ip-1]][out[op-1]] ) ,
//                     D(ip,op) + delEnd )
//   T_k(ip,op) = lse( T_{k+1}(ip,op-1) + sub[in[ip-2-k]][out[op-1]] ,  S(ip,op) + tanDup + len[k] )      (k < min(ip,P))
//
// S(0,0) = 0; a term whose condition does not hold, or whose cell is outside the band, is -inf; sums inside a term are formed
// left to right in fp64 and the lse calls nest as written.  The result is S(I,O), -inf when there is no path.  lse is the
// reference's table function (host/lsetable.hpp), which the kernel of pair_forward_device.h restates: the two are bit-identical.
#pragma once
#include <cstdint>

#include "pairalign.hpp"

namespace dnas {

// One thread, two rolling rows.  rev: out is read in place as its reverse complement (base j of it is 3 - out[O-1-j]).
// exactLse: mx + log1p(exp(-diff)) from the host libm in place of the table -- the pin between the recurrence and exact path
// sums, and what a caller without a GPU may prefer.
double forwardPairHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                       bool exactLse);

// The argument checks dnas_pair_likelihoods and dnas_pair_likelihoods_host share: as checkAlignArgs, without the op slots.
int checkForwardArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                     const int8_t* out_seqs, const int64_t* out_off, const double* out_ll);

}  // namespace dnas
