// Pair-HMM Viterbi alignment of an (original, read) pair under the mutator model: the most probable path of the pair HMM
// whose Forward matrix the E-step fills (fwdback_onchip.hip), traced back to a gapped pair.  This file is the plain
// single-threaded statement of the recurrence (include/dnastore_amd.h, dnas_align_pairs): the specification the kernel in
// pair_align_kernels.hip is held to bit for bit, and the CPU baseline.
//
//   D(ip,op)   = best of  [d0] S(ip-1,op) + delOpen        [d1] D(ip-1,op) + delExtend                  (ip > 0)
//   S(ip,op)   = best of  [s0] S(ip-1,op-1) + noGap + sub[in[ip-1]][out[op-1]]                          (ip > 0, op > 0)
//                         [s1] T_0(ip,op-1) + sub[in[ip-1]][out[op-1]]                                  (ip > 0, op > 0, P > 0)
//                         [s2] D(ip,op) + delEnd
//   T_k(ip,op) = best of  [t0] T_{k+1}(ip,op-1) + sub[in[ip-2-k]][out[op-1]]                            (op > 0, k+1 < min(ip,P))
//                         [t1] S(ip,op) + tanDup + len[k]                                               (k < min(ip,P))
//
// S(0,0) = 0, everything else starts at -inf; sums are formed left to right in fp64; "best of" takes the candidates in the
// order listed and the first strictly greater one wins; a cell outside the band reads as -inf.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "model.hpp"

namespace dnas {

constexpr int kAlignMaxLen = 13;        // duplication lengths: a cell's choices are P + 3 bits of a 16-bit word
constexpr int64_t kAlignMaxSeq = 1 << 20;

// one op byte per alignment column: kind | n << 2
enum : uint8_t { kOpMatch = 0, kOpDelete = 1, kOpDup = 2 };

struct PairScores {   // MutatorScores (what FlatModel::build derives): log probabilities, -inf where a probability is 0
  double delOpen, tanDup, noGap, delExtend, delEnd, sub[16];
  double len[kAlignMaxLen];
  int P;
  static PairScores from(const MutatorParams& p);   // P <= kAlignMaxLen is the caller's check
};

// The band: cell (ip, op) is inside iff lo <= op - ip <= hi.  band < 0: every cell.
struct PairBand {
  int64_t lo, hi;
  PairBand(int64_t I, int64_t O, int64_t band) {
    const int64_t b = band < 0 || band > I + O + 1 ? I + O + 1 : band;
    lo = (O < I ? O - I : 0) - b;
    hi = (O > I ? O - I : 0) + b;
  }
  int64_t rowLo(int64_t ip) const { return ip + lo > 0 ? ip + lo : 0; }
  int64_t rowHi(int64_t ip, int64_t O) const { return ip + hi < O ? ip + hi : O; }
  int64_t cells(int64_t I, int64_t O) const {
    int64_t n = 0;
    for (int64_t ip = 0; ip <= I; ++ip) n += rowHi(ip, O) - rowLo(ip) + 1;
    return n;
  }
};

// -> the score S(I,O) (-inf: no path, ops left empty) and the op bytes in alignment order.
double alignPairHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band,
                     std::vector<uint8_t>* ops);

// The op bytes of one pair spelled out; any output may be null.  rowIn / rowOut: the gapped rows; cmIn[I+1] / cmOut[O+1]: the
// guide arrays as stockholm.cpp derives them from the rows; counts[21 + nLen]: the path's moves in MutatorCounts order.
// Throws std::invalid_argument when the ops do not describe a path of the model over these sequences.
void expandAlignment(int nLen, const int8_t* in, int64_t I, const int8_t* out, int64_t O, const uint8_t* ops, int64_t nOps,
                     std::string* rowIn, std::string* rowOut, int32_t* cmIn, int32_t* cmOut, double* counts);

// "# STOCKHOLM 1.0", two "name row" lines and "//" per pair; a read named like its original gets the suffix "/read".
std::string writeStockholm(int64_t n, const char* const* namesIn, const char* const* namesOut, const char* const* rowsIn,
                           const char* const* rowsOut);

// The argument checks dnas_align_pairs and dnas_align_pairs_host share (DNAS_OK or the code, dnas_last_error set): null
// pointers, n_len, offsets, sequence lengths, base codes and the size of every op slot.
int checkAlignArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                   const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_ops, const uint64_t* ops_off,
                   const uint32_t* out_n_ops, const double* out_score, const uint8_t* out_status);

}  // namespace dnas
