// Sampling reads from the mutator pair HMM (include/dnastore_amd.h, dnas_simulate_reads).  This file is the definition, stated
// once for the host statement (simulate.cpp) and the kernels (simulate_kernels.hip): the counter-based generator, how a draw is
// named, the thresholds, and what one input position does with its draws.  A position's outcome is a function of its own draws
// and one entry bit (was a deletion open when it was entered), so the statement walks the positions in order and the kernels
// give every lane a position and resolve the entry bits afterwards; both call simExtend and simPosition below.
//
// Where the sampler departs from the pair HMM the kernels score.  The pair HMM is not normalised at its edges -- there is no
// duplication of a length above ip, and at ip == I nothing but duplications -- so a sampler has to say what happens to the
// probability that is missing there:
//   * a draw in the duplication interval [tDel, tDup) that cannot be taken (no length fits, or the cap below) counts as a match;
//   * near the start (ip < P) the duplication's length is drawn from pLen truncated to its first ip entries, renormalised;
//   * at ip == I everything but a duplication ends the read;
//   * a position makes at most kSimMaxDups duplications, the draws in the interval after that count as matches;
//   * a deletion that reaches ip == I ends there without a draw, where the model charges delEnd.
// Inside (P <= ip < I) and below the cap the sampler is the model: tests/test_simulate_cpu.py holds the ratio of the two to its
// closed forms.
#pragma once
#include <cstdint>
#include <vector>

#include "../../../include/dnastore_amd.h"
#include "cluster.hpp"

namespace dnas {

constexpr int kSimMaxDups = 16;                          // duplications of one position
constexpr int kSimMaxLen = 32;                           // n_len of dnas_mutator_params
constexpr int64_t kSimMaxStrand = (int64_t)1 << 20;      // bases of a strand: a read's bases and ops then fit 32 bits
constexpr uint32_t kSimPerRead = 0xFFFFFFFFu;            // the position of the per-read draws
constexpr uint8_t kSimOpMatch = 0, kSimOpDelete = 1, kSimOpDup = 2;   // the kinds of dnas_align_pairs' op bytes

// Philox4x32-10 (Salmon et al., SC'11): the words of counter ctr under key (k0, k1).
DNAS_HD inline void philox4x32(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0], p1 = (uint64_t)0xCD9E8D57u * ctr[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1;
    ctr[0] = n0, ctr[1] = (uint32_t)p1, ctr[2] = n2, ctr[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// The draws of (seed, read, position), j = 0, 1, ...: call c = j / 2 of the generator has the counter (c, position, read) and the
// seed's halves as its key; draw 2c is its words 0 and 1, draw 2c + 1 its words 2 and 3, the top 53 bits of the 64.  The last
// call is kept: a position takes its draws in ascending order.
struct SimDraws {
  uint32_t k0, k1, position, readLo, readHi;
  uint32_t call = 0xFFFFFFFFu, w[4];
  DNAS_HD SimDraws(uint64_t seed, uint64_t read, uint32_t pos)
      : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), position(pos), readLo((uint32_t)read), readHi((uint32_t)(read >> 32)) {}
  DNAS_HD uint64_t bits(uint32_t j) {
    if ((j >> 1) != call) {
      call = j >> 1;
      w[0] = call, w[1] = position, w[2] = readLo, w[3] = readHi;
      philox4x32(w, k0, k1);
    }
    const uint64_t x = j & 1 ? (uint64_t)w[2] | (uint64_t)w[3] << 32 : (uint64_t)w[0] | (uint64_t)w[1] << 32;
    return x >> 11;
  }
  DNAS_HD double draw(uint32_t j) { return (double)bits(j) * 0x1p-53; }   // exact: 53 bits, a power of two
};

// What the draws are compared with: sums formed once on the host, left to right, in fp64.
struct SimThresholds {
  double tDel, tDup, delExtend, reverseProb;
  double sub[3];                                         // transition, the smaller transversion, the larger one
  double cum[kSimMaxLen];                                // cum[k] = pLen[0] + ... + pLen[k]
  int32_t P;
  static SimThresholds from(const dnas_mutator_params& p, double reverseProb) {
    SimThresholds t{};
    t.tDel = p.p_del_open;
    t.tDup = p.p_del_open + p.p_tan_dup;
    t.delExtend = p.p_del_extend;
    t.reverseProb = reverseProb;
    t.sub[0] = p.p_transition;
    t.sub[1] = p.p_transition + p.p_transversion / 2;
    t.sub[2] = p.p_transition + p.p_transversion;
    t.P = p.n_len;
    double c = 0;
    for (int k = 0; k < p.n_len && k < kSimMaxLen; ++k) t.cum[k] = c = c + p.p_len[k];
    return t;
  }
};

// The base a copy of x comes out as under draw u: its transition partner x ^ 2, the smaller of the two other codes, the larger.
DNAS_HD inline int simSubstitute(const SimThresholds& th, int x, double u) {
  if (u < th.sub[0]) return x ^ 2;
  if (u < th.sub[1]) return (x ^ 1) < (x ^ 3) ? x ^ 1 : x ^ 3;
  if (u < th.sub[2]) return (x ^ 1) < (x ^ 3) ? x ^ 3 : x ^ 1;
  return x;
}

// Draw 0 of a position entered with a deletion open: the deletion takes the position's base too.
DNAS_HD inline bool simExtend(const SimThresholds& th, SimDraws& d, int64_t ip, int64_t I) { return ip < I && d.draw(0) < th.delExtend; }

// Position ip of a strand in[0..I) once no deletion is open (the S loop, draws 1, 2, ...): emit(base or -1, op byte) per alignment
// column in order.  True when the position opens a deletion (the next one is entered in D).
template <class Emit>
DNAS_HD inline bool simPosition(const SimThresholds& th, SimDraws& d, const int8_t* in, int64_t ip, int64_t I, Emit&& emit) {
  const int n = ip < th.P ? (int)ip : th.P;
  const bool canDup = n > 0 && th.cum[n - 1] > 0;
  uint32_t j = 1;
  for (int dups = 0;;) {
    const double u = d.draw(j++);
    if (u < th.tDel && ip < I) {
      emit(-1, (uint8_t)(kSimOpDelete | 1u << 2));
      return true;
    }
    if (u >= th.tDel && u < th.tDup && canDup && dups < kSimMaxDups) {
      const double v = d.draw(j++) * th.cum[n - 1];
      int k = 0;
      while (k < n - 1 && !(v < th.cum[k])) ++k;
      for (int t = k; t >= 0; --t)
        emit(simSubstitute(th, in[ip - 1 - t] & 3, d.draw(j++)), (uint8_t)(kSimOpDup | (t == k ? (unsigned)(k + 1) << 2 : 0u)));
      ++dups;
      continue;
    }
    if (ip < I) emit(simSubstitute(th, in[ip] & 3, d.draw(j++)), kSimOpMatch);
    return false;
  }
}

// The entry bits of 64 consecutive positions from their ballots.  gen: the position opens a deletion; ext: draw 0 extends; carry:
// the first position is entered in D.  Position i is entered in D iff position i - 1 opened a deletion, or was entered in D and
// extended: the carries of an addition whose generate bits are gen and whose propagate bits are ext.  -> the mask of the
// positions entered in D, *carryOut for the position after the last.
DNAS_HD inline uint64_t simEntryBits(uint64_t gen, uint64_t ext, unsigned carry, unsigned* carryOut) {
  const uint64_t a = gen | ext, b = gen, sum = a + b + carry;
  *carryOut = (unsigned)(((a & b) | ((a | b) & ~sum)) >> 63);
  return sum ^ a ^ b;
}

// DNAS_OK or the code, dnas_last_error set: what dnas_simulate_reads and dnas_simulate_reads_host check.
int checkSimulateArgs(const dnas_mutator_params* params, int64_t n_strands, const int8_t* strand_seqs, const int64_t* strand_off,
                      int64_t n_reads, const int64_t* read_strand, double reverse_prob, int want_ops, int8_t** out_seqs,
                      int64_t** out_off, uint8_t** out_reversed, uint8_t** out_ops, int64_t** out_ops_off, const uint8_t* out_status);

// The statement for one read: read `index` of strand in[0..I) -> its bases as handed out (reverse-complemented when the per-read
// draw says so) appended to seq, its op bytes (of the read before that reversal) to ops when ops is not null.  -> reversed.
bool simulateReadHost(const SimThresholds& th, uint64_t seed, uint64_t index, const int8_t* in, int64_t I, std::vector<int8_t>* seq,
                      std::vector<uint8_t>* ops);

// The ragged outputs of a call, malloc'd for the caller (dnas_free): lengths -> offsets, data copied.
int simulateHandOut(int64_t n_reads, const std::vector<int8_t>& seqs, const std::vector<int64_t>& off, const std::vector<uint8_t>& reversed,
                    int want_ops, const std::vector<uint8_t>& ops, const std::vector<int64_t>& opsOff, int8_t** out_seqs, int64_t** out_off,
                    uint8_t** out_reversed, uint8_t** out_ops, int64_t** out_ops_off);

}  // namespace dnas
