// Demultiplexing and trimming a pool of reads by primer pairs (include/dnastore_amd.h, dnas_trim_reads).  This file holds what
// the host statement (trim.cpp) and the kernels (trim_kernels.hip) share, stated once for both: an anchor's limit, a candidate's
// acceptance and total, the running best of a read under the (total, k, s) order with the runner-up of another pair, the merge
// of two such states, and the outputs that follow from one.  The search itself is not shared: the statement runs the two-row
// dynamic program, the kernels Myers' bit-vector recurrence (cluster_gate.hpp).  The kernels' search step, TrimSearch, is stated
// here all the same, so that a host program can run the kernels' own text (tools/bitvector_host_check.cpp).
#pragma once
#include <cstdint>

#include "../cluster_gate.hpp"
#include "cluster.hpp"

namespace dnas {

constexpr int kTrimMaxPrimer = 64;                       // a primer is one word of the bit-vector recurrence
constexpr int32_t kTrimNone = 0x7FFFFFFF;                // no total

// What a search answers: the smallest E[c] and the largest column that attains it.
struct TrimHit {
  int32_t e, c;
};

// One search of the kernels: a primer of m rows in one word of the bit-vector recurrence, hin = 0 (row 0 is free in every column).
struct TrimSearch {
  uint64_t Pv = ~(uint64_t)0, Mv = 0;
  int32_t score;
  TrimHit hit;
  DNAS_HD explicit TrimSearch(int32_t m) : score(m), hit{m, 0} {}
  // column c (1-based) of a window of w columns, whose base is b
  DNAS_HD __attribute__((always_inline)) void step(const uint64_t* eq, int b, uint64_t rowBit, int32_t c, int32_t w) {
    const uint64_t lo = b & 1 ? eq[1] : eq[0], hi = b & 1 ? eq[3] : eq[2];
    (void)gateBlock(Pv, Mv, b & 2 ? hi : lo, 0, rowBit, score);
    if (c <= w && score <= hit.e) hit = TrimHit{score, c};
  }
};

// An anchor of m bases is within its limit iff e <= trimLimit(permille, m).
DNAS_HD inline int32_t trimLimit(int32_t maxEditPermille, int32_t m) { return (int32_t)((int64_t)maxEditPermille * m / 1000); }

// The columns a search of a pattern of m rows walks in a text of n bases.
DNAS_HD inline int32_t trimWindow(int32_t m, int32_t n, int32_t maxOffset) {
  return maxOffset < 0 || maxOffset >= n || m + maxOffset >= n ? n : m + maxOffset;
}

// A read's state while its candidates pass by: the winner so far and the smallest total of another pair's accepted candidate.
struct TrimBest {
  int32_t total = kTrimNone, pair = -1, strand = 0;      // the smallest (total, pair, strand) among the accepted candidates
  int32_t eF = -1, eR = -1, cF = 0, cR = 0;              // ... its anchors
  int32_t second = kTrimNone;                            // the smallest total among accepted candidates of a pair != pair
  int32_t anchored = 0;                                  // 1: some candidate had its anchors within their limits
};

// Candidate (k, s) of a read of n bases with the hits f (of F_k) and r (of reverse(R_k)) -> b.
DNAS_HD inline void trimOffer(TrimBest& b, int32_t k, int32_t s, int32_t n, TrimHit f, int32_t mF, TrimHit r, int32_t mR,
                              int32_t maxEditPermille, int32_t anchors, int32_t minPayload) {
  const int32_t limF = trimLimit(maxEditPermille, mF), limR = trimLimit(maxEditPermille, mR);
  const bool inF = f.e <= limF, inR = r.e <= limR;
  if (anchors == 0 ? !(inF && inR) : !(inF || inR)) return;
  b.anchored = 1;
  if (!inF) f = TrimHit{-1, 0};
  if (!inR) r = TrimHit{-1, 0};
  if ((int64_t)f.c + r.c + minPayload > n) return;
  const int32_t total = (inF ? f.e : limF + 1) + (inR ? r.e : limR + 1);
  if (k == b.pair) {
    if (total < b.total || (total == b.total && s < b.strand)) b.total = total, b.strand = s, b.eF = f.e, b.eR = r.e, b.cF = f.c, b.cR = r.c;
  } else if (total < b.total || (total == b.total && k < b.pair)) {
    b.second = b.total;                                  // (the old winner is now the best of another pair: it was at most b.second)
    b.total = total, b.pair = k, b.strand = s, b.eF = f.e, b.eR = r.e, b.cF = f.c, b.cR = r.c;
  } else if (total < b.second) {
    b.second = total;
  }
}

// a <- the state of a's candidates and o's together (the two saw different pairs, or the same ones: either is right).
DNAS_HD inline void trimMerge(TrimBest& a, const TrimBest& o) {
  const int32_t anchored = a.anchored | o.anchored;
  if (o.pair < 0) {
    a.anchored = anchored;
    return;
  }
  if (a.pair < 0) {
    a = o;
    a.anchored = anchored;
    return;
  }
  if (a.pair == o.pair) {
    const int32_t second = a.second < o.second ? a.second : o.second;
    if (o.total < a.total || (o.total == a.total && o.strand < a.strand)) a = o;
    a.second = second;
  } else {
    const bool oWins = o.total < a.total || (o.total == a.total && o.pair < a.pair);
    const TrimBest lose = oWins ? a : o;
    if (oWins) a = o;
    if (lose.total < a.second) a.second = lose.total;    // (the loser's own runner-up is no smaller than its total)
  }
  a.anchored = anchored;
}

// The outputs of a read of n bases from its final state.
DNAS_HD inline void trimFinish(const TrimBest& b, int32_t n, int32_t* pair, uint8_t* strand, int32_t* begin, int32_t* end, int32_t* edits,
                               int32_t* second, uint8_t* status) {
  const bool won = b.pair >= 0;
  *pair = won ? b.pair : -1;
  *strand = (uint8_t)(won ? b.strand : 0);
  *begin = !won ? 0 : b.strand ? b.cR : b.cF;
  *end = !won ? 0 : b.strand ? n - b.cF : n - b.cR;
  edits[0] = won ? b.eF : -1;
  edits[1] = won ? b.eR : -1;
  *second = won && b.second != kTrimNone ? b.second : -1;
  *status = (uint8_t)(won ? DNAS_TRIM_OK : b.anchored ? DNAS_TRIM_TOO_SHORT : DNAS_TRIM_NO_ANCHOR);
}

// Base c of the text of the search of strand s: F_k reads the strand from its front, reverse(R_k) from its end.
DNAS_HD inline int32_t trimTextBase(const int8_t* read, int32_t n, int32_t s, bool fromEnd, int32_t c) {
  // strand 0 is the read, strand 1 its reverse complement v[c] = 3 - read[n - 1 - c]; from the end the text is v[n - 1 - c]
  const int32_t b = (s == 1) == fromEnd ? read[c] & 3 : read[n - 1 - c] & 3;
  return s ? 3 - b : b;
}

// DNAS_OK or the code, dnas_last_error set: what dnas_trim_reads and dnas_trim_reads_host check.
int checkTrimArgs(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t n_reads, const int8_t* read_seqs,
                  const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors, int32_t min_payload,
                  const int32_t* out_pair, const uint8_t* out_strand, const int32_t* out_begin, const int32_t* out_end,
                  const int32_t* out_edits, const int32_t* out_second, const uint8_t* out_status);

// search(p, t) of the definition for the text of strand s (trimTextBase): the two-row dynamic program.  pat is read backwards
// when patReversed (reverse(R_k)).
TrimHit trimSearchHost(const int8_t* pat, int32_t m, bool patReversed, const int8_t* read, int32_t n, int32_t s, bool fromEnd,
                       int32_t maxOffset);

// The statement over reads [first, last): one thread.  The arguments were checked.
void trimReadsHost(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t first, int64_t last,
                   const int8_t* read_seqs, const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors,
                   int32_t min_payload, int32_t* out_pair, uint8_t* out_strand, int32_t* out_begin, int32_t* out_end, int32_t* out_edits,
                   int32_t* out_second, uint8_t* out_status);

}  // namespace dnas
