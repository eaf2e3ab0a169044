// Consensus reads (include/dnastore_amd.h, dnas_cluster_consensus): the reads of a cluster aligned to a template, the columns of
// the alignments voted into integer counters, a new template emitted from them, round after round.  This file holds what the host
// statement and the kernels (polish_kernels.hip) share -- the layout of a cluster's table and the emit of one gap, stated once
// for both --, the argument checks, and the statement itself.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pairalign.hpp"

#if defined(__HIP__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif

namespace dnas {

// A cluster's table: word 0 is V, then 25 words per position p = 0 .. I (a position is a template base and the gap before it;
// p = I is the gap after the last base): M[p][4], D[p], N[p][4], B[p][4][4].
constexpr int kPolishRow = 25;
DNAS_HD inline size_t polishWords(int64_t I) { return 1 + (size_t)kPolishRow * (size_t)(I + 1); }
DNAS_HD inline size_t polishM(int64_t p, int base) { return 1 + (size_t)kPolishRow * (size_t)p + (size_t)base; }
DNAS_HD inline size_t polishD(int64_t p) { return 1 + (size_t)kPolishRow * (size_t)p + 4; }
DNAS_HD inline size_t polishN(int64_t p, int k) { return 1 + (size_t)kPolishRow * (size_t)p + 5 + (size_t)k; }
DNAS_HD inline size_t polishB(int64_t p, int k, int base) { return 1 + (size_t)kPolishRow * (size_t)p + 9 + 4 * (size_t)k + (size_t)base; }

// What step 3 emits for g: n <= DNAS_POLISH_MAX_INSERT + 1 bases, base j at bits 2j of `bases`.
struct PolishGap {
  int n;
  unsigned bases;
};
DNAS_HD inline PolishGap polishEmitGap(const uint32_t* tab, int64_t g, int64_t I, const int8_t* t) {
  PolishGap e{0, 0};
  const uint32_t V = tab[0];
  for (int k = 0; k < DNAS_POLISH_MAX_INSERT && 2 * tab[polishN(g, k)] > V; ++k) {
    int best = 0;
    for (int b = 1; b < 4; ++b)
      if (tab[polishB(g, k, b)] > tab[polishB(g, k, best)]) best = b;
    e.bases |= (unsigned)best << (2 * e.n++);
  }
  if (g < I && !(2 * tab[polishD(g)] > V)) {
    int best = 0;
    for (int b = 1; b < 4; ++b)
      if (tab[polishM(g, b)] > tab[polishM(g, best)]) best = b;
    const int tb = t[g] & 3;
    if (tab[polishM(g, tb)] == tab[polishM(g, best)]) best = tb;
    e.bases |= (unsigned)best << (2 * e.n++);
  }
  return e;
}

// The bases a round can add to a template of I bases whose reads are at most maxO long: an insertion base needs more than V / 2
// of the V voters' duplication columns, of which there are at most V x maxO, and a gap takes at most DNAS_POLISH_MAX_INSERT.
inline int64_t polishCapacity(int64_t I, int64_t maxO) { return I + std::min<int64_t>(DNAS_POLISH_MAX_INSERT * (I + 1), 2 * maxO); }

// DNAS_OK or the code, dnas_last_error set: what dnas_cluster_consensus and dnas_cluster_consensus_host check.
int checkPolishArgs(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, const int8_t* tmpl_seqs, const int64_t* tmpl_off,
                    int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                    const int64_t* cluster_read_off, int32_t rounds_max, int8_t* const* out_seqs, const int64_t* out_off,
                    const int32_t* out_rounds, const uint8_t* out_converged, const int32_t* out_voters, const uint8_t* out_status);

// One cluster's state between rounds, and what the host makes of a round's outcome -- the same for the statement and the GPU.
struct PolishCluster {
  int32_t rounds = 0, voters = 0;
  uint8_t converged = 0, status = DNAS_POLISH_OK;
  bool active = true;
  // the round that just ran had `voters` voters and changed the template or not; roundsRun counts it
  void after(int32_t votersNow, bool changed, int32_t roundsRun, int32_t roundsMax) {
    voters = votersNow;
    if (votersNow == 0) { status = DNAS_POLISH_NO_VOTERS; active = false; return; }
    status = DNAS_POLISH_OK;
    if (!changed) { converged = 1; active = false; return; }
    ++rounds;
    if (roundsRun >= roundsMax) active = false;
  }
};

// One round of one cluster: the oriented reads aligned to t, walked, the new template emitted -> V.
int32_t polishRoundHost(const PairScores& sc, int64_t band, const std::vector<int8_t>& t, const std::vector<std::vector<int8_t>>& reads,
                        std::vector<int8_t>* out);

// The statement: one thread, alignPairHost per pair.  The arguments were checked.
void clusterConsensusHost(const PairScores& sc, int64_t band, int64_t n_clusters, const int8_t* tmpl_seqs, const int64_t* tmpl_off,
                          const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand, const int64_t* cluster_read_off,
                          int32_t rounds_max, std::vector<std::vector<int8_t>>* seqs, int32_t* out_rounds, uint8_t* out_converged,
                          int32_t* out_voters, uint8_t* out_status);

// The consensus reads concatenated into a malloc'd array (dnas_free) and their offsets.
int polishExport(const std::vector<std::vector<int8_t>>& seqs, int8_t** out_seqs, int64_t* out_off);

}  // namespace dnas
