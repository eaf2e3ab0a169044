// Consensus by rescoring (include/dnastore_amd.h, dnas_consensus_score): of a cluster's candidate strands, the one under which
// the cluster's reads have the largest joint pair-HMM Viterbi score -- the sum over the reads of S(I,O) of pairalign.hpp.  This
// file holds what the host statement and the kernels (consensus_kernels.hip) share: the item arithmetic, the pick of a
// cluster's winner from its candidates' totals, stated once for both, and the argument checks.
#pragma once
#include <cstdint>

#include "pairalign.hpp"

#if defined(__HIP__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif

namespace dnas {

// The pick over a cluster's totals in candidate order.  best: the first total strictly greater than every earlier one (and than
// -inf); second: the largest among the others.  When the winner passes from candidate X to a later Y, every total seen so far
// is at most X's: the runner-up is the old best.
struct ConsensusFold {
  double best, second;
  int64_t winner;
  DNAS_HD ConsensusFold() : best(-__builtin_huge_val()), second(-__builtin_huge_val()), winner(-1) {}
  DNAS_HD void add(double total, int64_t cand) {
    if (total > best) {
      second = best;
      best = total;
      winner = cand;
    } else if (total > second) {
      second = total;
    }
  }
  DNAS_HD static uint8_t status(int64_t cands, int64_t reads, int64_t winner) {
    return cands == 0 ? DNAS_CONSENSUS_NO_CANDIDATES
                      : reads == 0 ? DNAS_CONSENSUS_NO_READS : (winner < 0 ? DNAS_CONSENSUS_NO_PATH : DNAS_CONSENSUS_OK);
  }
};

// Which items a call has.  Cluster c's are itemOff[c] .. itemOff[c+1] - 1, candidate-major: item itemOff[c] + j * reads + i is
// (candidate clusterCandOff[c] + j, read clusterReadOff[c] + i).  itemOff has one entry per cluster and one more; it is the only
// thing derived from the inputs, no list of items exists anywhere.
struct ConsensusItems {
  int64_t nClusters;
  const int64_t *clusterCandOff, *clusterReadOff, *itemOff;
  // the c with off[c] <= x < off[c+1] (clusters without candidates, reads or items are stepped over)
  DNAS_HD int64_t find(const int64_t* off, int64_t x) const {
    int64_t lo = 0, hi = nClusters;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
  }
  DNAS_HD int64_t reads(int64_t c) const { return clusterReadOff[c + 1] - clusterReadOff[c]; }
  DNAS_HD int64_t cands(int64_t c) const { return clusterCandOff[c + 1] - clusterCandOff[c]; }
  DNAS_HD void itemAt(int64_t g, int64_t* cand, int64_t* read) const {
    const int64_t c = find(itemOff, g), local = g - itemOff[c], n = reads(c);
    *cand = clusterCandOff[c] + local / n;
    *read = clusterReadOff[c] + local % n;
  }
  DNAS_HD int64_t candOfItem(int64_t g) const {
    int64_t cand, read;
    itemAt(g, &cand, &read);
    return cand;
  }
  // candidate j's first item (it has reads(c) of them, c its cluster)
  DNAS_HD int64_t firstItemOf(int64_t j, int64_t c) const { return itemOff[c] + (j - clusterCandOff[c]) * reads(c); }
};

// DNAS_OK or the code, dnas_last_error set: what dnas_consensus_score and dnas_consensus_score_host check.
int checkConsensusArgs(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand, const int8_t* cand_seqs,
                       const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads, const int8_t* read_seqs,
                       const int64_t* read_off, const uint8_t* read_strand, const int64_t* cluster_read_off, const int64_t* out_winner,
                       const double* out_total, const double* out_second, const uint8_t* out_status);

// The statement: one thread, alignPairHost per item (score_mode DNAS_SCORE_FORWARD: forwardPairHost in table mode), the sums left
// to right, the pick above.  The arguments were checked.
void consensusScoreHost(const PairScores& sc, int64_t band, int64_t n_clusters, const int8_t* cand_seqs, const int64_t* cand_off,
                        const int64_t* cluster_cand_off, const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                        const int64_t* cluster_read_off, int64_t* out_winner, double* out_total, double* out_second,
                        uint8_t* out_status, double* out_totals, int score_mode = DNAS_SCORE_VITERBI);

// What the _ex entries check beyond checkConsensusArgs: the mode, and that posteriors are asked of the forward mode only.
int checkScoreMode(int score_mode, const double* out_posterior);

// P(candidate | the cluster's reads) under a uniform prior over the cluster's listed candidates, from forward-mode totals: for a
// cluster with status OK exp(total_j - Z), Z = m + log(sum_j exp(total_j - m)), m the largest total, the sum in candidate order
// in fp64 (a -inf total gives 0); 0 for every candidate of a cluster with any other status.  Host libm on the GPU path and in
// the statement alike: the two agree bit for bit.
void consensusPosteriors(int64_t n_clusters, const int64_t* cluster_cand_off, const uint8_t* status, const double* totals,
                         double* out_posterior);

}  // namespace dnas
