#include "consensus.hpp"

#include <cmath>
#include <string>
#include <vector>

#include "../errors.hpp"
#include "pairforward.hpp"

namespace dnas {

namespace {

// one concatenated set of sequences: offsets from 0 that ascend, lengths within the aligner's limit, base codes 0..3
int checkSeqs(const char* what, int64_t n, const int8_t* seqs, const int64_t* off) {
  if (n == 0) return DNAS_OK;
  if (!seqs || !off) return fail(DNAS_E_INVALID, "consensus: null argument");
  if (off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = off[i + 1] - off[i];
    if (len < 0) return fail(DNAS_E_INVALID, std::string(what) + " " + std::to_string(i) + ": inconsistent offsets");
    if (len > kAlignMaxSeq) return fail(DNAS_E_UNSUPPORTED, std::string(what) + " " + std::to_string(i) + ": longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < off[n]; ++j) if (seqs[j] < 0 || seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

int checkClusterOff(const char* what, int64_t n_clusters, const int64_t* off, int64_t n) {
  if (!off) return fail(DNAS_E_INVALID, "consensus: null argument");
  if (off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t c = 0; c < n_clusters; ++c)
    if (off[c + 1] < off[c]) return fail(DNAS_E_INVALID, "cluster " + std::to_string(c) + ": inconsistent " + what + " offsets");
  if (off[n_clusters] != n)
    return fail(DNAS_E_INVALID, std::string("consensus: the clusters' ") + what + " offsets end at " + std::to_string(off[n_clusters]) + ", not at " + std::to_string(n));
  return DNAS_OK;
}

}  // namespace

int checkConsensusArgs(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand, const int8_t* cand_seqs,
                       const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads, const int8_t* read_seqs,
                       const int64_t* read_off, const uint8_t* read_strand, const int64_t* cluster_read_off, const int64_t* out_winner,
                       const double* out_total, const double* out_second, const uint8_t* out_status) {
  if (!params || n_clusters < 0 || n_cand < 0 || n_reads < 0) return fail(DNAS_E_INVALID, "consensus: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "consensus: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen) return fail(DNAS_E_UNSUPPORTED, "consensus: more than 13 duplication lengths");
  if (n_clusters && (!out_winner || !out_total || !out_second || !out_status)) return fail(DNAS_E_INVALID, "consensus: null argument");
  if (int rc = checkClusterOff("candidate", n_clusters, cluster_cand_off, n_cand)) return rc;
  if (int rc = checkClusterOff("read", n_clusters, cluster_read_off, n_reads)) return rc;
  if (int rc = checkSeqs("candidate", n_cand, cand_seqs, cand_off)) return rc;
  if (int rc = checkSeqs("read", n_reads, read_seqs, read_off)) return rc;
  if (read_strand)
    for (int64_t i = 0; i < n_reads; ++i)
      if (read_strand[i] > 1) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": strand must be 0 or 1");
  return DNAS_OK;
}

void consensusScoreHost(const PairScores& sc, int64_t band, int64_t n_clusters, const int8_t* cand_seqs, const int64_t* cand_off,
                        const int64_t* cluster_cand_off, const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                        const int64_t* cluster_read_off, int64_t* out_winner, double* out_total, double* out_second,
                        uint8_t* out_status, double* out_totals, int score_mode) {
  std::vector<std::vector<int8_t>> oriented;             // the cluster's reads as they are scored
  for (int64_t c = 0; c < n_clusters; ++c) {
    const int64_t r0 = cluster_read_off[c], r1 = cluster_read_off[c + 1];
    oriented.assign((size_t)(r1 - r0), {});
    for (int64_t i = r0; i < r1; ++i) {
      const int8_t* const b = read_seqs + read_off[i];
      const int64_t O = read_off[i + 1] - read_off[i];
      std::vector<int8_t>& o = oriented[(size_t)(i - r0)];
      o.resize((size_t)O);
      for (int64_t j = 0; j < O; ++j) o[(size_t)j] = read_strand && read_strand[i] ? (int8_t)(3 - b[O - 1 - j]) : b[j];
    }
    ConsensusFold fold;
    for (int64_t j = cluster_cand_off[c]; j < cluster_cand_off[c + 1]; ++j) {
      double total = 0.0;
      for (int64_t i = r0; i < r1; ++i) {
        const int8_t* const a = cand_seqs + cand_off[j];
        const int8_t* const b = oriented[(size_t)(i - r0)].data();
        const int64_t I = cand_off[j + 1] - cand_off[j], O = read_off[i + 1] - read_off[i];
        total += score_mode == DNAS_SCORE_FORWARD ? forwardPairHost(sc, a, I, b, O, band, false, false)
                                                  : alignPairHost(sc, a, I, b, O, band, nullptr);
      }
      if (out_totals) out_totals[j] = total;
      fold.add(total, j);
    }
    const uint8_t status = ConsensusFold::status(cluster_cand_off[c + 1] - cluster_cand_off[c], r1 - r0, fold.winner);
    const bool ok = status == DNAS_CONSENSUS_OK;
    out_status[c] = status;
    out_winner[c] = ok ? fold.winner : -1;
    out_total[c] = ok ? fold.best : -__builtin_huge_val();
    out_second[c] = ok ? fold.second : -__builtin_huge_val();
  }
}

int checkScoreMode(int score_mode, const double* out_posterior) {
  if (score_mode != DNAS_SCORE_VITERBI && score_mode != DNAS_SCORE_FORWARD)
    return fail(DNAS_E_INVALID, "score_mode must be DNAS_SCORE_VITERBI or DNAS_SCORE_FORWARD");
  if (out_posterior && score_mode != DNAS_SCORE_FORWARD)
    return fail(DNAS_E_INVALID, "posteriors need DNAS_SCORE_FORWARD: Viterbi totals are not likelihoods");
  return DNAS_OK;
}

void consensusPosteriors(int64_t n_clusters, const int64_t* cluster_cand_off, const uint8_t* status, const double* totals,
                         double* out_posterior) {
  for (int64_t c = 0; c < n_clusters; ++c) {
    const int64_t j0 = cluster_cand_off[c], j1 = cluster_cand_off[c + 1];
    if (status[c] != DNAS_CONSENSUS_OK) {
      for (int64_t j = j0; j < j1; ++j) out_posterior[j] = 0.0;
      continue;
    }
    double m = -__builtin_huge_val();
    for (int64_t j = j0; j < j1; ++j) if (totals[j] > m) m = totals[j];
    double sum = 0.0;
    for (int64_t j = j0; j < j1; ++j) sum += std::exp(totals[j] - m);
    const double Z = m + std::log(sum);
    for (int64_t j = j0; j < j1; ++j) out_posterior[j] = std::exp(totals[j] - Z);
  }
}

}  // namespace dnas
