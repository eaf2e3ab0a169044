#include "cluster.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../errors.hpp"

namespace dnas {

void clusterSketchHost(const int8_t* seq, int64_t len, int k, int m, uint32_t* sig) {
  for (int t = 0; t < m; ++t) sig[t] = kClusterNoSig;
  for (int64_t p = 0; p + k <= len; ++p) {
    const uint64_t c = clusterKmerCode(seq + p, k);
    for (int t = 0; t < m; ++t) sig[t] = std::min(sig[t], clusterHash(c, t));
  }
}

int64_t clusterComponents(int64_t n, const int64_t* read_off, int k, int min_shared, const std::vector<ClusterEdge>& edges,
                          int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand, uint8_t* out_status, int64_t* conflicts) {
  std::vector<int64_t> parent((size_t)n);
  std::vector<uint8_t> parity((size_t)n, 0);             // orientation relative to the parent
  for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = i;
  std::vector<int64_t> path;
  // -> the root of x; parity[x] then is x's orientation relative to it (the path is compressed)
  const auto find = [&](int64_t x) {
    path.clear();
    while (parent[(size_t)x] != x) path.push_back(x), x = parent[(size_t)x];
    uint8_t above = 0;                                   // orientation of the node above relative to the root
    for (size_t q = path.size(); q-- > 0;) {
      const int64_t y = path[q];
      above = parity[(size_t)y] ^= above;
      parent[(size_t)y] = x;
    }
    return x;
  };
  *conflicts = 0;
  for (const ClusterEdge& e : edges) {
    const int64_t ri = find(e.i), rj = find(e.j);
    const uint8_t s = (uint8_t)(parity[(size_t)e.i] ^ parity[(size_t)e.j] ^ (uint8_t)e.strand);   // root of j relative to root of i
    if (ri == rj) {
      if (s) ++*conflicts;
      continue;
    }
    const int64_t top = std::min(ri, rj), sub = std::max(ri, rj);
    parent[(size_t)sub] = top;
    parity[(size_t)sub] = s;
  }
  int64_t clusters = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = find(i), len = read_off[i + 1] - read_off[i];
    out_root[i] = r;
    out_strand[i] = parity[(size_t)i];
    out_cluster[i] = r == i ? clusters++ : out_cluster[r];   // (a root is the smallest index of its component: it came first)
    out_status[i] = len == 0 ? DNAS_CLUSTER_EMPTY : (min_shared >= 1 && len < k ? DNAS_CLUSTER_NO_SKETCH : DNAS_CLUSTER_OK);
  }
  return clusters;
}

int checkClusterArgs(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared, int64_t n_reads,
                     const int8_t* read_seqs, const int64_t* read_off, const int64_t* out_root, const int64_t* out_cluster,
                     const uint8_t* out_strand, const uint8_t* out_status) {
  if (!params || n_reads < 0) return fail(DNAS_E_INVALID, "cluster reads: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "cluster reads: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen) return fail(DNAS_E_UNSUPPORTED, "cluster reads: more than 13 duplication lengths");
  if (k < 1 || k > 31) return fail(DNAS_E_INVALID, "cluster reads: k must be 1 .. 31");
  if (m != 16 && m != 32 && m != 64) return fail(DNAS_E_INVALID, "cluster reads: the sketch has 16, 32 or 64 positions");
  if (min_shared < 0) return fail(DNAS_E_INVALID, "cluster reads: min_shared must be at least 0");
  if (n_reads >= ((int64_t)1 << 31)) return fail(DNAS_E_UNSUPPORTED, "cluster reads: 2^31 reads or more");
  if (n_reads == 0) return DNAS_OK;
  if (!read_seqs || !read_off || !out_root || !out_cluster || !out_strand || !out_status)
    return fail(DNAS_E_INVALID, "cluster reads: null argument");
  if (read_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t O = read_off[i + 1] - read_off[i];
    if (O < 0) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": inconsistent offsets");
    if (O > kAlignMaxSeq) return fail(DNAS_E_UNSUPPORTED, "read " + std::to_string(i) + ": longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < read_off[n_reads]; ++j) if (read_seqs[j] < 0 || read_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

int checkClusterGate(int32_t max_edit_permille) {
  if (max_edit_permille < -1 || max_edit_permille > 1000) return fail(DNAS_E_INVALID, "cluster reads: max_edit_permille must be -1 .. 1000");
  return DNAS_OK;
}

int checkEditArgs(int64_t n_pairs, const int64_t* pair_ij, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                  const int32_t* out_dist) {
  if (n_pairs < 0) return fail(DNAS_E_INVALID, "edit distances: bad argument");
  const dnas_mutator_params none{};
  const int64_t i64 = 0;
  const uint8_t u8 = 0;
  if (const int rc = checkClusterArgs(&none, 0, 1, 16, 0, n_reads, read_seqs, read_off, &i64, &i64, &u8, &u8)) return rc;
  if (n_pairs == 0) return DNAS_OK;
  if (!pair_ij || !out_dist) return fail(DNAS_E_INVALID, "edit distances: null argument");
  for (int64_t q = 0; q < 2 * n_pairs; ++q)
    if (pair_ij[q] < 0 || pair_ij[q] >= n_reads)
      return fail(DNAS_E_INVALID, "edit distances: pair " + std::to_string(q / 2) + " names a read outside 0 .. n_reads - 1");
  return DNAS_OK;
}

int32_t editDistanceHost(const int8_t* a, int64_t la, const int8_t* b, int64_t lb, bool rcB) {
  std::vector<int32_t> prev((size_t)lb + 1), cur((size_t)lb + 1);
  for (int64_t j = 0; j <= lb; ++j) prev[(size_t)j] = (int32_t)j;
  for (int64_t i = 1; i <= la; ++i) {
    cur[0] = (int32_t)i;
    for (int64_t j = 1; j <= lb; ++j) {
      const int8_t bj = rcB ? (int8_t)(3 - b[lb - j]) : b[j - 1];
      const int32_t sub = prev[(size_t)j - 1] + (a[i - 1] != bj), del = prev[(size_t)j] + 1, ins = cur[(size_t)j - 1] + 1;
      cur[(size_t)j] = std::min(sub, std::min(del, ins));
    }
    prev.swap(cur);
  }
  return prev[(size_t)lb];
}

int clusterExportEdges(const std::vector<ClusterEdge>& edges, int64_t** out_edge_ij, double** out_edge_score, uint8_t** out_edge_strand,
                       int64_t* out_n_edges) {
  const size_t n = edges.size();
  if (out_n_edges) *out_n_edges = (int64_t)n;
  if (out_edge_ij) *out_edge_ij = nullptr;
  if (out_edge_score) *out_edge_score = nullptr;
  if (out_edge_strand) *out_edge_strand = nullptr;
  int64_t* ij = out_edge_ij ? (int64_t*)malloc(std::max<size_t>(n, 1) * 2 * sizeof(int64_t)) : nullptr;
  double* score = out_edge_score ? (double*)malloc(std::max<size_t>(n, 1) * sizeof(double)) : nullptr;
  uint8_t* strand = out_edge_strand ? (uint8_t*)malloc(std::max<size_t>(n, 1)) : nullptr;
  if ((out_edge_ij && !ij) || (out_edge_score && !score) || (out_edge_strand && !strand)) {
    free(ij); free(score); free(strand);
    return fail(DNAS_E_NOMEM, "out of memory");
  }
  for (size_t e = 0; e < n; ++e) {
    if (ij) ij[2 * e] = edges[e].i, ij[2 * e + 1] = edges[e].j;
    if (score) score[e] = edges[e].score;
    if (strand) strand[e] = (uint8_t)edges[e].strand;
  }
  if (out_edge_ij) *out_edge_ij = ij;
  if (out_edge_score) *out_edge_score = score;
  if (out_edge_strand) *out_edge_strand = strand;
  return DNAS_OK;
}

void clusterReadsHost(const PairScores& sc, int64_t band, int k, int m, int min_shared, double min_score_per_nt,
                      int32_t max_edit_permille, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int64_t* out_root,
                      int64_t* out_cluster, uint8_t* out_strand,
                      uint8_t* out_status, std::vector<ClusterEdge>* edges, std::vector<ClusterCandidate>* candidates,
                      dnas_cluster_stats* stats, dnas_cluster_gate_stats* gate) {
  *stats = dnas_cluster_stats{};
  if (gate) *gate = dnas_cluster_gate_stats{};
  edges->clear();
  if (candidates) candidates->clear();
  if (n_reads == 0) return;
  std::vector<uint32_t> sig((size_t)n_reads * (size_t)m);
  for (int64_t i = 0; i < n_reads; ++i)
    clusterSketchHost(read_seqs + read_off[i], read_off[i + 1] - read_off[i], k, m, sig.data() + (size_t)i * (size_t)m);
  stats->pairs = n_reads * (n_reads - 1) / 2;
  std::vector<int8_t> rc;
  int64_t passed = 0;                                    // candidates that are scored: all of them without the gate
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t I = read_off[i + 1] - read_off[i];
    for (int64_t j = i + 1; j < n_reads; ++j) {
      const int64_t O = read_off[j + 1] - read_off[j];
      const int shared = min_shared > 0 ? clusterShared(sig.data() + (size_t)i * (size_t)m, sig.data() + (size_t)j * (size_t)m, m) : 0;
      if (!clusterCandidate(shared, min_shared, I, O)) continue;
      const int8_t* const b = read_seqs + read_off[j];
      ++stats->candidates;
      if (max_edit_permille >= 0) {
        const int8_t* const a = read_seqs + read_off[i];
        const int32_t e0 = editDistanceHost(a, I, b, O, false), e1 = editDistanceHost(a, I, b, O, true);
        const bool pass = clusterGatePass(e0, e1, max_edit_permille, I, O);
        if (gate) {
          ++gate->tested;
          gate->passed += pass;
          gate->long_pairs += clusterGateWords(I, O) > kClusterGateRegWords;
          gate->word_steps += clusterGateWordSteps(I, O);
        }
        if (!pass) continue;
      }
      ++passed;
      rc.resize((size_t)O);
      for (int64_t q = 0; q < O; ++q) rc[(size_t)q] = (int8_t)(3 - b[O - 1 - q]);
      ClusterCandidate c{i, j, {0, 0}};
      c.score[0] = alignPairHost(sc, read_seqs + read_off[i], I, b, O, band, nullptr);
      c.score[1] = alignPairHost(sc, read_seqs + read_off[i], I, rc.data(), O, band, nullptr);
      stats->cells += 2 * PairBand(I, O, band).cells(I, O);
      ClusterEdge e{i, j, 0, 0};
      if (clusterPick(c.score[0], c.score[1], min_score_per_nt, O, &e.score, &e.strand)) edges->push_back(e);
      if (candidates) candidates->push_back(c);
    }
  }
  stats->items = 2 * passed;
  stats->edges = (int64_t)edges->size();
  stats->clusters = clusterComponents(n_reads, read_off, k, min_shared, *edges, out_root, out_cluster, out_strand, out_status,
                                      &stats->strand_conflicts);
}

}  // namespace dnas
