// Clustering a pool of reads (include/dnastore_amd.h, dnas_cluster_reads): the connected components of the graph whose edges are
// the pairs of reads a k-mer sketch lets through and the pair-HMM Viterbi score S(I,O) of pairalign.hpp confirms.  This file
// holds what the host statement and the kernels (cluster_kernels.hip) share, stated once for both: the k-mer code and its hash,
// the candidate test on two signatures, the pick of a pair's orientation and the test against the floor, and the union over
// the sorted edges, which is host code on both paths.
#pragma once
#include <cstdint>
#include <vector>

#include "pairalign.hpp"

#if defined(__HIP__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif

namespace dnas {

constexpr uint32_t kClusterNoSig = 0xFFFFFFFFu;

// The splitmix64 finaliser.
DNAS_HD inline uint64_t clusterMix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// The canonical code of the k-mer s[0..k): the smaller of its 2-bit code and its reverse complement's.
DNAS_HD inline uint64_t clusterKmerCode(const int8_t* s, int k) {
  uint64_t f = 0, r = 0;
  for (int q = 0; q < k; ++q) {
    f = f << 2 | (uint64_t)(s[q] & 3);
    r = r << 2 | (uint64_t)(3 - (s[k - 1 - q] & 3));
  }
  return f < r ? f : r;
}

// What k-mer code c offers position t of a signature.
DNAS_HD inline uint32_t clusterHash(uint64_t c, int t) {
  return (uint32_t)(clusterMix64(c + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
}

// Positions at which two signatures hold the same value, a read shorter than k (all kClusterNoSig) sharing none.
DNAS_HD inline int clusterShared(const uint32_t* a, const uint32_t* b, int m) {
  int shared = 0;
  for (int t = 0; t < m; ++t) shared += a[t] == b[t] && a[t] != kClusterNoSig;
  return shared;
}

// Is (i, j) a candidate: min_shared positions shared, or with min_shared = 0 (the filter is off) two reads that are not empty.
DNAS_HD inline bool clusterCandidate(int shared, int minShared, int64_t lenI, int64_t lenJ) {
  return minShared > 0 ? shared >= minShared : lenI > 0 && lenJ > 0;
}

struct ClusterEdge {
  int64_t i, j;
  double score;
  int32_t strand;
};

// A candidate's two item scores -> its better orientation (the reverse complement only when strictly greater) and whether it
// is an edge: one fp64 multiply, one compare.
DNAS_HD inline bool clusterPick(double forward, double reverse, double minScorePerNt, int64_t lenJ, double* best, int32_t* strand) {
  *strand = reverse > forward ? 1 : 0;
  *best = *strand ? reverse : forward;
  return *best >= minScorePerNt * (double)lenJ;
}

// The edit-distance gate between the candidate test and the score (include/dnastore_amd.h): e0 = d(read i, read j), e1 = d(read i,
// reverse complement of read j); the candidate passes iff the smaller is within max_edit_permille thousandths of the longer read,
// rounded down.  Integers only.
DNAS_HD inline bool clusterGatePass(int32_t e0, int32_t e1, int32_t maxEditPermille, int64_t lenI, int64_t lenJ) {
  const int64_t limit = (int64_t)maxEditPermille * (lenI > lenJ ? lenI : lenJ) / 1000;
  return (int64_t)(e0 < e1 ? e0 : e1) <= limit;
}

// The gate's unit of work: 64-row words of the shorter read (the pattern of the kernels).  A pair's both orientations step
// 2 x words x (length of the longer read) word-columns; more than kClusterGateRegWords words is the long route.
constexpr int kClusterGateRegWords = 8;
DNAS_HD inline int64_t clusterGateWords(int64_t lenI, int64_t lenJ) { return ((lenI < lenJ ? lenI : lenJ) + 63) / 64; }
DNAS_HD inline int64_t clusterGateWordSteps(int64_t lenI, int64_t lenJ) {
  return 2 * clusterGateWords(lenI, lenJ) * (lenI > lenJ ? lenI : lenJ);
}

inline bool clusterEdgeLess(const ClusterEdge& a, const ClusterEdge& b) { return a.i != b.i ? a.i < b.i : a.j < b.j; }

struct ClusterCandidate {
  int64_t i, j;
  double score[2];                                       // item 0: read j as given, item 1: its reverse complement
};

// The Levenshtein distance of a[0..la) and b[0..lb), or with rcB of a and the reverse complement of b: the two-row dynamic
// program, which is the statement the kernels of cluster_gate_kernels.hip are held to.
int32_t editDistanceHost(const int8_t* a, int64_t la, const int8_t* b, int64_t lb, bool rcB);

// DNAS_OK or the code: what dnas_edit_distances and dnas_edit_distances_host check.
int checkEditArgs(int64_t n_pairs, const int64_t* pair_ij, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                  const int32_t* out_dist);

// DNAS_OK, or DNAS_E_INVALID for a max_edit_permille outside -1 .. 1000.
int checkClusterGate(int32_t max_edit_permille);

// sig[m] of one read.
void clusterSketchHost(const int8_t* seq, int64_t len, int k, int m, uint32_t* sig);

// Union-find with parity over the edges, which are sorted by (i, j): root (the smallest index of the component), the dense id
// in order of first appearance, the orientation relative to the root and the status of every read.  -> the number of clusters;
// *conflicts: edges inside one component whose strand contradicts the parities (ignored).
int64_t clusterComponents(int64_t n, const int64_t* read_off, int k, int min_shared, const std::vector<ClusterEdge>& edges,
                          int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand, uint8_t* out_status, int64_t* conflicts);

// DNAS_OK or the code, dnas_last_error set: what dnas_cluster_reads and dnas_cluster_reads_host check.
int checkClusterArgs(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared, int64_t n_reads,
                     const int8_t* read_seqs, const int64_t* read_off, const int64_t* out_root, const int64_t* out_cluster,
                     const uint8_t* out_strand, const uint8_t* out_status);

// The edge outputs of the C ABI from the sorted edges: library-allocated (dnas_free), each may be null.
int clusterExportEdges(const std::vector<ClusterEdge>& edges, int64_t** out_edge_ij, double** out_edge_score, uint8_t** out_edge_strand,
                       int64_t* out_n_edges);

// The statement: one thread.  Signatures, every pair i < j through the candidate test in (i, j) order, with max_edit_permille >= 0
// the gate (a candidate that fails is not scored), alignPairHost for the two items of a candidate, the pick, the union.  The
// arguments were checked.  candidates: null, or receives every candidate that was scored.  gate: null, or receives the counts.
void clusterReadsHost(const PairScores& sc, int64_t band, int k, int m, int min_shared, double min_score_per_nt,
                      int32_t max_edit_permille, int64_t n_reads,
                      const int8_t* read_seqs, const int64_t* read_off, int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand,
                      uint8_t* out_status, std::vector<ClusterEdge>* edges, std::vector<ClusterCandidate>* candidates,
                      dnas_cluster_stats* stats, dnas_cluster_gate_stats* gate);

}  // namespace dnas
