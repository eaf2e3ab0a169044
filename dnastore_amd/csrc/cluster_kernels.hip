// dnas_cluster_reads: the reads of a pool that are copies of one strand (include/dnastore_amd.h), bit-identical to
// clusterReadsHost (host/cluster.cpp).
//
// Sketch.  A wave per read: lanes take k-mer positions and keep the m running minima in registers, a wave min-reduction per
// position of the signature follows.  Integer arithmetic, stated once for host and device in host/cluster.hpp.
//
// Filter.  A tiled all-pairs compare of signatures.  A work-group owns a tile of 64 rows i and walks the column tiles j from its
// own diagonal to the end; both tiles are staged in LDS with a row stride of m + 1 words (lane l reads the signature of column
// l: with a stride of m all 64 lanes would stand on one bank).  A wave owns 16 rows of the tile, a lane a column, which it
// holds in registers while the 16 rows pass by as LDS broadcasts.  The count pass leaves every row's candidates; after a prefix
// sum on the host the emit pass walks the same tiles again and files the candidates of a band [lo, hi) of the list, by ballot and
// prefix popcount: a wave meets its row's j in ascending order, so the list is in (i, j) order without a sort or an atomic.
//
// The sketch, score and edge kernels and what happens to a band behind its list are in cluster_device.h, shared with the
// persistent clusterer (clusterer_kernels.hip).
//
// Score.  paScoreChunk of pair_align_device.h with an itemAt that reads (i, j) from the band's list: two items per pair, the
// second against the reverse complement of read j.  The launch plan, the chunk loop and the fan-out over devices are the shared
// ones.
//
// Edge.  One thread per pair picks the orientation, tests the floor (clusterPick, host/cluster.hpp) and appends the edge; the
// host sorts the edges before clusterComponents unites them.
//
// Gate.  With max_edit_permille >= 0 a band's list goes through the edit-distance gate first (cluster_gate_kernels.hip), which
// leaves the survivors in a second list; score and pick then walk that one.
#include "cluster_device.h"

namespace {

constexpr int kClTile = 64;                              // rows and columns of a filter tile
constexpr int kClWaves = 4;                              // waves of a filter work-group
constexpr int kClRowsPerWave = kClTile / kClWaves;

// A work-group's row tile against every column tile from its diagonal on.  Rows i0 .. i0 + 63 below rowEnd, columns below n.
// EMIT = false: count[i] = the candidates (i, j), j > i, of every row.  EMIT = true: rowOff[i] is the position of row i's first
// candidate in the call's list; those at positions lo <= pos < hi go to list[pos - lo].
template <int M, bool EMIT>
__device__ __forceinline__ void clFilterTile(int64_t n, const uint32_t* __restrict__ sig, const int64_t* __restrict__ readOff,
                                             int minShared, int64_t i0, int64_t rowEnd, int64_t* __restrict__ count,
                                             const int64_t* __restrict__ rowOff, int64_t lo, int64_t hi, ClPair* __restrict__ list) {
  constexpr int kStride = M + 1;
  __shared__ uint32_t rowSig[kClTile * kStride], colSig[kClTile * kStride];
  __shared__ uint8_t rowFull[kClTile], colFull[kClTile];   // the read is not empty
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  for (int idx = tid; idx < kClTile * M; idx += 64 * kClWaves) {
    const int r = idx / M, t = idx % M;
    rowSig[r * kStride + t] = i0 + r < rowEnd ? sig[(i0 + r) * M + t] : dnas::kClusterNoSig;
  }
  if (tid < kClTile) rowFull[tid] = i0 + tid < rowEnd && readOff[i0 + tid + 1] > readOff[i0 + tid];

  int run[kClRowsPerWave];                               // per row of this wave: candidates met so far (wave-uniform)
#pragma unroll
  for (int rr = 0; rr < kClRowsPerWave; ++rr) run[rr] = 0;
  int64_t base[kClRowsPerWave];
#pragma unroll
  for (int rr = 0; rr < kClRowsPerWave; ++rr) {
    const int64_t i = i0 + wv * kClRowsPerWave + rr;
    base[rr] = EMIT && i < rowEnd ? rowOff[i] : 0;
  }

  for (int64_t j0 = i0; j0 < n; j0 += kClTile) {
    __syncthreads();                                     // the row tile is staged; the last column tile has been read
    for (int idx = tid; idx < kClTile * M; idx += 64 * kClWaves) {
      const int r = idx / M, t = idx % M;
      colSig[r * kStride + t] = j0 + r < n ? sig[(j0 + r) * M + t] : dnas::kClusterNoSig;
    }
    if (tid < kClTile) colFull[tid] = j0 + tid < n && readOff[j0 + tid + 1] > readOff[j0 + tid];
    __syncthreads();
    const int64_t j = j0 + lane;
    uint32_t col[M];
    if (minShared > 0) {
#pragma unroll
      for (int t = 0; t < M; ++t) col[t] = colSig[lane * kStride + t];
    }
#pragma unroll
    for (int rr = 0; rr < kClRowsPerWave; ++rr) {
      const int r = wv * kClRowsPerWave + rr;
      const int64_t i = i0 + r;
      if (i >= rowEnd) continue;                         // (wave-uniform)
      int shared = 0;
      if (minShared > 0) {
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const uint32_t a = rowSig[r * kStride + t];
          shared += a == col[t] && a != dnas::kClusterNoSig;
        }
      }
      const bool cand = j < n && j > i && dnas::clusterCandidate(shared, minShared, rowFull[r], colFull[lane]);
      const unsigned long long mask = __ballot(cand);
      if (EMIT && cand) {
        const int64_t pos = base[rr] + run[rr] + __popcll(mask & ((1ull << lane) - 1));
        if (pos >= lo && pos < hi) list[pos - lo] = ClPair{(int32_t)i, (int32_t)j};
      }
      run[rr] += __popcll(mask);
    }
  }
  if (!EMIT && lane == 0) {
#pragma unroll
    for (int rr = 0; rr < kClRowsPerWave; ++rr) {
      const int64_t i = i0 + wv * kClRowsPerWave + rr;
      if (i < rowEnd) count[i] = run[rr];
    }
  }
}

// Row tile tileFirst + blockIdx.x * tileStride of the pool (the devices of a call interleave the tiles).
template <int M>
__global__ __launch_bounds__(64 * kClWaves) void cluster_filter_count_kernel(int64_t n, const uint32_t* __restrict__ sig,
                                                                            const int64_t* __restrict__ readOff, int minShared,
                                                                            int64_t tileFirst, int64_t tileStride,
                                                                            int64_t* __restrict__ count) {
  const int64_t i0 = (tileFirst + (int64_t)blockIdx.x * tileStride) * kClTile;
  if (i0 >= n) return;
  clFilterTile<M, false>(n, sig, readOff, minShared, i0, n, count, nullptr, 0, 0, nullptr);
}

// The band [lo, hi) of the list, whose candidates lie in the rows rowFirst .. rowEnd - 1: row tile blockIdx.x from rowFirst on.
template <int M>
__global__ __launch_bounds__(64 * kClWaves) void cluster_filter_emit_kernel(int64_t n, const uint32_t* __restrict__ sig,
                                                                           const int64_t* __restrict__ readOff, int minShared,
                                                                           int64_t rowFirst, int64_t rowEnd,
                                                                           const int64_t* __restrict__ rowOff, int64_t lo, int64_t hi,
                                                                           ClPair* __restrict__ list) {
  const int64_t i0 = rowFirst + (int64_t)blockIdx.x * kClTile;
  if (i0 >= rowEnd) return;
  clFilterTile<M, true>(n, sig, readOff, minShared, i0, rowEnd, nullptr, rowOff, lo, hi, list);
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct ClCall {
  dnas::PairScores hs;
  int band, k, m, minShared;
  double minScorePerNt;
  int64_t n;
  const int8_t* readSeqs;
  const int64_t* readOff;
  int maxO = 0;
  int64_t capPairs = 0;                                  // a band's pairs at most
  int32_t maxEditPermille = -1;                          // the gate, -1: none
  std::vector<int64_t> gateWords;                        // with the gate, per row i: words of the longest pattern a pair (i, j > i) can have
};

// Pass 1 of worker w of W: the reads, all signatures, and the candidate counts of the row tiles w, w + W, ... into count
// (rows of other workers' tiles are left alone).
int clSketchAndCount(const ClCall& c, ClDevice& d, int64_t w, int64_t W, std::vector<int64_t>* count) {
  DNAS_HIP_TRY(hipSetDevice(d.device));
  int rc;
  if ((rc = d.bufs.open())) return rc;
  for (hipEvent_t& e : d.ev) DNAS_HIP_TRY(hipEventCreate(&e));
  (void)hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, d.device);
  const int64_t n = c.n;
  if ((rc = paUpload(d.bufs, &d.dReads, c.readSeqs, (size_t)c.readOff[n]))) return rc;
  if ((rc = paUpload(d.bufs, &d.dReadOff, c.readOff, (size_t)n + 1))) return rc;
  if ((rc = paUpload(d.bufs, &d.dSub, c.hs.sub, 16))) return rc;
  if ((rc = paAlloc(d.bufs, &d.dSig, (size_t)n * (size_t)c.m))) return rc;
  if ((rc = paAlloc(d.bufs, &d.dCount, (size_t)n))) return rc;
  if ((rc = paAlloc(d.bufs, &d.dRowOff, (size_t)n + 1))) return rc;
  hipStream_t stream = d.bufs.stream;
  DNAS_HIP_TRY(hipMemsetAsync(d.dCount, 0, (size_t)n * sizeof(int64_t), stream));

  const unsigned sketchBlocks = (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)d.cus * 8);
  rc = d.timed(&d.stats.sketch_ms, [&] {
    clDispatchM(c.m, [&](auto mm) {
      hipLaunchKernelGGL(cluster_sketch_kernel<decltype(mm)::value>, dim3(sketchBlocks), dim3(256), 0, stream, n, d.dReads, d.dReadOff,
                         c.k, d.dSig);
    });
  });
  if (rc) return rc;

  const int64_t tiles = (n + kClTile - 1) / kClTile, mine = w < tiles ? (tiles - w + W - 1) / W : 0;
  if (mine > 0) {
    rc = d.timed(&d.stats.filter_ms, [&] {
      clDispatchM(c.m, [&](auto mm) {
        hipLaunchKernelGGL(cluster_filter_count_kernel<decltype(mm)::value>, dim3((unsigned)mine), dim3(64 * kClWaves), 0, stream, n,
                           d.dSig, d.dReadOff, c.minShared, w, W, d.dCount);
      });
    });
    if (rc) return rc;
  }
  std::vector<int64_t> all((size_t)n);
  DNAS_HIP_TRY(hipMemcpy(all.data(), d.dCount, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int64_t t = w; t < tiles; t += W)
    for (int64_t i = t * kClTile; i < std::min(n, (t + 1) * kClTile); ++i) (*count)[(size_t)i] = all[(size_t)i];
  return DNAS_OK;
}

// Pass 2: the bands `mine` of the list (band b is [b * capPairs, ...)), whose row offsets are rowOff: emit, score, pick.
int clScoreBands(const ClCall& c, ClDevice& d, const std::vector<int64_t>& rowOff, const std::vector<int64_t>& mine) {
  if (mine.empty()) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(d.device));
  hipStream_t stream = d.bufs.stream;
  const int64_t n = c.n, total = rowOff[(size_t)n];
  DNAS_HIP_TRY(hipMemcpy(d.dRowOff, rowOff.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));

  const PaScores sc = PaScores::from(c.hs);
  ClBand bd;
  bd.hs = &c.hs, bd.band = c.band, bd.minScorePerNt = c.minScorePerNt, bd.maxEditPermille = c.maxEditPermille, bd.readOff = c.readOff;
  int rc;
  if ((rc = paPlanScore(sc.P, clScoreKernelOf(), d.cus, c.maxO, "DNAS_CLUSTER_CHUNK", 2 * c.capPairs, &bd.plan))) return rc;
  bd.plan.chunkItems = 2 * c.capPairs;                   // a band is one chunk: DNAS_CLUSTER_CHUNK counts pairs, the plan read it as items

  if ((rc = paAlloc(d.bufs, &bd.dList, (size_t)c.capPairs))) return rc;
  if ((rc = paAlloc(d.bufs, &bd.dChunk, (size_t)bd.plan.chunkItems))) return rc;
  if ((rc = paAlloc(d.bufs, &bd.dBnd, bd.plan.bndDoubles()))) return rc;
  if ((rc = paAlloc(d.bufs, &bd.dEdgeCount, 1))) return rc;
  if ((rc = paAlloc(d.bufs, &bd.dEdges, (size_t)c.capPairs))) return rc;
  const bool gated = c.maxEditPermille >= 0;
  ClGate gate;
  if (gated) {
    if ((rc = gate.open(d.cus, *std::max_element(c.gateWords.begin(), c.gateWords.end())))) return rc;
    if ((rc = paAlloc(d.bufs, &bd.dSurv, (size_t)c.capPairs))) return rc;
    bd.gate = &gate;
  }

  PaCellMemo memo(c.maxO, c.maxO, c.band);
  for (int64_t b : mine) {
    const int64_t lo = b * c.capPairs, hi = std::min(total, lo + c.capPairs), pairs = hi - lo;
    // the rows with candidates in [lo, hi): from the last row that starts at or before lo to the first that starts at or after hi
    const int64_t rowFirst = std::upper_bound(rowOff.begin(), rowOff.end(), lo) - rowOff.begin() - 1;
    const int64_t rowEnd = std::lower_bound(rowOff.begin(), rowOff.end(), hi) - rowOff.begin();
    const unsigned tiles = (unsigned)((rowEnd - rowFirst + kClTile - 1) / kClTile);
    rc = d.timed(&d.stats.filter_ms, [&] {
      clDispatchM(c.m, [&](auto mm) {
        hipLaunchKernelGGL(cluster_filter_emit_kernel<decltype(mm)::value>, dim3(tiles), dim3(64 * kClWaves), 0, stream, n, d.dSig,
                           d.dReadOff, c.minShared, rowFirst, rowEnd, d.dRowOff, lo, hi, bd.dList);
      });
    });
    if (rc) return rc;
    const int64_t boundWords = gated ? *std::max_element(c.gateWords.begin() + rowFirst, c.gateWords.begin() + rowEnd) : 0;
    if ((rc = clRunBand(d, bd, memo, pairs, boundWords))) return rc;
  }
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_cluster_reads_gated(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                        double min_score_per_nt, int32_t max_edit_permille, int64_t n_reads, const int8_t* read_seqs,
                                        const int64_t* read_off, int device_id, int64_t* out_root, int64_t* out_cluster,
                                        uint8_t* out_strand, uint8_t* out_status, int64_t** out_edge_ij, double** out_edge_score,
                                        uint8_t** out_edge_strand, int64_t* out_n_edges, dnas_cluster_stats* out_stats,
                                        dnas_cluster_gate_stats* out_gate) {
  dnas_cluster_stats total{};
  dnas_cluster_gate_stats gate{};
  if (out_stats) *out_stats = total;
  if (out_gate) *out_gate = gate;
  if (const int rc = dnas::checkClusterArgs(params, band, k, m, min_shared, n_reads, read_seqs, read_off, out_root, out_cluster, out_strand,
                                            out_status))
    return rc;
  if (const int rc = dnas::checkClusterGate(max_edit_permille)) return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    std::vector<dnas::ClusterEdge> edges;
    if (n_reads == 0) return dnas::clusterExportEdges(edges, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges);
    ClCall c{dnas::PairScores::from(dnas::MutatorParams::fromC(*params)), band, k, m, min_shared, min_score_per_nt, n_reads, read_seqs, read_off};
    for (int64_t r = 0; r < n_reads; ++r) c.maxO = std::max(c.maxO, (int)(read_off[r + 1] - read_off[r]));
    c.maxEditPermille = max_edit_permille;
    if (max_edit_permille >= 0) {
      c.gateWords.assign((size_t)n_reads, 0);
      int64_t longest = 0;                               // among the reads after r
      for (int64_t r = n_reads - 1; r >= 0; --r) {
        c.gateWords[(size_t)r] = dnas::clusterGateWords(read_off[r + 1] - read_off[r], longest);
        longest = std::max(longest, read_off[r + 1] - read_off[r]);
      }
    }
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = devices.size();
    std::vector<std::unique_ptr<ClDevice>> devs;
    for (int device : devices) devs.emplace_back(new ClDevice), devs.back()->device = device;
    const auto closeAll = [&] {                          // (buffers are freed on the device that holds them)
      for (auto& d : devs) (void)hipSetDevice(d->device), d.reset();
    };

    std::vector<int64_t> rowOff((size_t)n_reads + 1, 0);
    {
      std::vector<int64_t> count((size_t)n_reads, 0);
      const int rc = dnas::forEachDevice(devices, [&](size_t w) { return clSketchAndCount(c, *devs[w], (int64_t)w, (int64_t)W, &count); });
      if (rc != DNAS_OK) return closeAll(), rc;
      for (int64_t i = 0; i < n_reads; ++i) rowOff[(size_t)i + 1] = rowOff[(size_t)i] + count[(size_t)i];
    }
    const int64_t candidates = rowOff[(size_t)n_reads];
    // a band: 2^21 pairs (2^22 items, a chunk of the score kernels), with several devices at most a quarter of a device's share
    c.capPairs = (int64_t)1 << 21;
    if (W > 1) c.capPairs = std::min<int64_t>(c.capPairs, (candidates + 4 * (int64_t)W - 1) / (4 * (int64_t)W));
    if (const char* s = getenv("DNAS_CLUSTER_CHUNK")) c.capPairs = std::min<int64_t>(c.capPairs, atoll(s));
    c.capPairs = std::max<int64_t>(c.capPairs, 1);
    const int64_t bands = (candidates + c.capPairs - 1) / c.capPairs;
    std::vector<int64_t> cost((size_t)bands);
    for (int64_t b = 0; b < bands; ++b) cost[(size_t)b] = std::min(candidates, (b + 1) * c.capPairs) - b * c.capPairs;
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    {
      const int rc = dnas::forEachDevice(devices, [&](size_t w) { return clScoreBands(c, *devs[w], rowOff, shard[w]); });
      if (rc != DNAS_OK) return closeAll(), rc;
    }
    for (const auto& d : devs) {
      total.sketch_ms = std::max(total.sketch_ms, d->stats.sketch_ms);
      total.filter_ms = std::max(total.filter_ms, d->stats.filter_ms);
      total.score_ms = std::max(total.score_ms, d->stats.score_ms);
      total.fold_ms = std::max(total.fold_ms, d->stats.fold_ms);
      total.candidates += d->stats.candidates;
      total.items += d->stats.items;
      total.cells += d->stats.cells;
      total.chunks += d->stats.chunks;
      gate.gate_ms = std::max(gate.gate_ms, d->gate.gate_ms);
      gate.tested += d->gate.tested;
      gate.passed += d->gate.passed;
      gate.long_pairs += d->gate.long_pairs;
      gate.word_steps += d->gate.word_steps;
      edges.insert(edges.end(), d->edges.begin(), d->edges.end());
    }
    closeAll();
    std::sort(edges.begin(), edges.end(), dnas::clusterEdgeLess);
    total.pairs = n_reads * (n_reads - 1) / 2;
    total.edges = (int64_t)edges.size();
    total.clusters = dnas::clusterComponents(n_reads, read_off, k, min_shared, edges, out_root, out_cluster, out_strand, out_status,
                                             &total.strand_conflicts);
    if (out_stats) *out_stats = total;
    if (out_gate) *out_gate = gate;
    return dnas::clusterExportEdges(edges, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges);
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

extern "C" int dnas_cluster_reads(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                  double min_score_per_nt, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                  int device_id, int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand, uint8_t* out_status,
                                  int64_t** out_edge_ij, double** out_edge_score, uint8_t** out_edge_strand, int64_t* out_n_edges,
                                  dnas_cluster_stats* out_stats) {
  return dnas_cluster_reads_gated(params, band, k, m, min_shared, min_score_per_nt, -1, n_reads, read_seqs, read_off, device_id, out_root,
                                  out_cluster, out_strand, out_status, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges, out_stats,
                                  nullptr);
}
