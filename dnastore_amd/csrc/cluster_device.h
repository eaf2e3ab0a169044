// What the one-shot clustering call (cluster_kernels.hip) and the persistent clusterer (clusterer_kernels.hip) share on the
// device side: the sketch, score and edge kernels, a worker's state, and what happens to a band of the candidate list once a
// filter has emitted it (gate, score, pick, fetch).  The two filters differ, everything behind the list is stated here once.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "cluster_gate.hpp"
#include "devices.hpp"
#include "errors.hpp"
#include "host/cluster.hpp"
#include "host/pairalign.hpp"
#include "pair_align_device.h"

namespace {

// Reads 0 .. n - 1 of off (offsets into seqs) -> sig[r * M ..).
template <int M>
__global__ __launch_bounds__(256) void cluster_sketch_kernel(int64_t n, const int8_t* __restrict__ seqs, const int64_t* __restrict__ off,
                                                             int k, uint32_t* __restrict__ sig) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nWaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t r = wave; r < n; r += nWaves) {
    const int8_t* const s = seqs + off[r];
    const int64_t kmers = off[r + 1] - off[r] - k + 1;
    uint32_t mn[M];
#pragma unroll
    for (int t = 0; t < M; ++t) mn[t] = dnas::kClusterNoSig;
    for (int64_t p = lane; p < kmers; p += 64) {
      const uint64_t c = dnas::clusterKmerCode(s + p, k);
#pragma unroll
      for (int t = 0; t < M; ++t) {
        const uint32_t h = dnas::clusterHash(c, t);
        mn[t] = h < mn[t] ? h : mn[t];
      }
    }
    uint32_t mine = dnas::kClusterNoSig;                 // lane t ends up with position t
#pragma unroll
    for (int t = 0; t < M; ++t) {
      uint32_t v = mn[t];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
        v = o < v ? o : v;
      }
      if (lane == t) mine = v;
    }
    if (lane < M) sig[r * M + lane] = mine;
  }
}

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void cluster_score_kernel(
    PaScores sc, const double* __restrict__ subTable, int band, int ldsCols, int64_t first, int64_t count,
    const ClPair* __restrict__ list, const int8_t* __restrict__ readSeqs, const int64_t* __restrict__ readOff, double* bndScratch,
    int64_t bndStride, double* __restrict__ chunk) {
  const auto itemAt = [&](int64_t g) -> PaItem {         // pair g / 2 of the band: read j as a mutated copy of read i, g % 2 its strand
    const ClPair p = list[g >> 1];
    const int I = (int)(readOff[p.i + 1] - readOff[p.i]), O = (int)(readOff[p.j + 1] - readOff[p.j]);
    return {readSeqs + readOff[p.i], readSeqs + readOff[p.j], I, O, (g & 1) != 0};
  };
  paScoreChunk<KP>(sc, subTable, band, ldsCols, first, count, itemAt, bndScratch, bndStride, chunk);
}

// The pairs first / 2 .. of the band, whose item scores are chunk[0 .. 2 pairs).
__global__ void cluster_edge_kernel(int64_t firstPair, int64_t pairs, const ClPair* __restrict__ list, const double* __restrict__ chunk,
                                    const int64_t* __restrict__ readOff, double minScorePerNt, unsigned long long* __restrict__ nEdges,
                                    dnas::ClusterEdge* __restrict__ edges) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= pairs) return;
  const ClPair p = list[firstPair + q];
  dnas::ClusterEdge e{p.i, p.j, 0, 0};
  if (dnas::clusterPick(chunk[2 * q], chunk[2 * q + 1], minScorePerNt, readOff[p.j + 1] - readOff[p.j], &e.score, &e.strand))
    edges[atomicAdd(nEdges, 1ull)] = e;
}

// ---------------------------------------------------------------------------------------------------------------- host side

// f(std::integral_constant<int, M>) for the sketch size m, which the argument check left in {16, 32, 64}.
template <class F>
auto clDispatchM(int m, F&& f) {
  if (m == 16) return f(std::integral_constant<int, 16>{});
  if (m == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// What one worker of a call holds between its two passes.
struct ClDevice {
  int device = 0, cus = 256;
  PaBuffers bufs;
  int8_t* dReads = nullptr;
  int64_t *dReadOff = nullptr, *dCount = nullptr, *dRowOff = nullptr;
  uint32_t* dSig = nullptr;
  double* dSub = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  dnas_cluster_stats stats{};
  dnas_cluster_gate_stats gate{};
  std::vector<dnas::ClusterEdge> edges;
  ~ClDevice() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
  // the kernel launched by `launch`, timed into *ms
  template <class Launch>
  int timed(double* ms, Launch&& launch) {
    DNAS_HIP_TRY(hipEventRecord(ev[0], bufs.stream));
    launch();
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(ev[1], bufs.stream));
    DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
    float t = 0;
    DNAS_HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
    *ms += t;
    return DNAS_OK;
  }
};

inline auto clScoreKernelOf() {
  return [](auto kp) { return &cluster_score_kernel<decltype(kp)::value>; };
}

// A band's device buffers (capPairs pairs each, the chunk 2 capPairs scores) and what scoring it needs to know.
struct ClBand {
  const dnas::PairScores* hs = nullptr;
  int band = 0;
  double minScorePerNt = 0;
  int32_t maxEditPermille = -1;
  const int64_t* readOff = nullptr;                      // host
  PaLaunchPlan plan;
  ClPair *dList = nullptr, *dSurv = nullptr;             // dSurv with the gate only: the pairs of the band that passed
  double *dChunk = nullptr, *dBnd = nullptr;
  unsigned long long* dEdgeCount = nullptr;
  dnas::ClusterEdge* dEdges = nullptr;
  const ClGate* gate = nullptr;
  std::vector<ClPair> list;                              // scratch
};

// The band's list dList[0 .. pairs) has been emitted on d's stream; boundWords bounds its patterns for the gate.  Gate, score,
// pick; the edges are appended to d.edges and the counts added to d.stats and d.gate.
inline int clRunBand(ClDevice& d, ClBand& b, PaCellMemo& memo, int64_t pairs, int64_t boundWords) {
  hipStream_t stream = d.bufs.stream;
  int rc;
  DNAS_HIP_TRY(hipMemsetAsync(b.dEdgeCount, 0, sizeof(unsigned long long), stream));
  int64_t scored = pairs;                                // the pairs of the band that are scored, in dScored
  const ClPair* dScored = b.dList;
  if (b.maxEditPermille >= 0) {
    DNAS_HIP_TRY(hipMemsetAsync(b.gate->counts.get(), 0, 3 * sizeof(unsigned long long), stream));
    rc = d.timed(&d.gate.gate_ms, [&] {
      b.gate->run(stream, pairs, b.dList, d.dReads, d.dReadOff, boundWords, b.maxEditPermille, nullptr, b.dSurv);
    });
    if (rc) return rc;
    unsigned long long counts[3];
    DNAS_HIP_TRY(hipMemcpy(counts, b.gate->counts.get(), sizeof counts, hipMemcpyDeviceToHost));
    d.gate.tested += pairs;
    d.gate.passed += (int64_t)counts[0];
    d.gate.long_pairs += (int64_t)counts[1];
    d.gate.word_steps += (int64_t)counts[2];
    scored = (int64_t)counts[0];
    dScored = b.dSurv;
  }

  const PaScores sc = PaScores::from(*b.hs);
  const auto kernelOf = clScoreKernelOf();
  const auto score = [&](int64_t first, int64_t count) {
    paDispatchKP(sc.P, [&](auto kp) {
      hipLaunchKernelGGL(kernelOf(kp), dim3(b.plan.blocks(count)), dim3(64 * kPaWavesPerBlock), b.plan.ldsBytes, stream, sc, d.dSub, b.band,
                         b.plan.ldsCols, first, count, dScored, d.dReads, d.dReadOff, b.dBnd, b.plan.bndStride, b.dChunk);
    });
  };
  const auto pick = [&](int64_t first, int64_t count) {
    hipLaunchKernelGGL(cluster_edge_kernel, dim3((unsigned)((count / 2 + 255) / 256)), dim3(256), 0, stream, first / 2, count / 2, dScored,
                       b.dChunk, d.dReadOff, b.minScorePerNt, b.dEdgeCount, b.dEdges);
  };
  const auto after = [&](int64_t, int64_t) { return hipSuccess; };
  if ((rc = paRunChunks(d.bufs, 2 * scored, b.plan.chunkItems, score, pick, after, &d.stats))) return rc;

  unsigned long long nEdges = 0;
  DNAS_HIP_TRY(hipMemcpy(&nEdges, b.dEdgeCount, sizeof nEdges, hipMemcpyDeviceToHost));
  const size_t have = d.edges.size();
  d.edges.resize(have + (size_t)nEdges);
  if (nEdges) DNAS_HIP_TRY(hipMemcpy(d.edges.data() + have, b.dEdges, (size_t)nEdges * sizeof(dnas::ClusterEdge), hipMemcpyDeviceToHost));
  b.list.resize((size_t)scored);
  if (scored) DNAS_HIP_TRY(hipMemcpy(b.list.data(), dScored, (size_t)scored * sizeof(ClPair), hipMemcpyDeviceToHost));
  for (const ClPair& p : b.list)
    d.stats.cells += 2 * memo.cells(b.readOff[p.i + 1] - b.readOff[p.i], b.readOff[p.j + 1] - b.readOff[p.j]);
  d.stats.candidates += pairs;
  d.stats.items += 2 * scored;
  return DNAS_OK;
}

}  // namespace
