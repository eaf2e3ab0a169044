// The edit-distance gate of dnas_cluster_reads_gated and dnas_edit_distances (include/dnastore_amd.h), bit-identical to
// editDistanceHost and clusterGatePass (host/cluster.cpp, host/cluster.hpp).  The recurrence is stated in cluster_gate.hpp.
//
// A thread per pair, a wave per work-group.  The pattern is the shorter read of the pair, the text the longer: the words a thread
// carries are set by the pattern and the columns it walks by the text, and d(i, j) = d(j, i), d(i, rc j) = d(j, rc i), so either
// read may be the pattern.  (Read i is shared by most lanes of a wave, but a shared pattern would save only the mask build, a few
// percent of a pair; a short pattern halves the words of every column.)  Both orientations advance in one loop over the text's
// columns: the second reads the text from its end with 3 - b, and both use the one table of match masks.
//
// Register route, edit_distance_kernel<W>, W = 1, 2, 4, 8: Pv[W], Mv[W] and the score of each orientation in registers, the masks
// Peq[base][word][thread] in LDS -- 64 threads x 8 bytes are the 64 banks of a ds_read_b64, whatever base each lane asks for.  A
// launch takes the smallest W that holds the longest pattern the list can have; pairs of more than regWords (8, or
// DNAS_CLUSTER_GATE_WORDS) words are left to the long route, edit_distance_long_kernel, whose masks and vectors live in a slice
// of a device buffer laid out [word][thread]: any length, no speed.  Each kernel skips the other's pairs.
//
// GATE = false stores both distances of every pair.  GATE = true tests them against the limit and compacts the survivors: a
// ballot and a popcount per wave, one atomic per wave, the survivors in any order (the edges are sorted at the end).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "cluster_gate.hpp"
#include "devices.hpp"
#include "errors.hpp"
#include "pair_align_device.h"

namespace {

constexpr int kGateLanes = 64;                           // threads of a work-group: one wave
constexpr size_t kGateScratchBytes = (size_t)256 << 20;  // the long route's slices at most

struct GateView {
  const int8_t *pat, *txt;
  int m, n;                                              // m <= n
  int64_t lenI, lenJ;
};

__device__ __forceinline__ GateView gateView(ClPair p, const int8_t* __restrict__ seqs, const int64_t* __restrict__ off) {
  const int64_t oi = off[p.i], oj = off[p.j], li = off[p.i + 1] - oi, lj = off[p.j + 1] - oj;
  return lj < li ? GateView{seqs + oj, seqs + oi, (int)lj, (int)li, li, lj} : GateView{seqs + oi, seqs + oj, (int)li, (int)lj, li, lj};
}

// Does the register route serve a pattern of `words` words?
__host__ __device__ inline bool gateInRegs(int64_t words, int regWords) { return regWords > 0 && words <= regWords; }

__device__ __forceinline__ unsigned long long gateWaveSum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// What a wave does with the distances of its pairs (every lane of the wave arrives here; `mine`: the lane has a pair of this kernel).
template <bool GATE>
__device__ __forceinline__ void gateFinish(bool mine, bool longRoute, int64_t q, ClPair p, const GateView& v, const int32_t* e,
                                           int32_t maxEditPermille, int32_t* __restrict__ dist, ClPair* __restrict__ surv,
                                           unsigned long long* __restrict__ counts) {
  if (!GATE) {
    if (mine) dist[2 * q] = e[0], dist[2 * q + 1] = e[1];
    return;
  }
  const int lane = threadIdx.x & 63;
  const bool pass = mine && dnas::clusterGatePass(e[0], e[1], maxEditPermille, v.lenI, v.lenJ);
  const unsigned long long passMask = __ballot(pass), mineMask = __ballot(mine);
  if (mineMask == 0) return;                             // (wave-uniform)
  const unsigned long long steps = gateWaveSum(mine ? (unsigned long long)dnas::clusterGateWordSteps(v.lenI, v.lenJ) : 0ull);
  unsigned long long base = 0;
  if (lane == 0) {
    if (passMask) base = atomicAdd(&counts[0], (unsigned long long)__popcll(passMask));
    if (longRoute) atomicAdd(&counts[1], (unsigned long long)__popcll(mineMask));
    atomicAdd(&counts[2], steps);
  }
  base = __shfl(base, 0);
  if (pass) surv[base + __popcll(passMask & ((1ull << lane) - 1))] = p;
}

template <int W, bool GATE>
__global__ __launch_bounds__(kGateLanes) void edit_distance_kernel(int64_t pairs, const ClPair* __restrict__ list,
                                                                   const int8_t* __restrict__ seqs, const int64_t* __restrict__ off,
                                                                   int regWords, int32_t maxEditPermille, int32_t* __restrict__ dist,
                                                                   ClPair* __restrict__ surv, unsigned long long* __restrict__ counts) {
  __shared__ uint64_t peq[4 * W * kGateLanes];           // [base][word][thread]
  const int lane = threadIdx.x;
  for (int64_t q0 = (int64_t)blockIdx.x * kGateLanes; q0 < pairs; q0 += (int64_t)gridDim.x * kGateLanes) {
    const int64_t q = q0 + lane;
    ClPair p{0, 0};
    GateView v{nullptr, nullptr, 0, 0, 0, 0};
    int32_t e[2] = {0, 0};
    bool mine = false;
    if (q < pairs) {
      p = list[q];
      v = gateView(p, seqs, off);
      const int words = (v.m + 63) >> 6;
      mine = gateInRegs(words, regWords) && words <= W;
    }
    if (mine) dnas::gatePairWords<W>(v.pat, v.m, v.txt, v.n, peq + lane, kGateLanes, e);
    gateFinish<GATE>(mine, false, q, p, v, e, maxEditPermille, dist, surv, counts);
  }
}

// Thread t of the grid's T owns scratch[x * T + t], x < 8 maxWords.
template <bool GATE>
__global__ __launch_bounds__(kGateLanes) void edit_distance_long_kernel(int64_t pairs, const ClPair* __restrict__ list,
                                                                        const int8_t* __restrict__ seqs, const int64_t* __restrict__ off,
                                                                        int regWords, int maxWords, uint64_t* __restrict__ scratch,
                                                                        int32_t maxEditPermille, int32_t* __restrict__ dist,
                                                                        ClPair* __restrict__ surv, unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x;
  const int64_t threads = (int64_t)gridDim.x * kGateLanes, tid = (int64_t)blockIdx.x * kGateLanes + lane;
  for (int64_t q0 = (int64_t)blockIdx.x * kGateLanes; q0 < pairs; q0 += threads) {
    const int64_t q = q0 + lane;
    ClPair p{0, 0};
    GateView v{nullptr, nullptr, 0, 0, 0, 0};
    int32_t e[2] = {0, 0};
    bool mine = false;
    if (q < pairs) {
      p = list[q];
      v = gateView(p, seqs, off);
      const int words = (v.m + 63) >> 6;
      mine = !gateInRegs(words, regWords) && words <= maxWords;   // (a longer pattern than the slice holds cannot be: open() sized it)
    }
    if (mine) dnas::gatePairLong(v.pat, v.m, v.txt, v.n, scratch + tid, threads, e);
    gateFinish<GATE>(mine, true, q, p, v, e, maxEditPermille, dist, surv, counts);
  }
}

// f(std::integral_constant<int, W>) for the smallest instance that holds `words` words (at most 8).
template <class F>
void gateDispatchW(int64_t words, F&& f) {
  if (words <= 1) f(std::integral_constant<int, 1>{});
  else if (words <= 2) f(std::integral_constant<int, 2>{});
  else if (words <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

}  // namespace

int ClGate::open(int cus_, int64_t callBoundWords) {
  cus = cus_;
  regWords = dnas::kClusterGateRegWords;
  if (const char* s = getenv("DNAS_CLUSTER_GATE_WORDS")) regWords = std::max(0, std::min(regWords, atoi(s)));
  DNAS_HIP_TRY(counts.assign(3));
  longWords = 0;
  if (!gateInRegs(callBoundWords, regWords)) {
    longWords = (int)std::max<int64_t>(callBoundWords, 1);
    const size_t perWave = (size_t)8 * (size_t)longWords * kGateLanes * sizeof(uint64_t);
    longBlocks = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)cus * 4, kGateScratchBytes / perWave));
    DNAS_HIP_TRY(scratch.assign(perWave * longBlocks / sizeof(uint64_t)));
  }
  return DNAS_OK;
}

void ClGate::run(hipStream_t stream, int64_t pairs, const ClPair* list, const int8_t* readSeqs, const int64_t* readOff, int64_t boundWords,
                 int32_t maxEditPermille, int32_t* dist, ClPair* surv) const {
  if (pairs <= 0) return;
  const int64_t waves = (pairs + kGateLanes - 1) / kGateLanes;
  const auto both = [&](auto&& launch) {                 // launch(std::bool_constant<GATE>)
    if (dist) launch(std::false_type{});
    else launch(std::true_type{});
  };
  if (regWords > 0) {
    const unsigned blocks = (unsigned)std::min<int64_t>(waves, (int64_t)cus * 32);
    gateDispatchW(std::min<int64_t>(boundWords, regWords), [&](auto ww) {
      both([&](auto gate) {
        hipLaunchKernelGGL((edit_distance_kernel<decltype(ww)::value, decltype(gate)::value>), dim3(blocks), dim3(kGateLanes), 0, stream, pairs,
                           list, readSeqs, readOff, regWords, maxEditPermille, dist, surv, counts.get());
      });
    });
  }
  if (longWords > 0 && !gateInRegs(boundWords, regWords)) {
    const unsigned blocks = (unsigned)std::min<int64_t>(waves, longBlocks);
    both([&](auto gate) {
      hipLaunchKernelGGL((edit_distance_long_kernel<decltype(gate)::value>), dim3(blocks), dim3(kGateLanes), 0, stream, pairs, list, readSeqs,
                         readOff, regWords, longWords, scratch.get(), maxEditPermille, dist, surv, counts.get());
    });
  }
}

namespace {

// One worker of dnas_edit_distances: the pairs `mine` (chunks of chunkPairs pairs of the call's list) on one device.
int gateDistancesOn(int device, const std::vector<int64_t>& mine, int64_t chunkPairs, int64_t n_pairs, const int64_t* pair_ij,
                    int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int32_t* out_dist) {
  if (mine.empty()) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  PaBuffers bufs;
  int rc, cus = 256;
  if ((rc = bufs.open())) return rc;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  std::vector<ClPair> list;
  int64_t boundWords = 0;
  for (int64_t c : mine)
    for (int64_t q = c * chunkPairs; q < std::min(n_pairs, (c + 1) * chunkPairs); ++q) {
      const int64_t i = pair_ij[2 * q], j = pair_ij[2 * q + 1];
      list.push_back(ClPair{(int32_t)i, (int32_t)j});
      boundWords = std::max(boundWords, dnas::clusterGateWords(read_off[i + 1] - read_off[i], read_off[j + 1] - read_off[j]));
    }
  int8_t* dReads = nullptr;
  int64_t* dReadOff = nullptr;
  ClPair* dList = nullptr;
  int32_t* dDist = nullptr;
  if ((rc = paUpload(bufs, &dReads, read_seqs, (size_t)read_off[n_reads]))) return rc;
  if ((rc = paUpload(bufs, &dReadOff, read_off, (size_t)n_reads + 1))) return rc;
  if ((rc = paUpload(bufs, &dList, list.data(), list.size()))) return rc;
  if ((rc = paAlloc(bufs, &dDist, 2 * list.size()))) return rc;
  ClGate gate;
  if ((rc = gate.open(cus, boundWords))) return rc;
  gate.run(bufs.stream, (int64_t)list.size(), dList, dReads, dReadOff, boundWords, 0, dDist, nullptr);
  DNAS_HIP_TRY(hipGetLastError());
  DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
  std::vector<int32_t> dist(2 * list.size());
  DNAS_HIP_TRY(hipMemcpy(dist.data(), dDist, dist.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  size_t at = 0;
  for (int64_t c : mine)
    for (int64_t q = c * chunkPairs; q < std::min(n_pairs, (c + 1) * chunkPairs); ++q, ++at)
      out_dist[2 * q] = dist[2 * at], out_dist[2 * q + 1] = dist[2 * at + 1];
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_edit_distances(int64_t n_pairs, const int64_t* pair_ij, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                   int device_id, int32_t* out_dist) {
  if (const int rc = dnas::checkEditArgs(n_pairs, pair_ij, n_reads, read_seqs, read_off, out_dist)) return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  if (n_pairs == 0) return DNAS_OK;
  try {
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const int64_t W = (int64_t)devices.size();
    // the pairs are dealt in chunks: 2^16 pairs, with several devices at most a quarter of a device's share, by their word steps
    const int64_t chunkPairs = std::max<int64_t>(kGateLanes, std::min<int64_t>((int64_t)1 << 16, W > 1 ? (n_pairs + 4 * W - 1) / (4 * W) : n_pairs));
    const int64_t chunks = (n_pairs + chunkPairs - 1) / chunkPairs;
    std::vector<int64_t> cost((size_t)chunks, 0);
    for (int64_t q = 0; q < n_pairs; ++q) {
      const int64_t i = pair_ij[2 * q], j = pair_ij[2 * q + 1];
      cost[(size_t)(q / chunkPairs)] += 1 + dnas::clusterGateWordSteps(read_off[i + 1] - read_off[i], read_off[j + 1] - read_off[j]);
    }
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, (size_t)W);
    return dnas::forEachDevice(devices, [&](size_t w) {
      return gateDistancesOn(devices[w], shard[w], chunkPairs, n_pairs, pair_ij, n_reads, read_seqs, read_off, out_dist);
    });
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
