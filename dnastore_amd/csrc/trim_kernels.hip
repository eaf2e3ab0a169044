// dnas_trim_reads (include/dnastore_amd.h, "Demultiplexing and trimming"), bit-identical to trimReadsHost (host/trim.cpp).  What a
// candidate is worth and how a read's candidates fold is host/trim.hpp, shared with the statement; the search is here.
//
// The search is Myers' bit-vector recurrence for approximate matching: gateBlock (cluster_gate.hpp) with hin = 0, so that row 0 is
// free in every column (D[0][c] = 0), a primer of at most 64 rows one word, the score read off the bit of row m.  Rows above m in
// the word compute garbage that never reaches a lower bit.  One search's state and its column step are TrimSearch (host/trim.hpp),
// which a host program runs too (tools/bitvector_host_check.cpp); the statement does not.
//
// trim_pack_kernel     the two windows of every read -- its first and its last W columns, the last ones backwards -- 16 bases to
//                      a dword, laid out [dword][read]: the search kernel's loads are then one dword per lane and 16 columns, the
//                      lanes of a wave contiguous, however long the reads are and wherever they lie.
// trim_search_kernel   a thread per read, a wave per work-group, an item is (64 reads, a chunk of the pairs).  k is wave-uniform:
//                      the pair's two mask sets (F, reverse(R)) and lengths come from the call's table, every lane loading the
//                      same 72 bytes (the compiler emits vector loads at a uniform address, not scalar ones), and a lane picks
//                      the mask of its base with three selects.  The four searches of (read, pair) advance in one loop
//                      over the columns: F on the front window with b and on the end window with 3 - b (strand 1), reverse(R) on
//                      the end window with b and on the front window with 3 - b.  Four independent chains of about twenty 64-bit
//                      operations per column are what a lane has to overlap; there is no carry between words and no LDS.  The
//                      lane's state over its chunk (TrimBest) goes to rec[chunk][read].
// trim_fold_kernel     a thread per read merges the chunks' states in the (total, k, s) order and writes the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "cluster_gate.hpp"
#include "devices.hpp"
#include "errors.hpp"
#include "host/trim.hpp"
#include "pair_align_device.h"

namespace {

constexpr int kTrimLanes = 64;                           // threads of a work-group: one wave
constexpr size_t kTrimRecBytes = (size_t)1 << 30;        // the chunks' states at most

struct TrimPairMasks {
  uint64_t eqF[4], eqR[4];                               // gateMasks of F_k and of reverse(R_k)
  int32_t mF, mR;
};

__global__ __launch_bounds__(256) void trim_pack_kernel(int64_t N, int64_t G, int32_t W, const int8_t* __restrict__ seqs,
                                                        const int64_t* __restrict__ off, uint32_t* __restrict__ front,
                                                        uint32_t* __restrict__ end) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= N * G) return;
  const int64_t r = tid % N, g = tid / N, o = off[r];
  const int64_t n = off[r + 1] - o, lim = n < W ? n : W;
  uint32_t f = 0, e = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int64_t c = 16 * g + u;
    if (c < lim) {
      f |= (uint32_t)(seqs[o + c] & 3) << (2 * u);
      e |= (uint32_t)(seqs[o + n - 1 - c] & 3) << (2 * u);
    }
  }
  front[tid] = f;
  end[tid] = e;
}

__global__ __launch_bounds__(kTrimLanes) void trim_search_kernel(int64_t N, int64_t groups, int32_t K, int32_t pairChunk,
                                                                 const TrimPairMasks* __restrict__ tab, const int64_t* __restrict__ off,
                                                                 const uint32_t* __restrict__ front, const uint32_t* __restrict__ end,
                                                                 int32_t maxOffset, int32_t maxEditPermille, int32_t anchors,
                                                                 int32_t minPayload, dnas::TrimBest* __restrict__ rec,
                                                                 unsigned long long* __restrict__ columns) {
  const int lane = threadIdx.x;
  const int64_t group = (int64_t)blockIdx.x % groups, chunk = (int64_t)blockIdx.x / groups;
  const int64_t r = group * kTrimLanes + lane;
  const bool active = r < N;
  const int32_t n = active ? (int32_t)(off[r + 1] - off[r]) : 0;
  const int32_t k0 = (int32_t)chunk * pairChunk, k1 = K - k0 < pairChunk ? K : k0 + pairChunk;
  dnas::TrimBest best;
  unsigned long long walked = 0;
  for (int32_t k = k0; k < k1; ++k) {
    const TrimPairMasks pm = tab[k];
    const int32_t wF = dnas::trimWindow(pm.mF, n, maxOffset), wR = dnas::trimWindow(pm.mR, n, maxOffset);
    const int32_t wmax = wF > wR ? wF : wR;              // (0 for a lane without a read: it loads nothing)
    const uint64_t bitF = (uint64_t)1 << (pm.mF - 1), bitR = (uint64_t)1 << (pm.mR - 1);
    dnas::TrimSearch f0(pm.mF), r0(pm.mR), f1(pm.mF), r1(pm.mR);   // (anchor, strand)
    for (int32_t c0 = 0; c0 < wmax; c0 += 16) {
      const uint32_t fw = front[(int64_t)(c0 >> 4) * N + r], ew = end[(int64_t)(c0 >> 4) * N + r];
      const int32_t cols = wmax - c0 < 16 ? wmax - c0 : 16;
      for (int32_t u = 0; u < cols; ++u) {
        const int bf = (int)(fw >> (2 * u) & 3), be = (int)(ew >> (2 * u) & 3);
        const int32_t c = c0 + u + 1;
        f0.step(pm.eqF, bf, bitF, c, wF);
        r0.step(pm.eqR, be, bitR, c, wR);
        f1.step(pm.eqF, 3 - be, bitF, c, wF);
        r1.step(pm.eqR, 3 - bf, bitR, c, wR);
      }
    }
    if (active) {
      dnas::trimOffer(best, k, 0, n, f0.hit, pm.mF, r0.hit, pm.mR, maxEditPermille, anchors, minPayload);
      dnas::trimOffer(best, k, 1, n, f1.hit, pm.mF, r1.hit, pm.mR, maxEditPermille, anchors, minPayload);
      walked += 2ull * (unsigned long long)(wF + wR);
    }
  }
  if (active) rec[chunk * N + r] = best;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) walked += __shfl_xor(walked, d);
  if (lane == 0 && walked) atomicAdd(columns, walked);
}

__global__ __launch_bounds__(256) void trim_fold_kernel(int64_t N, int64_t chunks, const dnas::TrimBest* __restrict__ rec,
                                                        const int64_t* __restrict__ off, int32_t* __restrict__ pair,
                                                        uint8_t* __restrict__ strand, int32_t* __restrict__ begin, int32_t* __restrict__ end,
                                                        int32_t* __restrict__ edits, int32_t* __restrict__ second,
                                                        uint8_t* __restrict__ status) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  dnas::TrimBest b = rec[r];
  for (int64_t ch = 1; ch < chunks; ++ch) dnas::trimMerge(b, rec[ch * N + r]);
  dnas::trimFinish(b, (int32_t)(off[r + 1] - off[r]), pair + r, strand + r, begin + r, end + r, edits + 2 * r, second + r, status + r);
}

struct TrimCall {
  int32_t maxOffset, maxEditPermille, anchors, minPayload;
  int32_t K;
  const TrimPairMasks* tab;                              // host
  int32_t maxM;                                          // the longest primer
};

// The pairs of a chunk: enough chunks for cus x 64 items (64 reads, chunk) when the reads alone make fewer, the chunks' states within
// kTrimRecBytes and the grid within 2^31 work-groups; DNAS_TRIM_PAIR_CHUNK (testing aid) forces it inside those bounds.
int32_t trimPairChunk(int cus, int64_t groups, int64_t N, int32_t K) {
  const int64_t target = (int64_t)cus * 64;
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(K, (target + groups - 1) / groups));
  int64_t pairChunk = (K + chunks - 1) / chunks;
  if (const char* s = getenv("DNAS_TRIM_PAIR_CHUNK")) pairChunk = std::max<int64_t>(1, std::min<int64_t>(K, atoll(s)));
  const int64_t maxChunks = std::max<int64_t>(1, std::min<int64_t>((int64_t)(kTrimRecBytes / sizeof(dnas::TrimBest)) / N, (((int64_t)1 << 31) - 1) / groups));
  pairChunk = std::max<int64_t>(pairChunk, (K + maxChunks - 1) / maxChunks);
  return (int32_t)pairChunk;
}

// One device's share: n reads (seqs, off: offsets from 0) -> the outputs at index 0 .. n - 1.
int trimOn(int device, const TrimCall& call, int64_t n, const int8_t* seqs, const int64_t* off, int32_t* pair, uint8_t* strand, int32_t* begin,
           int32_t* end, int32_t* edits, int32_t* second, uint8_t* status, dnas_trim_stats* stats) {
  if (n == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  PaBuffers bufs;
  int rc, cus = 256;
  if ((rc = bufs.open())) return rc;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  int64_t maxLen = 0;
  for (int64_t i = 0; i < n; ++i) maxLen = std::max(maxLen, off[i + 1] - off[i]);
  const int32_t W = dnas::trimWindow(call.maxM, (int32_t)maxLen, call.maxOffset);
  const int64_t G = std::max<int64_t>(1, (W + 15) / 16), groups = (n + kTrimLanes - 1) / kTrimLanes;
  const int32_t pairChunk = trimPairChunk(cus, groups, n, call.K);
  const int64_t chunks = (call.K + pairChunk - 1) / pairChunk;

  int8_t* dSeqs = nullptr;
  int64_t* dOff = nullptr;
  TrimPairMasks* dTab = nullptr;
  uint32_t *dFront = nullptr, *dEnd = nullptr;
  dnas::TrimBest* dRec = nullptr;
  unsigned long long* dColumns = nullptr;
  int32_t *dPair = nullptr, *dBegin = nullptr, *dEndOut = nullptr, *dEdits = nullptr, *dSecond = nullptr;
  uint8_t *dStrand = nullptr, *dStatus = nullptr;
  if ((rc = paUpload(bufs, &dSeqs, seqs, (size_t)off[n]))) return rc;
  if ((rc = paUpload(bufs, &dOff, off, (size_t)n + 1))) return rc;
  if ((rc = paUpload(bufs, &dTab, call.tab, (size_t)call.K))) return rc;
  if ((rc = paAlloc(bufs, &dFront, (size_t)(G * n)))) return rc;
  if ((rc = paAlloc(bufs, &dEnd, (size_t)(G * n)))) return rc;
  if ((rc = paAlloc(bufs, &dRec, (size_t)(chunks * n)))) return rc;
  if ((rc = paAlloc(bufs, &dColumns, 1))) return rc;
  if ((rc = paAlloc(bufs, &dPair, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dStrand, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dBegin, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dEndOut, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dEdits, 2 * (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dSecond, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dStatus, (size_t)n))) return rc;

  DNAS_HIP_TRY(hipMemsetAsync(dColumns, 0, sizeof(unsigned long long), bufs.stream));
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
  hipLaunchKernelGGL(trim_pack_kernel, dim3((unsigned)((G * n + 255) / 256)), dim3(256), 0, bufs.stream, n, G, W, dSeqs, dOff, dFront, dEnd);
  hipLaunchKernelGGL(trim_search_kernel, dim3((unsigned)(groups * chunks)), dim3(kTrimLanes), 0, bufs.stream, n, groups, call.K, pairChunk, dTab,
                     dOff, dFront, dEnd, call.maxOffset, call.maxEditPermille, call.anchors, call.minPayload, dRec, dColumns);
  hipLaunchKernelGGL(trim_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, bufs.stream, n, chunks, dRec, dOff, dPair, dStrand,
                     dBegin, dEndOut, dEdits, dSecond, dStatus);
  DNAS_HIP_TRY(hipGetLastError());
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
  DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
  float ms = 0;
  DNAS_HIP_TRY(hipEventElapsedTime(&ms, bufs.ev[0], bufs.ev[1]));
  unsigned long long columns = 0;
  DNAS_HIP_TRY(hipMemcpy(&columns, dColumns, sizeof columns, hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(pair, dPair, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(strand, dStrand, (size_t)n, hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(begin, dBegin, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(end, dEndOut, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(edits, dEdits, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(second, dSecond, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(status, dStatus, (size_t)n, hipMemcpyDeviceToHost));
  stats->kernel_ms = ms;
  stats->items = groups * chunks;
  stats->columns = (int64_t)columns;
  stats->chunks = chunks;
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_trim_reads(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t n_reads, const int8_t* read_seqs,
                               const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors, int32_t min_payload,
                               int device_id, int32_t* out_pair, uint8_t* out_strand, int32_t* out_begin, int32_t* out_end,
                               int32_t* out_edits, int32_t* out_second, uint8_t* out_status, dnas_trim_stats* out_stats) {
  if (out_stats) *out_stats = dnas_trim_stats{};
  if (const int rc = dnas::checkTrimArgs(n_pairs, primer_seqs, primer_off, n_reads, read_seqs, read_off, max_offset, max_edit_permille, anchors,
                                         min_payload, out_pair, out_strand, out_begin, out_end, out_edits, out_second, out_status))
    return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  if (n_reads == 0) return DNAS_OK;
  try {
    if (n_pairs == 0) {                                  // no candidate: the outputs of an untouched state
      for (int64_t i = 0; i < n_reads; ++i)
        dnas::trimFinish(dnas::TrimBest{}, (int32_t)(read_off[i + 1] - read_off[i]), out_pair + i, out_strand + i, out_begin + i, out_end + i,
                         out_edits + 2 * i, out_second + i, out_status + i);
      return DNAS_OK;
    }
    std::vector<TrimPairMasks> tab((size_t)n_pairs);
    TrimCall call{max_offset, max_edit_permille, anchors, min_payload, (int32_t)n_pairs, tab.data(), 0};
    for (int64_t k = 0; k < n_pairs; ++k) {
      TrimPairMasks& pm = tab[(size_t)k];
      pm.mF = (int32_t)(primer_off[2 * k + 1] - primer_off[2 * k]);
      pm.mR = (int32_t)(primer_off[2 * k + 2] - primer_off[2 * k + 1]);
      int8_t rev[dnas::kTrimMaxPrimer];
      for (int32_t q = 0; q < pm.mR; ++q) rev[q] = primer_seqs[primer_off[2 * k + 2] - 1 - q];
      dnas::gateMasks(primer_seqs + primer_off[2 * k], pm.mF, 0, pm.eqF);
      dnas::gateMasks(rev, pm.mR, 0, pm.eqR);
      call.maxM = std::max(call.maxM, std::max(pm.mF, pm.mR));
    }
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const int64_t W = (int64_t)devices.size();
    std::vector<dnas_trim_stats> stats((size_t)W);
    int rc;
    if (W == 1) {
      rc = dnas::forEachDevice(devices, [&](size_t) {
        return trimOn(devices[0], call, n_reads, read_seqs, read_off, out_pair, out_strand, out_begin, out_end, out_edits, out_second, out_status,
                      &stats[0]);
      });
    } else {
      // the reads are dealt in blocks: 2^16 reads, at most a quarter of a device's share, by the columns of their windows
      const int64_t blockReads = std::max<int64_t>(kTrimLanes, std::min<int64_t>((int64_t)1 << 16, (n_reads + 4 * W - 1) / (4 * W)));
      const int64_t blocks = (n_reads + blockReads - 1) / blockReads;
      std::vector<int64_t> cost((size_t)blocks, 0);
      for (int64_t i = 0; i < n_reads; ++i)
        cost[(size_t)(i / blockReads)] += 1 + dnas::trimWindow(call.maxM, (int32_t)(read_off[i + 1] - read_off[i]), max_offset);
      const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, (size_t)W);
      rc = dnas::forEachDevice(devices, [&](size_t w) {
        std::vector<int64_t> mine;                       // the reads of the worker's blocks
        for (int64_t b : shard[w])
          for (int64_t i = b * blockReads; i < std::min(n_reads, (b + 1) * blockReads); ++i) mine.push_back(i);
        const size_t n = mine.size();
        std::vector<int8_t> seqs;
        std::vector<int64_t> off;
        dnas::gatherShard(mine, read_seqs, read_off, &seqs, &off);
        std::vector<int32_t> pair(n + 1), begin(n + 1), end(n + 1), edits(2 * n + 2), second(n + 1);
        std::vector<uint8_t> strand(n + 1), status(n + 1);
        if (const int rcw = trimOn(devices[w], call, (int64_t)n, seqs.data(), off.data(), pair.data(), strand.data(), begin.data(), end.data(),
                                   edits.data(), second.data(), status.data(), &stats[w]))
          return rcw;
        for (size_t j = 0; j < n; ++j) {
          const int64_t i = mine[j];
          out_pair[i] = pair[j], out_strand[i] = strand[j], out_begin[i] = begin[j], out_end[i] = end[j];
          out_edits[2 * i] = edits[2 * j], out_edits[2 * i + 1] = edits[2 * j + 1], out_second[i] = second[j], out_status[i] = status[j];
        }
        return (int)DNAS_OK;
      });
    }
    if (rc) return rc;
    if (out_stats) {
      for (const dnas_trim_stats& s : stats) {
        out_stats->kernel_ms = std::max(out_stats->kernel_ms, s.kernel_ms);
        out_stats->items += s.items;
        out_stats->columns += s.columns;
        out_stats->chunks = std::max(out_stats->chunks, s.chunks);
      }
      for (int64_t i = 0; i < n_reads; ++i) out_stats->trimmed += out_status[i] == DNAS_TRIM_OK;
      out_stats->devices = W;
    }
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
