// dnas_align_pairs: the pair-HMM Viterbi alignment of host/pairalign.hpp on the GPU, bit-identical to alignPairHost.
//
// Fill.  A wave owns a pair and walks the batch with the grid's stride; there is no work-group barrier.  The wavefront over a
// pair's matrix is paWalkForward of pair_align_device.h under the Viterbi cell (stripes of 64 rows, lane skew, shuffles of S
// and D, T lanes in registers, the boundary row in LDS or in the wave's HBM scratch), here with its choice words recorded.  No
// score leaves the chip but S(I,O); what does is one 16-bit choice word per cell, filed under (stripe, step, lane).
//
// Traceback.  One thread per pair reads one choice word per move and writes op bytes from the end of the slot, then moves them
// to its start.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/pairalign.hpp"
#include "pair_align_device.h"

namespace {

constexpr uint64_t kPaSkip = ~0ull;

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void pair_align_fill_kernel(
    PaScores sc, const double* __restrict__ subTable, int band, int64_t first, int64_t count, const int8_t* __restrict__ inSeqs,
    const int64_t* __restrict__ inOff, const int8_t* __restrict__ outSeqs, const int64_t* __restrict__ outOff,
    const uint64_t* __restrict__ recOff, uint16_t* __restrict__ arena, double* bndScratch, int64_t bndStride,
    double* __restrict__ score) {
  __shared__ double lds[kPaWavesPerBlock][kPaLdsDoubles];
  const PaWave w = paWaveBegin(&lds[0][0], kPaLdsDoubles, subTable, bndScratch, bndStride);

  for (int64_t q = w.wave; q < count; q += w.nWaves) {
    const uint64_t ro = recOff[q];
    if (ro == kPaSkip) continue;
    const int64_t pair = first + q;
    const int I = (int)(inOff[pair + 1] - inOff[pair]), O = (int)(outOff[pair + 1] - outOff[pair]);
    PaViterbiCell<true> cell{arena + ro + w.lane, PaGeom(I, O, band).stepsMax};
    paWalkForward<KP>(sc, w.lds, PaBoundary(w.lds + 16, kPaLdsCols, w.bndMem, O), w.lane, band,
                      PaItem{inSeqs + inOff[pair], outSeqs + outOff[pair], I, O, false}, score + pair, cell);
  }
}

__global__ void pair_align_traceback_kernel(int band, int64_t first, int64_t count, const int64_t* __restrict__ inOff,
                                            const int64_t* __restrict__ outOff, const uint64_t* __restrict__ recOff,
                                            const uint16_t* __restrict__ arena, const double* __restrict__ score,
                                            uint8_t* __restrict__ ops, const uint64_t* __restrict__ opsOff,
                                            uint32_t* __restrict__ nOps, uint8_t* __restrict__ status) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  const int64_t pair = first + q;
  const uint64_t ro = recOff[q];
  nOps[pair] = 0;
  if (ro == kPaSkip) { status[pair] = DNAS_ALIGN_TOO_LARGE; return; }
  if (!(score[pair] > paNegInf())) { status[pair] = DNAS_ALIGN_NO_PATH; return; }
  const int I = (int)(inOff[pair + 1] - inOff[pair]), O = (int)(outOff[pair + 1] - outOff[pair]);
  const PaGeom g(I, O, band);
  const uint16_t* const rec = arena + ro;
  uint8_t* const slot = ops + opsOff[pair];
  const int cap = I + O;                       // the host checked that the slot holds this many bytes
  int ip = I, op = O, state = -1, p = cap;     // state -1: S, -2: D, k >= 0: T_k
  int pend = -1;                               // the column met last: a duplication that opens there is only known a move later
  bool ok = true;
  for (int moves = 0; !(ip == 0 && op == 0 && state == -1); ++moves) {
    if (ip < 0 || op < g.rowLo(ip) || op > g.rowHi(ip, O) || moves > 2 * cap + 2) { ok = false; break; }
    const unsigned w = rec[g.wordAt(ip, op)];
    int col = -1;
    if (state == -1) {
      const unsigned c = w & 3u;
      if (c == 0) { col = dnas::kOpMatch; --ip; --op; }
      else if (c == 1) { col = dnas::kOpDup; --op; state = 0; }
      else state = -2;
    } else if (state == -2) {
      if (w & 4u) { col = dnas::kOpDelete; --ip; }
      else { col = dnas::kOpDelete | 1 << 2; --ip; state = -1; }
    } else {
      if (w & (8u << state)) { pend |= (state + 1) << 2; state = -1; }
      else { col = dnas::kOpDup; --op; ++state; }
    }
    if (col >= 0) {
      if (pend >= 0) {
        if (p == 0) { ok = false; break; }
        slot[--p] = (uint8_t)pend;
      }
      pend = col;
    }
  }
  if (ok && pend >= 0) {
    if (p == 0) ok = false;
    else slot[--p] = (uint8_t)pend;
  }
  if (!ok) { status[pair] = DNAS_ALIGN_TRACEBACK_FAIL; return; }
  const int n = cap - p;
  for (int i = 0; i < n; ++i) slot[i] = slot[p + i];
  nOps[pair] = (uint32_t)n;
  status[pair] = DNAS_ALIGN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host side

// One device.  The arguments were checked by dnas_align_pairs; results go to the caller's arrays.
int paAlignOnDevice(const dnas::PairScores& hs, int band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                    const int8_t* out_seqs, const int64_t* out_off, int device, size_t arena_bytes, uint8_t* out_ops,
                    const uint64_t* ops_off, uint32_t* out_n_ops, double* out_score, uint8_t* out_status, dnas_align_stats* stats) {
  *stats = dnas_align_stats{};
  if (n == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  PaBuffers bufs;
  int rc;
  if ((rc = bufs.open())) return rc;

  // the traceback record of every pair, and the batches the arena takes
  std::vector<size_t> words((size_t)n);
  size_t total = 0, largest = 0;
  int maxO = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int I = (int)(in_off[i + 1] - in_off[i]), O = (int)(out_off[i + 1] - out_off[i]);
    words[(size_t)i] = PaGeom(I, O, band).words();
    total += words[(size_t)i];
    largest = std::max(largest, words[(size_t)i]);
    maxO = std::max(maxO, O);
    stats->cells += dnas::PairBand(I, O, band).cells(I, O);
  }
  size_t arenaWords;
  if (arena_bytes) {
    arenaWords = arena_bytes / 2;
  } else {
    size_t freeB = 0, totalB = 0;
    DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
    arenaWords = std::min(total, freeB / 2 / 2);          // half of what is free: the sequences and the results need room too
  }
  arenaWords = std::min(arenaWords, total);

  const PaScores sc = PaScores::from(hs);

  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  PaLaunchPlan plan;
  plan.cut(cus, 2, maxO, n);                               // 64 KiB of static LDS per work-group: two of them share a CU

  int8_t *dIn = nullptr, *dOut = nullptr;
  int64_t *dInOff = nullptr, *dOutOff = nullptr;
  uint64_t *dOpsOff = nullptr, *dRecOff = nullptr;
  double *dSub = nullptr, *dScore = nullptr, *dBnd = nullptr;
  uint16_t* dArena = nullptr;
  uint8_t *dOps = nullptr, *dStatus = nullptr;
  uint32_t* dNOps = nullptr;
  const size_t nOpsBytes = (size_t)ops_off[n];
  if ((rc = paUpload(bufs, &dIn, in_seqs, (size_t)in_off[n]))) return rc;
  if ((rc = paUpload(bufs, &dOut, out_seqs, (size_t)out_off[n]))) return rc;
  if ((rc = paUpload(bufs, &dInOff, in_off, (size_t)n + 1))) return rc;
  if ((rc = paUpload(bufs, &dOutOff, out_off, (size_t)n + 1))) return rc;
  if ((rc = paUpload(bufs, &dOpsOff, ops_off, (size_t)n + 1))) return rc;
  if ((rc = paUpload(bufs, &dSub, hs.sub, 16))) return rc;
  if ((rc = paAlloc(bufs, &dRecOff, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dScore, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dStatus, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dNOps, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dOps, nOpsBytes))) return rc;
  if ((rc = paAlloc(bufs, &dArena, arenaWords))) return rc;
  if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;

  // batches of consecutive pairs; a pair whose record alone exceeds the arena is skipped inside its batch
  std::vector<uint64_t> recOff((size_t)n);
  std::vector<std::pair<int64_t, int64_t>> batches;
  {
    int64_t b0 = 0;
    size_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
      const size_t w = words[(size_t)i];
      if (w > arenaWords) { recOff[(size_t)i] = kPaSkip; ++stats->pairs_too_large; continue; }
      if (used + w > arenaWords) { batches.emplace_back(b0, i); b0 = i; used = 0; }
      recOff[(size_t)i] = used;
      used += w;
    }
    batches.emplace_back(b0, n);
  }
  DNAS_HIP_TRY(hipMemcpy(dRecOff, recOff.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  stats->batches = (int64_t)batches.size();

  for (const auto& bt : batches) {
    const int64_t first = bt.first, count = bt.second - bt.first;
    if (count == 0) continue;
    DNAS_HIP_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
    paDispatchKP(sc.P, [&](auto kp) {
      hipLaunchKernelGGL(pair_align_fill_kernel<decltype(kp)::value>, dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), 0, bufs.stream,
                         sc, dSub, band, first, count, dIn, dInOff, dOut, dOutOff, dRecOff + first, dArena, dBnd, plan.bndStride, dScore);
    });
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
    hipLaunchKernelGGL(pair_align_traceback_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, bufs.stream, band, first, count,
                       dInOff, dOutOff, dRecOff + first, dArena, dScore, dOps, dOpsOff, dNOps, dStatus);
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(bufs.ev[2], bufs.stream));
    DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
    float fill = 0, tb = 0;
    DNAS_HIP_TRY(hipEventElapsedTime(&fill, bufs.ev[0], bufs.ev[1]));
    DNAS_HIP_TRY(hipEventElapsedTime(&tb, bufs.ev[1], bufs.ev[2]));
    stats->fill_ms += fill;
    stats->traceback_ms += tb;
  }
  DNAS_HIP_TRY(hipMemcpy(out_score, dScore, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_status, dStatus, (size_t)n, hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_n_ops, dNOps, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nOpsBytes) DNAS_HIP_TRY(hipMemcpy(out_ops, dOps, nOpsBytes, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i)
    if (out_status[i] == DNAS_ALIGN_TOO_LARGE) out_score[i] = std::numeric_limits<double>::quiet_NaN();
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_align_pairs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                                const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, int device_id,
                                size_t arena_bytes, uint8_t* out_ops, const uint64_t* ops_off, uint32_t* out_n_ops, double* out_score,
                                uint8_t* out_status, dnas_align_stats* out_stats) {
  if (const int rc = dnas::checkAlignArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_ops, ops_off, out_n_ops,
                                           out_score, out_status))
    return rc;
  dnas_align_stats total{};
  if (out_stats) *out_stats = total;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = devices.size();
    if (W == 1 || n_pairs == 0) {
      const int rc = paAlignOnDevice(hs, band, n_pairs, in_seqs, in_off, out_seqs, out_off, devices[0], arena_bytes, out_ops, ops_off,
                                     out_n_ops, out_score, out_status, &total);
      if (rc == DNAS_OK && out_stats) *out_stats = total;
      return rc;
    }
    // every GPU of the node: the pairs dealt by the cells of their bands, one host thread per device, results scattered back
    std::vector<int64_t> cost((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) {
      const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
      const dnas::PairBand bd(I, O, band);
      cost[(size_t)i] = (I + 1) * std::min(O + 1, bd.hi - bd.lo + 1);
    }
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    std::vector<dnas_align_stats> stats(W);
    const int rc = dnas::forEachDevice(devices, [&](size_t k) {
      const std::vector<int64_t>& mine = shard[k];
      const size_t m = mine.size();
      std::vector<int8_t> in, outs;
      std::vector<int64_t> inOff, outOff;
      dnas::gatherShard(mine, in_seqs, in_off, &in, &inOff);
      dnas::gatherShard(mine, out_seqs, out_off, &outs, &outOff);
      std::vector<uint64_t> opsOff(m + 1);
      for (size_t j = 0; j <= m; ++j) opsOff[j] = (uint64_t)(inOff[j] + outOff[j]);
      std::vector<uint8_t> ops((size_t)opsOff.back() + 1), status(m + 1);
      std::vector<uint32_t> nOps(m + 1);
      std::vector<double> score(m + 1);
      const int rc = paAlignOnDevice(hs, band, (int64_t)m, in.data(), inOff.data(), outs.data(), outOff.data(), devices[k], arena_bytes,
                                     ops.data(), opsOff.data(), nOps.data(), score.data(), status.data(), &stats[k]);
      if (rc != DNAS_OK) return rc;
      for (size_t j = 0; j < m; ++j) {
        const int64_t i = mine[j];
        out_score[i] = score[j];
        out_status[i] = status[j];
        out_n_ops[i] = nOps[j];
        std::copy(ops.begin() + (size_t)opsOff[j], ops.begin() + (size_t)opsOff[j] + nOps[j], out_ops + ops_off[i]);
      }
      return DNAS_OK;
    });
    if (rc != DNAS_OK) return rc;
    for (size_t k = 0; k < W; ++k) {
      total.fill_ms = std::max(total.fill_ms, stats[k].fill_ms);
      total.traceback_ms = std::max(total.traceback_ms, stats[k].traceback_ms);
      total.cells += stats[k].cells;
      total.batches += stats[k].batches;
      total.pairs_too_large += stats[k].pairs_too_large;
    }
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
