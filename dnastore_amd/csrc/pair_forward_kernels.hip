// dnas_pair_likelihoods: the forward score of host/pairforward.hpp per (original, read) pair on the GPU, bit-identical to
// forwardPairHost in table mode.  The kernel is paScoreChunk of pair_align_device.h built with the sum-product cell of
// pair_forward_device.h; the launch plan, the chunk loop and the fan-out over devices are the shared ones.  An
// item is a pair, and a chunk of scores lands where the pair's result belongs: there is nothing to fold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/pairforward.hpp"
#include "pair_forward_device.h"

namespace {

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void pair_forward_score_kernel(
    PaScores sc, const double* __restrict__ subTable, const double* __restrict__ lseTab, int band, int ldsCols, int64_t first,
    int64_t count, const int8_t* __restrict__ inSeqs, const int64_t* __restrict__ inOff, const int8_t* __restrict__ outSeqs,
    const int64_t* __restrict__ outOff, const uint8_t* __restrict__ outRev, double* bndScratch, int64_t bndStride,
    double* __restrict__ chunk) {
  const auto itemAt = [&](int64_t g) -> PaItem {
    return {inSeqs + inOff[g], outSeqs + outOff[g], (int)(inOff[g + 1] - inOff[g]), (int)(outOff[g + 1] - outOff[g]),
            outRev != nullptr && outRev[g] != 0};
  };
  paScoreChunk<KP>(sc, subTable, band, ldsCols, first, count, itemAt, bndScratch, bndStride, chunk, PaForwardScoreCell{lseTab});
}

struct PfChunkStats {
  double score_ms = 0, fold_ms = 0;
  int64_t chunks = 0;
};

// One device.  The arguments were checked; results go to the caller's array.
int pfRunOnDevice(int device, const dnas::PairScores& hs, int band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                  const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev, double* out_ll, dnas_forward_stats* stats) {
  *stats = dnas_forward_stats{};
  if (n == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  stats->items = n;
  int maxO = 0;
  int64_t maxI = 0;
  for (int64_t i = 0; i < n; ++i) {
    maxI = std::max(maxI, in_off[i + 1] - in_off[i]);
    maxO = std::max(maxO, (int)(out_off[i + 1] - out_off[i]));
  }
  PaCellMemo memo(maxI, maxO, band);
  for (int64_t i = 0; i < n; ++i) stats->cells += memo.cells(in_off[i + 1] - in_off[i], out_off[i + 1] - out_off[i]);

  const PaScores sc = PaScores::from(hs);
  const auto kernelOf = [](auto kp) { return &pair_forward_score_kernel<decltype(kp)::value>; };
  PaLaunchPlan plan;
  int rc;
  if ((rc = paPlanScore(sc.P, kernelOf, cus, maxO, "DNAS_FORWARD_CHUNK", n, &plan))) return rc;

  PaBuffers bufs;
  if ((rc = bufs.open())) return rc;
  int8_t *dIn = nullptr, *dOut = nullptr;
  int64_t *dInOff = nullptr, *dOutOff = nullptr;
  uint8_t* dRev = nullptr;
  double *dSub = nullptr, *dTab = nullptr, *dScore = nullptr, *dBnd = nullptr;
  const std::vector<double>& tab = dnas::lseTable();
  if ((rc = paUpload(bufs, &dIn, in_seqs, (size_t)in_off[n]))) return rc;
  if ((rc = paUpload(bufs, &dOut, out_seqs, (size_t)out_off[n]))) return rc;
  if ((rc = paUpload(bufs, &dInOff, in_off, (size_t)n + 1))) return rc;
  if ((rc = paUpload(bufs, &dOutOff, out_off, (size_t)n + 1))) return rc;
  if (out_rev && (rc = paUpload(bufs, &dRev, out_rev, (size_t)n))) return rc;
  if ((rc = paUpload(bufs, &dSub, hs.sub, 16))) return rc;
  if ((rc = paUpload(bufs, &dTab, tab.data(), tab.size()))) return rc;
  if ((rc = paAlloc(bufs, &dScore, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;

  const auto score = [&](int64_t first, int64_t count) {
    paDispatchKP(sc.P, [&](auto kp) {
      hipLaunchKernelGGL(kernelOf(kp), dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), plan.ldsBytes, bufs.stream, sc, dSub, dTab,
                         band, plan.ldsCols, first, count, dIn, dInOff, dOut, dOutOff, dRev, dBnd, plan.bndStride, dScore + first);
    });
  };
  PfChunkStats cs;
  if ((rc = paRunChunks(bufs, n, plan.chunkItems, score, [](int64_t, int64_t) {}, [](int64_t, int64_t) { return hipSuccess; }, &cs)))
    return rc;
  stats->score_ms = cs.score_ms;
  stats->chunks = cs.chunks;
  DNAS_HIP_TRY(hipMemcpy(out_ll, dScore, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_pair_likelihoods(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                                     const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                                     int device_id, double* out_ll, dnas_forward_stats* out_stats) {
  if (const int rc = dnas::checkForwardArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_ll)) return rc;
  dnas_forward_stats total{};
  if (out_stats) *out_stats = total;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = devices.size();
    if (W == 1 || n_pairs == 0) {
      const int rc = pfRunOnDevice(devices[0], hs, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, out_ll, &total);
      if (rc == DNAS_OK && out_stats) *out_stats = total;
      return rc;
    }
    // every GPU of the node: the pairs dealt as dnas_align_pairs deals them, results scattered back under the caller's indices
    std::vector<int64_t> cost((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) {
      const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
      const dnas::PairBand bd(I, O, band);
      cost[(size_t)i] = (I + 1) * std::min(O + 1, bd.hi - bd.lo + 1);
    }
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    std::vector<dnas_forward_stats> stats(W);
    const int rc = dnas::forEachDevice(devices, [&](size_t k) {
      const std::vector<int64_t>& mine = shard[k];
      const size_t m = mine.size();
      std::vector<int8_t> in, outs;
      std::vector<int64_t> inOff, outOff;
      dnas::gatherShard(mine, in_seqs, in_off, &in, &inOff);
      dnas::gatherShard(mine, out_seqs, out_off, &outs, &outOff);
      std::vector<uint8_t> rev(m + 1);
      if (out_rev) for (size_t j = 0; j < m; ++j) rev[j] = out_rev[mine[j]];
      std::vector<double> ll(m + 1);
      const int rc = pfRunOnDevice(devices[k], hs, band, (int64_t)m, in.data(), inOff.data(), outs.data(), outOff.data(),
                                   out_rev ? rev.data() : nullptr, ll.data(), &stats[k]);
      if (rc != DNAS_OK) return rc;
      for (size_t j = 0; j < m; ++j) out_ll[mine[j]] = ll[j];
      return DNAS_OK;
    });
    if (rc != DNAS_OK) return rc;
    for (size_t k = 0; k < W; ++k) {
      total.score_ms = std::max(total.score_ms, stats[k].score_ms);
      total.items += stats[k].items;
      total.cells += stats[k].cells;
      total.chunks += stats[k].chunks;
    }
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
