// dnas_consensus_score: of every cluster's candidate strands the one under which the cluster's reads score highest together
// (include/dnastore_amd.h), bit-identical to consensusScoreHost (host/consensus.cpp).
//
// Score.  The work is, per cluster, candidates x reads pair-HMM scores, and nothing but scores: the kernel is paScoreChunk of
// pair_align_device.h, the launch plan, the chunk loop and the fan-out over devices are the shared ones.  What
// is stated here is the item -- (candidate, read, strand), derived from the work index by bisecting the per-cluster item
// offsets (ConsensusItems, host/consensus.hpp): no expanded list exists on the host or in HBM.  Items are candidate-major, so
// the waves of a block, which hold consecutive items, mostly share their candidate.  A read with strand 1 is read in place as
// its reverse complement.  dnas_consensus_score_ex with DNAS_SCORE_FORWARD runs the same items, plan and fold under the
// sum-product cell of pair_forward_device.h (consensus_forward_kernel): an item's score is then the forward score, and the
// posteriors are formed on the host from the per-candidate totals (consensusPosteriors, host/consensus.cpp).
//
// Fold.  One thread per candidate adds that candidate's scores of the chunk, in item order, to its total in a per-candidate
// device array that starts at 0.0: a candidate whose reads span chunks is summed chunk after chunk in stream order, which is
// the order of the statement.  After the last chunk one thread per cluster picks winner and runner-up with ConsensusFold.
// Device memory beyond the sequences, the offsets and the per-candidate and per-cluster outputs is the one chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/consensus.hpp"
#include "host/pairalign.hpp"
#include "pair_forward_device.h"

namespace {

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void consensus_score_kernel(
    PaScores sc, const double* __restrict__ subTable, int band, int ldsCols, int64_t first, int64_t count, dnas::ConsensusItems items,
    const int8_t* __restrict__ candSeqs, const int64_t* __restrict__ candOff, const int8_t* __restrict__ readSeqs,
    const int64_t* __restrict__ readOff, const uint8_t* __restrict__ readStrand, double* bndScratch, int64_t bndStride,
    double* __restrict__ chunk) {
  const auto itemAt = [&](int64_t g) -> PaItem {
    int64_t j, i;
    items.itemAt(g, &j, &i);
    const int I = (int)(candOff[j + 1] - candOff[j]), O = (int)(readOff[i + 1] - readOff[i]);
    return {candSeqs + candOff[j], readSeqs + readOff[i], I, O, readStrand != nullptr && readStrand[i] != 0};
  };
  paScoreChunk<KP>(sc, subTable, band, ldsCols, first, count, itemAt, bndScratch, bndStride, chunk);
}

// The same items under the sum-product cell (score_mode DNAS_SCORE_FORWARD): an item's score is the forward score.
template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void consensus_forward_kernel(
    PaScores sc, const double* __restrict__ subTable, const double* __restrict__ lseTab, int band, int ldsCols, int64_t first,
    int64_t count, dnas::ConsensusItems items, const int8_t* __restrict__ candSeqs, const int64_t* __restrict__ candOff,
    const int8_t* __restrict__ readSeqs, const int64_t* __restrict__ readOff, const uint8_t* __restrict__ readStrand,
    double* bndScratch, int64_t bndStride, double* __restrict__ chunk) {
  const auto itemAt = [&](int64_t g) -> PaItem {
    int64_t j, i;
    items.itemAt(g, &j, &i);
    const int I = (int)(candOff[j + 1] - candOff[j]), O = (int)(readOff[i + 1] - readOff[i]);
    return {candSeqs + candOff[j], readSeqs + readOff[i], I, O, readStrand != nullptr && readStrand[i] != 0};
  };
  paScoreChunk<KP>(sc, subTable, band, ldsCols, first, count, itemAt, bndScratch, bndStride, chunk, PaForwardScoreCell{lseTab});
}

__global__ void consensus_init_kernel(int64_t nCand, double* __restrict__ total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nCand) total[j] = 0.0;
}

// The candidates candFirst .. candFirst + candCount - 1 are those that may have items in the chunk [first, first + count).
__global__ void consensus_fold_kernel(int64_t first, int64_t count, int64_t candFirst, int64_t candCount, dnas::ConsensusItems items,
                                      const double* __restrict__ chunk, double* __restrict__ total) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= candCount) return;
  const int64_t j = candFirst + k, c = items.find(items.clusterCandOff, j);
  const int64_t g0 = items.firstItemOf(j, c), g1 = g0 + items.reads(c);
  const int64_t lo = g0 > first ? g0 : first, hi = g1 < first + count ? g1 : first + count;
  if (lo >= hi) return;
  double t = total[j];
  for (int64_t g = lo; g < hi; ++g) t += chunk[g - first];
  total[j] = t;
}

__global__ void consensus_pick_kernel(dnas::ConsensusItems items, const double* __restrict__ total, int64_t* __restrict__ winner,
                                      double* __restrict__ best, double* __restrict__ second, uint8_t* __restrict__ status) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= items.nClusters) return;
  dnas::ConsensusFold f;
  for (int64_t j = items.clusterCandOff[c]; j < items.clusterCandOff[c + 1]; ++j) f.add(total[j], j);
  const uint8_t st = dnas::ConsensusFold::status(items.cands(c), items.reads(c), f.winner);
  const bool ok = st == DNAS_CONSENSUS_OK;
  status[c] = st;
  winner[c] = ok ? f.winner : -1;
  best[c] = ok ? f.best : paNegInf();
  second[c] = ok ? f.second : paNegInf();
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct CsInputs {
  int64_t nClusters, nCand, nReads;
  const int8_t* candSeqs;
  const int64_t *candOff, *clusterCandOff;
  const int8_t* readSeqs;
  const int64_t* readOff;
  const uint8_t* readStrand;
  const int64_t* clusterReadOff;
};

// Cells inside the band over all items.
int64_t csCells(const CsInputs& in, int band) {
  int64_t maxI = 0, maxO = 0;
  for (int64_t j = 0; j < in.nCand; ++j) maxI = std::max(maxI, in.candOff[j + 1] - in.candOff[j]);
  for (int64_t i = 0; i < in.nReads; ++i) maxO = std::max(maxO, in.readOff[i + 1] - in.readOff[i]);
  PaCellMemo memo(maxI, maxO, band);
  int64_t total = 0;
  for (int64_t c = 0; c < in.nClusters; ++c)
    for (int64_t j = in.clusterCandOff[c]; j < in.clusterCandOff[c + 1]; ++j) {
      const int64_t I = in.candOff[j + 1] - in.candOff[j];
      for (int64_t i = in.clusterReadOff[c]; i < in.clusterReadOff[c + 1]; ++i) total += memo.cells(I, in.readOff[i + 1] - in.readOff[i]);
    }
  return total;
}

// One device.  The arguments were checked; results go to the caller's arrays (out_totals may be null).
int csRunOnDevice(int device, const dnas::PairScores& hs, int band, int scoreMode, const CsInputs& in, int64_t* out_winner,
                  double* out_total, double* out_second, uint8_t* out_status, double* out_totals, dnas_consensus_stats* stats) {
  *stats = dnas_consensus_stats{};
  stats->candidates = in.nCand;
  if (in.nClusters == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  std::vector<int64_t> itemOff((size_t)in.nClusters + 1, 0);
  for (int64_t c = 0; c < in.nClusters; ++c)
    itemOff[(size_t)c + 1] = itemOff[(size_t)c] + (in.clusterCandOff[c + 1] - in.clusterCandOff[c]) * (in.clusterReadOff[c + 1] - in.clusterReadOff[c]);
  const dnas::ConsensusItems hostItems{in.nClusters, in.clusterCandOff, in.clusterReadOff, itemOff.data()};
  const int64_t total = itemOff.back();
  stats->items = total;
  stats->cells = csCells(in, band);
  int maxO = 0;
  for (int64_t i = 0; i < in.nReads; ++i) maxO = std::max(maxO, (int)(in.readOff[i + 1] - in.readOff[i]));

  const PaScores sc = PaScores::from(hs);
  const auto kernelOf = [](auto kp) { return &consensus_score_kernel<decltype(kp)::value>; };
  const auto forwardOf = [](auto kp) { return &consensus_forward_kernel<decltype(kp)::value>; };
  const bool forward = scoreMode == DNAS_SCORE_FORWARD;
  PaLaunchPlan plan;
  int rc;
  if ((rc = forward ? paPlanScore(sc.P, forwardOf, cus, maxO, "DNAS_CONSENSUS_CHUNK", total, &plan)
                    : paPlanScore(sc.P, kernelOf, cus, maxO, "DNAS_CONSENSUS_CHUNK", total, &plan)))
    return rc;

  PaBuffers bufs;                                        // this run's stream, events and memory
  if ((rc = bufs.open())) return rc;
  hipStream_t stream = bufs.stream;
  int8_t *dCands = nullptr, *dReads = nullptr;
  int64_t *dCandOff = nullptr, *dReadOff = nullptr, *dClusterCandOff = nullptr, *dClusterReadOff = nullptr, *dItemOff = nullptr,
          *dWinner = nullptr;
  uint8_t *dStrand = nullptr, *dStatus = nullptr;
  double *dSub = nullptr, *dTotals = nullptr, *dBest = nullptr, *dSecond = nullptr, *dChunk = nullptr, *dBnd = nullptr, *dTab = nullptr;
  const int64_t zero = 0;
  const size_t nc = (size_t)in.nClusters;
  if ((rc = paUpload(bufs, &dCands, in.candSeqs, in.nCand ? (size_t)in.candOff[in.nCand] : 0))) return rc;
  if ((rc = paUpload(bufs, &dCandOff, in.nCand ? in.candOff : &zero, (size_t)in.nCand + 1))) return rc;
  if ((rc = paUpload(bufs, &dReads, in.readSeqs, in.nReads ? (size_t)in.readOff[in.nReads] : 0))) return rc;
  if ((rc = paUpload(bufs, &dReadOff, in.nReads ? in.readOff : &zero, (size_t)in.nReads + 1))) return rc;
  if (in.readStrand && (rc = paUpload(bufs, &dStrand, in.readStrand, (size_t)in.nReads))) return rc;
  if ((rc = paUpload(bufs, &dClusterCandOff, in.clusterCandOff, nc + 1))) return rc;
  if ((rc = paUpload(bufs, &dClusterReadOff, in.clusterReadOff, nc + 1))) return rc;
  if ((rc = paUpload(bufs, &dItemOff, (const int64_t*)itemOff.data(), nc + 1))) return rc;
  if ((rc = paUpload(bufs, &dSub, hs.sub, 16))) return rc;
  if (forward && (rc = paUpload(bufs, &dTab, dnas::lseTable().data(), dnas::lseTable().size()))) return rc;
  if ((rc = paAlloc(bufs, &dTotals, (size_t)in.nCand))) return rc;
  if ((rc = paAlloc(bufs, &dWinner, nc))) return rc;
  if ((rc = paAlloc(bufs, &dBest, nc))) return rc;
  if ((rc = paAlloc(bufs, &dSecond, nc))) return rc;
  if ((rc = paAlloc(bufs, &dStatus, nc))) return rc;
  if ((rc = paAlloc(bufs, &dChunk, (size_t)plan.chunkItems))) return rc;
  if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;
  const dnas::ConsensusItems items{in.nClusters, dClusterCandOff, dClusterReadOff, dItemOff};

  if (in.nCand) {
    hipLaunchKernelGGL(consensus_init_kernel, dim3((unsigned)((in.nCand + 255) / 256)), dim3(256), 0, stream, in.nCand, dTotals);
    DNAS_HIP_TRY(hipGetLastError());
  }
  const auto score = [&](int64_t first, int64_t count) {
    paDispatchKP(sc.P, [&](auto kp) {
      if (forward)
        hipLaunchKernelGGL(forwardOf(kp), dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), plan.ldsBytes, stream, sc, dSub, dTab,
                           band, plan.ldsCols, first, count, items, dCands, dCandOff, dReads, dReadOff, dStrand, dBnd, plan.bndStride,
                           dChunk);
      else
        hipLaunchKernelGGL(kernelOf(kp), dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), plan.ldsBytes, stream, sc, dSub, band,
                           plan.ldsCols, first, count, items, dCands, dCandOff, dReads, dReadOff, dStrand, dBnd, plan.bndStride, dChunk);
    });
  };
  const auto fold = [&](int64_t first, int64_t count) {
    const int64_t candFirst = hostItems.candOfItem(first), candCount = hostItems.candOfItem(first + count - 1) - candFirst + 1;
    hipLaunchKernelGGL(consensus_fold_kernel, dim3((unsigned)((candCount + 255) / 256)), dim3(256), 0, stream, first, count, candFirst,
                       candCount, items, dChunk, dTotals);
  };
  if ((rc = paRunChunks(bufs, total, plan.chunkItems, score, fold, [](int64_t, int64_t) { return hipSuccess; }, stats))) return rc;
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], stream));
  hipLaunchKernelGGL(consensus_pick_kernel, dim3((unsigned)((in.nClusters + 255) / 256)), dim3(256), 0, stream, items, dTotals, dWinner,
                     dBest, dSecond, dStatus);
  DNAS_HIP_TRY(hipGetLastError());
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[2], stream));
  DNAS_HIP_TRY(hipStreamSynchronize(stream));
  float pick = 0;
  DNAS_HIP_TRY(hipEventElapsedTime(&pick, bufs.ev[1], bufs.ev[2]));
  stats->fold_ms += pick;
  DNAS_HIP_TRY(hipMemcpy(out_winner, dWinner, nc * sizeof(int64_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_total, dBest, nc * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_second, dSecond, nc * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_status, dStatus, nc, hipMemcpyDeviceToHost));
  if (out_totals && in.nCand) DNAS_HIP_TRY(hipMemcpy(out_totals, dTotals, (size_t)in.nCand * sizeof(double), hipMemcpyDeviceToHost));
  return DNAS_OK;
}

}  // namespace

namespace {

// dnas_consensus_score_ex after its checks.  Posteriors come from the per-candidate totals on the host (consensusPosteriors).
int csScore(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand, const int8_t* cand_seqs,
            const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
            const uint8_t* read_strand, const int64_t* cluster_read_off, int device_id, int score_mode, int64_t* out_winner,
            double* out_total, double* out_second, uint8_t* out_status, double* out_totals, dnas_consensus_stats* out_stats) {
  dnas_consensus_stats total{};
  if (out_stats) *out_stats = total;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    const CsInputs all{n_clusters, n_cand, n_reads, cand_seqs, cand_off, cluster_cand_off, read_seqs, read_off, read_strand, cluster_read_off};
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = devices.size();
    if (W == 1 || n_clusters == 0) {
      const int rc = csRunOnDevice(devices[0], hs, band, score_mode, all, out_winner, out_total, out_second, out_status, out_totals, &total);
      if (rc == DNAS_OK && out_stats) *out_stats = total;
      return rc;
    }
    // every GPU of the node: the clusters dealt by candidates x sum of (read length + 1), one host thread per device, every
    // device's candidates, reads and offsets gathered for it, results scattered back under the caller's indices
    std::vector<int64_t> cost((size_t)n_clusters);
    for (int64_t c = 0; c < n_clusters; ++c) {
      const int64_t r0 = cluster_read_off[c], r1 = cluster_read_off[c + 1];
      cost[(size_t)c] = (cluster_cand_off[c + 1] - cluster_cand_off[c]) * ((r1 > r0 ? read_off[r1] - read_off[r0] : 0) + (r1 - r0));
    }
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    std::vector<dnas_consensus_stats> stats(W);
    const int rc = dnas::forEachDevice(devices, [&](size_t k) {
      const std::vector<int64_t>& mine = shard[k];
      const size_t m = mine.size();
      std::vector<int64_t> candIds, readIds, clCandOff(1, 0), clReadOff(1, 0), candOff, readOff;
      for (int64_t c : mine) {
        for (int64_t j = cluster_cand_off[c]; j < cluster_cand_off[c + 1]; ++j) candIds.push_back(j);
        for (int64_t i = cluster_read_off[c]; i < cluster_read_off[c + 1]; ++i) readIds.push_back(i);
        clCandOff.push_back((int64_t)candIds.size());
        clReadOff.push_back((int64_t)readIds.size());
      }
      std::vector<int8_t> cands, reads;
      dnas::gatherShard(candIds, cand_seqs, cand_off, &cands, &candOff);
      dnas::gatherShard(readIds, read_seqs, read_off, &reads, &readOff);
      std::vector<uint8_t> strand(readIds.size() + 1);
      if (read_strand) for (size_t q = 0; q < readIds.size(); ++q) strand[q] = read_strand[readIds[q]];
      const CsInputs part{(int64_t)m, clCandOff.back(), clReadOff.back(), cands.data(), candOff.data(), clCandOff.data(), reads.data(),
                          readOff.data(), read_strand ? strand.data() : nullptr, clReadOff.data()};
      std::vector<int64_t> winner(m + 1);
      std::vector<double> best(m + 1), second(m + 1), totals((size_t)part.nCand + 1);
      std::vector<uint8_t> status(m + 1);
      const int rc = csRunOnDevice(devices[k], hs, band, score_mode, part, winner.data(), best.data(), second.data(), status.data(), totals.data(), &stats[k]);
      if (rc != DNAS_OK) return rc;
      for (size_t q = 0; q < m; ++q) {
        const int64_t c = mine[q];
        out_winner[c] = winner[q] < 0 ? -1 : winner[q] - clCandOff[q] + cluster_cand_off[c];
        out_total[c] = best[q];
        out_second[c] = second[q];
        out_status[c] = status[q];
        if (out_totals) std::copy(totals.begin() + clCandOff[q], totals.begin() + clCandOff[q + 1], out_totals + cluster_cand_off[c]);
      }
      return DNAS_OK;
    });
    if (rc != DNAS_OK) return rc;
    for (size_t k = 0; k < W; ++k) {
      total.score_ms = std::max(total.score_ms, stats[k].score_ms);
      total.fold_ms = std::max(total.fold_ms, stats[k].fold_ms);
      total.items += stats[k].items;
      total.cells += stats[k].cells;
      total.chunks += stats[k].chunks;
    }
    total.candidates = n_cand;
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

}  // namespace

extern "C" int dnas_consensus_score_ex(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand,
                                       const int8_t* cand_seqs, const int64_t* cand_off, const int64_t* cluster_cand_off,
                                       int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                                       const int64_t* cluster_read_off, int device_id, int score_mode, int64_t* out_winner,
                                       double* out_total, double* out_second, uint8_t* out_status, double* out_totals,
                                       double* out_posterior, dnas_consensus_stats* out_stats) {
  if (const int rc = dnas::checkConsensusArgs(params, band, n_clusters, n_cand, cand_seqs, cand_off, cluster_cand_off, n_reads, read_seqs,
                                              read_off, read_strand, cluster_read_off, out_winner, out_total, out_second, out_status))
    return rc;
  if (const int rc = dnas::checkScoreMode(score_mode, out_posterior)) return rc;
  try {
    std::vector<double> own;                                 // the posteriors need every total
    if (out_posterior && !out_totals) {
      own.resize((size_t)n_cand + 1);
      out_totals = own.data();
    }
    const int rc = csScore(params, band, n_clusters, n_cand, cand_seqs, cand_off, cluster_cand_off, n_reads, read_seqs, read_off,
                           read_strand, cluster_read_off, device_id, score_mode, out_winner, out_total, out_second, out_status,
                           out_totals, out_stats);
    if (rc != DNAS_OK) return rc;
    if (out_posterior) dnas::consensusPosteriors(n_clusters, cluster_cand_off, out_status, out_totals, out_posterior);
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  }
}

extern "C" int dnas_consensus_score(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand,
                                    const int8_t* cand_seqs, const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads,
                                    const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                                    const int64_t* cluster_read_off, int device_id, int64_t* out_winner, double* out_total,
                                    double* out_second, uint8_t* out_status, double* out_totals, dnas_consensus_stats* out_stats) {
  return dnas_consensus_score_ex(params, band, n_clusters, n_cand, cand_seqs, cand_off, cluster_cand_off, n_reads, read_seqs, read_off,
                                 read_strand, cluster_read_off, device_id, DNAS_SCORE_VITERBI, out_winner, out_total, out_second,
                                 out_status, out_totals, nullptr, out_stats);
}
