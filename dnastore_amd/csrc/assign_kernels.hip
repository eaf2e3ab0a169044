// dnas_assign_reads: which original, in which orientation, each read of a pool came from (include/dnastore_amd.h), bit-identical
// to assignReadsHost (host/assign.cpp).
//
// Score.  The work is N x K x strands pair-HMM scores and nothing but scores: the kernel is paScoreChunk of pair_align_device.h,
// the launch plan, the chunk loop and the fan-out over devices are the shared ones.  What is stated here is the
// item -- (read, candidate, strand), derived from the work index: no expanded list exists on the host or in HBM.  The reverse
// strand is read in place, 3 - b[O-1-j], as the 64-base chunks are loaded.
//
// Fold.  One thread per read folds that read's scores of the chunk in item order into (best, original, strand, second) with
// AssignFold (host/assign.hpp), the state in per-read device arrays: a read whose items span chunks is folded chunk after
// chunk in stream order.  Device memory beyond the sequences and the per-read outputs is the one chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/assign.hpp"
#include "host/pairalign.hpp"
#include "pair_align_device.h"

namespace {

// What says which items a run has: without candidate lists every read has K candidates, with them read r's are
// candIdx[candOff[r] .. candOff[r+1]); each candidate is strands items.  Candidate slots are counted over the whole run.
struct AsItems {
  int64_t nReads, K;
  int mode;
  const int64_t* candOff;
  const int64_t* candIdx;
  __host__ __device__ int strands() const { return dnas::strandsOf(mode); }
  __host__ __device__ int64_t slot0(int64_t r) const { return candOff ? candOff[r] : r * K; }
  __host__ __device__ int64_t readOfSlot(int64_t c) const {
    if (!candOff) return c / K;
    int64_t lo = 0, hi = nReads;                         // the r with candOff[r] <= c < candOff[r+1]
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (candOff[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
  }
  __host__ __device__ int64_t origOfSlot(int64_t c, int64_t r) const { return candOff ? candIdx[c] : c - r * K; }
};

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void assign_score_kernel(
    PaScores sc, const double* __restrict__ subTable, int band, int ldsCols, int64_t first, int64_t count, AsItems items,
    const int8_t* __restrict__ origSeqs, const int64_t* __restrict__ origOff, const int8_t* __restrict__ readSeqs,
    const int64_t* __restrict__ readOff, double* bndScratch, int64_t bndStride, double* __restrict__ chunk) {
  const int strands = items.strands();
  const auto itemAt = [&](int64_t g) -> PaItem {         // candidate slot g / strands of its read against the original it names
    const int64_t c = g / strands;
    const int strand = dnas::strandAt(items.mode, (int)(g - c * strands));
    const int64_t r = items.readOfSlot(c), o = items.origOfSlot(c, r);
    const int I = (int)(origOff[o + 1] - origOff[o]), O = (int)(readOff[r + 1] - readOff[r]);
    return {origSeqs + origOff[o], readSeqs + readOff[r], I, O, strand != 0};
  };
  paScoreChunk<KP>(sc, subTable, band, ldsCols, first, count, itemAt, bndScratch, bndStride, chunk);
}

__global__ void assign_init_kernel(AsItems items, double* __restrict__ best, double* __restrict__ second,
                                   int64_t* __restrict__ original, uint8_t* __restrict__ strand, uint8_t* __restrict__ status) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= items.nReads) return;
  const dnas::AssignFold f;
  best[r] = f.best;
  second[r] = f.second;
  original[r] = f.original;
  strand[r] = (uint8_t)f.strand;
  status[r] = f.status((items.slot0(r + 1) - items.slot0(r)) * items.strands());
}

// The reads readFirst .. readFirst + readCount - 1 are those with items in the chunk [first, first + count).
__global__ void assign_fold_kernel(int64_t first, int64_t count, int64_t readFirst, int64_t readCount, AsItems items,
                                   const double* __restrict__ chunk, double* __restrict__ best, double* __restrict__ second,
                                   int64_t* __restrict__ original, uint8_t* __restrict__ strand, uint8_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= readCount) return;
  const int64_t r = readFirst + i;
  const int strands = items.strands();
  const int64_t g0 = items.slot0(r) * strands, g1 = items.slot0(r + 1) * strands;
  const int64_t lo = g0 > first ? g0 : first, hi = g1 < first + count ? g1 : first + count;
  if (lo >= hi) return;
  dnas::AssignFold f;
  f.best = best[r];
  f.second = second[r];
  f.original = original[r];
  f.strand = strand[r];
  for (int64_t g = lo; g < hi; ++g) {
    const int64_t c = g / strands;
    f.add(chunk[g - first], items.origOfSlot(c, r), dnas::strandAt(items.mode, (int)(g - c * strands)));
  }
  best[r] = f.best;
  second[r] = f.second;
  original[r] = f.original;
  strand[r] = (uint8_t)f.strand;
  status[r] = f.status(g1 - g0);
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct AsDevice {
  int device = 0, cus = 256;
  PaBuffers bufs;                                        // the stream, the events, and the originals
  int8_t* dOrig = nullptr;
  int64_t* dOrigOff = nullptr;
  double* dSub = nullptr;
};

}  // namespace

struct dnas_assigner {
  dnas::PairScores hs;
  int band = 0;
  int64_t K = 0;
  std::vector<int64_t> origLen;
  std::vector<std::unique_ptr<AsDevice>> devs;
};

namespace {

int asOpenDevice(const dnas_assigner& h, int device, const int8_t* orig_seqs, const int64_t* orig_off, AsDevice& d) {
  d.device = device;
  DNAS_HIP_TRY(hipSetDevice(device));
  int rc;
  if ((rc = d.bufs.open())) return rc;
  (void)hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, device);
  const int64_t zero = 0;
  if ((rc = paUpload(d.bufs, &d.dOrig, orig_seqs, h.K ? (size_t)orig_off[h.K] : 0))) return rc;
  if ((rc = paUpload(d.bufs, &d.dOrigOff, h.K ? orig_off : &zero, (size_t)h.K + 1))) return rc;
  if ((rc = paUpload(d.bufs, &d.dSub, h.hs.sub, 16))) return rc;
  return DNAS_OK;
}

// Cells inside the band over all items.
int64_t asCells(const dnas_assigner& h, const AsItems& items, const int64_t* read_off, int maxO) {
  PaCellMemo memo(h.origLen.empty() ? 0 : *std::max_element(h.origLen.begin(), h.origLen.end()), maxO, h.band);
  std::map<int64_t, int64_t> lengths;                    // without candidate lists: how many originals of each length
  if (!items.candOff) for (int64_t I : h.origLen) ++lengths[I];
  int64_t total = 0;
  for (int64_t r = 0; r < items.nReads; ++r) {
    const int64_t O = read_off[r + 1] - read_off[r];
    if (items.candOff)
      for (int64_t c = items.candOff[r]; c < items.candOff[r + 1]; ++c) total += memo.cells(h.origLen[(size_t)items.candIdx[c]], O);
    else
      for (const auto& kv : lengths) total += kv.second * memo.cells(kv.first, O);
  }
  return total * items.strands();
}

// One device.  The arguments were checked; results go to the caller's arrays.
int asRunOnDevice(const dnas_assigner& h, AsDevice& d, int64_t n, const int8_t* read_seqs, const int64_t* read_off, int strand_mode,
                  const int64_t* cand_off, const int64_t* cand_idx, int64_t* out_original, uint8_t* out_strand, double* out_score,
                  double* out_second, uint8_t* out_status, double* out_item_scores, dnas_assign_stats* stats) {
  *stats = dnas_assign_stats{};
  if (n == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(d.device));
  hipStream_t stream = d.bufs.stream;
  const AsItems hostItems{n, h.K, strand_mode, cand_off, cand_idx};
  const int strands = hostItems.strands();
  const int64_t total = hostItems.slot0(n) * strands;
  stats->items = total;
  int maxO = 0;
  for (int64_t r = 0; r < n; ++r) maxO = std::max(maxO, (int)(read_off[r + 1] - read_off[r]));
  stats->cells = asCells(h, hostItems, read_off, maxO);

  const PaScores sc = PaScores::from(h.hs);
  const auto kernelOf = [](auto kp) { return &assign_score_kernel<decltype(kp)::value>; };
  PaLaunchPlan plan;
  int rc;
  if ((rc = paPlanScore(sc.P, kernelOf, d.cus, maxO, "DNAS_ASSIGN_CHUNK", total, &plan))) return rc;

  PaBuffers bufs;                                        // this run's memory
  int8_t* dReads = nullptr;
  int64_t *dReadOff = nullptr, *dCandOff = nullptr, *dCandIdx = nullptr, *dOriginal = nullptr;
  double *dBest = nullptr, *dSecond = nullptr, *dChunk = nullptr, *dBnd = nullptr;
  uint8_t *dStrand = nullptr, *dStatus = nullptr;
  if ((rc = paUpload(bufs, &dReads, read_seqs, (size_t)read_off[n]))) return rc;
  if ((rc = paUpload(bufs, &dReadOff, read_off, (size_t)n + 1))) return rc;
  if (cand_off) {
    if ((rc = paUpload(bufs, &dCandOff, cand_off, (size_t)n + 1))) return rc;
    if ((rc = paUpload(bufs, &dCandIdx, cand_idx, (size_t)cand_off[n]))) return rc;
  }
  if ((rc = paAlloc(bufs, &dOriginal, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dBest, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dSecond, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dStrand, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dStatus, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dChunk, (size_t)plan.chunkItems))) return rc;
  if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;
  const AsItems items{n, h.K, strand_mode, dCandOff, dCandIdx};

  hipLaunchKernelGGL(assign_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, items, dBest, dSecond, dOriginal,
                     dStrand, dStatus);
  DNAS_HIP_TRY(hipGetLastError());
  const auto score = [&](int64_t first, int64_t count) {
    paDispatchKP(sc.P, [&](auto kp) {
      hipLaunchKernelGGL(kernelOf(kp), dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), plan.ldsBytes, stream, sc, d.dSub, h.band,
                         plan.ldsCols, first, count, items, d.dOrig, d.dOrigOff, dReads, dReadOff, dBnd, plan.bndStride, dChunk);
    });
  };
  const auto fold = [&](int64_t first, int64_t count) {
    const int64_t readFirst = hostItems.readOfSlot(first / strands), readLast = hostItems.readOfSlot((first + count - 1) / strands);
    const int64_t readCount = readLast - readFirst + 1;
    hipLaunchKernelGGL(assign_fold_kernel, dim3((unsigned)((readCount + 255) / 256)), dim3(256), 0, stream, first, count, readFirst,
                       readCount, items, dChunk, dBest, dSecond, dOriginal, dStrand, dStatus);
  };
  const auto copyScores = [&](int64_t first, int64_t count) {
    if (!out_item_scores) return hipSuccess;
    return hipMemcpyAsync(out_item_scores + first, dChunk, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, stream);
  };
  if ((rc = paRunChunks(d.bufs, total, plan.chunkItems, score, fold, copyScores, stats))) return rc;
  DNAS_HIP_TRY(hipStreamSynchronize(stream));                  // (without items no chunk ran: the init kernel before the copies)
  DNAS_HIP_TRY(hipMemcpy(out_original, dOriginal, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_strand, dStrand, (size_t)n, hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_score, dBest, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_second, dSecond, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_status, dStatus, (size_t)n, hipMemcpyDeviceToHost));
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_assigner_create(const dnas_mutator_params* params, int32_t band, int64_t n_originals, const int8_t* orig_seqs,
                                    const int64_t* orig_off, int device_id, dnas_assigner** out) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "assign reads: null argument");
  *out = nullptr;
  if (const int rc = dnas::checkAssignOriginals(params, band, n_originals, orig_seqs, orig_off)) return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    std::unique_ptr<dnas_assigner> h(new dnas_assigner);
    h->hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    h->band = band;
    h->K = n_originals;
    for (int64_t i = 0; i < n_originals; ++i) h->origLen.push_back(orig_off[i + 1] - orig_off[i]);
    for (int device : dnas::pickDevices(device_id)) {
      h->devs.emplace_back(new AsDevice);
      if (const int rc = asOpenDevice(*h, device, orig_seqs, orig_off, *h->devs.back())) return rc;
    }
    *out = h.release();
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

extern "C" void dnas_assigner_destroy(dnas_assigner* h) {
  if (!h) return;
  for (auto& d : h->devs) (void)hipSetDevice(d->device), d.reset();      // (buffers are freed on the device that holds them)
  delete h;
}

extern "C" int dnas_assigner_run(dnas_assigner* h, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode,
                                 const int64_t* cand_off, const int64_t* cand_idx, int64_t* out_original, uint8_t* out_strand,
                                 double* out_score, double* out_second, uint8_t* out_status, double* out_item_scores,
                                 dnas_assign_stats* out_stats) {
  if (!h) return dnas::fail(DNAS_E_INVALID, "assign reads: null handle");
  if (const int rc = dnas::checkAssignReads(h->K, n_reads, read_seqs, read_off, strand_mode, cand_off, cand_idx, out_original, out_strand,
                                            out_score, out_second, out_status))
    return rc;
  dnas_assign_stats total{};
  if (out_stats) *out_stats = total;
  try {
    const size_t W = h->devs.size();
    if (W == 1 || n_reads == 0) {
      const int rc = asRunOnDevice(*h, *h->devs[0], n_reads, read_seqs, read_off, strand_mode, cand_off, cand_idx, out_original,
                                   out_strand, out_score, out_second, out_status, out_item_scores, &total);
      if (rc == DNAS_OK && out_stats) *out_stats = total;
      return rc;
    }
    // every GPU of the node: the reads dealt by their items x (length + 1), one host thread per device, results scattered back
    const AsItems all{n_reads, h->K, strand_mode, cand_off, cand_idx};
    const int strands = all.strands();
    std::vector<int64_t> cost((size_t)n_reads);
    for (int64_t r = 0; r < n_reads; ++r) cost[(size_t)r] = (all.slot0(r + 1) - all.slot0(r)) * strands * (read_off[r + 1] - read_off[r] + 1);
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    std::vector<int> devices;
    for (const auto& d : h->devs) devices.push_back(d->device);
    std::vector<dnas_assign_stats> stats(W);
    const int rc = dnas::forEachDevice(devices, [&](size_t k) {
      const std::vector<int64_t>& mine = shard[k];
      const size_t m = mine.size();
      std::vector<int8_t> reads;
      std::vector<int64_t> readOff, candIdx, candOff, itemOff(1, 0);
      dnas::gatherShard(mine, read_seqs, read_off, &reads, &readOff);
      if (cand_off) dnas::gatherShard(mine, cand_idx, cand_off, &candIdx, &candOff);
      for (int64_t r : mine) itemOff.push_back(itemOff.back() + (all.slot0(r + 1) - all.slot0(r)) * strands);
      std::vector<int64_t> original(m + 1);
      std::vector<uint8_t> strand(m + 1), status(m + 1);
      std::vector<double> score(m + 1), second(m + 1), itemScores(out_item_scores ? (size_t)itemOff.back() + 1 : 0);
      const int rc = asRunOnDevice(*h, *h->devs[k], (int64_t)m, reads.data(), readOff.data(), strand_mode, cand_off ? candOff.data() : nullptr,
                                   cand_off ? candIdx.data() : nullptr, original.data(), strand.data(), score.data(), second.data(),
                                   status.data(), out_item_scores ? itemScores.data() : nullptr, &stats[k]);
      if (rc != DNAS_OK) return rc;
      for (size_t j = 0; j < m; ++j) {
        const int64_t r = mine[j];
        out_original[r] = original[j];
        out_strand[r] = strand[j];
        out_score[r] = score[j];
        out_second[r] = second[j];
        out_status[r] = status[j];
        if (out_item_scores)
          std::copy(itemScores.begin() + itemOff[j], itemScores.begin() + itemOff[j + 1], out_item_scores + all.slot0(r) * strands);
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
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

extern "C" int dnas_assign_reads(const dnas_mutator_params* params, int32_t band, int64_t n_originals, const int8_t* orig_seqs,
                                 const int64_t* orig_off, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                 int strand_mode, const int64_t* cand_off, const int64_t* cand_idx, int device_id, int64_t* out_original,
                                 uint8_t* out_strand, double* out_score, double* out_second, uint8_t* out_status,
                                 double* out_item_scores, dnas_assign_stats* out_stats) {
  dnas_assigner* h = nullptr;
  if (const int rc = dnas_assigner_create(params, band, n_originals, orig_seqs, orig_off, device_id, &h)) return rc;
  const int rc = dnas_assigner_run(h, n_reads, read_seqs, read_off, strand_mode, cand_off, cand_idx, out_original, out_strand, out_score,
                                   out_second, out_status, out_item_scores, out_stats);
  dnas_assigner_destroy(h);
  return rc;
}
