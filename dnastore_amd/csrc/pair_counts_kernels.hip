// dnas_pair_counts and dnas_baum_welch_pairs: the marginal E-step of host/paircounts.hpp on the GPU and the EM loop of
// host/baumwelch.hpp over it.  The kernel is pcCountsPair of pair_counts_device.h: a wave owns a pair and walks the list with the
// grid's stride, the forward pass parking every cell in the wave's scratch, the backward pass meeting it there.  Launch plan,
// chunk loop, buffers and the fan-out over devices are the shared ones; the scratch plan -- the grid is cut
// until the scratch of all its waves fits the arena -- is pair_counts_plan.hpp's, shared with dnas_pair_profiles.  The call's totals are formed on the host from the
// per-pair slots in pair order, so they do not depend on grid, chunking or device count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <memory>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/baumwelch.hpp"
#include "host/paircounts.hpp"
#include "host/pairforward.hpp"
#include "pair_counts_device.h"
#include "pair_counts_plan.hpp"

namespace {

// Dynamic LDS, per wave: 16 substitution scores, 2 ldsCols boundary doubles, the [16][64] substitution counters.
template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void pair_counts_kernel(
    PaScores sc, const double* __restrict__ subTable, const double* __restrict__ lseTab, int band, int ldsCols, int64_t first,
    int64_t count, const int64_t* __restrict__ runIdx, const int8_t* __restrict__ inSeqs, const int64_t* __restrict__ inOff,
    const int8_t* __restrict__ outSeqs, const int64_t* __restrict__ outOff, const uint8_t* __restrict__ outRev, double* bndScratch,
    int64_t bndStride, double* parkScratch, int64_t parkStride, int64_t maxWaves, double* __restrict__ slots, int slotStride) {
  extern __shared__ double lds[];
  // (a wave beyond maxWaves fills its LDS slice too before it leaves: the block's LDS has the slice, and bndMem is only formed)
  const PaWave w = paWaveBegin(lds, (size_t)(16 + 2 * ldsCols + kPcSubSlots), subTable, bndScratch, bndStride);
  const int64_t nWaves = w.nWaves < maxWaves ? w.nWaves : maxWaves;
  if (w.wave >= nWaves) return;                                // the arena holds no scratch for this wave (no barrier follows)
  double* const scr = parkScratch + w.wave * parkStride;

  for (int64_t q = w.wave; q < count; q += nWaves) {
    const int64_t g = runIdx[first + q];
    const PaItem it{inSeqs + inOff[g], outSeqs + outOff[g], (int)(inOff[g + 1] - inOff[g]), (int)(outOff[g + 1] - outOff[g]),
                    outRev != nullptr && outRev[g] != 0};
    pcCountsPair<KP>(sc, lseTab, w.lds, ldsCols, w.bndMem, scr, w.lane, band, it, slots + g * slotStride);
  }
}

// One device's share of a call or a fit: sequences, table and scratch go up once, estep() runs the kernel under new parameters.
class PcDevice {
 public:
  // The arguments were checked.  P duplication lengths for the life of the object.
  int open(int device, int band, int P, int64_t n, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs,
           const int64_t* out_off, const uint8_t* out_rev, size_t arena_bytes) {
    const auto occupancy = [&](size_t ldsBytes, int* perCu) {
      return paDispatchKP(P, [&](auto kp) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCu, &pair_counts_kernel<decltype(kp)::value>, 64 * kPaWavesPerBlock, ldsBytes);
      });
    };
    if (const int rc = w_.open(device, band, P, n, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes, (size_t)P + 2, kPcLdsCols,
                               16 + kPcSubSlots, (int64_t)1 << 22, occupancy))
      return rc;
    if (w_.run.empty()) return DNAS_OK;
    return paAlloc(w_.bufs, &dSlots_, (size_t)n * (size_t)(21 + P + 2));
  }

  // One E-step: pairCounts[n x nc], pairLl[n], pairBack[n] (may be null), status[n] of this device's pairs.
  int estep(const dnas::PairScores& hs, double* pairCounts, double* pairLl, double* pairBack, uint8_t* status,
            dnas_counts_stats* stats) {
    *stats = dnas_counts_stats{};
    const int nc = 21 + w_.P, stride = nc + 2;
    const int64_t nRun = (int64_t)w_.run.size();
    if (nRun > 0) {
      DNAS_HIP_TRY(hipSetDevice(w_.device));
      const PaScores sc = PaScores::from(hs);
      DNAS_HIP_TRY(hipMemcpy(w_.dSub, hs.sub, 16 * sizeof(double), hipMemcpyHostToDevice));
      const PaLaunchPlan& plan = w_.plan;
      const auto launch = [&](int64_t first, int64_t count) {
        paDispatchKP(w_.P, [&](auto kp) {
          hipLaunchKernelGGL(pair_counts_kernel<decltype(kp)::value>, dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock),
                             plan.ldsBytes, w_.bufs.stream, sc, w_.dSub, w_.dTab, w_.band, plan.ldsCols, first, count, w_.dRun, w_.dIn,
                             w_.dInOff, w_.dOut, w_.dOutOff, w_.dRev, w_.dBnd, plan.bndStride, w_.dPark, w_.parkStride, w_.waves,
                             dSlots_, stride);
        });
      };
      PcChunkStats cs;
      if (const int rc = paRunChunks(w_.bufs, nRun, plan.chunkItems, launch, [](int64_t, int64_t) {},
                                     [](int64_t, int64_t) { return hipSuccess; }, &cs))
        return rc;
      slots_.resize((size_t)w_.n * (size_t)stride);
      DNAS_HIP_TRY(hipMemcpy(slots_.data(), dSlots_, slots_.size() * sizeof(double), hipMemcpyDeviceToHost));
      stats->kernel_ms = cs.score_ms;
      stats->chunks = cs.chunks;
    }
    stats->cells = w_.cells;
    stats->scratch_bytes = w_.scratchBytes;
    stats->pairs_too_large = w_.tooLarge;
    stats->waves = nRun > 0 ? w_.waves : 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), neg = -std::numeric_limits<double>::infinity();
    for (int64_t i = 0; i < w_.n; ++i) {
      double* c = pairCounts + (size_t)i * (size_t)nc;
      if (w_.status[(size_t)i] == DNAS_COUNTS_TOO_LARGE) {
        std::fill(c, c + nc, 0.);
        pairLl[i] = nan;
        if (pairBack) pairBack[i] = nan;
        status[i] = DNAS_COUNTS_TOO_LARGE;
        continue;
      }
      const double* slot = slots_.data() + (size_t)i * (size_t)stride;
      std::copy(slot, slot + nc, c);
      pairLl[i] = slot[nc];
      if (pairBack) pairBack[i] = slot[nc + 1];
      status[i] = slot[nc] > neg ? DNAS_COUNTS_OK : DNAS_COUNTS_NO_PATH;
    }
    return DNAS_OK;
  }

 private:
  PcWorkspace w_;
  std::vector<double> slots_;
  double* dSlots_ = nullptr;
};

// The pairs of a call dealt over the devices as dnas_align_pairs deals them; estep() gathers every device's results under the
// caller's indices and forms the totals in pair order.
class PcFit {
 public:
  int open(int device_id, int band, int P, int64_t n, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs,
           const int64_t* out_off, const uint8_t* out_rev, size_t arena_bytes) {
    n_ = n;
    nc_ = 21 + P;
    pcDeal(device_id, band, n, in_off, out_off, &devices_, &shard_);
    const size_t W = devices_.size();
    dev_.clear();
    for (size_t k = 0; k < W; ++k) dev_.emplace_back(new PcDevice);
    if (W == 1) return dev_[0]->open(devices_[0], band, P, n, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes);
    return dnas::forEachDevice(devices_, [&](size_t k) {
      const std::vector<int64_t>& mine = shard_[k];
      const size_t m = mine.size();
      std::vector<int8_t> in, outs;
      std::vector<int64_t> inOff, outOff;
      dnas::gatherShard(mine, in_seqs, in_off, &in, &inOff);
      dnas::gatherShard(mine, out_seqs, out_off, &outs, &outOff);
      std::vector<uint8_t> rev(m + 1);
      if (out_rev) for (size_t j = 0; j < m; ++j) rev[j] = out_rev[mine[j]];
      return dev_[k]->open(devices_[k], band, P, (int64_t)m, in.data(), inOff.data(), outs.data(), outOff.data(),
                           out_rev ? rev.data() : nullptr, arena_bytes);
    });
  }

  // out_pair_counts and out_pair_ll_backward may be null.
  int estep(const dnas_mutator_params& params, double* out_counts, double* out_ll, double* out_pair_counts, double* out_pair_ll,
            double* out_pair_ll_backward, uint8_t* out_status, dnas_counts_stats* out_stats) {
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(params));
    const size_t W = dev_.size();
    dnas_counts_stats total{};
    if (!out_pair_counts) {
      ownCounts_.resize((size_t)std::max<int64_t>(n_, 1) * (size_t)nc_);
      out_pair_counts = ownCounts_.data();
    }
    if (W == 1) {
      if (const int rc = dev_[0]->estep(hs, out_pair_counts, out_pair_ll, out_pair_ll_backward, out_status, &total)) return rc;
    } else {
      std::vector<dnas_counts_stats> stats(W);
      const int rc = dnas::forEachDevice(devices_, [&](size_t k) {
        const std::vector<int64_t>& mine = shard_[k];
        const size_t m = mine.size();
        std::vector<double> c((m + 1) * (size_t)nc_), ll(m + 1), back(m + 1);
        std::vector<uint8_t> st(m + 1);
        if (const int rc = dev_[k]->estep(hs, c.data(), ll.data(), back.data(), st.data(), &stats[k])) return rc;
        for (size_t j = 0; j < m; ++j) {
          std::copy(c.begin() + (ptrdiff_t)(j * (size_t)nc_), c.begin() + (ptrdiff_t)((j + 1) * (size_t)nc_),
                    out_pair_counts + (size_t)mine[j] * (size_t)nc_);
          out_pair_ll[mine[j]] = ll[j];
          if (out_pair_ll_backward) out_pair_ll_backward[mine[j]] = back[j];
          out_status[mine[j]] = st[j];
        }
        return DNAS_OK;
      });
      if (rc != DNAS_OK) return rc;
      for (size_t k = 0; k < W; ++k) {
        total.kernel_ms = std::max(total.kernel_ms, stats[k].kernel_ms);
        total.cells += stats[k].cells;
        total.chunks += stats[k].chunks;
        total.scratch_bytes += stats[k].scratch_bytes;
        total.pairs_too_large += stats[k].pairs_too_large;
        total.waves += stats[k].waves;
      }
    }
    dnas::pairCountsTotals(n_, nc_, out_pair_counts, out_pair_ll, out_status, out_counts, out_ll);
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  }

 private:
  int64_t n_ = 0;
  int nc_ = 21;
  std::vector<int> devices_;
  std::vector<std::unique_ptr<PcDevice>> dev_;
  std::vector<std::vector<int64_t>> shard_;
  std::vector<double> ownCounts_;
};

}  // namespace

extern "C" int dnas_pair_counts(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                                const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                                int device_id, size_t arena_bytes, double* out_counts, double* out_ll, double* out_pair_counts,
                                double* out_pair_ll, double* out_pair_ll_backward, uint8_t* out_status, dnas_counts_stats* out_stats) {
  if (const int rc = dnas::checkCountsArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_counts, out_ll, out_pair_ll,
                                           out_status))
    return rc;
  if (out_stats) *out_stats = dnas_counts_stats{};
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  return pcGuarded([&] {
    PcFit fit;
    if (const int rc = fit.open(device_id, band, params->n_len, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes))
      return rc;
    return fit.estep(*params, out_counts, out_ll, out_pair_counts, out_pair_ll, out_pair_ll_backward, out_status, out_stats);
  });
}

extern "C" int dnas_baum_welch_pairs(const dnas_mutator_params* init, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                                     const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                                     int device_id, size_t arena_bytes, int32_t max_iterations, dnas_mutator_params* out,
                                     int32_t* out_iterations, dnas_mutator_params* out_trace_params, double* out_trace_ll,
                                     int32_t* out_n_trace) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "pair counts: null argument");
  if (max_iterations < 0) return dnas::fail(DNAS_E_INVALID, "baum-welch on pairs: negative max_iterations");
  std::vector<double> pairLl((size_t)std::max<int64_t>(n_pairs, 1));
  std::vector<uint8_t> status((size_t)std::max<int64_t>(n_pairs, 1));
  double counts0[21 + 32], ll0 = 0;
  if (const int rc = dnas::checkCountsArgs(init, band, n_pairs, in_seqs, in_off, out_seqs, out_off, counts0, &ll0, pairLl.data(),
                                           status.data()))
    return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  return pcGuarded([&] {
    PcFit fit;    // sequences, table and scratch go to the GPU once for the whole fit
    if (const int rc = fit.open(device_id, band, init->n_len, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes))
      return rc;
    int32_t seenN = 0;
    const int rc = dnas::baumWelchLoop(
        *init, max_iterations,
        [&](const dnas_mutator_params& cur, double* counts, double* ll) {
          return fit.estep(cur, counts, ll, nullptr, pairLl.data(), nullptr, status.data(), nullptr);
        },
        [&](const dnas_mutator_params& cur, double ll) {
          if (out_trace_params) out_trace_params[seenN] = cur;
          if (out_trace_ll) out_trace_ll[seenN] = ll;
          ++seenN;
        },
        out, out_iterations);
    if (out_n_trace) *out_n_trace = seenN;
    return rc;
  });
}
