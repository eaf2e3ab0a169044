// dnas_pair_profiles: the posteriors of dnas_pair_counts kept per row of the original (include/dnastore_amd.h) on the GPU.  The
// kernel is pcProfilePair of pair_counts_device.h: the two passes of pair_counts_kernel with the profile policy, which stores a
// lane's accumulators at the end of every stripe instead of summing the lanes at the end of the pair.  The policy forms no T_k
// emission, so pass 1 parks S and D only: two planes of scratch per wave where the counts kernel has P + 2.  Scratch plan, launch
// plan, chunk loop, buffers and the fan-out over devices are those of dnas_pair_counts (pair_counts_plan.hpp).
//
// A launch writes the blocks of its chunk's pairs back to back into one device buffer, which the host copies out and walks in
// pair order before the next launch overwrites it: the caller's copy (out_pair_profiles) and the aggregate are formed from it, so
// a call without out_pair_profiles never holds more than a chunk's blocks.  A chunk is cut so that they stay within
// kPpChunkBytes.  With several devices the pair order is only met again when all of them are done, so every block is gathered
// under the caller's index first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/paircounts.hpp"
#include "pair_counts_device.h"
#include "pair_counts_plan.hpp"

namespace {

constexpr size_t kPpChunkBytes = (size_t)1 << 31;       // the profile blocks of one launch at most

// Dynamic LDS, per wave: 16 substitution scores, 2 ldsCols boundary doubles, the [4][64] match counters.  blockAt[q]: the doubles
// in front of the block of the q-th pair that is run; a launch's blocks start at `blocks`.
template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void pair_profile_kernel(
    PaScores sc, const double* __restrict__ subTable, const double* __restrict__ lseTab, int band, int ldsCols, int64_t first,
    int64_t count, const int64_t* __restrict__ runIdx, const int8_t* __restrict__ inSeqs, const int64_t* __restrict__ inOff,
    const int8_t* __restrict__ outSeqs, const int64_t* __restrict__ outOff, const uint8_t* __restrict__ outRev, double* bndScratch,
    int64_t bndStride, double* parkScratch, int64_t parkStride, int64_t maxWaves, const int64_t* __restrict__ blockAt,
    double* __restrict__ blocks, double* __restrict__ z) {
  extern __shared__ double lds[];
  // (a wave beyond maxWaves fills its LDS slice too before it leaves: the block's LDS has the slice, and bndMem is only formed)
  const PaWave w = paWaveBegin(lds, (size_t)(16 + 2 * ldsCols + kPpMatchSlots), subTable, bndScratch, bndStride);
  const int64_t nWaves = w.nWaves < maxWaves ? w.nWaves : maxWaves;
  if (w.wave >= nWaves) return;                                // the arena holds no scratch for this wave (no barrier follows)
  double* const scr = parkScratch + w.wave * parkStride;

  for (int64_t q = w.wave; q < count; q += nWaves) {
    const int64_t g = runIdx[first + q];
    const PaItem it{inSeqs + inOff[g], outSeqs + outOff[g], (int)(inOff[g + 1] - inOff[g]), (int)(outOff[g + 1] - outOff[g]),
                    outRev != nullptr && outRev[g] != 0};
    pcProfilePair<KP>(sc, lseTab, w.lds, ldsCols, w.bndMem, scr, w.lane, band, it, blocks + (blockAt[first + q] - blockAt[first]), z + g);
  }
}

// One device's share of a call.
class PpDevice {
 public:
  // The arguments were checked.
  int open(int device, int band, int P, int64_t n, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs,
           const int64_t* out_off, const uint8_t* out_rev, size_t arena_bytes) {
    const size_t W = (size_t)(DNAS_PROFILE_DUP + P);
    int64_t maxI = 0;
    for (int64_t i = 0; i < n; ++i) maxI = std::max(maxI, in_off[i + 1] - in_off[i]);
    const int64_t chunkCap = (int64_t)std::min<size_t>(kPpChunkBytes / (W * (size_t)(maxI + 1) * sizeof(double)), (size_t)1 << 22);
    const auto occupancy = [&](size_t ldsBytes, int* perCu) {
      return paDispatchKP(P, [&](auto kp) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCu, &pair_profile_kernel<decltype(kp)::value>, 64 * kPaWavesPerBlock, ldsBytes);
      });
    };
    if (const int rc = w_.open(device, band, P, n, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes, /* S and D */ 2, kPpLdsCols,
                               16 + kPpMatchSlots, chunkCap, occupancy))
      return rc;
    rows_.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) rows_[(size_t)i] = in_off[i + 1] - in_off[i] + 1;
    const int64_t nRun = (int64_t)w_.run.size();
    if (nRun == 0) return DNAS_OK;
    blockAt_.assign(1, 0);
    for (int64_t i : w_.run) blockAt_.push_back(blockAt_.back() + (int64_t)W * rows_[(size_t)i]);
    int64_t most = 0;
    for (int64_t first = 0; first < nRun; first += w_.plan.chunkItems)
      most = std::max(most, blockAt_[(size_t)std::min(first + w_.plan.chunkItems, nRun)] - blockAt_[(size_t)first]);
    host_.resize((size_t)most);
    z_.resize((size_t)n);
    int rc;
    if ((rc = paUpload(w_.bufs, &dBlockAt_, blockAt_.data(), blockAt_.size()))) return rc;
    if ((rc = paAlloc(w_.bufs, &dBlocks_, (size_t)most))) return rc;
    return paAlloc(w_.bufs, &dZ_, (size_t)n);
  }

  // pairLl[n], status[n] of this device's pairs; sink(i, block) is called once per pair in pair order, block the pair's
  // (6 + P) x (I + 1) doubles, valid during the call, or null for a pair that is not OK.
  template <class Sink>
  int run(const dnas::PairScores& hs, double* pairLl, uint8_t* status, dnas_counts_stats* stats, Sink&& sink) {
    *stats = dnas_counts_stats{};
    const int64_t nRun = (int64_t)w_.run.size();
    const double nan = std::numeric_limits<double>::quiet_NaN(), neg = -std::numeric_limits<double>::infinity();
    int64_t next = 0;                                            // the pairs before it were handed to the sink
    const auto skipTo = [&](int64_t g) {                         // the pairs that are not run
      for (; next < g; ++next) {
        pairLl[next] = nan;
        status[next] = DNAS_COUNTS_TOO_LARGE;
        sink(next, (const double*)nullptr);
      }
    };
    if (nRun > 0) {
      DNAS_HIP_TRY(hipSetDevice(w_.device));
      const PaScores sc = PaScores::from(hs);
      DNAS_HIP_TRY(hipMemcpy(w_.dSub, hs.sub, 16 * sizeof(double), hipMemcpyHostToDevice));
      const PaLaunchPlan& plan = w_.plan;
      const auto launch = [&](int64_t first, int64_t count) {
        paDispatchKP(w_.P, [&](auto kp) {
          hipLaunchKernelGGL(pair_profile_kernel<decltype(kp)::value>, dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock),
                             plan.ldsBytes, w_.bufs.stream, sc, w_.dSub, w_.dTab, w_.band, plan.ldsCols, first, count, w_.dRun, w_.dIn,
                             w_.dInOff, w_.dOut, w_.dOutOff, w_.dRev, w_.dBnd, plan.bndStride, w_.dPark, w_.parkStride, w_.waves,
                             dBlockAt_, dBlocks_, dZ_);
        });
      };
      const auto collect = [&](int64_t first, int64_t count) {
        const int64_t at = blockAt_[(size_t)first], g0 = w_.run[(size_t)first], g1 = w_.run[(size_t)(first + count - 1)];
        const size_t bytes = (size_t)(blockAt_[(size_t)(first + count)] - at) * sizeof(double);
        hipError_t e = hipMemcpyAsync(host_.data(), dBlocks_, bytes, hipMemcpyDeviceToHost, w_.bufs.stream);
        if (e == hipSuccess)
          e = hipMemcpyAsync(z_.data() + g0, dZ_ + g0, (size_t)(g1 - g0 + 1) * sizeof(double), hipMemcpyDeviceToHost, w_.bufs.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(w_.bufs.stream);
        if (e != hipSuccess) return e;
        for (int64_t q = first; q < first + count; ++q) {
          const int64_t g = w_.run[(size_t)q];
          skipTo(g);
          const bool ok = z_[(size_t)g] > neg;
          pairLl[g] = z_[(size_t)g];
          status[g] = ok ? DNAS_COUNTS_OK : DNAS_COUNTS_NO_PATH;
          sink(g, ok ? host_.data() + (blockAt_[(size_t)q] - at) : (const double*)nullptr);
          next = g + 1;
        }
        return hipSuccess;
      };
      PcChunkStats cs;
      if (const int rc = paRunChunks(w_.bufs, nRun, plan.chunkItems, launch, [](int64_t, int64_t) {}, collect, &cs)) return rc;
      stats->kernel_ms = cs.score_ms;
      stats->chunks = cs.chunks;
    }
    skipTo(w_.n);
    stats->cells = w_.cells;
    stats->scratch_bytes = w_.scratchBytes;
    stats->pairs_too_large = w_.tooLarge;
    stats->waves = nRun > 0 ? w_.waves : 0;
    return DNAS_OK;
  }

 private:
  PcWorkspace w_;
  std::vector<int64_t> rows_, blockAt_;
  std::vector<double> host_, z_;
  int64_t* dBlockAt_ = nullptr;
  double *dBlocks_ = nullptr, *dZ_ = nullptr;
};

// block (null: zeros) to the place of pair i in the caller's layout.
void ppPlace(double* all, size_t W, const int64_t* in_off, int64_t i, const double* block) {
  const size_t len = W * (size_t)(in_off[i + 1] - in_off[i] + 1);
  double* const dst = all + W * (size_t)(in_off[i] + i);
  if (block) std::copy(block, block + len, dst);
  else std::fill(dst, dst + len, 0.);
}

}  // namespace

extern "C" int dnas_pair_profiles(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                                  const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                                  int device_id, size_t arena_bytes, int32_t anchor, int64_t n_positions, double* out_profile,
                                  int64_t* out_coverage, double* out_pair_profiles, double* out_pair_ll, uint8_t* out_status,
                                  dnas_counts_stats* out_stats) {
  if (const int rc = dnas::checkProfileArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, anchor, n_positions, out_profile,
                                            out_coverage, out_pair_ll, out_status))
    return rc;
  if (out_stats) *out_stats = dnas_counts_stats{};
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  return pcGuarded([&] {
    const int P = params->n_len;
    const size_t W = (size_t)(DNAS_PROFILE_DUP + P);
    const int64_t n = n_pairs;
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    dnas::ProfileSum sum(P, anchor, n_positions, out_profile, out_coverage);
    std::vector<int> devices;
    std::vector<std::vector<int64_t>> shard;
    pcDeal(device_id, band, n, in_off, out_off, &devices, &shard);
    dnas_counts_stats total{};
    if (devices.size() == 1) {
      PpDevice dev;
      if (const int rc = dev.open(devices[0], band, P, n, in_seqs, in_off, out_seqs, out_off, out_rev, arena_bytes)) return rc;
      const int rc = dev.run(hs, out_pair_ll, out_status, &total, [&](int64_t i, const double* block) {
        if (out_pair_profiles) ppPlace(out_pair_profiles, W, in_off, i, block);
        if (block) sum.add(in_seqs + in_off[i], in_off[i + 1] - in_off[i], block);
      });
      if (rc != DNAS_OK) return rc;
    } else {
      std::vector<double> own;
      double* all = out_pair_profiles;
      if (!all) {
        own.resize(W * (size_t)(in_off[n] + n));
        all = own.data();
      }
      std::vector<dnas_counts_stats> stats(devices.size());
      const int rc = dnas::forEachDevice(devices, [&](size_t k) {
        const std::vector<int64_t>& mine = shard[k];
        const size_t m = mine.size();
        std::vector<int8_t> in, outs;
        std::vector<int64_t> inOff, outOff;
        dnas::gatherShard(mine, in_seqs, in_off, &in, &inOff);
        dnas::gatherShard(mine, out_seqs, out_off, &outs, &outOff);
        std::vector<uint8_t> rev(m + 1), st(m + 1);
        std::vector<double> ll(m + 1);
        if (out_rev) for (size_t j = 0; j < m; ++j) rev[j] = out_rev[mine[j]];
        PpDevice dev;
        if (const int rc = dev.open(devices[k], band, P, (int64_t)m, in.data(), inOff.data(), outs.data(), outOff.data(),
                                    out_rev ? rev.data() : nullptr, arena_bytes))
          return rc;
        if (const int rc = dev.run(hs, ll.data(), st.data(), &stats[k],
                                   [&](int64_t j, const double* block) { ppPlace(all, W, in_off, mine[(size_t)j], block); }))
          return rc;
        for (size_t j = 0; j < m; ++j) {
          out_pair_ll[mine[j]] = ll[j];
          out_status[mine[j]] = st[j];
        }
        return DNAS_OK;
      });
      if (rc != DNAS_OK) return rc;
      for (int64_t i = 0; i < n; ++i)
        if (out_status[i] == DNAS_COUNTS_OK) sum.add(in_seqs + in_off[i], in_off[i + 1] - in_off[i], all + W * (size_t)(in_off[i] + i));
      for (const dnas_counts_stats& s : stats) {
        total.kernel_ms = std::max(total.kernel_ms, s.kernel_ms);
        total.cells += s.cells;
        total.chunks += s.chunks;
        total.scratch_bytes += s.scratch_bytes;
        total.pairs_too_large += s.pairs_too_large;
        total.waves += s.waves;
      }
    }
    if (out_stats) *out_stats = total;
    return DNAS_OK;
  });
}
