// What the two-pass kernels over a pair's whole band (pair_counts_kernel, pair_profile_kernel) share on the host: the pairs and the
// table on the device, and the scratch plan -- the grid is cut until the parked forward cells of all its waves fit the arena, a
// pair whose scratch alone exceeds the arena is left out as DNAS_COUNTS_TOO_LARGE.  The kernels differ in what a wave keeps in
// LDS beside the boundary row, and so in the columns that row may have there.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "devices.hpp"
#include "host/lsetable.hpp"
#include "pair_align_device.h"

namespace {

struct PcWorkspace {
  int device = 0, band = 0, P = 0;
  int64_t n = 0, cells = 0, tooLarge = 0, waves = 0, parkStride = 0, scratchBytes = 0, maxI = 0;
  std::vector<uint8_t> status;       // per pair: OK or TOO_LARGE
  std::vector<int64_t> run;          // the pairs that are run, ascending
  PaLaunchPlan plan;
  PaBuffers bufs;
  int8_t *dIn = nullptr, *dOut = nullptr;
  int64_t *dInOff = nullptr, *dOutOff = nullptr, *dRun = nullptr;
  uint8_t* dRev = nullptr;
  double *dSub = nullptr, *dTab = nullptr, *dBnd = nullptr, *dPark = nullptr;

  // The arguments were checked.  planes: the values pass 1 parks per cell; ldsColsMax: the columns of a boundary row in LDS at
  // most; ldsOther: the doubles a wave keeps in LDS besides that row; chunkCap: pairs per launch at most; occupancy(ldsBytes,
  // &perCu) -> hipError_t asks the runtime how many work-groups of the kernel fit a CU.  Nothing is allocated when no pair is run.
  template <class Occupancy>
  int open(int device_, int band_, int P_, int64_t n_, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs,
           const int64_t* out_off, const uint8_t* out_rev, size_t arena_bytes, size_t planes, int ldsColsMax, int ldsOther,
           int64_t chunkCap, Occupancy&& occupancy) {
    device = device_;
    band = band_;
    P = P_;
    n = n_;
    status.assign((size_t)std::max<int64_t>(n, 1), DNAS_COUNTS_OK);
    if (n == 0) return DNAS_OK;
    DNAS_HIP_TRY(hipSetDevice(device));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);

    // the scratch a pair asks of the wave that takes it, and the arena
    std::vector<size_t> words((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      words[(size_t)i] = PaGeom((int)(in_off[i + 1] - in_off[i]), (int)(out_off[i + 1] - out_off[i]), band).words();
    size_t arena = arena_bytes;
    if (!arena_bytes) {
      size_t freeB = 0, totalB = 0;
      DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
      arena = freeB / 2;                                         // half of what is free: the aligner's rule
    }
    size_t maxWords = 0;
    int maxO = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (words[(size_t)i] * planes * sizeof(double) > arena) {
        status[(size_t)i] = DNAS_COUNTS_TOO_LARGE;
        ++tooLarge;
        continue;
      }
      run.push_back(i);
      maxWords = std::max(maxWords, words[(size_t)i]);
      maxI = std::max(maxI, in_off[i + 1] - in_off[i]);
      maxO = std::max(maxO, (int)(out_off[i + 1] - out_off[i]));
    }
    const int64_t nRun = (int64_t)run.size();
    if (nRun == 0) return DNAS_OK;
    PaCellMemo memo(maxI, maxO, band);
    for (int64_t i : run) cells += memo.cells(in_off[i + 1] - in_off[i], out_off[i + 1] - out_off[i]);

    // the grid: what the shared plan gives, cut until every wave's scratch fits the arena
    plan.chunkItems = std::max<int64_t>(1, chunkCap);
    if (const char* s = getenv("DNAS_COUNTS_CHUNK")) plan.chunkItems = std::max<int64_t>(1, std::min<int64_t>(plan.chunkItems, atoll(s)));
    plan.chunkItems = std::max<int64_t>(1, std::min(plan.chunkItems, nRun));
    plan.ldsCols = std::min(maxO + 1, ldsColsMax);
    plan.ldsBytes = (size_t)kPaWavesPerBlock * (size_t)(2 * plan.ldsCols + ldsOther) * sizeof(double);
    int perCu = 1;
    DNAS_HIP_TRY(occupancy(plan.ldsBytes, &perCu));
    plan.cut(cus, std::max(perCu, 1), maxO, plan.chunkItems);
    plan.bndStride = maxO + 1 > ldsColsMax ? 2 * ((int64_t)maxO + 1) : 0;   // these kernels' boundary row leaves LDS earlier
    parkStride = (int64_t)(maxWords * planes);
    const size_t perWave = (size_t)parkStride * sizeof(double);
    waves = std::min<int64_t>((int64_t)plan.maxBlocks * kPaWavesPerBlock, (int64_t)(arena / perWave));
    waves = std::max<int64_t>(1, std::min(waves, plan.chunkItems));
    plan.maxBlocks = (int)((waves + kPaWavesPerBlock - 1) / kPaWavesPerBlock);
    scratchBytes = (int64_t)((size_t)waves * perWave);

    int rc;
    if ((rc = bufs.open())) return rc;
    const std::vector<double>& tab = dnas::lseTable();
    if ((rc = paUpload(bufs, &dIn, in_seqs, (size_t)in_off[n]))) return rc;
    if ((rc = paUpload(bufs, &dOut, out_seqs, (size_t)out_off[n]))) return rc;
    if ((rc = paUpload(bufs, &dInOff, in_off, (size_t)n + 1))) return rc;
    if ((rc = paUpload(bufs, &dOutOff, out_off, (size_t)n + 1))) return rc;
    if (out_rev && (rc = paUpload(bufs, &dRev, out_rev, (size_t)n))) return rc;
    if ((rc = paUpload(bufs, &dRun, run.data(), run.size()))) return rc;
    if ((rc = paUpload(bufs, &dTab, tab.data(), tab.size()))) return rc;
    if ((rc = paAlloc(bufs, &dSub, (size_t)16))) return rc;
    if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;
    if ((rc = paAlloc(bufs, &dPark, (size_t)waves * (size_t)parkStride))) return rc;
    return DNAS_OK;
  }
};

struct PcChunkStats {
  double score_ms = 0, fold_ms = 0;
  int64_t chunks = 0;
};

// The fan-out of a call over the devices as dnas_align_pairs deals the pairs: shard[k] holds the caller's indices of device k's
// pairs.  One device, or no pairs: devices and shard have one entry and shard[0] is empty (the device takes the call as it is).
inline void pcDeal(int device_id, int band, int64_t n, const int64_t* in_off, const int64_t* out_off, std::vector<int>* devices,
                   std::vector<std::vector<int64_t>>* shard) {
  *devices = dnas::pickDevices(device_id);
  if (devices->size() == 1 || n == 0) {
    devices->resize(1);
    shard->assign(1, {});
    return;
  }
  std::vector<int64_t> cost((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
    const dnas::PairBand bd(I, O, band);
    cost[(size_t)i] = (I + 1) * std::min(O + 1, bd.hi - bd.lo + 1);
  }
  *shard = dnas::snakeDeal(cost, devices->size());
}

template <class F>
int pcGuarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

}  // namespace
