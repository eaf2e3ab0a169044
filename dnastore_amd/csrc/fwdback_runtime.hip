// Host side of the forward-backward path: dnas_fwdback_estep (expectedCounts,
// reference src/fwdback.cpp:190-209) and dnas_baum_welch (baumWelchParams,
// fwdback.cpp:211-230 with MutatorCounts::mlParams / logPrior, mutator.cpp:167-214).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "device_buffer.hpp"
#include "devices.hpp"
#include "errors.hpp"
#include "fwdback_device.h"
#include "host/baumwelch.hpp"
#include "host/lsetable.hpp"
#include "host/model.hpp"

extern "C" __global__ void fwdback_estep_kernel(FbArgs, const int8_t*, const int64_t*, const int8_t*, const int64_t*,
                                                const int32_t*, const int64_t*, const int32_t*, const int64_t*,
                                                const double*, double*, double*, double*, double*, int64_t, int, int64_t, const int64_t*);
#define FB_ONCHIP_ARGS FbArgs, const int8_t*, const int64_t*, const int8_t*, const int64_t*, const int32_t*, const int64_t*, const int32_t*, \
                       const int64_t*, const double*, const int64_t*, int64_t, double*, double*, int, unsigned long long*, double*, int
// <lanes per pair>x<cells per row served>; p6: up to 6 duplication lengths (the CLI's default model) in registers
extern "C" __global__ void fwdback_onchip8x16_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip16x16_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip16x32_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip32x32_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip8x16p6_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip16x16p6_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip16x32p6_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_onchip32x32p6_kernel(FB_ONCHIP_ARGS);
extern "C" __global__ void fwdback_reduce_kernel(const double*, const double*, int64_t, int, double*);
extern "C" __global__ void fwdback_validate_kernel(int64_t, const int8_t*, const int64_t*, const int8_t*, const int64_t*, const int32_t*,
                                                   const int64_t*, const int32_t*, const int64_t*, unsigned*);
extern "C" __global__ void fwdback_census_kernel(int64_t, int, const int64_t*, const int64_t*, const int32_t*, const int64_t*, const int32_t*,
                                                 const int64_t*, int64_t*);

using dnas::DevBuf;

#ifndef DNAS_FB_WAVES_PER_CU
#define DNAS_FB_WAVES_PER_CU 12     // 4 SIMDs x DNAS_FB_MIN_WAVES of fwdback_onchip.hip
#endif

namespace {

using dnas::lseTable;     // the reference's table of log(1 + exp(-x)), host/lsetable.hpp

bool isTransition(int x, int y) { return x != y && (x & 1) == (y & 1); }

constexpr int kFbLanes[4] = {8, 16, 16, 32}, kFbRowCells[4] = {16, 16, 32, 32};   // the four wavefront kernels

}  // namespace

// ---- the persistent handle ---------------------------------------------------------------------------
// What is per device (the log-sum-exp table, a stream), what is per database (the pairs, their envelope widths per
// guide mode, the result buffers) and what is per E-step (the scores) are uploaded / computed once each; an EM run
// calls dnas_fb_estep up to 100 times on the same handle.
struct dnas_fb {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf<double> dTab;
  // database
  int64_t nPairs = 0;
  int P = -1;                    // pLen size the per-pair buffers are sized for
  int maxInLen = 0;
  std::vector<int64_t> inOff, outOff;                        // host copies of the sequence offsets (routing by length, statistics)
  DevBuf<int8_t> dIn, dOut;
  DevBuf<int64_t> dInOff, dOutOff, dCiOff, dCoOff;
  DevBuf<int32_t> dCi, dCo;
  DevBuf<double> dCounts, dLL, dPartial;
  DevBuf<unsigned long long> dLseOps;
  // per guide mode (0: the envelope is maxDistance = P wide, 1: strict) and P: which kernel takes which pair.  onchip[q]: the
  // wavefront kernels, kFbLanes[q] lanes per pair for envelope rows of up to kFbRowCells[q] cells; the narrow ones (q = 0, 2) take
  // the pairs whose rows meet hi(ip) - lo(ip + W) < W (fwdback_onchip.hip), i.e. every alignment that runs down a diagonal
  struct Route { int P = -1; int maxInOnchip[4] = {0, 0, 0, 0}, maxSteps[4] = {1, 1, 1, 1}; std::vector<int64_t> onchip[4], streaming; std::vector<int64_t> cells; std::vector<int> width;
                 DevBuf<int64_t> dOnchip[4], dStreaming; };
  Route route[2];
  // streaming kernel arenas: replaced by exactly what a batch needs when that is more than they hold
  DevBuf<double> dFwd, dRows;
  DevBuf<double> dScratch;           // on-chip kernels: checkpoints and duplication lanes of the pair slots
  int cus = 256;
  dnas_fb_stats stats{};
  // device_id = -1: one ordinary handle per device, each holding its shard of the pairs; of the members above only nPairs (the
  // whole database) and stats (summed over the devices) are used then
  std::vector<dnas_fb*> sub;
  std::vector<int> devices;                  // per sub-handle: its device
  std::vector<std::vector<int64_t>> shard;   // per sub-handle: the caller's indices of its pairs, ascending
};

namespace {

// n elements of src in a device buffer of their own (one element at least)
template <class T>
int fbUpload(DevBuf<T>& dst, const T* src, size_t n) {
  DNAS_HIP_TRY(dst.assign(n));
  if (n) DNAS_HIP_TRY(hipMemcpy(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
  return DNAS_OK;
}

void fbFreeDatabase(dnas_fb* h) {
  h->dIn.reset(); h->dOut.reset(); h->dInOff.reset(); h->dOutOff.reset(); h->dCiOff.reset(); h->dCoOff.reset();
  h->dCi.reset(); h->dCo.reset(); h->dCounts.reset(); h->dLL.reset(); h->dPartial.reset();
  for (auto& r : h->route) r = dnas_fb::Route{};
  h->nPairs = 0; h->P = -1;
}

// The host checks of a database (the kernels trust the offsets; bases and guide columns are checked on the GPU), naming pairs by
// the caller's index.
int checkOffsets(int64_t n_pairs, const int64_t* in_off, const int64_t* out_off, const int64_t* cm_in_off, const int64_t* cm_out_off,
                 int* maxIn) {
  if (in_off[0] != 0 || out_off[0] != 0 || cm_in_off[0] != 0 || cm_out_off[0] != 0) return dnas::fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t inLen = in_off[i + 1] - in_off[i], outLen = out_off[i + 1] - out_off[i];
    if (inLen < 0 || outLen < 0 || cm_in_off[i + 1] - cm_in_off[i] != inLen + 1 || cm_out_off[i + 1] - cm_out_off[i] != outLen + 1)
      return dnas::fail(DNAS_E_INVALID, "pair " + std::to_string(i) + ": inconsistent offsets");
    if (inLen > 30000 || outLen > 30000) return dnas::fail(DNAS_E_UNSUPPORTED, "pair " + std::to_string(i) + ": sequences longer than 30000");
    *maxIn = std::max<int>(*maxIn, (int)inLen);
  }
  return DNAS_OK;
}

// ---- device_id = -1: the pairs dealt over one handle per device -----------------------------------------------------------
// Pairs are independent (the reference sums counts and log-likelihood over them, fwdback.cpp:197-207): every sub-handle runs the
// E-step on its shard, and the host adds the shards' results in device order.

// every sub-handle without a database, as fbFreeDatabase leaves a one-device handle
void fbFreeShards(dnas_fb* h) {
  for (dnas_fb* s : h->sub) {
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    fbFreeDatabase(s);
  }
  for (auto& sh : h->shard) sh.clear();
  h->nPairs = 0;
}

int fbCreateAll(dnas_fb** out) {
  const std::vector<int> devices = dnas::pickDevices(-1);
  dnas_fb* h = new dnas_fb();
  for (int d : devices) {
    dnas_fb* s = nullptr;
    const int rc = dnas_fb_create(d, &s);
    if (rc != DNAS_OK) { dnas_fb_destroy(h); return rc; }
    h->sub.push_back(s);
  }
  h->shard.resize(devices.size());
  h->devices = devices;
  *out = h;
  return DNAS_OK;
}

int fbLoadAll(dnas_fb* h, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off,
              const int32_t* cm_in, const int64_t* cm_in_off, const int32_t* cm_out, const int64_t* cm_out_off) {
  fbFreeShards(h);
  if (n_pairs == 0) return DNAS_OK;
  int maxIn = 0;
  if (const int rc = checkOffsets(n_pairs, in_off, out_off, cm_in_off, cm_out_off, &maxIn)) return rc;
  std::vector<int64_t> cost((size_t)n_pairs);
  for (int64_t i = 0; i < n_pairs; ++i) cost[(size_t)i] = (in_off[i + 1] - in_off[i]) + (out_off[i + 1] - out_off[i]);
  h->shard = dnas::snakeDeal(cost, h->sub.size());
  const int rc = dnas::forEachDevice(h->devices, [&](size_t k) {
    const std::vector<int64_t>& mine = h->shard[k];
    if ((int64_t)mine.size() == n_pairs)       // one device: the caller's arrays as they are
      return dnas_fb_load_pairs(h->sub[k], n_pairs, in_seqs, in_off, out_seqs, out_off, cm_in, cm_in_off, cm_out, cm_out_off);
    std::vector<int8_t> in, outs;
    std::vector<int32_t> ci, co;
    std::vector<int64_t> inOff, outOff, ciOff, coOff;
    dnas::gatherShard(mine, in_seqs, in_off, &in, &inOff);
    dnas::gatherShard(mine, out_seqs, out_off, &outs, &outOff);
    dnas::gatherShard(mine, cm_in, cm_in_off, &ci, &ciOff);
    dnas::gatherShard(mine, cm_out, cm_out_off, &co, &coOff);
    return dnas_fb_load_pairs(h->sub[k], (int64_t)mine.size(), in.data(), inOff.data(), outs.data(), outOff.data(), ci.data(), ciOff.data(),
                              co.data(), coOff.data());
  });
  if (rc != DNAS_OK) { fbFreeShards(h); return rc; }
  h->nPairs = n_pairs;
  return DNAS_OK;
}

int fbEstepAll(dnas_fb* h, const dnas_mutator_params* p, int strict, double* out_counts, double* out_ll, double* out_pair_ll) {
  const size_t W = h->sub.size(), nc = 21 + (size_t)p->n_len;
  std::vector<std::vector<double>> counts(W, std::vector<double>(nc)), per(W);
  std::vector<double> lls(W);
  std::vector<dnas_fb_stats> stats(W);
  const int rc = dnas::forEachDevice(h->devices, [&](size_t k) {
    if (out_pair_ll) per[k].resize(h->shard[k].size());
    int r = dnas_fb_estep(h->sub[k], p, strict, counts[k].data(), &lls[k], out_pair_ll ? per[k].data() : nullptr);
    if (r == DNAS_OK) r = dnas_fb_last_stats(h->sub[k], &stats[k]);
    return r;
  });
  if (rc != DNAS_OK) return rc;
  // the reduction, in device order (with one device: that device's values as they are)
  for (size_t j = 0; j < nc; ++j) out_counts[j] = counts[0][j];
  *out_ll = lls[0];
  h->stats = stats[0];
  for (size_t k = 1; k < W; ++k) {
    for (size_t j = 0; j < nc; ++j) out_counts[j] += counts[k][j];
    *out_ll += lls[k];
    dnas_fb_stats& s = h->stats;
    s.kernel_ms = std::max(s.kernel_ms, stats[k].kernel_ms);
    s.pairs_onchip += stats[k].pairs_onchip;
    s.pairs_streaming += stats[k].pairs_streaming;
    s.pairs_narrow += stats[k].pairs_narrow;
    s.lse_ops += stats[k].lse_ops;
    s.out_nt += stats[k].out_nt;
  }
  if (out_pair_ll)
    for (size_t k = 0; k < W; ++k)
      for (size_t j = 0; j < h->shard[k].size(); ++j) out_pair_ll[h->shard[k][j]] = per[k][j];
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_fb_create(int device_id, dnas_fb** out) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "dnas_fb_create: null argument");
  *out = nullptr;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  if (device_id == -1) return fbCreateAll(out);
  DNAS_HIP_TRY(hipSetDevice(device_id));
  std::unique_ptr<dnas_fb, void (*)(dnas_fb*)> made(new dnas_fb(), dnas_fb_destroy);     // destroyed unless it is handed out
  dnas_fb* const h = made.get();
  h->device = device_id;
  DNAS_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  DNAS_HIP_TRY(hipEventCreate(&h->ev0));
  DNAS_HIP_TRY(hipEventCreate(&h->ev1));
  const std::vector<double>& tab = lseTable();
  DNAS_HIP_TRY(h->dTab.assign(tab.size()));
  DNAS_HIP_TRY(hipMemcpy(h->dTab.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(h->dLseOps.assign(1));
  (void)hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device_id);
  *out = made.release();
  return DNAS_OK;
}

extern "C" void dnas_fb_destroy(dnas_fb* h) {
  if (!h) return;
  if (!h->sub.empty()) {
    for (dnas_fb* s : h->sub) dnas_fb_destroy(s);
    delete h;
    return;
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;                      // the device memory: every owner frees its own, this device current
}

extern "C" int dnas_fb_load_pairs(dnas_fb* h, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off, const int8_t* out_seqs,
                                  const int64_t* out_off, const int32_t* cm_in, const int64_t* cm_in_off, const int32_t* cm_out,
                                  const int64_t* cm_out_off) {
  if (!h || n_pairs < 0) return dnas::fail(DNAS_E_INVALID, "dnas_fb_load_pairs: bad argument");
  if (n_pairs > 0 && (!in_seqs || !in_off || !out_seqs || !out_off || !cm_in || !cm_in_off || !cm_out || !cm_out_off))
    return dnas::fail(DNAS_E_INVALID, "dnas_fb_load_pairs: null argument");
  if (!h->sub.empty()) return fbLoadAll(h, n_pairs, in_seqs, in_off, out_seqs, out_off, cm_in, cm_in_off, cm_out, cm_out_off);
  DNAS_HIP_TRY(hipSetDevice(h->device));
  DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
  fbFreeDatabase(h);
  if (n_pairs == 0) return DNAS_OK;
  // ---- validate (the kernels trust these): the offsets here, every base and guide column on the GPU once they are there
  int maxIn = 0;
  if (const int rc = checkOffsets(n_pairs, in_off, out_off, cm_in_off, cm_out_off, &maxIn)) return rc;
  struct Unload {                 // a database that did not load whole is no database
    dnas_fb* h;
    ~Unload() { if (h) fbFreeDatabase(h); }
  } unload{h};
  const size_t nIn = (size_t)in_off[n_pairs], nOut = (size_t)out_off[n_pairs];
  const size_t nCi = (size_t)cm_in_off[n_pairs], nCo = (size_t)cm_out_off[n_pairs];
  int rc;
  if ((rc = fbUpload(h->dIn, in_seqs, nIn)) || (rc = fbUpload(h->dOut, out_seqs, nOut)) ||
      (rc = fbUpload(h->dInOff, in_off, (size_t)n_pairs + 1)) || (rc = fbUpload(h->dOutOff, out_off, (size_t)n_pairs + 1)) ||
      (rc = fbUpload(h->dCi, cm_in, nCi)) || (rc = fbUpload(h->dCo, cm_out, nCo)) ||
      (rc = fbUpload(h->dCiOff, cm_in_off, (size_t)n_pairs + 1)) || (rc = fbUpload(h->dCoOff, cm_out_off, (size_t)n_pairs + 1)))
    return rc;
  DNAS_HIP_TRY(h->dLL.assign((size_t)n_pairs));
  {
    // every base in 0..3, every guide column array non-decreasing: one thread per pair (h->dLseOps doubles as the flag word)
    DNAS_HIP_TRY(hipMemsetAsync(h->dLseOps.get(), 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(fwdback_validate_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, h->stream, n_pairs, h->dIn.get(), h->dInOff.get(), h->dOut.get(),
                       h->dOutOff.get(), h->dCi.get(), h->dCiOff.get(), h->dCo.get(), h->dCoOff.get(), (unsigned*)h->dLseOps.get());
    DNAS_HIP_TRY(hipGetLastError());
    unsigned flags = 0;
    DNAS_HIP_TRY(hipMemcpyAsync(&flags, h->dLseOps.get(), sizeof flags, hipMemcpyDeviceToHost, h->stream));
    DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
    if (flags & 1u) return dnas::fail(DNAS_E_BAD_BASE, "bad base");
    if (flags & 2u) return dnas::fail(DNAS_E_INVALID, "cm_in / cm_out must be non-decreasing");
  }
  unload.h = nullptr;
  h->nPairs = n_pairs;
  h->maxInLen = maxIn;
  h->inOff.assign(in_off, in_off + n_pairs + 1);
  h->outOff.assign(out_off, out_off + n_pairs + 1);
  return DNAS_OK;
}

extern "C" int dnas_fb_estep(dnas_fb* h, const dnas_mutator_params* p, int strict, double* out_counts, double* out_ll,
                             double* out_pair_ll) {
  if (!h || !p || !out_counts || !out_ll) return dnas::fail(DNAS_E_INVALID, "dnas_fb_estep: null argument");
  const int P = p->n_len, nc = 21 + P;
  if (P < 0 || P > kFbMaxLen) return dnas::fail(DNAS_E_UNSUPPORTED, "pLen longer than 32 entries");
  for (int k = 0; k < nc; ++k) out_counts[k] = 0;
  *out_ll = 0;
  h->stats = dnas_fb_stats{};
  const int64_t n_pairs = h->nPairs;
  if (n_pairs == 0) return DNAS_OK;
  if (!h->sub.empty()) return fbEstepAll(h, p, strict, out_counts, out_ll, out_pair_ll);
  DNAS_HIP_TRY(hipSetDevice(h->device));

  // ---- scores (MutatorScores, mutator.cpp:56-75)
  FbArgs a{};
  a.P = P;
  a.maxDistance = strict ? 0 : P;                            // fwdback.cpp:17
  a.delOpen = std::log(p->p_del_open);
  a.tanDup = std::log(p->p_tan_dup);
  a.noGap = std::log(1. - p->p_del_open - p->p_tan_dup);
  a.delExtend = std::log(p->p_del_extend);
  a.delEnd = std::log(1. - p->p_del_extend);
  const double nullScore = std::log(1. / 4.), pMatch = 1. - p->p_transition - p->p_transversion;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      a.sub[i * 4 + j] = (i == j ? std::log(pMatch) : (isTransition(i, j) ? std::log(p->p_transition) : std::log(p->p_transversion / 2))) - nullScore;
  for (int k = 0; k < P; ++k) a.len[k] = std::log(p->p_len[k]);

  // ---- which kernel takes which pair: the on-chip kernels serve envelope rows of up to 16 or 32 cells (16 or 32 lanes per
  // pair) and up to 8 duplication lengths; the census depends on the envelope half-width (P, or 0 with strict guides) and is kept
  dnas_fb::Route& rt = h->route[strict ? 1 : 0];
  if (rt.P != P) {
    for (auto& q : rt.dOnchip) q.reset();
    rt.dStreaming.reset();
    for (auto& list : rt.onchip) list.clear();
    rt.streaming.clear();
    rt.cells.assign((size_t)n_pairs, 1);
    rt.width.assign((size_t)n_pairs, 1);
    const int Dm = a.maxDistance;
    const bool forceStreaming = getenv("DNAS_FB_STREAMING") != nullptr;
    // the on-chip kernels keep a pair's envelope bounds in LDS: a pair whose input is too long for that goes to the streaming
    // kernel like the pairs with wider envelope rows (never fail the call for it)
    int longest[4] = {0, 0, 0, 0};
    for (int q = 0; q < 4; ++q)
      while ((size_t)(kFbWave / kFbLanes[q]) * fbOnchipPairDoubles(kFbLanes[q], longest[q] + 64) * sizeof(double) <= kFbOnchipLdsLimit) longest[q] += 64;
    for (int& v : rt.maxInOnchip) v = 0;
    for (int& v : rt.maxSteps) v = 1;
    const bool noNarrow = getenv("DNAS_FB_NO_NARROW") != nullptr;       // (measurement: the round-3 routing, W = the row capacity)
    // the envelope census of every pair -- cells, widest row, wavefront steps, whether half the lanes do -- on the GPU
    // (fwdback_census_kernel: one thread per pair; on the host this loop took longer than the E-step itself)
    std::vector<int64_t> census((size_t)n_pairs * 3);
    {
      DevBuf<int64_t> dCensus;
      DNAS_HIP_TRY(dCensus.assign(census.size()));
      hipLaunchKernelGGL(fwdback_census_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, h->stream, n_pairs, Dm, h->dInOff.get(), h->dOutOff.get(),
                         h->dCi.get(), h->dCiOff.get(), h->dCo.get(), h->dCoOff.get(), dCensus.get());
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(census.data(), dCensus.get(), census.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      DNAS_HIP_TRY(e);
    }
    for (int64_t i = 0; i < n_pairs; ++i) {
      const int64_t inLen = h->inOff[i + 1] - h->inOff[i];
      const int w = (int)(census[3 * (size_t)i + 1] & 0xffff);
      const bool fits8 = (census[3 * (size_t)i + 1] >> 16) & 1, fits16 = (census[3 * (size_t)i + 1] >> 17) & 1;
      rt.cells[(size_t)i] = census[3 * (size_t)i];
      rt.width[(size_t)i] = w;
      // (every threshold below is restated from its definition in tests/fb_census.py, and tests/test_gpu_fwdback_edges.py puts
      // pairs on both sides of each)
      int kind = w <= 16 ? 1 : (w <= 32 ? 3 : 4);            // the full-width kernel of the row capacity ...
      // ... or half the lanes, when every lane has left its row before its next one comes up (Forward: rows ip, ip + W;
      // Backward walks the same rows the other way: the same inequalities)
      if (kind < 4 && !noNarrow && (kind == 1 ? fits8 : fits16)) --kind;
      // (LO[] / HI[] of the on-chip kernels are int16: checkOffsets has refused every sequence longer than 30 000)
      const bool chip = kind < 4 && P <= 8 && inLen <= longest[kind] && !forceStreaming;
      (chip ? rt.onchip[kind] : rt.streaming).push_back(i);
      if (chip) {
        rt.maxInOnchip[kind] = std::max<int>(rt.maxInOnchip[kind], (int)inLen);
        rt.maxSteps[kind] = std::max<int>(rt.maxSteps[kind], (int)census[3 * (size_t)i + 2]);   // a = ip + op from lo(0) to inLen + hi(inLen)
      }
    }
    // the pairs of a wave walk in step: neighbours in the list should be of a length (longest first)
    // (a stable counting sort by input length: the lengths are at most 30 000, the lists 10^5 .. 10^6 long)
    for (auto& list : rt.onchip) {
      if (list.size() < 2) continue;
      int64_t longestIn = 0;
      for (int64_t x : list) longestIn = std::max(longestIn, h->inOff[x + 1] - h->inOff[x]);
      std::vector<int64_t> start((size_t)longestIn + 2, 0);
      for (int64_t x : list) ++start[(size_t)(longestIn - (h->inOff[x + 1] - h->inOff[x])) + 1];
      for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
      std::vector<int64_t> sorted(list.size());
      for (int64_t x : list) sorted[(size_t)start[(size_t)(longestIn - (h->inOff[x + 1] - h->inOff[x]))]++] = x;
      list.swap(sorted);
    }
    for (int q = 0; q < 4; ++q)
      if (const int rc = fbUpload(rt.dOnchip[q], rt.onchip[q].data(), rt.onchip[q].size())) return rc;
    if (const int rc = fbUpload(rt.dStreaming, rt.streaming.data(), rt.streaming.size())) return rc;
    rt.P = P;
  }
  if (h->P != P) {   // result buffers are sized by the number of counts
    h->dCounts.reset(); h->dPartial.reset();
    DNAS_HIP_TRY(h->dCounts.assign((size_t)n_pairs * nc));
    DNAS_HIP_TRY(h->dPartial.assign((size_t)256 * (nc + 1)));
    h->P = P;
  }
  DNAS_HIP_TRY(hipMemsetAsync(h->dLseOps.get(), 0, sizeof(unsigned long long), h->stream));
  DNAS_HIP_TRY(hipEventRecord(h->ev0, h->stream));

  // ---- on-chip kernels: a wave per work-group (8 pairs of 8 lanes, 4 of 16, or 2 of 32), persistent over the list
  for (int w = 0; w < 4; ++w) {
    if (rt.onchip[w].empty()) continue;
    const int W = kFbLanes[w], RW = kFbRowCells[w], ppg = kFbWave / W;
    const size_t lds = (size_t)ppg * fbOnchipPairDoubles(W, rt.maxInOnchip[w]) * sizeof(double);   // <= kFbOnchipLdsLimit by the routing
    const int64_t nL = (int64_t)rt.onchip[w].size();
    // work-groups (= waves) a CU holds: 160 KB of LDS, and 16 waves of the kernel's 128 registers per lane
    const int perCu = std::max(1, std::min(DNAS_FB_WAVES_PER_CU, (int)((size_t)(160 * 1024) / lds)));
    // every wave keeps the Forward cells of the pairs it works on in HBM (2.7 MB for 256-nt pairs): the waves of a launch are
    // bounded by a scratch budget (16 GB, a quarter of what is free) when the inputs are long
    (void)RW;
    const size_t waveBytes = fbOnchipWaveDoubles(rt.maxSteps[w]) * sizeof(double);
    size_t freeB = 0, totalB = 0;
    DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
    const size_t scratchBytes = h->dScratch.capacity() * sizeof(double);
    const size_t budget = std::max<size_t>(scratchBytes, std::min<size_t>((size_t)16 << 30, (freeB + scratchBytes) / 4));
    const int64_t slotsMax = std::max<int64_t>(1, (int64_t)(budget / waveBytes));
    const unsigned grid = (unsigned)std::min<int64_t>(std::min<int64_t>((nL + ppg - 1) / ppg, (int64_t)h->cus * perCu), slotsMax);
    const size_t need = (size_t)grid * waveBytes;
    if (need > scratchBytes) {
      DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
      DNAS_HIP_TRY(h->dScratch.assign(need / sizeof(double)));
    }
    void (*const kernels[2][4])(FB_ONCHIP_ARGS) = {
        {fwdback_onchip8x16_kernel, fwdback_onchip16x16_kernel, fwdback_onchip16x32_kernel, fwdback_onchip32x32_kernel},
        {fwdback_onchip8x16p6_kernel, fwdback_onchip16x16p6_kernel, fwdback_onchip16x32p6_kernel, fwdback_onchip32x32p6_kernel}};
    auto kernel = kernels[P <= 6 ? 1 : 0][w];
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kFbWave), lds, h->stream, a, h->dIn.get(), h->dInOff.get(),
                       h->dOut.get(), h->dOutOff.get(), h->dCi.get(), h->dCiOff.get(), h->dCo.get(), h->dCoOff.get(), h->dTab.get(), rt.dOnchip[w].get(), nL, h->dCounts.get(), h->dLL.get(), rt.maxInOnchip[w],
                       h->dLseOps.get(), h->dScratch.get(), rt.maxSteps[w]);
    DNAS_HIP_TRY(hipGetLastError());
  }
  // ---- streaming kernel for the rest: the interleaved Forward arena holds cellCap cells for each of B pairs
  if (!rt.streaming.empty()) {
    const size_t W = (size_t)P + 2;
    size_t freeB = 0, totalB = 0;
    DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
    const size_t budget = std::max<size_t>((h->dFwd.capacity() + h->dRows.capacity()) * sizeof(double), std::min<size_t>((size_t)((double)freeB * 0.5), (size_t)16 << 30));
    const int64_t nS = (int64_t)rt.streaming.size();
    int64_t start = 0;
    while (start < nS) {
      int64_t end = start, cap = 0;
      int rowCap = 1;
      while (end < nS && end - start < (1 << 16)) {
        const int64_t c2 = std::max(cap, rt.cells[(size_t)rt.streaming[(size_t)end]]);
        const int r2 = std::max(rowCap, rt.width[(size_t)rt.streaming[(size_t)end]]);
        const size_t need = ((size_t)c2 + 2 * (size_t)r2) * W * sizeof(double) * (size_t)(end - start + 1);
        if (need > budget && end > start) break;
        cap = c2; rowCap = r2; ++end;
      }
      const int nB = (int)(end - start);
      const size_t fwdNeed = (size_t)cap * W * sizeof(double) * nB, rowNeed = 2 * (size_t)rowCap * W * sizeof(double) * nB;
      if (fwdNeed > h->dFwd.capacity() * sizeof(double)) {
        DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
        DNAS_HIP_TRY(h->dFwd.assign(fwdNeed / sizeof(double)));
      }
      if (rowNeed > h->dRows.capacity() * sizeof(double)) {
        DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
        DNAS_HIP_TRY(h->dRows.assign(rowNeed / sizeof(double)));
      }
      a.rowCap = rowCap;
      hipLaunchKernelGGL(fwdback_estep_kernel, dim3((nB + kFbThreads - 1) / kFbThreads), dim3(kFbThreads), 0, h->stream, a, h->dIn.get(), h->dInOff.get(),
                         h->dOut.get(), h->dOutOff.get(), h->dCi.get(), h->dCiOff.get(), h->dCo.get(), h->dCoOff.get(), h->dTab.get(), h->dFwd.get(), h->dRows.get(), h->dCounts.get(), h->dLL.get(), start, nB, cap,
                         (const int64_t*)rt.dStreaming.get());
      DNAS_HIP_TRY(hipGetLastError());
      start = end;     // (the next batch reuses the arenas: same stream, in order)
    }
  }
  DNAS_HIP_TRY(hipEventRecord(h->ev1, h->stream));

  // ---- reduction over pairs: fixed-shape tree, block partials added in order on the host
  const int nBlocks = (int)std::min<int64_t>(256, (n_pairs + 255) / 256);
  hipLaunchKernelGGL(fwdback_reduce_kernel, dim3(nBlocks), dim3(256), 0, h->stream, h->dCounts.get(), h->dLL.get(), n_pairs, nc, h->dPartial.get());
  DNAS_HIP_TRY(hipGetLastError());
  std::vector<double> partial((size_t)nBlocks * (nc + 1));
  DNAS_HIP_TRY(hipMemcpyAsync(partial.data(), h->dPartial.get(), partial.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out_pair_ll) DNAS_HIP_TRY(hipMemcpyAsync(out_pair_ll, h->dLL.get(), (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  unsigned long long ops = 0;
  DNAS_HIP_TRY(hipMemcpyAsync(&ops, h->dLseOps.get(), sizeof ops, hipMemcpyDeviceToHost, h->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(h->stream));
  for (int b = 0; b < nBlocks; ++b) {
    for (int k = 0; k < nc; ++k) out_counts[k] += partial[(size_t)b * (nc + 1) + k];
    *out_ll += partial[(size_t)b * (nc + 1) + nc];
  }
  float ms = 0;
  DNAS_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->stats.kernel_ms = ms;
  h->stats.pairs_onchip = (int64_t)(rt.onchip[0].size() + rt.onchip[1].size() + rt.onchip[2].size() + rt.onchip[3].size());
  h->stats.pairs_narrow = (int64_t)(rt.onchip[0].size() + rt.onchip[2].size());
  h->stats.pairs_streaming = (int64_t)rt.streaming.size();
  h->stats.lse_ops = (int64_t)ops;
  int64_t ntOut = 0;
  for (int64_t i = 0; i < n_pairs; ++i) ntOut += h->outOff[i + 1] - h->outOff[i];
  h->stats.out_nt = ntOut;
  return DNAS_OK;
}

extern "C" int dnas_fb_last_stats(const dnas_fb* h, dnas_fb_stats* out) {
  if (!h || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = h->stats;
  return DNAS_OK;
}

extern "C" int dnas_fb_devices(const dnas_fb* h) { return h ? std::max<int>(1, (int)h->sub.size()) : 0; }

// expectedCounts in one call (host pointers in, counts out): a handle for the length of the call
extern "C" int dnas_fwdback_estep(const dnas_mutator_params* p, int strict, int64_t n_pairs, const int8_t* in_seqs,
                                  const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off,
                                  const int32_t* cm_in, const int64_t* cm_in_off, const int32_t* cm_out,
                                  const int64_t* cm_out_off, int device_id, double* out_counts, double* out_ll,
                                  double* out_pair_ll) {
  if (!p || n_pairs < 0 || !out_counts || !out_ll) return dnas::fail(DNAS_E_INVALID, "dnas_fwdback_estep: null argument");
  dnas_fb* h = nullptr;
  int rc = dnas_fb_create(device_id, &h);
  if (rc == DNAS_OK) rc = dnas_fb_load_pairs(h, n_pairs, in_seqs, in_off, out_seqs, out_off, cm_in, cm_in_off, cm_out, cm_out_off);
  if (rc == DNAS_OK) rc = dnas_fb_estep(h, p, strict, out_counts, out_ll, out_pair_ll);
  dnas_fb_destroy(h);
  return rc;
}

// ---- Baum-Welch driver (host): the EM loop of host/baumwelch.hpp around the GPU E-step --------
extern "C" int dnas_baum_welch(const dnas_mutator_params* init, int strict, int64_t n_pairs, const int8_t* in_seqs,
                               const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const int32_t* cm_in,
                               const int64_t* cm_in_off, const int32_t* cm_out, const int64_t* cm_out_off, int device_id,
                               dnas_mutator_params* out, int32_t* out_iterations) {
  if (!init || !out) return dnas::fail(DNAS_E_INVALID, "dnas_baum_welch: null argument");
  // one handle for the whole EM run: the database and the log-sum-exp table go to the GPU once
  dnas_fb* h = nullptr;
  int rc0 = dnas_fb_create(device_id, &h);
  if (rc0 == DNAS_OK) rc0 = dnas_fb_load_pairs(h, n_pairs, in_seqs, in_off, out_seqs, out_off, cm_in, cm_in_off, cm_out, cm_out_off);
  if (rc0 != DNAS_OK) { dnas_fb_destroy(h); return rc0; }
  const int rc = dnas::baumWelchLoop(
      *init, 0, [&](const dnas_mutator_params& cur, double* counts, double* ll) { return dnas_fb_estep(h, &cur, strict, counts, ll, nullptr); },
      [](const dnas_mutator_params&, double) {}, out, out_iterations);
  dnas_fb_destroy(h);
  return rc;
}
