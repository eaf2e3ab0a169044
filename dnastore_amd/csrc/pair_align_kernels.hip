// dnas_align_pairs: the pair-HMM Viterbi alignment of host/pairalign.hpp on the GPU, bit-identical to alignPairHost.
//
// Fill.  A wave owns a pair and walks the batch with the grid's stride; there is no work-group barrier.  The rows of the
// matrix are taken in stripes of 64: lane l owns row 64 s + l and is skewed one column per lane, at step t it stands on
// column c0 + t - l (c0: the first column of the stripe's band).  S and D of the row above are what lane l - 1 computed one step
// earlier (lane shuffle), the diagonal S what it computed two steps earlier (the value shuffled at the step before, kept); the
// duplication lanes T_0 .. T_{P-1} of (ip, op - 1) never leave the lane's registers, the output base travels down the lanes with
// the scores.  Lane 63's S and D go to a boundary row of O + 1 columns -- in LDS while that fits, else in the wave's scratch in
// HBM -- from which lane 0 of the next stripe reads them: any band width and the full matrix are served.  No score leaves the
// chip but S(I,O); what does is one 16-bit choice word per cell (bits 0-1: S took s0 / s1 / s2, bit 2: D took d1, bit 3 + k:
// T_k took t1), filed under (stripe, step, lane): a wave's store is 128 consecutive bytes.
//
// Traceback.  One thread per pair reads one choice word per move and writes op bytes from the end of the slot, then moves them
// to its start.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/pairalign.hpp"

namespace {

constexpr int kPaWavesPerBlock = 4;
constexpr int kPaLdsDoubles = 2048;                      // per wave: 16 substitution scores, then the boundary row
constexpr int kPaLdsCols = (kPaLdsDoubles - 16) / 2;     // columns (O + 1) a boundary row in LDS holds
constexpr uint64_t kPaSkip = ~0ull;

struct PaScores {
  double delOpen, tanDup, noGap, delExtend, delEnd;
  double len[dnas::kAlignMaxLen];
  int P;
};

// What fill and traceback agree on: the band as host/pairalign.hpp defines it, and where a cell's choice word lies.
struct PaGeom {
  int lo, hi, stepsMax, stripes;
  __host__ __device__ PaGeom(int I, int O, int band) {
    const int b = band < 0 || band > I + O + 1 ? I + O + 1 : band;
    lo = (O < I ? O - I : 0) - b;
    hi = (O > I ? O - I : 0) + b;
    // a stripe of rows r0 .. r0 + 63 runs from column c0 = rowLo(r0) to rowHi(r0 + 63), lane 63 another 63 steps behind
    const long w = (long)hi - lo + 1 + 126, f = (long)O + 64;
    stepsMax = (int)(w < f ? w : f);
    stripes = I / 64 + 1;
  }
  __host__ __device__ int rowLo(int ip) const { return ip + lo > 0 ? ip + lo : 0; }
  __host__ __device__ int rowHi(int ip, int O) const { return ip + hi < O ? ip + hi : O; }
  __host__ __device__ size_t words() const { return (size_t)stripes * (size_t)stepsMax * 64; }
  __host__ __device__ size_t wordAt(int ip, int op) const {
    const int s = ip >> 6, l = ip & 63;
    return ((size_t)s * (size_t)stepsMax + (size_t)(op - rowLo(s << 6) + l)) * 64 + (size_t)l;
  }
};

__device__ inline double paNegInf() { return -__builtin_huge_val(); }

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void pair_align_fill_kernel(
    PaScores sc, const double* __restrict__ subTable, int band, int64_t first, int64_t count, const int8_t* __restrict__ inSeqs,
    const int64_t* __restrict__ inOff, const int8_t* __restrict__ outSeqs, const int64_t* __restrict__ outOff,
    const uint64_t* __restrict__ recOff, uint16_t* __restrict__ arena, double* bndScratch, int64_t bndStride,
    double* __restrict__ score) {
  __shared__ double lds[kPaWavesPerBlock][kPaLdsDoubles];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * kPaWavesPerBlock + wv, nWaves = (int64_t)gridDim.x * kPaWavesPerBlock;
  double* const sub = lds[wv];
  double* const bndLds = lds[wv] + 16;
  if (lane < 16) sub[lane] = subTable[lane];
  __builtin_amdgcn_wave_barrier();
  double* const bndMem = bndScratch + wave * bndStride;
  const double NEG = paNegInf();
  const int P = sc.P;

  for (int64_t q = wave; q < count; q += nWaves) {
    const uint64_t ro = recOff[q];
    if (ro == kPaSkip) continue;
    const int64_t pair = first + q;
    const int I = (int)(inOff[pair + 1] - inOff[pair]), O = (int)(outOff[pair + 1] - outOff[pair]);
    const int8_t* const a = inSeqs + inOff[pair];
    const int8_t* const b = outSeqs + outOff[pair];
    uint16_t* const rec = arena + ro;
    const PaGeom g(I, O, band);
    const bool useLds = O + 1 <= kPaLdsCols;

    for (int s = 0; s < g.stripes; ++s) {
      const int r0 = s << 6, r = r0 + lane;
      const bool row = r <= I;
      const int rlo = row ? g.rowLo(r) : 1, rhi = row ? g.rowHi(r, O) : 0;
      const int c0 = g.rowLo(r0);
      const int last = I - r0 < 63 ? I - r0 : 63;
      const int tmax = g.rowHi(r0 + last, O) - c0 + last;
      const int ulo = g.rowLo(r0 - 1), uhi = g.rowHi(r0 - 1, O);     // the row above the stripe (s > 0)
      const int kmax = row ? (r < P ? r : P) : 0;
      unsigned ctx = 0;                                              // in[r-1-k] at bits 2k: the bases this row compares with
#pragma unroll
      for (int k = 0; k <= KP; ++k)
        if (row && r - 1 - k >= 0) ctx |= ((unsigned)a[r - 1 - k] & 3u) << (2 * k);
      double T[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) T[k] = NEG;
      double Sdiag = NEG, pubS = NEG, pubD = NEG;
      int ypub = 0, ychunk = 0;
      if (lane == 0 && s > 0 && c0 >= 1)
        Sdiag = useLds ? bndLds[2 * (c0 - 1)]
                       : __hip_atomic_load(bndMem + 2 * (size_t)(c0 - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint16_t* const recStripe = rec + (size_t)s * (size_t)g.stepsMax * 64 + lane;

      for (int t = 0; t <= tmax; ++t) {
        if ((t & 63) == 0) {                                         // the next 64 output bases lane 0 will hand down
          const int j = c0 + t - 1 + lane;
          ychunk = j >= 0 && j < O ? (int)b[j] & 3 : 0;
        }
        double Sup = __shfl_up(pubS, 1), Dup = __shfl_up(pubD, 1);
        int y = __shfl_up(ypub, 1);
        const int y0 = __shfl(ychunk, t & 63);
        const int op = c0 + t - lane;
        if (lane == 0) {
          y = y0;
          Sup = Dup = NEG;
          if (s > 0 && op >= ulo && op <= uhi) {
            if (useLds) {
              Sup = bndLds[2 * op];
              Dup = bndLds[2 * op + 1];
            } else {
              Sup = __hip_atomic_load(bndMem + 2 * (size_t)op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              Dup = __hip_atomic_load(bndMem + 2 * (size_t)op + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
        const bool active = op >= rlo && op <= rhi;
        double S = NEG, D = NEG;
        if (active) {
          unsigned word = 0;
          double c;
          c = Sup + sc.delOpen;
          if (c > D) D = c;
          c = Dup + sc.delExtend;
          if (c > D) { D = c; word = 4u; }
          if (r == 0 && op == 0) {
            S = 0;
          } else {
            const double sub0 = sub[(ctx & 3u) * 4 + y];
            c = Sdiag + sc.noGap + sub0;
            if (c > S) S = c;
            c = T[0] + sub0;
            if (c > S) { S = c; word = (word & ~3u) | 1u; }
            c = D + sc.delEnd;
            if (c > S) { S = c; word = (word & ~3u) | 2u; }
          }
          const double open = S + sc.tanDup;
#pragma unroll
          for (int k = 0; k < KP; ++k) {
            double best = NEG;
            if (k + 1 < KP) {
              c = T[k + 1] + sub[((ctx >> (2 * k + 2)) & 3u) * 4 + y];
              if (c > best) best = c;
            }
            c = open + sc.len[k];
            if (c > best) { best = c; word |= 8u << k; }
            T[k] = k < kmax ? best : NEG;
          }
          recStripe[(size_t)t * 64] = (uint16_t)word;
          if (lane == 63) {
            if (useLds) {
              bndLds[2 * op] = S;
              bndLds[2 * op + 1] = D;
            } else {
              __hip_atomic_store(bndMem + 2 * (size_t)op, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(bndMem + 2 * (size_t)op + 1, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          if (r == I && op == O) score[pair] = S;
        }
        Sdiag = Sup;
        pubS = S;
        pubD = D;
        ypub = y;
      }
      // the next stripe's lane 0 reads what this stripe's lane 63 wrote
      if (useLds) __builtin_amdgcn_wave_barrier();
      else __threadfence();
    }
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

struct PaBuffers {
  std::vector<void*> mem;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~PaBuffers() {
    for (void* q : mem) (void)hipFree(q);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

#define PA_TRY(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return dnas::fail(DNAS_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
int paAlloc(PaBuffers& bufs, T** out, size_t n) {
  void* q = nullptr;
  PA_TRY(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  bufs.mem.push_back(q);
  *out = (T*)q;
  return DNAS_OK;
}

template <class T>
int paUpload(PaBuffers& bufs, T** out, const T* src, size_t n) {
  if (const int rc = paAlloc(bufs, out, n)) return rc;
  if (n) PA_TRY(hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice));
  return DNAS_OK;
}

// One device.  The arguments were checked by dnas_align_pairs; results go to the caller's arrays.
int paAlignOnDevice(const dnas::PairScores& hs, int band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                    const int8_t* out_seqs, const int64_t* out_off, int device, size_t arena_bytes, uint8_t* out_ops,
                    const uint64_t* ops_off, uint32_t* out_n_ops, double* out_score, uint8_t* out_status, dnas_align_stats* stats) {
  *stats = dnas_align_stats{};
  if (n == 0) return DNAS_OK;
  PA_TRY(hipSetDevice(device));
  PaBuffers bufs;
  PA_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
  for (hipEvent_t& e : bufs.ev) PA_TRY(hipEventCreate(&e));

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
    PA_TRY(hipMemGetInfo(&freeB, &totalB));
    arenaWords = std::min(total, freeB / 2 / 2);          // half of what is free: the sequences and the results need room too
  }
  arenaWords = std::min(arenaWords, total);

  PaScores sc{};
  sc.delOpen = hs.delOpen; sc.tanDup = hs.tanDup; sc.noGap = hs.noGap; sc.delExtend = hs.delExtend; sc.delEnd = hs.delEnd;
  for (int k = 0; k < dnas::kAlignMaxLen; ++k) sc.len[k] = hs.len[k];
  sc.P = hs.P;

  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  // 64 KiB of LDS per work-group: two of them share a CU
  int maxBlocks = (int)std::min<int64_t>(cus * 2, (n + kPaWavesPerBlock - 1) / kPaWavesPerBlock);
  if (const char* s = getenv("DNAS_ALIGN_BLOCKS")) maxBlocks = std::max(1, std::min(maxBlocks, atoi(s)));   // testing aid: a small grid
  const int64_t bndStride = maxO + 1 > kPaLdsCols ? 2 * ((int64_t)maxO + 1) : 0;
  // boundary rows in HBM: one per wave of the grid, the grid cut so that they stay within 1 GiB
  if (bndStride) maxBlocks = (int)std::max<int64_t>(1, std::min<int64_t>(maxBlocks, ((int64_t)1 << 30) / (bndStride * 8 * kPaWavesPerBlock)));

  int8_t *dIn = nullptr, *dOut = nullptr;
  int64_t *dInOff = nullptr, *dOutOff = nullptr;
  uint64_t *dOpsOff = nullptr, *dRecOff = nullptr;
  double *dSub = nullptr, *dScore = nullptr, *dBnd = nullptr;
  uint16_t* dArena = nullptr;
  uint8_t *dOps = nullptr, *dStatus = nullptr;
  uint32_t* dNOps = nullptr;
  const size_t nOpsBytes = (size_t)ops_off[n];
  int rc;
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
  if ((rc = paAlloc(bufs, &dBnd, (size_t)bndStride * (size_t)maxBlocks * kPaWavesPerBlock))) return rc;

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
  PA_TRY(hipMemcpy(dRecOff, recOff.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  stats->batches = (int64_t)batches.size();

  for (const auto& bt : batches) {
    const int64_t first = bt.first, count = bt.second - bt.first;
    if (count == 0) continue;
    const unsigned blocks = (unsigned)std::min<int64_t>((count + kPaWavesPerBlock - 1) / kPaWavesPerBlock, maxBlocks);
    PA_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
#define PA_FILL(KP)                                                                                                              \
  hipLaunchKernelGGL(pair_align_fill_kernel<KP>, dim3(blocks), dim3(64 * kPaWavesPerBlock), 0, bufs.stream, sc, dSub, band, first, \
                     count, dIn, dInOff, dOut, dOutOff, dRecOff + first, dArena, dBnd, bndStride, dScore)
    if (sc.P <= 2) PA_FILL(2);
    else if (sc.P <= 6) PA_FILL(6);
    else PA_FILL(13);
#undef PA_FILL
    PA_TRY(hipGetLastError());
    PA_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
    hipLaunchKernelGGL(pair_align_traceback_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, bufs.stream, band, first, count,
                       dInOff, dOutOff, dRecOff + first, dArena, dScore, dOps, dOpsOff, dNOps, dStatus);
    PA_TRY(hipGetLastError());
    PA_TRY(hipEventRecord(bufs.ev[2], bufs.stream));
    PA_TRY(hipStreamSynchronize(bufs.stream));
    float fill = 0, tb = 0;
    PA_TRY(hipEventElapsedTime(&fill, bufs.ev[0], bufs.ev[1]));
    PA_TRY(hipEventElapsedTime(&tb, bufs.ev[1], bufs.ev[2]));
    stats->fill_ms += fill;
    stats->traceback_ms += tb;
  }
  PA_TRY(hipMemcpy(out_score, dScore, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  PA_TRY(hipMemcpy(out_status, dStatus, (size_t)n, hipMemcpyDeviceToHost));
  PA_TRY(hipMemcpy(out_n_ops, dNOps, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nOpsBytes) PA_TRY(hipMemcpy(out_ops, dOps, nOpsBytes, hipMemcpyDeviceToHost));
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
  int have = 0;
  if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return dnas::fail(DNAS_E_DEVICE, "no HIP device available");
  if (device_id < -1 || device_id >= have) return dnas::fail(DNAS_E_INVALID, "device_id out of range");
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
    std::vector<int> rcs(W, DNAS_OK);
    std::vector<std::string> errs(W);
    std::vector<dnas_align_stats> stats(W);
    auto run = [&](size_t k) {
      try {
        const std::vector<int64_t>& mine = shard[k];
        const size_t m = mine.size();
        std::vector<int64_t> inOff(1, 0), outOff(1, 0);
        std::vector<uint64_t> opsOff(1, 0);
        for (int64_t i : mine) {
          inOff.push_back(inOff.back() + in_off[i + 1] - in_off[i]);
          outOff.push_back(outOff.back() + out_off[i + 1] - out_off[i]);
          opsOff.push_back(opsOff.back() + (uint64_t)((in_off[i + 1] - in_off[i]) + (out_off[i + 1] - out_off[i])));
        }
        std::vector<int8_t> in((size_t)inOff.back() + 1), outs((size_t)outOff.back() + 1);
        for (size_t j = 0; j < m; ++j) {
          std::copy(in_seqs + in_off[mine[j]], in_seqs + in_off[mine[j] + 1], in.begin() + inOff[j]);
          std::copy(out_seqs + out_off[mine[j]], out_seqs + out_off[mine[j] + 1], outs.begin() + outOff[j]);
        }
        std::vector<uint8_t> ops((size_t)opsOff.back() + 1), status(m + 1);
        std::vector<uint32_t> nOps(m + 1);
        std::vector<double> score(m + 1);
        rcs[k] = paAlignOnDevice(hs, band, (int64_t)m, in.data(), inOff.data(), outs.data(), outOff.data(), devices[k], arena_bytes,
                                 ops.data(), opsOff.data(), nOps.data(), score.data(), status.data(), &stats[k]);
        if (rcs[k] == DNAS_OK)
          for (size_t j = 0; j < m; ++j) {
            const int64_t i = mine[j];
            out_score[i] = score[j];
            out_status[i] = status[j];
            out_n_ops[i] = nOps[j];
            std::copy(ops.begin() + (size_t)opsOff[j], ops.begin() + (size_t)opsOff[j] + nOps[j], out_ops + ops_off[i]);
          }
      } catch (const std::bad_alloc&) {
        rcs[k] = dnas::fail(DNAS_E_NOMEM, "out of memory");
      }
      if (rcs[k] != DNAS_OK) errs[k] = dnas::lastErrorSlot();
    };
    std::vector<std::thread> workers;
    for (size_t k = 0; k < W; ++k) workers.emplace_back(run, k);
    for (auto& t : workers) t.join();
    for (size_t k = 0; k < W; ++k)
      if (rcs[k] != DNAS_OK) return dnas::fail(rcs[k], "device " + std::to_string(devices[k]) + ": " + errs[k]);
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
