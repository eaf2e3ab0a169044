// dnas_rs_encode, dnas_rs_decode (include/dnastore_amd.h, "The outer code"), byte-identical to rsEncodeHost / rsDecodeHost
// (host/rs.cpp).  The field, a position's locator and the solver of a column with errors are host/rs.hpp, shared with the
// statement; the plan of a block and the uniform path are here.
//
// rs_block_kernel   the uniform part.  A work-group takes (block, tile of up to 128 columns).  The strands of a block are rows of L bytes, so the tile
//                   comes in coalesced, row by row, into LDS (dwords when L is a multiple of 4), erased rows as zeros; nothing
//                   gathers a column from global memory.
//   the plan        all columns of a block share the erasure set: wave 0 lists the erased positions with ballots, thread i holds
//                   coefficient i of the erasure locator while its factors are multiplied in, thread q the inverse locator of
//                   erased position q and 1 / prod (1 + X_m / X_q), the denominator of its value.
//   syndromes       an item is (syndrome i, dword of four columns): Horner over the n rows with the lane's constant alpha^i.  Four
//                   bytes times a constant is eight masked XORs of the constant's doublings, which the lane keeps spread over the
//                   bytes of eight registers: no table, no LDS traffic but the row's dword.  Lanes of one row read consecutive
//                   dwords, lanes of different syndromes the same ones (a broadcast): no bank conflict.
//   the product     S(x) gamma(x) mod x^r, an item per (coefficient, dword).  Coefficients f .. r-1 are the Forney syndromes: a
//                   column in which one of them is not zero holds errors, flagged with an LDS atomic OR.  Coefficients 0 .. f-1
//                   are the numerator of the erasure values.
//   the fill        an item is (erased position q, dword): Horner over the f coefficients with 1 / X_q, times the denominator; the
//                   bytes of flagged columns are masked out.
//   the way out     the tile goes back row by row as it came, with statuses from LDS; a tile with flagged columns also leaves its
//                   syndromes, row by row, and the block's plan (erased positions, locator) for the second kernel.
// rs_solve_kernel   the data-dependent part, after the uniform loops and not inside them: a thread per flagged column runs
//                   rsSolveColumn on the column's syndromes -- Berlekamp-Massey, the root search, the values, the re-check -- with
//                   log / antilog tables in LDS (random byte look-ups: bank conflicts of several ways, which is why the uniform
//                   loops have none), XORs its corrections into the output and counts out_fixed with integer atomics.  A thread of
//                   an unflagged column reads one status byte and leaves: a pool without errors pays a launch and that byte.
//                   The solver's arrays would cost the uniform loops their registers (one wave per SIMD, or spills, when the two
//                   were one kernel); apart, rs_block_kernel has 58 VGPRs and no scratch.
// Encoding is the same kernel: the r parity positions are the erasures of a block whose k data rows are all there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "device_buffer.hpp"
#include "devices.hpp"
#include "errors.hpp"
#include "host/rs.hpp"

namespace {

constexpr int kRsTile = 128;                             // columns of a tile: 255 rows of it are 32 640 bytes of LDS
constexpr int kRsThreads = 256;
constexpr int64_t kRsChunkBytes = (int64_t)1 << 30;      // the block bytes of a launch at most

constexpr uint8_t kRsToSolve = 255;                      // a column's status between the two kernels

// What the columns of a block share, from rs_block_kernel to rs_solve_kernel.
struct RsPlan {
  uint8_t f, erased[dnas::kRsMaxR], gamma[dnas::kRsMaxR + 1];
};

__device__ const dnas::GfTables kGfDevice = dnas::makeGfTables();

__device__ inline uint32_t gfDouble(uint32_t c) { return ((c << 1) ^ (c & 0x80 ? 0x11d : 0)) & 0xff; }

// Four bytes times one constant: bit b of every byte selects the constant's b-th doubling.
struct GfMul4 {
  uint32_t spread[8];                                    // (c alpha^b) in every byte
  __device__ explicit GfMul4(uint32_t c) {
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      spread[b] = c * 0x01010101u;
      c = gfDouble(c);
    }
  }
  __device__ __attribute__((always_inline)) uint32_t operator()(uint32_t w) const {
    uint32_t acc = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint32_t bit = (w >> b) & 0x01010101u;
      acc ^= ((bit << 8) - bit) & spread[b];             // 0xff in the bytes whose bit b is set
    }
    return acc;
  }
};

// 0xff in every byte of w that is not zero
__device__ inline uint32_t nonzeroBytes(uint32_t w) {
  const uint32_t bit = ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
  return (bit << 8) - bit;
}

// in: [B][nin][L], rows nin .. n-1 absent (encoding: nin = k); present: [B][n], or null when the rows below nin are all there.
__global__ __launch_bounds__(kRsThreads) void rs_block_kernel(int n, int r, int L, int nin, int tiles, int strideW,
                                                              const uint8_t* __restrict__ in, const uint8_t* __restrict__ present,
                                                              uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                              uint8_t* __restrict__ errors, uint8_t* __restrict__ syndromes,
                                                              RsPlan* __restrict__ plans, unsigned long long* __restrict__ counters) {
  extern __shared__ uint32_t dyn[];
  __shared__ dnas::GfTables gf;
  __shared__ uint8_t presentS[256], erasedS[dnas::kRsMaxR], gammaS[dnas::kRsMaxR + 4], xinvS[dnas::kRsMaxR], denS[dnas::kRsMaxR];
  __shared__ uint8_t statusS[kRsTile];
  __shared__ uint32_t flag4[kRsTile / 4];
  __shared__ int nErasedS, nFlaggedS;

  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int64_t blk = (int64_t)blockIdx.x / tiles;
  const int tile = (int)((int64_t)blockIdx.x % tiles);
  const int j0 = tile * kRsTile, Lt = L - j0 < kRsTile ? L - j0 : kRsTile, Lw = (Lt + 3) >> 2;
  const int stride = strideW * 4;
  uint32_t *wordW = dyn, *synW = dyn + n * strideW, *prodW = synW + r * strideW;
  uint8_t *wordB = (uint8_t*)wordW, *synB = (uint8_t*)synW;
  const uint8_t* inBlk = in + blk * nin * (int64_t)L + j0;
  uint8_t* outBlk = out + blk * n * (int64_t)L + j0;
  const bool dwords = (L & 3) == 0;                      // then every row of every tile begins on a dword

  for (int i = tid; i < (int)(sizeof(dnas::GfTables) / 4); i += nthreads) ((uint32_t*)&gf)[i] = ((const uint32_t*)&kGfDevice)[i];
  for (int p = tid; p < 256; p += nthreads) {
    presentS[p] = p < n ? (present ? present[blk * n + p] != 0 : p < nin) : 1;
  }
  if (tid < kRsTile / 4) flag4[tid] = 0;
  if (tid == 0) nFlaggedS = 0;
  __syncthreads();

  // ---- the plan: erased positions, in ascending order (the first 64 of them; more than r is a failed block) ----
  if (tid < 64) {
    int count = 0;
    for (int base = 0; base < 256; base += 64) {
      const bool gone = !presentS[base + tid];
      const unsigned long long votes = __ballot(gone);
      const int at = count + __popcll(votes & (((unsigned long long)1 << tid) - 1));
      if (gone && at < dnas::kRsMaxR) erasedS[at] = (uint8_t)(base + tid);
      count += __popcll(votes);
    }
    if (tid == 0) nErasedS = count;
  }
  // ---- the tile, erased rows as zeros ----
  if (dwords) {
    for (int idx = tid; idx < n * Lw; idx += nthreads) {
      const int p = idx / Lw, jw = idx - p * Lw;
      wordW[p * strideW + jw] = p < nin && presentS[p] ? *(const uint32_t*)(inBlk + p * (int64_t)L + 4 * jw) : 0;
    }
  } else {
    for (int idx = tid; idx < n * 4 * Lw; idx += nthreads) {
      const int p = idx / (4 * Lw), j = idx - p * 4 * Lw;
      wordB[p * stride + j] = j < Lt && p < nin && presentS[p] ? inBlk[p * (int64_t)L + j] : 0;
    }
  }
  __syncthreads();
  const int f = nErasedS;
  const bool hopeless = f > r;                           // uniform over the work-group

  if (!hopeless) {
    if (tid <= dnas::kRsMaxR) gammaS[tid] = tid == 0;
    if (tid < f) {
      const uint8_t Xi = dnas::rsLocatorInverse(gf, n, erasedS[tid]);
      uint8_t den = 1;
      for (int m = 0; m < f; ++m)
        if (m != tid) den = dnas::gfMul(gf, den, (uint8_t)(1 ^ dnas::gfMul(gf, dnas::rsLocator(gf, n, erasedS[m]), Xi)));
      xinvS[tid] = Xi;
      denS[tid] = dnas::gfDiv(gf, 1, den);
    }
    __syncthreads();
    for (int q = 0; q < f; ++q) {                        // gamma <- gamma (1 - X_q x)
      uint8_t next = 0;
      const bool mine = tid >= 1 && tid <= q + 1;
      if (mine) next = (uint8_t)(gammaS[tid] ^ dnas::gfMul(gf, dnas::rsLocator(gf, n, erasedS[q]), gammaS[tid - 1]));
      __syncthreads();
      if (mine) gammaS[tid] = next;
      __syncthreads();
    }

    // ---- syndromes: S_i = the word at alpha^i, Horner over the rows ----
    for (int it = tid; it < r * Lw; it += nthreads) {
      const int i = it / Lw, jw = it - i * Lw;
      const GfMul4 timesAlphaI(gf.exp[i]);
      uint32_t acc = 0;
      for (int p = 0; p < n; ++p) acc = timesAlphaI(acc) ^ wordW[p * strideW + jw];
      synW[i * strideW + jw] = acc;
    }
    __syncthreads();

    // ---- S gamma mod x^r; coefficients f .. r-1 flag the columns with errors ----
    for (int it = tid; it < r * Lw; it += nthreads) {
      const int t = it / Lw, jw = it - t * Lw;
      const int top = t < f ? t : f;
      uint32_t acc = 0;
      for (int a = 0; a <= top; ++a) acc ^= GfMul4(gammaS[a])(synW[(t - a) * strideW + jw]);
      prodW[t * strideW + jw] = acc;
      if (t >= f && acc) atomicOr(&flag4[jw], acc);
    }
    __syncthreads();

    // ---- erasure values of the columns without errors ----
    for (int it = tid; it < f * Lw; it += nthreads) {
      const int q = it / Lw, jw = it - q * Lw;
      const GfMul4 timesXinv(xinvS[q]);
      uint32_t acc = 0;
      for (int t = f - 1; t >= 0; --t) acc = timesXinv(acc) ^ prodW[t * strideW + jw];
      wordW[erasedS[q] * strideW + jw] = GfMul4(denS[q])(acc) & ~nonzeroBytes(flag4[jw]);
    }
  }
  for (int j = tid; j < Lt; j += nthreads) {
    const bool flagged = !hopeless && ((flag4[j >> 2] >> (8 * (j & 3))) & 0xff) != 0;
    statusS[j] = hopeless ? DNAS_RS_FAILED : flagged ? kRsToSolve : DNAS_RS_OK;
    if (flagged) atomicAdd(&nFlaggedS, 1);
  }
  __syncthreads();
  const int nFlagged = nFlaggedS;

  // ---- the way out ----
  if (dwords) {
    for (int idx = tid; idx < n * Lw; idx += nthreads) {
      const int p = idx / Lw, jw = idx - p * Lw;
      *(uint32_t*)(outBlk + p * (int64_t)L + 4 * jw) = wordW[p * strideW + jw];
    }
  } else {
    for (int idx = tid; idx < n * 4 * Lw; idx += nthreads) {
      const int p = idx / (4 * Lw), j = idx - p * 4 * Lw;
      if (j < Lt) outBlk[p * (int64_t)L + j] = wordB[p * stride + j];
    }
  }
  if (status)
    for (int j = tid; j < Lt; j += nthreads) {
      status[blk * L + j0 + j] = statusS[j];
      errors[blk * L + j0 + j] = 0;
    }
  // ---- what rs_solve_kernel needs for the flagged columns: their syndromes, row by row, and the block's plan ----
  if (nFlagged) {
    uint8_t* synBlk = syndromes + blk * r * (int64_t)L + j0;
    for (int idx = tid; idx < r * Lt; idx += nthreads) {
      const int i = idx / Lt, j = idx - i * Lt;
      synBlk[i * (int64_t)L + j] = synB[i * stride + j];
    }
    RsPlan* mine = plans + blk;                          // (every flagged tile of the block writes the same bytes)
    if (tid == 0) mine->f = (uint8_t)f;
    if (tid < f) mine->erased[tid] = erasedS[tid];
    if (tid <= f) mine->gamma[tid] = gammaS[tid];
    if (tid == 0) atomicAdd(counters, (unsigned long long)nFlagged);
  }
}

// The columns rs_block_kernel flagged, a thread each: the solver on the column's syndromes, its corrections XORed into the output.
// (Four waves per SIMD: the solver's arrays then live in scratch, not in 389 registers at one wave per SIMD, and the kernel takes
// 24.5 ms instead of 84.3 ms on bench_outer.py's arm (a) -- its time is the latency of dependent table look-ups, which more waves hide.)
__global__ __launch_bounds__(kRsThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void rs_solve_kernel(int n, int r, int L, int64_t columns, const uint8_t* __restrict__ present,
                                                              const uint8_t* __restrict__ syndromes, const RsPlan* __restrict__ plans,
                                                              uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                              uint8_t* __restrict__ errors, int32_t* __restrict__ fixed) {
  __shared__ dnas::GfTables gf;
  for (int i = threadIdx.x; i < (int)(sizeof(dnas::GfTables) / 4); i += blockDim.x) ((uint32_t*)&gf)[i] = ((const uint32_t*)&kGfDevice)[i];
  __syncthreads();
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= columns || status[col] != kRsToSolve) return;
  const int64_t blk = col / L, j = col - blk * L;
  const RsPlan* plan = plans + blk;
  const int f = plan->f;
  uint8_t S[dnas::kRsMaxR], fixPos[dnas::kRsMaxR], fixVal[dnas::kRsMaxR];
  for (int i = 0; i < r; ++i) S[i] = syndromes[(blk * r + i) * L + j];
  int nFix = 0, nErr = 0;
  const int st = dnas::rsSolveColumn(gf, n, r, f, plan->erased, plan->gamma, present + blk * n, S, fixPos, fixVal, &nFix, &nErr);
  status[col] = (uint8_t)st;
  errors[col] = (uint8_t)nErr;
  for (int q = 0; q < nFix; ++q) {
    out[(blk * n + fixPos[q]) * L + j] ^= fixVal[q];
    if (q >= f) atomicAdd(&fixed[blk * n + fixPos[q]], 1);
  }
}

struct RsCall {
  int32_t n, k, L, nin;                                  // nin: the rows a block has in the input (k: encoding)
  const uint8_t *in, *present;                           // host; present null when encoding
  uint8_t *out, *status, *errors;                        // host; status, errors, fixed null when encoding
  int32_t* fixed;
};

// One device's share, blocks [first, last) of the call, in launches of at most `chunk` blocks.
int rsOn(int device, const RsCall& call, int64_t first, int64_t last, dnas_rs_stats* stats) {
  if (first >= last) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  const int64_t n = call.n, L = call.L, nin = call.nin;
  const int r = call.n - call.k;
  const int tiles = (int)((L + kRsTile - 1) / kRsTile);
  const int strideW = (int)((std::min<int64_t>(L, kRsTile) + 3) / 4);
  const size_t lds = (size_t)(n + 2 * r) * strideW * sizeof(uint32_t);
  const int items = r * strideW;
  const int threads = std::min(kRsThreads, std::max(128, (items + 63) / 64 * 64));   // (the plan wants a thread per locator coefficient: 65)
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(kRsChunkBytes / (n * L), (((int64_t)1 << 30)) / tiles));
  if (const char* s = getenv("DNAS_RS_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, atoll(s)));
  chunk = std::min(chunk, last - first);

  dnas::DevBuf<uint8_t> dIn, dPresent, dOut, dStatus, dErrors;
  dnas::DevBuf<int32_t> dFixed;
  dnas::DevBuf<RsPlan> dPlans;
  dnas::DevBuf<uint8_t> dSyndromes;
  dnas::DevBuf<unsigned long long> dCounters;
  DNAS_HIP_TRY(dIn.assign((size_t)(chunk * nin * L)));
  DNAS_HIP_TRY(dOut.assign((size_t)(chunk * n * L)));
  DNAS_HIP_TRY(dCounters.assign(1));
  if (call.present) {
    DNAS_HIP_TRY(dPresent.assign((size_t)(chunk * n)));
    DNAS_HIP_TRY(dStatus.assign((size_t)(chunk * L)));
    DNAS_HIP_TRY(dErrors.assign((size_t)(chunk * L)));
    DNAS_HIP_TRY(dFixed.assign((size_t)(chunk * n)));
    DNAS_HIP_TRY(dPlans.assign((size_t)chunk));
    DNAS_HIP_TRY(dSyndromes.assign((size_t)(chunk * r * L)));
  }
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  DNAS_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct Closer {
    hipStream_t& s;
    hipEvent_t* e;
    ~Closer() {
      if (e[0]) (void)hipEventDestroy(e[0]);
      if (e[1]) (void)hipEventDestroy(e[1]);
      (void)hipStreamDestroy(s);
    }
  } closer{stream, ev};
  DNAS_HIP_TRY(hipEventCreate(&ev[0]));
  DNAS_HIP_TRY(hipEventCreate(&ev[1]));
  DNAS_HIP_TRY(hipMemsetAsync(dCounters.get(), 0, sizeof(unsigned long long), stream));

  for (int64_t b0 = first; b0 < last; b0 += chunk) {
    const int64_t nb = std::min(chunk, last - b0);
    DNAS_HIP_TRY(hipMemcpyAsync(dIn.get(), call.in + b0 * nin * L, (size_t)(nb * nin * L), hipMemcpyHostToDevice, stream));
    if (call.present) {
      DNAS_HIP_TRY(hipMemcpyAsync(dPresent.get(), call.present + b0 * n, (size_t)(nb * n), hipMemcpyHostToDevice, stream));
      DNAS_HIP_TRY(hipMemsetAsync(dFixed.get(), 0, (size_t)(nb * n) * sizeof(int32_t), stream));
    }
    DNAS_HIP_TRY(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(rs_block_kernel, dim3((unsigned)(nb * tiles)), dim3((unsigned)threads), lds, stream, (int)n, r, (int)L, (int)nin, tiles,
                       strideW, dIn.get(), call.present ? dPresent.get() : (const uint8_t*)nullptr, dOut.get(),
                       call.present ? dStatus.get() : (uint8_t*)nullptr, call.present ? dErrors.get() : (uint8_t*)nullptr,
                       call.present ? dSyndromes.get() : (uint8_t*)nullptr, call.present ? dPlans.get() : (RsPlan*)nullptr, dCounters.get());
    if (call.present)
      hipLaunchKernelGGL(rs_solve_kernel, dim3((unsigned)((nb * L + kRsThreads - 1) / kRsThreads)), dim3(kRsThreads), 0, stream, (int)n, r, (int)L,
                         nb * L, dPresent.get(), dSyndromes.get(), dPlans.get(), dOut.get(), dStatus.get(), dErrors.get(), dFixed.get());
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(ev[1], stream));
    DNAS_HIP_TRY(hipMemcpyAsync(call.out + b0 * n * L, dOut.get(), (size_t)(nb * n * L), hipMemcpyDeviceToHost, stream));
    if (call.present) {
      DNAS_HIP_TRY(hipMemcpyAsync(call.status + b0 * L, dStatus.get(), (size_t)(nb * L), hipMemcpyDeviceToHost, stream));
      DNAS_HIP_TRY(hipMemcpyAsync(call.errors + b0 * L, dErrors.get(), (size_t)(nb * L), hipMemcpyDeviceToHost, stream));
      DNAS_HIP_TRY(hipMemcpyAsync(call.fixed + b0 * n, dFixed.get(), (size_t)(nb * n) * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
    DNAS_HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    DNAS_HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    stats->kernel_ms += ms;
    stats->launches += 1;
  }
  unsigned long long flagged = 0;
  DNAS_HIP_TRY(hipMemcpyAsync(&flagged, dCounters.get(), sizeof flagged, hipMemcpyDeviceToHost, stream));
  DNAS_HIP_TRY(hipStreamSynchronize(stream));
  stats->columns_solved = (int64_t)flagged;
  stats->columns = (last - first) * L;
  return DNAS_OK;
}

// device_id = -1: contiguous ranges of blocks, one per device
int rsRun(const RsCall& call, int64_t B, int device_id, dnas_rs_stats* out_stats) {
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  if (B == 0) return DNAS_OK;
  try {
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const int64_t W = (int64_t)devices.size();
    std::vector<dnas_rs_stats> stats((size_t)W);
    const int rc = dnas::forEachDevice(devices, [&](size_t w) {
      return rsOn(devices[w], call, B * (int64_t)w / W, B * ((int64_t)w + 1) / W, &stats[w]);
    });
    if (rc) return rc;
    if (out_stats) {
      for (const dnas_rs_stats& s : stats) {
        out_stats->kernel_ms = std::max(out_stats->kernel_ms, s.kernel_ms);
        out_stats->columns += s.columns;
        out_stats->columns_solved += s.columns_solved;
        out_stats->launches += s.launches;
      }
      out_stats->devices = W;
    }
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

}  // namespace

extern "C" int dnas_rs_encode(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t* data, uint8_t* out_blocks, dnas_rs_stats* out_stats,
                              int device_id) {
  if (out_stats) *out_stats = dnas_rs_stats{};
  if (const int rc = dnas::checkRsCode(n, k, L, B)) return rc;
  if (B && (!data || !out_blocks)) return dnas::fail(DNAS_E_INVALID, "reed-solomon: null argument");
  const RsCall call{n, k, L, k, data, nullptr, out_blocks, nullptr, nullptr, nullptr};
  return rsRun(call, B, device_id, out_stats);
}

extern "C" int dnas_rs_decode(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t* blocks, const uint8_t* present, uint8_t* out_blocks,
                              uint8_t* out_status, uint8_t* out_errors, int32_t* out_fixed, dnas_rs_stats* out_stats, int device_id) {
  if (out_stats) *out_stats = dnas_rs_stats{};
  if (const int rc = dnas::checkRsCode(n, k, L, B)) return rc;
  if (B && (!blocks || !present || !out_blocks || !out_status || !out_errors || !out_fixed))
    return dnas::fail(DNAS_E_INVALID, "reed-solomon: null argument");
  const RsCall call{n, k, L, n, blocks, present, out_blocks, out_status, out_errors, out_fixed};
  return rsRun(call, B, device_id, out_stats);
}
