// dnas_simulate_reads (include/dnastore_amd.h, "simulating reads"), bit-identical to simulateReadHost (host/simulate.cpp).  The
// generator, the thresholds and what a position does with its draws are host/simulate.hpp, shared with the statement; how the
// positions of a read are spread over a wave and put back in order is here.
//
// A wave takes a read, its lanes the positions 64 chunk + lane.  A lane runs the S loop of its position (simPosition) and keeps
// the numbers of bases and ops it made, whether it opened a deletion, and whether its draw 0 would extend one (simExtend).  Two
// ballots of those bits and the carry bit of the chunk before give the positions that are entered with a deletion open
// (simEntryBits: the carries of one 64-bit addition); such a lane whose draw 0 extends is swallowed -- one op, no base.  An
// inclusive scan over the lanes (bases and ops packed into one word: a lane makes at most 16 x 32 + 1 of each, a chunk less than
// 2^16) plus the running totals places every lane's columns.
//
// simulate_kernel<false>   the first pass: a read's totals of bases and ops, and its orientation.
// simulate_kernel<true>    the second pass over a batch, after the host's exclusive scan of the totals: the same draws again,
//                          bases and ops stored at their places -- a lane whose position made one column (nearly all) stores
//                          what the count left in its registers, neighbouring lanes neighbouring bytes; a lane with more runs
//                          its S loop once more with a storing emit.  A read handed out reversed is stored back to front,
//                          complemented; its ops are not.
// Both are persistent: a grid of at most 8 work-groups of four waves per CU walks the reads with the grid's stride.
//
// simulate_thread_kernel   the same two passes with a thread per read, the statement's loop as it stands: kept for comparison
//                          (DNAS_SIMULATE_THREAD_PER_READ=1; DESIGN.md 4.11 has the two side by side), never the default.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/simulate.hpp"
#include "pair_align_device.h"

namespace {

constexpr int kSimWavesPerBlock = 4;
constexpr int64_t kSimSkip = -1;                         // the place of a read that is too large for the arena

// What a lane keeps of its position's S loop.
struct SimLane {
  uint32_t bases = 0, ops = 0;
  int lastBase = 0;
  uint8_t lastOp = 0;
};

template <bool WRITE>
__global__ __launch_bounds__(64 * kSimWavesPerBlock) void simulate_kernel(
    const dnas::SimThresholds* __restrict__ thGlobal, uint64_t seed, int64_t first, int64_t count, const int8_t* __restrict__ strands,
    const int64_t* __restrict__ strandOff, const int64_t* __restrict__ readStrand, const uint64_t* __restrict__ readIndex,
    uint32_t* __restrict__ totals, uint8_t* __restrict__ reversedOut, const int64_t* __restrict__ basePlace,
    const int64_t* __restrict__ opsPlace, int wantOps, uint8_t* __restrict__ arena) {
  __shared__ dnas::SimThresholds th;
  {
    const uint32_t* src = (const uint32_t*)thGlobal;
    uint32_t* dst = (uint32_t*)&th;
    for (unsigned w = threadIdx.x; w < sizeof(dnas::SimThresholds) / 4; w += blockDim.x) dst[w] = src[w];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kSimWavesPerBlock + (threadIdx.x >> 6), nWaves = (int64_t)gridDim.x * kSimWavesPerBlock;

  for (int64_t q = wave; q < count; q += nWaves) {
    const int64_t r = first + q;
    const int64_t s = readStrand[r];
    const int8_t* in = strands + strandOff[s];
    const int64_t I = strandOff[s + 1] - strandOff[s];
    const uint64_t index = readIndex[r];
    dnas::SimDraws perRead(seed, index, dnas::kSimPerRead);
    const bool reversed = perRead.draw(0) < th.reverseProb;
    int64_t bp = 0, opl = 0;
    uint32_t len = 0, nOps = 0;
    if (WRITE) {
      bp = basePlace[r], opl = opsPlace[r];
      if (bp == kSimSkip) continue;                      // (wave-uniform)
      len = totals[2 * r], nOps = totals[2 * r + 1];
    }
    uint32_t runBases = 0, runOps = 0;
    unsigned carry = 0;
    for (int64_t c0 = 0; c0 <= I; c0 += 64) {
      const int64_t ip = c0 + lane;
      const bool active = ip <= I;
      dnas::SimDraws d(seed, index, (uint32_t)ip);
      SimLane me;
      bool opens = false, ext = false;
      if (active) {
        ext = dnas::simExtend(th, d, ip, I);
        opens = dnas::simPosition(th, d, in, ip, I, [&](int base, uint8_t op) {
          if (base >= 0) ++me.bases, me.lastBase = base;
          ++me.ops, me.lastOp = op;
        });
      }
      unsigned carryOut;
      const uint64_t inD = dnas::simEntryBits(__ballot(opens), __ballot(ext), carry, &carryOut);
      carry = carryOut;
      const bool swallowed = ext && ((inD >> lane) & 1);
      if (swallowed) me.bases = 0, me.ops = 1, me.lastOp = dnas::kSimOpDelete;
      uint32_t incl = me.bases | me.ops << 16;
#pragma unroll
      for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const uint32_t up = __shfl_up(incl, dlt);
        if (lane >= dlt) incl += up;
      }
      const uint32_t total = __shfl(incl, 63);
      if (WRITE) {
        uint32_t pb = runBases + (incl & 0xFFFFu) - me.bases, po = runOps + (incl >> 16) - me.ops;
        auto put = [&](int base, uint8_t op) {
          if (base >= 0) {
            if (pb < len) arena[bp + (reversed ? len - 1 - pb : pb)] = (uint8_t)(reversed ? 3 - base : base);
            ++pb;
          }
          if (wantOps && po < nOps) arena[opl + po] = op;
          ++po;
        };
        if (me.ops == 1) put(me.bases ? me.lastBase : -1, me.lastOp);
        else if (me.ops > 1) (void)dnas::simPosition(th, d, in, ip, I, put);
      }
      runBases += total & 0xFFFFu;
      runOps += total >> 16;
    }
    if (!WRITE && lane == 0) {
      totals[2 * r] = runBases;
      totals[2 * r + 1] = runOps;
      reversedOut[r] = reversed ? 1 : 0;
    }
  }
}

template <bool WRITE>
__global__ __launch_bounds__(64 * kSimWavesPerBlock) void simulate_thread_kernel(
    const dnas::SimThresholds* __restrict__ thGlobal, uint64_t seed, int64_t first, int64_t count, const int8_t* __restrict__ strands,
    const int64_t* __restrict__ strandOff, const int64_t* __restrict__ readStrand, const uint64_t* __restrict__ readIndex,
    uint32_t* __restrict__ totals, uint8_t* __restrict__ reversedOut, const int64_t* __restrict__ basePlace,
    const int64_t* __restrict__ opsPlace, int wantOps, uint8_t* __restrict__ arena) {
  __shared__ dnas::SimThresholds th;
  {
    const uint32_t* src = (const uint32_t*)thGlobal;
    uint32_t* dst = (uint32_t*)&th;
    for (unsigned w = threadIdx.x; w < sizeof(dnas::SimThresholds) / 4; w += blockDim.x) dst[w] = src[w];
  }
  __syncthreads();
  const int64_t nThreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += nThreads) {
    const int64_t r = first + q;
    const int64_t s = readStrand[r];
    const int8_t* in = strands + strandOff[s];
    const int64_t I = strandOff[s + 1] - strandOff[s];
    const uint64_t index = readIndex[r];
    dnas::SimDraws perRead(seed, index, dnas::kSimPerRead);
    const bool reversed = perRead.draw(0) < th.reverseProb;
    int64_t bp = 0, opl = 0;
    uint32_t len = 0, nOps = 0;
    if (WRITE) {
      bp = basePlace[r], opl = opsPlace[r];
      if (bp == kSimSkip) continue;
      len = totals[2 * r], nOps = totals[2 * r + 1];
    }
    uint32_t pb = 0, po = 0;
    auto emit = [&](int base, uint8_t op) {
      if (base >= 0) {
        if (WRITE && pb < len) arena[bp + (reversed ? len - 1 - pb : pb)] = (uint8_t)(reversed ? 3 - base : base);
        ++pb;
      }
      if (WRITE && wantOps && po < nOps) arena[opl + po] = op;
      ++po;
    };
    bool inDel = false;
    for (int64_t ip = 0; ip <= I; ++ip) {
      dnas::SimDraws d(seed, index, (uint32_t)ip);
      if (inDel && dnas::simExtend(th, d, ip, I)) {
        emit(-1, dnas::kSimOpDelete);
        continue;
      }
      inDel = dnas::simPosition(th, d, in, ip, I, emit);
    }
    if (!WRITE) {
      totals[2 * r] = pb;
      totals[2 * r + 1] = po;
      reversedOut[r] = reversed ? 1 : 0;
    }
  }
}

template <class T>
using Malloced = std::unique_ptr<T, decltype(&free)>;

template <class T>
Malloced<T> mallocOf(size_t n) {
  Malloced<T> p((T*)malloc((n ? n : 1) * sizeof(T)), &free);
  if (!p) throw std::bad_alloc();
  return p;
}

// One device's result: its reads in the order they were given.
struct SimShard {
  Malloced<int8_t> seqs{nullptr, &free};
  Malloced<uint8_t> ops{nullptr, &free};
  std::vector<int64_t> off, opsOff;                      // n + 1 each
  std::vector<uint8_t> reversed, status;
  dnas_simulate_stats stats{};
};

bool simThreadPerRead() {
  const char* s = getenv("DNAS_SIMULATE_THREAD_PER_READ");
  return s && atoi(s) != 0;
}

unsigned simBlocks(int cus, int64_t count) {
  const int64_t perBlock = simThreadPerRead() ? 64 * kSimWavesPerBlock : kSimWavesPerBlock;   // reads a work-group takes at a time
  int64_t blocks = std::min<int64_t>((int64_t)cus * 8, (count + perBlock - 1) / perBlock);
  if (const char* s = getenv("DNAS_SIMULATE_BLOCKS")) blocks = std::min<int64_t>(blocks, atoll(s));
  return (unsigned)std::max<int64_t>(blocks, 1);
}

// One device's share: n reads, read q of strand readStrand[q] with the global index readIndex[q].
int simulateOn(int device, const dnas::SimThresholds& th, uint64_t seed, int64_t n_strands, const int8_t* strand_seqs, const int64_t* strand_off,
               int64_t n, const int64_t* readStrand, const uint64_t* readIndex, int wantOps, size_t arena_bytes, SimShard* out) {
  out->off.assign((size_t)n + 1, 0);
  out->opsOff.assign((size_t)n + 1, 0);
  out->reversed.assign((size_t)n, 0);
  out->status.assign((size_t)n, DNAS_SIM_OK);
  out->seqs = mallocOf<int8_t>(0);
  out->ops = mallocOf<uint8_t>(0);
  if (n == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipSetDevice(device));
  PaBuffers bufs;
  int rc, cus = 256;
  if ((rc = bufs.open())) return rc;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);

  dnas::SimThresholds* dTh = nullptr;
  int8_t* dStrands = nullptr;
  int64_t *dStrandOff = nullptr, *dReadStrand = nullptr, *dBasePlace = nullptr, *dOpsPlace = nullptr;
  uint64_t* dReadIndex = nullptr;
  uint32_t* dTotals = nullptr;
  uint8_t *dReversed = nullptr, *dArena = nullptr;
  if ((rc = paUpload(bufs, &dTh, &th, 1))) return rc;
  if ((rc = paUpload(bufs, &dStrands, strand_seqs, (size_t)strand_off[n_strands]))) return rc;
  if ((rc = paUpload(bufs, &dStrandOff, strand_off, (size_t)n_strands + 1))) return rc;
  if ((rc = paUpload(bufs, &dReadStrand, readStrand, (size_t)n))) return rc;
  if ((rc = paUpload(bufs, &dReadIndex, readIndex, (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dTotals, 2 * (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dReversed, (size_t)n))) return rc;

  // pass 1: every read's totals
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
  const bool threadPerRead = simThreadPerRead();
  hipLaunchKernelGGL(threadPerRead ? simulate_thread_kernel<false> : simulate_kernel<false>, dim3(simBlocks(cus, n)), dim3(64 * kSimWavesPerBlock), 0, bufs.stream, dTh, seed, (int64_t)0, n,
                     dStrands, dStrandOff, dReadStrand, dReadIndex, dTotals, dReversed, (const int64_t*)nullptr, (const int64_t*)nullptr,
                     wantOps, (uint8_t*)nullptr);
  DNAS_HIP_TRY(hipGetLastError());
  DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
  DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
  float ms = 0;
  DNAS_HIP_TRY(hipEventElapsedTime(&ms, bufs.ev[0], bufs.ev[1]));
  out->stats.count_ms = ms;
  std::vector<uint32_t> totals(2 * (size_t)n);
  DNAS_HIP_TRY(hipMemcpy(totals.data(), dTotals, totals.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out->reversed.data(), dReversed, (size_t)n, hipMemcpyDeviceToHost));

  // the arena, the batches of consecutive reads it takes, and every read's place in its batch: the bases of a batch first, then
  // its ops.  A read whose bytes alone exceed the arena is skipped inside its batch.
  auto need = [&](int64_t q) { return (size_t)totals[2 * (size_t)q] + (wantOps ? (size_t)totals[2 * (size_t)q + 1] : 0); };
  size_t total = 0;
  for (int64_t q = 0; q < n; ++q) total += need(q);
  size_t arena;
  if (arena_bytes) {
    arena = arena_bytes;
  } else {
    size_t freeB = 0, totalB = 0;
    DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
    arena = freeB / 2;
  }
  arena = std::min(arena, total);
  std::vector<int64_t> basePlace((size_t)n), opsPlace((size_t)n);
  struct Batch { int64_t first, last; size_t bases, ops; };
  std::vector<Batch> batches;
  {
    Batch b{0, 0, 0, 0};
    auto close = [&](int64_t last) {
      b.last = last;
      for (int64_t q = b.first; q < last; ++q)
        if (basePlace[(size_t)q] != kSimSkip) opsPlace[(size_t)q] += (int64_t)b.bases;
      if (b.bases + b.ops > 0) batches.push_back(b);
      b = Batch{last, last, 0, 0};
    };
    for (int64_t q = 0; q < n; ++q) {
      const size_t w = need(q);
      if (w > arena) {
        basePlace[(size_t)q] = kSimSkip, opsPlace[(size_t)q] = kSimSkip;
        out->status[(size_t)q] = DNAS_SIM_TOO_LARGE;
        ++out->stats.reads_too_large;
        totals[2 * (size_t)q] = totals[2 * (size_t)q + 1] = 0;
        continue;
      }
      if (b.bases + b.ops + w > arena) close(q);
      basePlace[(size_t)q] = (int64_t)b.bases, opsPlace[(size_t)q] = (int64_t)b.ops;
      b.bases += totals[2 * (size_t)q];
      if (wantOps) b.ops += totals[2 * (size_t)q + 1];
    }
    close(n);
  }
  for (int64_t q = 0; q < n; ++q) {
    out->off[(size_t)q + 1] = out->off[(size_t)q] + totals[2 * (size_t)q];
    out->opsOff[(size_t)q + 1] = out->opsOff[(size_t)q] + (wantOps ? totals[2 * (size_t)q + 1] : 0);
    out->stats.bases_in += strand_off[readStrand[q] + 1] - strand_off[readStrand[q]];
  }
  out->stats.bases_out = out->off[(size_t)n];
  out->stats.ops = out->opsOff[(size_t)n];
  out->seqs = mallocOf<int8_t>((size_t)out->off[(size_t)n]);
  out->ops = mallocOf<uint8_t>((size_t)out->opsOff[(size_t)n]);
  if (batches.empty()) return DNAS_OK;
  if ((rc = paUpload(bufs, &dBasePlace, basePlace.data(), (size_t)n))) return rc;
  if ((rc = paUpload(bufs, &dOpsPlace, opsPlace.data(), (size_t)n))) return rc;
  if ((rc = paAlloc(bufs, &dArena, arena))) return rc;

  // pass 2, batch by batch
  for (const Batch& b : batches) {
    const int64_t cnt = b.last - b.first;
    DNAS_HIP_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
    hipLaunchKernelGGL(threadPerRead ? simulate_thread_kernel<true> : simulate_kernel<true>, dim3(simBlocks(cus, cnt)), dim3(64 * kSimWavesPerBlock), 0, bufs.stream, dTh, seed, b.first, cnt,
                       dStrands, dStrandOff, dReadStrand, dReadIndex, dTotals, dReversed, dBasePlace, dOpsPlace, wantOps, dArena);
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
    DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
    DNAS_HIP_TRY(hipEventElapsedTime(&ms, bufs.ev[0], bufs.ev[1]));
    out->stats.write_ms += ms;
    ++out->stats.batches;
    if (b.bases) DNAS_HIP_TRY(hipMemcpy(out->seqs.get() + out->off[(size_t)b.first], dArena, b.bases, hipMemcpyDeviceToHost));
    if (b.ops) DNAS_HIP_TRY(hipMemcpy(out->ops.get() + out->opsOff[(size_t)b.first], dArena + b.bases, b.ops, hipMemcpyDeviceToHost));
  }
  return DNAS_OK;
}

template <class T>
T* copyOut(const std::vector<T>& v) {
  Malloced<T> p = mallocOf<T>(v.size());
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p.release();
}

}  // namespace

extern "C" int dnas_simulate_reads(const dnas_mutator_params* params, int64_t n_strands, const int8_t* strand_seqs, const int64_t* strand_off,
                                   int64_t n_reads, const int64_t* read_strand, uint64_t seed, uint64_t first_index, double reverse_prob,
                                   int want_ops, int device_id, size_t arena_bytes, int8_t** out_seqs, int64_t** out_off,
                                   uint8_t** out_reversed, uint8_t** out_ops, int64_t** out_ops_off, uint8_t* out_status,
                                   dnas_simulate_stats* out_stats) {
  if (out_stats) *out_stats = dnas_simulate_stats{};
  if (const int rc = dnas::checkSimulateArgs(params, n_strands, strand_seqs, strand_off, n_reads, read_strand, reverse_prob, want_ops, out_seqs,
                                             out_off, out_reversed, out_ops, out_ops_off, out_status))
    return rc;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    const dnas::SimThresholds th = dnas::SimThresholds::from(*params, reverse_prob);
    const int8_t none = 0;
    const int64_t noOff[1] = {0};
    if (n_strands == 0) strand_seqs = &none, strand_off = noOff;   // (then there is no read either)
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = n_reads == 0 ? 1 : devices.size();
    std::vector<std::vector<int64_t>> shard(W);
    if (W == 1) {
      shard[0].resize((size_t)n_reads);
      for (int64_t r = 0; r < n_reads; ++r) shard[0][(size_t)r] = r;
    } else {
      std::vector<int64_t> cost((size_t)n_reads);
      for (int64_t r = 0; r < n_reads; ++r) cost[(size_t)r] = 1 + strand_off[read_strand[r] + 1] - strand_off[read_strand[r]];
      shard = dnas::snakeDeal(cost, W);
    }
    std::vector<SimShard> part(W);
    const int rc = dnas::forEachDevice(std::vector<int>(devices.begin(), devices.begin() + (long)W), [&](size_t w) {
      const std::vector<int64_t>& mine = shard[w];
      std::vector<int64_t> strandOf(mine.size() + 1);
      std::vector<uint64_t> index(mine.size() + 1);
      for (size_t j = 0; j < mine.size(); ++j) strandOf[j] = read_strand[mine[j]], index[j] = first_index + (uint64_t)mine[j];
      return simulateOn(devices[w], th, seed, n_strands, strand_seqs, strand_off, (int64_t)mine.size(), strandOf.data(), index.data(), want_ops,
                        arena_bytes, &part[w]);
    });
    if (rc) return rc;

    dnas_simulate_stats st{};
    for (const SimShard& p : part) {
      st.count_ms = std::max(st.count_ms, p.stats.count_ms);
      st.write_ms = std::max(st.write_ms, p.stats.write_ms);
      st.batches += p.stats.batches, st.bases_in += p.stats.bases_in, st.bases_out += p.stats.bases_out, st.ops += p.stats.ops;
      st.reads_too_large += p.stats.reads_too_large;
    }
    st.devices = (int64_t)W;
    if (W == 1) {                                        // the shard is the result
      SimShard& p = part[0];
      Malloced<int64_t> off(copyOut(p.off), &free), opsOff(want_ops ? copyOut(p.opsOff) : nullptr, &free);
      Malloced<uint8_t> rev(copyOut(p.reversed), &free);
      if (n_reads) memcpy(out_status, p.status.data(), (size_t)n_reads);
      *out_seqs = p.seqs.release(), *out_off = off.release(), *out_reversed = rev.release();
      if (want_ops) *out_ops = p.ops.release(), *out_ops_off = opsOff.release();
    } else {                                             // the shards' reads go back to the caller's order
      std::vector<int64_t> off((size_t)n_reads + 1, 0), opsOff((size_t)n_reads + 1, 0);
      std::vector<uint8_t> rev((size_t)n_reads);
      for (size_t w = 0; w < W; ++w)
        for (size_t j = 0; j < shard[w].size(); ++j) {
          const size_t r = (size_t)shard[w][j];
          off[r + 1] = part[w].off[j + 1] - part[w].off[j], opsOff[r + 1] = part[w].opsOff[j + 1] - part[w].opsOff[j];
          rev[r] = part[w].reversed[j], out_status[r] = part[w].status[j];
        }
      for (int64_t r = 0; r < n_reads; ++r) off[(size_t)r + 1] += off[(size_t)r], opsOff[(size_t)r + 1] += opsOff[(size_t)r];
      Malloced<int8_t> seqs = mallocOf<int8_t>((size_t)off[(size_t)n_reads]);
      Malloced<uint8_t> ops = mallocOf<uint8_t>((size_t)opsOff[(size_t)n_reads]);
      for (size_t w = 0; w < W; ++w)
        for (size_t j = 0; j < shard[w].size(); ++j) {
          const size_t r = (size_t)shard[w][j];
          memcpy(seqs.get() + off[r], part[w].seqs.get() + part[w].off[j], (size_t)(off[r + 1] - off[r]));
          memcpy(ops.get() + opsOff[r], part[w].ops.get() + part[w].opsOff[j], (size_t)(opsOff[r + 1] - opsOff[r]));
        }
      Malloced<int64_t> offOut(copyOut(off), &free), opsOffOut(want_ops ? copyOut(opsOff) : nullptr, &free);
      Malloced<uint8_t> revOut(copyOut(rev), &free);
      *out_seqs = seqs.release(), *out_off = offOut.release(), *out_reversed = revOut.release();
      if (want_ops) *out_ops = ops.release(), *out_ops_off = opsOffOut.release();
    }
    if (out_stats) *out_stats = st;
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
