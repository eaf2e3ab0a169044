// The wavefront of the pair-HMM recurrences (host/pairalign.hpp, host/pairforward.hpp) and what the kernels that walk it share,
// stated once: the boundary row (PaBoundary), the base hand-over (PaBases), the wave prologue (paWaveBegin), the forward walk
// (paWalkForward) with the Viterbi cell that drives it (PaViterbiCell; the sum-product one is pair_forward_device.h's), the body of
// a score kernel (paScoreChunk), and on the host the launch plan, the dispatch on the number of duplication lengths, the chunk
// loop and the band-cell count.  Where a lane stands is pair_geom.h's.  Every Viterbi user is bit-identical to
// alignPairHost: pair_align_fill_kernel files a choice word per cell for the traceback, the score kernels keep S(I,O) only.
//
// A wave owns a pair.  The rows of the matrix are taken in stripes of 64: lane l owns row 64 s + l and is skewed one column
// per lane, at step t it stands on column c0 + t - l (c0: the first column of the stripe's band).  S and D of the row above
// are what lane l - 1 computed one step earlier (lane shuffle), the diagonal S what it computed two steps earlier (the value
// shuffled at the step before, kept); the duplication lanes T_0 .. T_{P-1} of (ip, op - 1) never leave the lane's registers,
// the output base travels down the lanes with the scores.  Lane 63's S and D go to a boundary row of O + 1 columns -- in LDS
// while that fits, else in the wave's scratch in HBM -- from which lane 0 of the next stripe reads them: any band width and
// the full matrix are served.  pair_counts_device.h walks the same stripes the other way.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "device_buffer.hpp"
#include "errors.hpp"
#include "host/pairalign.hpp"
#include "pair_geom.h"

namespace {

constexpr int kPaWavesPerBlock = 4;
constexpr int kPaLdsDoubles = 2048;                      // per wave: 16 substitution scores, then the boundary row
constexpr int kPaLdsCols = (kPaLdsDoubles - 16) / 2;     // columns (O + 1) a boundary row in LDS holds at most

struct PaScores {
  double delOpen, tanDup, noGap, delExtend, delEnd;
  double len[dnas::kAlignMaxLen];
  int P;
  static PaScores from(const dnas::PairScores& hs) {
    PaScores sc{};
    sc.delOpen = hs.delOpen; sc.tanDup = hs.tanDup; sc.noGap = hs.noGap; sc.delExtend = hs.delExtend; sc.delEnd = hs.delEnd;
    for (int k = 0; k < dnas::kAlignMaxLen; ++k) sc.len[k] = hs.len[k];
    sc.P = hs.P;
    return sc;
  }
};

__device__ inline double paNegInf() { return -__builtin_huge_val(); }

// The boundary row of a pair of O + 1 columns, S and D of a column side by side: ldsRow (of ldsCols columns) while the pair's
// fits there, else memRow, the wave's row in HBM, through relaxed agent-scope atomics.  One lane of a stripe stores, one lane of
// the next stripe loads, handOver() between the two.
struct PaBoundary {
  double *ldsRow, *memRow;
  bool useLds;
  __device__ PaBoundary(double* ldsRow_, int ldsCols, double* memRow_, int O) : ldsRow(ldsRow_), memRow(memRow_), useLds(O + 1 <= ldsCols) {}
  __device__ __forceinline__ double loadS(int op) const {
    return useLds ? ldsRow[2 * op] : __hip_atomic_load(memRow + 2 * (size_t)op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void load(int op, double& S, double& D) const {
    if (useLds) {
      S = ldsRow[2 * op];
      D = ldsRow[2 * op + 1];
    } else {
      S = __hip_atomic_load(memRow + 2 * (size_t)op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      D = __hip_atomic_load(memRow + 2 * (size_t)op + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __device__ __forceinline__ void store(int op, double S, double D) const {
    if (useLds) {
      ldsRow[2 * op] = S;
      ldsRow[2 * op + 1] = D;
    } else {
      __hip_atomic_store(memRow + 2 * (size_t)op, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(memRow + 2 * (size_t)op + 1, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __device__ __forceinline__ void handOver() const {
    if (useLds) __builtin_amdgcn_wave_barrier();
    else __threadfence();
  }
};

// One item of a walk: a[0..I) against b[0..O), or with rev against the reverse complement of b, read in place (base j of it
// is 3 - b[O-1-j]).
struct PaItem {
  const int8_t *a, *b;
  int I, O;
  bool rev;
};

// The base hand-over: the output bases a stripe's first lane feeds into the skew, 64 at a time.  At step u = 0, 1, .. of a stripe
// fetch(u, j0, dir, lane) has lane l load base j0 + dir * l every 64 steps (0 outside the read), and get(u) is the base that lane
// u & 63 loaded.  Forward j0 = c0 + t - 1 and dir = 1, backward j0 = c0 + t - last and dir = -1.  A walk calls fetch before its
// shuffles of S and D and get after them: with the base's shuffle issued first, every step's first wait covers one more LDS
// operation, which cost the sum-product walks 0.2 to 0.5 % (profiles/EXPERIMENTS.md).
struct PaBases {
  int chunk = 0;
  __device__ __forceinline__ void fetch(const PaItem& it, int u, int j0, int dir, int lane) {
    if ((u & 63) == 0) {
      const int j = j0 + dir * lane;
      chunk = j >= 0 && j < it.O ? (it.rev ? 3 - ((int)it.b[it.O - 1 - j] & 3) : (int)it.b[j] & 3) : 0;
    }
  }
  __device__ __forceinline__ int get(int u) const { return __shfl(chunk, u & 63); }
};

// The bases of the original a row compares with, packed: a[top - k] at bits 2k for k = 0 .. KP, 0 where a has no such base.
// top = r - 1 going forward (the match, then T_k's in[r-2-k]), r going back.
template <int KP>
__device__ __forceinline__ unsigned paContext(const PaItem& it, bool row, int top) {
  unsigned ctx = 0;
#pragma unroll
  for (int k = 0; k <= KP; ++k)
    if (row && top - k >= 0 && top - k < it.I) ctx |= ((unsigned)it.a[top - k] & 3u) << (2 * k);
  return ctx;
}

// The prologue of a kernel on this wavefront: which wave of the grid this is, its slice of the block's LDS (perWave doubles: the
// 16 substitution scores first, which are loaded here) and its boundary row in HBM.  The kernels with a body of their own call
// it; paScoreChunk keeps the same lines written out (see there).
struct PaWave {
  int lane;
  int64_t wave, nWaves;
  double *lds, *bndMem;
};

__device__ __forceinline__ PaWave paWaveBegin(double* lds, size_t perWave, const double* subTable, double* bndScratch, int64_t bndStride) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * kPaWavesPerBlock + wv, nWaves = (int64_t)gridDim.x * kPaWavesPerBlock;
  double* const sub = lds + (size_t)wv * perWave;
  if (lane < 16) sub[lane] = subTable[lane];
  __builtin_amdgcn_wave_barrier();
  return PaWave{lane, wave, nWaves, sub, bndScratch + wave * bndStride};
}

// The forward walk of one pair by the 64 lanes of one wave.  sub: the wave's 16 substitution scores in LDS.  For every cell of
// the band the lane that stands on it calls
//   cell.update<KP>(sc, sub, Sup, Dup, Sdiag, T, ctx, y, kmax, origin, s, t, r, op, S, D)
// with S and D of the row above, S of the diagonal, the lane's T_0 .. T_{KP-1} of (r, op - 1), the row's packed bases, the output
// base out[op-1], whether this is (0,0), and where it stands; the cell leaves S, D and T of (r, op).  The lane that stands on
// (I, O) writes S(I,O) to *scoreOut; that is every pair's last store.
template <int KP, class Cell>
__device__ __forceinline__ void paWalkForward(const PaScores& sc, const double* sub, const PaBoundary& bnd, int lane, int band,
                                              const PaItem& it, double* scoreOut, Cell& cell) {
  const double NEG = paNegInf();
  const int I = it.I, O = it.O;
  const PaGeom g(I, O, band);

  for (int s = 0; s < g.stripes; ++s) {
    const PaStripe st(g, I, O, sc.P, s, lane);
    const PaSpan up = st.above(g, O);
    const unsigned ctx = paContext<KP>(it, st.row, st.r - 1);
    double T[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) T[k] = NEG;
    double Sdiag = NEG, pubS = NEG, pubD = NEG;
    int ypub = 0;
    PaBases bases;
    if (lane == 0 && s > 0 && st.c0 >= 1) Sdiag = bnd.loadS(st.c0 - 1);

    for (int t = 0; t <= st.tmax; ++t) {
      bases.fetch(it, t, st.c0 + t - 1, 1, lane);
      double Sup = __shfl_up(pubS, 1), Dup = __shfl_up(pubD, 1);
      int y = __shfl_up(ypub, 1);
      const int y0 = bases.get(t);
      const int op = st.op(t);
      if (lane == 0) {
        y = y0;
        Sup = Dup = NEG;
        if (s > 0 && up.has(op)) bnd.load(op, Sup, Dup);
      }
      double S = NEG, D = NEG;
      if (st.active(op)) {
        cell.template update<KP>(sc, sub, Sup, Dup, Sdiag, T, ctx, y, st.kmax, st.r == 0 && op == 0, s, t, st.r, op, S, D);
        if (lane == 63) bnd.store(op, S, D);
        if (st.r == I && op == O) *scoreOut = S;
      }
      Sdiag = Sup;
      pubS = S;
      pubD = D;
      ypub = y;
    }
    bnd.handOver();      // the next stripe's lane 0 reads what this stripe's lane 63 wrote
  }
}

// The Viterbi cell: "best of" takes the candidates in the order host/pairalign.hpp lists them, the first strictly greater one
// wins.  RECORD: one 16-bit choice word per cell (bits 0-1: S took s0 / s1 / s2, bit 2: D took d1, bit 3 + k: T_k took t1) goes
// to rec, this lane's column of the pair's words, filed under (stripe, step, lane) as PaGeom::wordAt finds it: a wave's store is
// 128 consecutive bytes.
template <bool RECORD>
struct PaViterbiCell {
  uint16_t* rec = nullptr;
  int stepsMax = 0;
  template <int KP>
  __device__ __forceinline__ void update(const PaScores& sc, const double* sub, double Sup, double Dup, double Sdiag, double (&T)[KP],
                                         unsigned ctx, int y, int kmax, bool origin, int s, int t, int, int, double& S,
                                         double& D) const {
    const double NEG = paNegInf();
    S = D = NEG;
    unsigned word = 0;
    double c;
    c = Sup + sc.delOpen;
    if (c > D) D = c;
    c = Dup + sc.delExtend;
    if (c > D) { D = c; word = 4u; }
    if (origin) {
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
    if (RECORD) rec[((size_t)s * (size_t)stepsMax + (size_t)t) * 64] = (uint16_t)word;
  }
};

// One item of a score kernel under a cell of the shared walk; a cell on a body of its own overloads this (pair_forward_device.h).
template <int KP, class Cell>
__device__ __forceinline__ void paScorePair(const PaScores& sc, double* sub, int ldsCols, double* bndMem, int lane, int band,
                                            const PaItem& it, double* scoreOut, Cell& cell) {
  paWalkForward<KP>(sc, sub, PaBoundary(sub + 16, ldsCols, bndMem, it.O), lane, band, it, scoreOut, cell);
}

// The body of a score kernel: a wave owns an item and walks the chunk [first, first + count) with the grid's stride; the score
// of item first + q under the cell goes to chunk[q] and nothing else is stored.  itemAt(g) says which PaItem the call's item g
// is: that and the cell are all a score kernel states itself.  Dynamic LDS, per wave: 16 substitution scores, then ldsCols
// boundary columns.
template <int KP, class ItemAt, class Cell = PaViterbiCell<false>>
__device__ __forceinline__ void paScoreChunk(const PaScores& sc, const double* subTable, int band, int ldsCols, int64_t first,
                                             int64_t count, const ItemAt& itemAt, double* bndScratch, int64_t bndStride,
                                             double* chunk, Cell cell = Cell()) {
  extern __shared__ double lds[];
  // paWaveBegin's text, written out: through the call the KP = 13 sum-product instances spill 18 more SGPRs, 16 of them read back
  // in the step loop (profiles/EXPERIMENTS.md)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * kPaWavesPerBlock + wv, nWaves = (int64_t)gridDim.x * kPaWavesPerBlock;
  double* const sub = lds + (size_t)wv * (size_t)(16 + 2 * ldsCols);
  if (lane < 16) sub[lane] = subTable[lane];
  __builtin_amdgcn_wave_barrier();
  double* const bndMem = bndScratch + wave * bndStride;

  for (int64_t q = wave; q < count; q += nWaves) {
    const PaItem it = itemAt(first + q);
    paScorePair<KP>(sc, sub, ldsCols, bndMem, lane, band, it, chunk + q, cell);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct PaBuffers {
  dnas::DevPool mem;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int open() {                                           // the stream and the events, on the current device
    DNAS_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (hipEvent_t& e : ev) DNAS_HIP_TRY(hipEventCreate(&e));
    return DNAS_OK;
  }
  ~PaBuffers() {
    mem.reset();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

template <class T>
int paAlloc(PaBuffers& bufs, T** out, size_t n) {
  DNAS_HIP_TRY(bufs.mem.alloc(n, out));
  return DNAS_OK;
}

template <class T>
int paUpload(PaBuffers& bufs, T** out, const T* src, size_t n) {
  DNAS_HIP_TRY(bufs.mem.upload(src, n, out));
  return DNAS_OK;
}

// f(std::integral_constant<int, KP>) for the KP the kernels are built for that holds P duplication lengths.
template <class F>
auto paDispatchKP(int P, F&& f) {
  if (P <= 2) return f(std::integral_constant<int, 2>{});
  if (P <= 6) return f(std::integral_constant<int, 6>{});
  return f(std::integral_constant<int, 13>{});
}

// The grid of a kernel on this wavefront: a wave per item, at most perCu work-groups for each of cus CUs; DNAS_ALIGN_BLOCKS
// (testing aid) makes it smaller.  When the longest read's boundary row (maxO + 1 columns) does not fit LDS, every wave of the
// grid has one of bndStride doubles in HBM, and the grid is cut so that they stay within 1 GiB.
struct PaLaunchPlan {
  int maxBlocks = 1;
  int64_t bndStride = 0;
  int ldsCols = kPaLdsCols;                              // the score kernels': see paPlanScore
  size_t ldsBytes = 0;
  int64_t chunkItems = 0;
  void cut(int cus, int perCu, int maxO, int64_t items) {
    maxBlocks = (int)std::min<int64_t>((int64_t)cus * perCu, (items + kPaWavesPerBlock - 1) / kPaWavesPerBlock);
    if (const char* s = getenv("DNAS_ALIGN_BLOCKS")) maxBlocks = std::max(1, std::min(maxBlocks, atoi(s)));
    bndStride = maxO + 1 > kPaLdsCols ? 2 * ((int64_t)maxO + 1) : 0;
    if (bndStride) maxBlocks = (int)std::min<int64_t>(maxBlocks, ((int64_t)1 << 30) / (bndStride * 8 * kPaWavesPerBlock));
    maxBlocks = std::max(maxBlocks, 1);
  }
  unsigned blocks(int64_t count) const { return (unsigned)std::min<int64_t>((count + kPaWavesPerBlock - 1) / kPaWavesPerBlock, maxBlocks); }
  size_t bndDoubles() const { return (size_t)bndStride * (size_t)maxBlocks * kPaWavesPerBlock; }
};

// The plan of a score kernel over `total` items, kernelOf(kp) its instance for KP = kp().  A launch takes a chunk of 2^22 items
// (32 MiB of scores), fewer when the environment variable chunkEnv says so (testing aid).  Dynamic LDS is sized by the call's
// longest read: short reads leave room for more work-groups per CU, as many as the runtime says fit.
template <class KernelOf>
int paPlanScore(int P, KernelOf kernelOf, int cus, int maxO, const char* chunkEnv, int64_t total, PaLaunchPlan* plan) {
  plan->chunkItems = (int64_t)1 << 22;
  if (const char* s = getenv(chunkEnv)) plan->chunkItems = std::max<int64_t>(1, std::min<int64_t>(plan->chunkItems, atoll(s)));
  plan->chunkItems = std::max<int64_t>(1, std::min(plan->chunkItems, total));
  plan->ldsCols = std::min(maxO + 1, kPaLdsCols);
  plan->ldsBytes = (size_t)kPaWavesPerBlock * (size_t)(16 + 2 * plan->ldsCols) * sizeof(double);
  int perCu = 2;
  const hipError_t occupancyQuery = paDispatchKP(P, [&](auto kp) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernelOf(kp), 64 * kPaWavesPerBlock, plan->ldsBytes);
  });
  DNAS_HIP_TRY(occupancyQuery);
  plan->cut(cus, std::max(perCu, 1), maxO, plan->chunkItems);
  return DNAS_OK;
}

// [0, total) in the plan's chunks on t's stream: score(first, count) launches the score kernel into the chunk, fold(first, count)
// the kernel that folds the chunk into the call's state, after(first, count) enqueues what else needs the chunk before the next
// one overwrites it and returns its hipError_t.  HIP events around the two launches are summed into stats.
template <class Score, class Fold, class After, class Stats>
int paRunChunks(PaBuffers& t, int64_t total, int64_t chunkItems, Score&& score, Fold&& fold, After&& after, Stats* stats) {
  for (int64_t first = 0; first < total; first += chunkItems) {
    const int64_t count = std::min(chunkItems, total - first);
    DNAS_HIP_TRY(hipEventRecord(t.ev[0], t.stream));
    score(first, count);
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(t.ev[1], t.stream));
    fold(first, count);
    DNAS_HIP_TRY(hipGetLastError());
    DNAS_HIP_TRY(hipEventRecord(t.ev[2], t.stream));
    DNAS_HIP_TRY(after(first, count));
    DNAS_HIP_TRY(hipStreamSynchronize(t.stream));
    float scoreMs = 0, foldMs = 0;
    DNAS_HIP_TRY(hipEventElapsedTime(&scoreMs, t.ev[0], t.ev[1]));
    DNAS_HIP_TRY(hipEventElapsedTime(&foldMs, t.ev[1], t.ev[2]));
    stats->score_ms += scoreMs;
    stats->fold_ms += foldMs;
    ++stats->chunks;
  }
  return DNAS_OK;
}

// PairBand::cells per (I, O), evaluated once each: a call has few distinct lengths.  A table indexed by the two lengths while
// that is small (one load per item instead of a tree walk), else a map.
class PaCellMemo {
 public:
  PaCellMemo(int64_t maxI, int64_t maxO, int band)
      : band_(band), cols_(maxO + 1), table_((maxI + 1) * (maxO + 1) <= ((int64_t)1 << 22) ? (size_t)((maxI + 1) * (maxO + 1)) : 0, -1) {}
  int64_t cells(int64_t I, int64_t O) {
    if (!table_.empty()) {
      int64_t& slot = table_[(size_t)(I * cols_ + O)];
      if (slot < 0) slot = dnas::PairBand(I, O, band_).cells(I, O);
      return slot;
    }
    auto it = map_.find({I, O});
    if (it == map_.end()) it = map_.emplace(std::make_pair(I, O), dnas::PairBand(I, O, band_).cells(I, O)).first;
    return it->second;
  }

 private:
  int band_;
  int64_t cols_;
  std::vector<int64_t> table_;
  std::map<std::pair<int64_t, int64_t>, int64_t> map_;
};

}  // namespace
