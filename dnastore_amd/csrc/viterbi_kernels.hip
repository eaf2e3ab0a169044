// Hand-written gfx950 kernels for the Viterbi error decoder.
//
//   viterbi_fill_kernel       replaces the ViterbiMatrix constructor's lattice fill
//                             (reference src/viterbi.cpp:62-176)
//   viterbi_traceback_kernel  replaces ViterbiMatrix::traceback (src/viterbi.cpp:195-304)
//
// One work-group per read.  The lattice lives in HBM as [pos][lane][state] fp64
// (lanes S, D, T1..TD; the reference's AoS [pos][state][lane], viterbi.h:65-67, turned
// SoA so that every lane of a column is one coalesced stream).  The current column's S
// and D rows double as the working storage of the in-column max-plus fixpoint.
//
// All arithmetic is fp64 max/+ in the reference's operand order; no contraction, no
// fast-math (build with -ffp-contract=off).  max() is spelled (a < b ? b : a) == std::max.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "traceback_step.h"

namespace {

__device__ __forceinline__ double dmax(double a, double b) { return a < b ? b : a; }

constexpr double kNegInf = -__builtin_huge_val();

// Pull relaxation of one state inside the current column (the body of the reference's
// worklist loop, viterbi.cpp:112-158, seen from the destination side):
//   D(j) = max( D(j), max(D(src)+delExtend, S(src)+delOpen) + score   over emit-in,
//                     D(src)+score                                    over null-in )
//   S(j) = max( S(j), S(src)+score over null-in, D(j)+delEnd )
// Returns true when either cell grew.
__device__ __forceinline__ bool pull_state(const DevModel& m, int j, double* __restrict__ S, double* __restrict__ D) {
  const double d0 = D[j], s0 = S[j];
  double d = d0, s = s0;
  const int eb = m.einPtr[j], ee = m.einPtr[j + 1];
  for (int e = eb; e < ee; ++e) {
    const int src = m.einSrc[e];
    const double cand = dmax(D[src] + m.delExtend, S[src] + m.delOpen) + m.einScore[e];
    d = dmax(d, cand);
  }
  const int nb = m.ninPtr[j], ne = m.ninPtr[j + 1];
  for (int e = nb; e < ne; ++e) {
    const int src = m.ninSrc[e];
    const double sc = m.ninScore[e];
    d = dmax(d, D[src] + sc);
    s = dmax(s, S[src] + sc);
  }
  s = dmax(s, d + m.delEnd);
  bool grew = false;
  if (d > d0) { D[j] = d; grew = true; }
  if (s > s0) { S[j] = s; grew = true; }
  return grew;
}

// Mark every out-neighbour of j dirty for the next round.
__device__ __forceinline__ void mark_successors(const DevModel& m, int j, unsigned* maskNext) {
  const int eb = m.eoutPtr[j], ee = m.eoutPtr[j + 1];
  for (int e = eb; e < ee; ++e) {
    const int d = m.eoutDst[e];
    atomicOr(&maskNext[d >> 5], 1u << (d & 31));
  }
  const int nb = m.noutPtr[j], ne = m.noutPtr[j + 1];
  for (int e = nb; e < ne; ++e) {
    const int d = m.noutDst[e];
    atomicOr(&maskNext[d >> 5], 1u << (d & 31));
  }
}

__device__ __forceinline__ int slot_of(const DevModel& m, int st) { return m.slotOf ? m.slotOf[st] : st; }

// A cell that is in memory: S and D always, the duplication lanes where storedLanes > 2.
__device__ __forceinline__ double stored_cell(const DevModel& m, const double* __restrict__ lat, int slot, int ps, int ln) {
  return lat[((size_t)ps * m.storedLanes + (size_t)ln) * (size_t)m.Npad + (size_t)slot];
}

// One lattice cell of a state in lattice slot `slot`, whatever the storage tier.  With storedLanes == 2 the duplication
// lanes are not in memory; T(p,q) = max(T(p-1,q+1) + sub[ctx[q+1]][x_p], (S(p)+tanDup)+len[q]),
// T(0,.) = -inf (viterbi.cpp:105-106,161-168) is rebuilt from the state's own S cells, deepest
// element first -- the same fp64 operations in the same order as the fill, hence the same bits.
__device__ __forceinline__ double cell_at(const DevModel& m, const double* __restrict__ lat, const uint8_t* __restrict__ seq,
                                          int st, int slot, int ps, int ln) {
  const size_t stride = (size_t)m.Npad;
  if (ln < 2 || m.storedLanes > 2) return stored_cell(m, lat, slot, ps, ln);
  const int k = ln - 2, mdl = m.mdl[st];
  if (ps < 1 || k >= mdl) return kNegInf;
  const uint8_t* ctx = m.ctx + (size_t)st * m.D;
  int I = mdl - 1 - k;
  if (ps - 1 < I) I = ps - 1;
  double v = (lat[((size_t)(ps - I) * 2) * stride + (size_t)slot] + m.tanDup) + m.len[k + I];
  for (int i = I - 1; i >= 0; --i) {
    const int p = ps - i, q = k + i;
    v = dmax(v + m.sub[ctx[q + 1] * 4 + seq[p - 1]], (lat[((size_t)p * 2) * stride + (size_t)slot] + m.tanDup) + m.len[q]);
  }
  return v;
}

// Duplication lane k of a state at column ps from the state's node record (traceback_step.h: mdl, the context's bases 2 bits each,
// the lattice slot): cell_at's chain for at most four S cells (records exist for D <= 4), every one of them loaded before
// the chain is evaluated -- a loop over them would wait for each load in turn.  SL = lanes stored per column.
__device__ __forceinline__ double dup_cell_from_record(const double* __restrict__ lat, const uint8_t* __restrict__ seq, size_t SL, size_t stride,
                                                       int slot, int mdl, unsigned ctxBits, int ps, int k, double tanDup,
                                                       const double* subT, const double* lenT) {
  if (SL > 2) return lat[((size_t)ps * SL + (size_t)(2 + k)) * stride + (size_t)slot];
  if (ps < 1 || k >= mdl) return kNegInf;
  int I = mdl - 1 - k;
  if (ps - 1 < I) I = ps - 1;
  double sv[4];
  int xb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sv[i] = i <= I ? lat[((size_t)(ps - i) * SL) * stride + (size_t)slot] : 0.;
    xb[i] = i < I ? (int)seq[ps - i - 1] : 0;
  }
  double v = kNegInf;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    if (i == I) v = (sv[i] + tanDup) + lenT[k + i];
    else if (i < I) v = dmax(v + subT[((ctxBits >> (2 * (k + i + 1))) & 3u) * 4 + xb[i]], (sv[i] + tanDup) + lenT[k + i]);
  }
  return v;
}

}  // namespace

// Device-side guard of dnas_viterbi_batch_device: counts base codes outside 0..3.
extern "C" __global__ void check_bases_kernel(const uint8_t* __restrict__ bases, size_t n, unsigned long long* __restrict__ bad) {
  unsigned mine = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) mine += bases[i] > 3;
  if (mine) atomicAdd(bad, (unsigned long long)mine);
}

// -inf into every cell of the tier-C exchange buffers before a launch.
// Where should a cluster's sync words sit?  The members of a cluster agree on every lattice column through device-scope
// atomics and loads on a few words (viterbi_tiera.hip): operations performed at the memory side, whose round trip from an XCD
// depends on which memory channel the address belongs to (measured on MI355X: one ~980-nt read of the 46 670-state machine on
// 16 work-groups fills in 41.6 ms with its sync block at one address and in 54 ms 4 KB further on, same box, same process).
// Block b of this kernel (b = 0 .. 7: the XCD that block b, b + 8, ... of a launch are dispatched to) times `reps` dependent
// atomic round trips to each of nCand candidate addresses, pool + k * strideWords, and files the ticks under out[b * nCand + k].
extern "C" __global__ void sync_latency_kernel(unsigned* __restrict__ pool, int nCand, int strideWords, int reps,
                                               unsigned long long* __restrict__ out, unsigned* __restrict__ xccOut) {
  if (threadIdx.x != 0) return;
  const int b = (int)blockIdx.x;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xccOut[b] = xcc & 15u;
  for (int i = 0; i < nCand; ++i) {
    const int k = (i + b * 5) % nCand;      // (the blocks walk the candidates out of step)
    unsigned* const p = pool + (size_t)k * (size_t)strideWords;
    unsigned dep = __hip_atomic_fetch_add(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // warm: page tables, the line
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int r = 0; r < reps; ++r) dep = __hip_atomic_fetch_add(p + (dep & 0u), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t1 = __builtin_readcyclecounter();
    out[(size_t)b * nCand + k] = t1 - t0 + (dep & 0u);
  }
}

// Which XCD is next in the dispatcher's round?  (One block: the first block of the kernel launched right behind this one goes to
// the same XCD -- observed; a matter of speed only.)
extern "C" __global__ void xcc_probe_kernel(unsigned* __restrict__ out) {
  if (threadIdx.x != 0) return;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  *out = xcc & 15u;
}

extern "C" __global__ void fill_neginf_kernel(double* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = kNegInf;
}

// Bounded-memory decode: `n` doubles from src + row * srcStride to dst + row * dstStride for every row (one row per read
// of the group).  grid = (chunks, rows).
extern "C" __global__ void copy_rows_kernel(double* __restrict__ dst, const double* __restrict__ src, size_t dstStride,
                                            size_t srcStride, size_t n) {
  const double* s = src + (size_t)blockIdx.y * srcStride;
  double* d = dst + (size_t)blockIdx.y * dstStride;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// Test/diagnostic aid: the full (D+2)-lane lattice of one read in reference state order,
// out[(pos*(D+2)+lane)*N + state], whatever the storage tier.  grid = L+1, any block size.
extern "C" __global__ void expand_lattice_kernel(DevModel m, const uint8_t* __restrict__ seq, const double* __restrict__ lat,
                                                 double* __restrict__ out) {
  const int ps = blockIdx.x, lanes = m.D + 2, L = (int)gridDim.x - 1;
  for (int st = threadIdx.x; st < m.N; st += blockDim.x)
    for (int ln = 0; ln < lanes; ++ln) {
      double v = cell_at(m, lat, seq, st, slot_of(m, st), ps, ln);
      if (m.local && m.storedLanes == 2 && ln >= 2 && ps == L && st == m.N - 1 && L >= 1) {
        // local mode: the reference formed T(N-1, L, .) from S(N-1, L) BEFORE overwriting that cell with the
        // column maximum (viterbi.cpp:161-173); the fill kernel kept the earlier value behind the lattice
        const int k = ln - 2, mdl = m.mdl[st];
        if (k < mdl) {
          const double s0 = lat[(size_t)(L + 1) * 2 * (size_t)m.Npad];
          const double opened = (s0 + m.tanDup) + m.len[k];
          // T(L,k) = max( T(L-1,k+1) + sub[ctx[k+1]][x_L],  opened ):  the first term does not involve S(L)
          double shifted = kNegInf;
          if (k + 1 < mdl) shifted = cell_at(m, lat, seq, st, slot_of(m, st), ps - 1, ln + 1) + m.sub[m.ctx[(size_t)st * m.D + k + 1] * 4 + seq[ps - 1]];
          v = dmax(shifted, opened);
        }
      }
      out[((size_t)ps * lanes + ln) * m.N + st] = v;
    }
}

// grid = reads in this batch, block = kFillThreads.
// Dynamic LDS: two dirty-state bitmasks of maskWords 32-bit words each.
extern "C" __global__ void __launch_bounds__(kFillThreads)
viterbi_fill_kernel(DevModel m, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ readOff,
                    const int32_t* __restrict__ batchRead, const uint64_t* __restrict__ slotOff,
                    double* __restrict__ arena, double* __restrict__ outLoglike,
                    unsigned long long* __restrict__ roundsTotal, int maskWords,
                    const int* __restrict__ colRange) {   // [reads][2] first and last column to fill (bounded-memory decode), or null: 0 .. L
  extern __shared__ unsigned ldsMask[];
  __shared__ double redBuf[kFillThreads / 64];
  const int tid = threadIdx.x;
  const int T = blockDim.x;
  const int N = m.N, D_ = m.D, lanes = m.D + 2;
  const size_t Npad = (size_t)m.Npad;
  const int read = batchRead[blockIdx.x];
  const uint8_t* seq = bases + readOff[read];
  const int L = (int)(readOff[read + 1] - readOff[read]);
  double* lat = arena + slotOff[blockIdx.x];
  unsigned* mask0 = ldsMask;
  unsigned* mask1 = ldsMask + maskWords;
  const int maskBytes = (N + 7) >> 3;
  unsigned rounds = 0;

  for (int w = tid; w < 2 * maskWords; w += T) ldsMask[w] = 0;
  __syncthreads();

  // a segment c0 .. c1 of the read: the column before c0 is in the lattice (every lane is stored in this tier)
  int c0 = 0, c1 = L;
  if (colRange) { c0 = colRange[2 * blockIdx.x]; c1 = colRange[2 * blockIdx.x + 1]; }
  for (int pos = c0; pos <= c1; ++pos) {
    double* col = lat + (size_t)pos * lanes * Npad;
    double* S = col;
    double* Dc = col + Npad;
    const double* prev = col - (size_t)lanes * Npad;  // valid for pos > 0
    const int x = pos > 0 ? seq[pos - 1] : 0;

    // ---- phase A: S from the previous column (viterbi.cpp:92-95,101-103); D = -inf
    for (int j = tid; j < N; j += T) {
      double s;
      if (pos == 0) {
        s = (m.local || j == 0) ? 0. : kNegInf;  // viterbi.cpp:75-79
      } else {
        s = kNegInf;
        const int eb = m.einPtr[j], ee = m.einPtr[j + 1];
        for (int e = eb; e < ee; ++e)
          s = dmax(s, ((prev[m.einSrc[e]] + m.einScore[e]) + m.noGap) + m.sub[m.einBase[e] * 4 + x]);
        if (m.mdl[j] > 0) s = dmax(s, prev[2 * Npad + j] + m.sub[m.ctx[(size_t)j * D_] * 4 + x]);
      }
      S[j] = s;
      Dc[j] = kNegInf;
    }
    __syncthreads();

    // ---- phase B: in-column fixpoint (viterbi.cpp:97-99,110-159).  Round 1 visits every
    // state (the reference seeds its worklist with all of them); later rounds visit the
    // states whose predecessors grew.  Monotone max-plus => the least fixpoint reached is
    // independent of the visiting order.
    unsigned* cur = mask0;
    unsigned* nxt = mask1;
    {
      int marked = 0;
      for (int j = tid; j < N; j += T)
        if (pull_state(m, j, S, Dc)) { mark_successors(m, j, nxt); marked = 1; }
      ++rounds;
      int more = __syncthreads_or(marked);
      while (more) {
        unsigned* t = cur; cur = nxt; nxt = t;
        marked = 0;
        uint8_t* curBytes = reinterpret_cast<uint8_t*>(cur);
        for (int b = tid; b < maskBytes; b += T) {
          unsigned bits = curBytes[b];
          if (!bits) continue;
          curBytes[b] = 0;
          while (bits) {
            const int j = (b << 3) + __builtin_ctz(bits);
            bits &= bits - 1;
            if (pull_state(m, j, S, Dc)) { mark_successors(m, j, nxt); marked = 1; }
          }
        }
        ++rounds;
        more = __syncthreads_or(marked);
      }
    }

    // ---- phase C: duplication lanes (viterbi.cpp:105-106,161-168)
    for (int j = tid; j < N; j += T) {
      const double s = S[j];
      const int mdl = m.mdl[j];
      for (int k = 0; k < D_; ++k) {
        double t = kNegInf;
        if (pos > 0 && k < mdl) {
          if (k < mdl - 1) t = prev[(size_t)(3 + k) * Npad + j] + m.sub[m.ctx[(size_t)j * D_ + k + 1] * 4 + x];
          t = dmax(t, (s + m.tanDup) + m.len[k]);
        }
        col[(size_t)(2 + k) * Npad + j] = t;
      }
    }
    __syncthreads();
  }

  if (c1 < L) {   // not the read's last segment: no log-likelihood yet
    if (tid == 0) atomicAdd(roundsTotal, (unsigned long long)rounds);
    return;
  }
  // ---- local mode: loglike = best end state (viterbi.cpp:171-173)
  double* lastS = lat + (size_t)L * lanes * Npad;
  if (m.local) {
    double best = kNegInf;
    for (int j = tid; j < N; j += T) best = dmax(best, lastS[j]);
    for (int off = 32; off > 0; off >>= 1) best = dmax(best, __shfl_down(best, off, 64));
    if ((tid & 63) == 0) redBuf[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < T / 64; ++w) best = dmax(best, redBuf[w]);
      lastS[N - 1] = best;
      outLoglike[read] = best;
    }
  } else if (tid == 0) {
    outLoglike[read] = lastS[N - 1];
  }
  if (tid == 0) atomicAdd(roundsTotal, (unsigned long long)rounds);
}

// ---------------------------------------------------------------------------------------------------------------- traceback
// Two kernels replace ViterbiMatrix::traceback (viterbi.cpp:195-304): one thread per read, one wave per read.  What a step's
// candidates are, and in which order, is traceback_step.h's; what follows is what the kernels share -- a read's slots, the
// running best, the checkBest test, the event log, the symbol push, the closing -- with `writes`: this lane stores (always,
// for a thread; lane 0, for a wave).

// A walk that met more symbols than its slot holds (DNAS_READ_OUT_OVERFLOW) leaves the length it needs in the slot, which
// holds nothing else then: n as 8 bytes, lowest first, at the slot's front (include/dnastore_amd.h, dnas_slot_needed).  A slot
// of fewer than 8 bytes stays as the walk left it.  Byte stores: a slot begins wherever the caller's offsets say.
__device__ inline void store_needed_len(char* out, long cap, long n) {
  if (cap < 8) return;
  for (int k = 0; k < 8; ++k) out[k] = (char)(((unsigned long long)n >> (8 * k)) & 0xffu);
}

namespace {

// Read b of the batch: its bases, its lattice, its symbol slot, and its window of the optional event log -- what the
// traceback found (the reference's level-3 messages, viterbi.cpp:266-293), in the order it walks (from the end of the
// read): type << 62 | pos << 32 | payload.  1 substitution at pos: emitted base << 2 | read base; 2 deletion between pos-1
// and pos: the deleted base; 3 duplication at pos: count << 26 | bases (2 bits each, at most 13: kEventDupBases).
struct TbRead {
  int read, L;
  const uint8_t* seq;
  const double* lat;
  char* out;
  long cap;
  unsigned long long* ev;
  long evCap;
};

__device__ __forceinline__ TbRead open_read(int b, const uint8_t* bases, const uint64_t* readOff, const int32_t* batchRead,
                                            const uint64_t* slotOff, const double* arena, char* outSym, const uint64_t* outOff,
                                            unsigned long long* events, const uint64_t* evOff) {
  const int read = batchRead[b];
  return TbRead{read, (int)(readOff[read + 1] - readOff[read]), bases + readOff[read], arena + slotOff[b],
                outSym + outOff[read], (long)(outOff[read + 1] - outOff[read]),
                events ? events + evOff[read] : nullptr, events ? (long)(evOff[read + 1] - evOff[read]) : 0};
}

// Where a walk stands (curCell: the lattice cell it stands on, read when it was chosen as a candidate) and what it wrote.
struct Walk {
  int state, pos, mut;
  double curCell;
  long n, nEv;
  uint8_t status;
};

// A walk begins on S of the last state in the last column; without a path there, none (viterbi.cpp:198-201): false.
__device__ __forceinline__ bool begin_walk(const DevModel& m, const TbRead& rd, Walk& w) {
  w = Walk{m.N - 1, rd.L, 0, cell_at(m, rd.lat, rd.seq, m.N - 1, slot_of(m, m.N - 1), rd.L, 0), 0, 0, 0};
  return w.curCell > kNegInf;
}

// The start column: the end state's S cell, or every state's in a local model, as a source of candidates like a step's.
struct TbStartStep {
  const DevModel& m;
  int L;
  __device__ __forceinline__ int count() const { return m.local ? m.N : 1; }
  __device__ __forceinline__ TbCand at(int c) const {
    const int st = m.local ? c : m.N - 1;
    return TbCand{st, slot_of(m, st), L, 0, 0., 0, 0, true};
  }
};

// The running best of a step: the first strictly greater candidate wins (the reference's updateBest, viterbi.cpp:217-228).
struct TbBest {
  double score = kNegInf, cell = kNegInf;
  int state = 0, pos = 0, lane = 0;
  uint8_t in = 0, emit = 0;
  bool other = false, found = false;
};

__device__ __forceinline__ void take(TbBest& best, double score, double cell, const TbCand& c) {
  best = TbBest{score, cell, c.state, c.pos, c.lane, c.in, c.emit, c.other, true};
}

// One wave, one candidate per lane: the wave's first strictly greater one (= the largest value, lowest lane among equals)
// is merged into the running best, which candidates of earlier calls precede: strictly greater only.  Returns the winner's
// lane, or -1 when the best stayed.  kEmit: TbCand::emit goes along (the record path reports none).
template <bool kEmit>
__device__ __forceinline__ int wave_offer(TbBest& best, bool has, const TbCand& c, double v, int ln) {
  double bs = has ? v + c.trans : kNegInf;
  int bi = ln;
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(bs, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
  }
  if (!(bs > best.score)) return -1;
  take(best, bs, __shfl(v, bi, 64),
       TbCand{__shfl(c.state, bi, 64), 0, __shfl(c.pos, bi, 64), __shfl(c.lane, bi, 64), 0., (uint8_t)__shfl((int)c.in, bi, 64),
              kEmit ? (uint8_t)__shfl((int)c.emit, bi, 64) : (uint8_t)0, __shfl((int)c.other, bi, 64) != 0});
  return bi;
}

// A candidate's cell through the CSR arrays (a duplication lane that is not in memory is rebuilt from the state's S cells) ...
__device__ __forceinline__ double csr_cell(const DevModel& m, const TbRead& rd, const TbCand& c) {
  return cell_at(m, rd.lat, rd.seq, c.state, c.slot, c.pos, c.lane);
}

// ... and on the record path, where a duplication lane is the own one of the state whose record r is.
__device__ __forceinline__ double dup_cell(const DevModel& m, const TbRead& rd, const NodeRecord& r, const double* subT, const double* lenT, int ps, int k) {
  return dup_cell_from_record(rd.lat, rd.seq, (size_t)m.storedLanes, (size_t)m.Npad, r.ownSlot(), r.mdl(), r.ctxBits(), ps, k, m.tanDup, subT, lenT);
}

// A run of candidates for one thread.  They are independent loads: kTbChunk at a time the candidates are formed, then their
// cells loaded, then compared in order, so that a run costs a few memory latencies instead of one chain per candidate.
constexpr int kTbChunk = 4;
template <class At, class Cells>
__device__ __forceinline__ void thread_gather(int n, const At& at, const Cells& cells, TbBest& best) {
  for (int c0 = 0; c0 < n; c0 += kTbChunk) {
    TbCand c[kTbChunk];
    double v[kTbChunk];
#pragma unroll
    for (int i = 0; i < kTbChunk; ++i) if (c0 + i < n) c[i] = at(c0 + i);
#pragma unroll
    for (int i = 0; i < kTbChunk; ++i) v[i] = c0 + i < n ? cells(c[i]) : kNegInf;
#pragma unroll
    for (int i = 0; i < kTbChunk; ++i) if (c0 + i < n && v[i] + c[i].trans > best.score) take(best, v[i] + c[i].trans, v[i], c[i]);
  }
}


// A step's candidates, 64 at a time, one per lane of a wave.
template <class Step, class Cells>
__device__ __forceinline__ void wave_gather(const Step& s, const Cells& cells, int ln, TbBest& best) {
  const int total = s.count();
  for (int c0 = 0; c0 < total; c0 += 64) {
    const bool has = c0 + ln < total;
    const TbCand c = has ? s.at(c0 + ln) : TbCand{};
    wave_offer<true>(best, has, c, has ? cells(c) : kNegInf, ln);
  }
}

__device__ __forceinline__ NodeRecord load_record(const DevModel& m, int st) {
  return *reinterpret_cast<const NodeRecord*>(m.rec + (size_t)st * 16);
}

__device__ __forceinline__ void log_event(const TbRead& rd, Walk& w, bool writes, int type, int p, unsigned payload) {
  if (writes && w.nEv < rd.evCap)
    rd.ev[w.nEv] = ((unsigned long long)type << 62) | ((unsigned long long)(unsigned)p << 32) | (unsigned long long)payload;
  ++w.nEv;
}

// What the step from w to `best` found, if the log is on.  ctxAt(q): base q of the state's left context.
template <class Ctx>
__device__ __forceinline__ void log_step(const TbRead& rd, Walk& w, const TbBest& best, bool writes, const Ctx& ctxAt) {
  if (!rd.ev) return;
  if (w.mut == 0) {          // viterbi.cpp:266-267
    if (best.emit && best.pos < w.pos && rd.seq[w.pos - 1] != (uint8_t)(best.emit - 1))
      log_event(rd, w, writes, 1, w.pos - 1, ((unsigned)(best.emit - 1) << 2) | rd.seq[w.pos - 1]);
  } else if (w.mut == 1) {   // viterbi.cpp:278-279 (for a null in-edge the reference prints an uninitialised base: not reproduced)
    if (best.emit) log_event(rd, w, writes, 2, w.pos, (unsigned)(best.emit - 1));
  } else if (best.lane == 0) {   // viterbi.cpp:288-293: the duplicated bases, outermost first
    const int k = w.mut - 2;
    unsigned dupBases = 0;
    for (int q = k; q >= 0; --q) dupBases = (dupBases << 2) | (unsigned)ctxAt(q);
    log_event(rd, w, writes, 3, w.pos, ((unsigned)(k + 1) << 26) | (dupBases & 0x3ffffffu));
  }
}

// The reference's checkBest (viterbi.cpp:230-237): the best candidate must reproduce the cell the walk stands on to 1e-6.
// Then the walk moves there; false: DNAS_READ_TRACEBACK_FAIL.
__device__ __forceinline__ bool accept(Walk& w, const TbBest& best) {
  const double den = fabs(w.curCell) < 1e-6 ? 1. : w.curCell;
  if (!(fabs((best.score - w.curCell) / den) < 1e-6) || !best.found) { w.status = 3; return false; }
  w.state = best.state; w.pos = best.pos; w.mut = best.lane; w.curCell = best.cell;
  return true;
}

// trace.push_front (viterbi.cpp:299-300): the slot is filled from its end, and counted past its front.
__device__ __forceinline__ void push_symbol(const TbRead& rd, Walk& w, bool writes, uint8_t in) {
  if (!in) return;
  if (writes && w.n < rd.cap) rd.out[rd.cap - 1 - w.n] = (char)in;
  ++w.n;
}

// The end of a walk: the count of every event met, logged or not (the host compares it with the log), the status, and the
// symbols in forward order at the slot's front.
__device__ __forceinline__ void close_read(const TbRead& rd, const Walk& w, bool writes, uint32_t* outLen, uint8_t* outStatus, uint32_t* evLen) {
  if (!writes) return;
  if (evLen) evLen[rd.read] = (uint32_t)(w.nEv < 0xffffffffl ? w.nEv : 0xffffffffl);
  const uint8_t status = w.status == 0 && w.n > rd.cap ? 2 : w.status;   // 2: DNAS_READ_OUT_OVERFLOW
  if (status == 2) store_needed_len(rd.out, rd.cap, w.n);
  if (status == 0)
    for (long k = 0; k < w.n; ++k) rd.out[k] = rd.out[rd.cap - w.n + k];
  outLen[rd.read] = status == 0 ? (uint32_t)w.n : 0;
  outStatus[rd.read] = status;
}

}  // namespace

// One thread per read: the reference's sequential pointer chase, candidate order and
// strict '>' tie-breaking included (viterbi.cpp:217-228,247-301).
//
// Its step from a node record is unrolled by hand, in TbStep::at's order (tools/traceback_host_check.cpp holds the record
// source to the CSR one): the record names the in-edges, so every candidate's cell is requested at once -- and with
// it the RECORD of the candidate's state, one of which is the next step's: a step costs one memory latency instead of
// three (row pointers, edge fields, cells).  Driven through TbStep it took half as long again (profiles/EXPERIMENTS.md).
// On return cur is the record of the state the walk moves to.
__device__ __forceinline__ void thread_record_step(const DevModel& m, const TbRead& rd, const Walk& w, const double* subT, const double* lenT,
                                                   NodeRecord& cur, TbBest& best) {
  constexpr int kNull = NodeRecord::kNullEdge;
  const int nE = (int)cur.emitCount(), pos = w.pos, x = pos > 0 ? rd.seq[pos - 1] : 0;
  const bool hasNull = cur.nullCount() > 0;
  NodeRecord pre[kNull + 1];   // the records of the in-edges' sources
  int adopt = -1;              // the in-edge that won: cur becomes pre[adopt]
  const auto cell = [&](int ps, int ln, int slot) { return stored_cell(m, rd.lat, slot, ps, ln); };
  const auto score = [&](int e) { return m.recScore[cur.scoreIndex(e)]; };
  const auto offer = [&](double v, double trans, int st, int ps, int ln, uint8_t in, int e) {
    if (v + trans > best.score) { take(best, v + trans, v, TbCand{st, 0, ps, ln, trans, in, 0, e >= 0}); adopt = e; }
  };
  if (w.mut == 0) {
    double ve[kRecEmit], te[kRecEmit];
#pragma unroll
    for (int i = 0; i < kRecEmit; ++i) {
      ve[i] = kNegInf; te[i] = 0.;
      if (pos > 0 && i < nE) {
        ve[i] = cell(pos - 1, 0, cur.slot(i));
        te[i] = (score(i) + m.noGap) + subT[cur.base(i) * 4 + x];
        pre[i] = load_record(m, cur.src(i));
      }
    }
    double vn = kNegInf, tn = 0.;
    if (hasNull) { vn = cell(pos, 0, cur.slot(kNull)); tn = score(kNull); pre[kNull] = load_record(m, cur.src(kNull)); }
    const double vd = cell(pos, 1, cur.ownSlot());
    const bool hasT1 = cur.mdl() > 0 && pos > 0;
    const double vt = hasT1 ? dup_cell(m, rd, cur, subT, lenT, pos - 1, 0) : kNegInf;
#pragma unroll
    for (int i = 0; i < kRecEmit; ++i)
      if (pos > 0 && i < nE) offer(ve[i], te[i], cur.src(i), pos - 1, 0, cur.in(i), i);
    if (hasNull) offer(vn, tn, cur.src(kNull), pos, 0, cur.in(kNull), kNull);
    offer(vd, m.delEnd, w.state, pos, 1, 0, -1);
    if (hasT1) offer(vt, subT[cur.ctx(0) * 4 + x], w.state, pos - 1, 2, 0, -1);
  } else if (w.mut == 1) {
    double vD[kRecEmit], vS[kRecEmit], sc[kRecEmit];
#pragma unroll
    for (int i = 0; i < kRecEmit; ++i) {
      vD[i] = vS[i] = kNegInf; sc[i] = 0.;
      if (i < nE) {
        vD[i] = cell(pos, 1, cur.slot(i));
        vS[i] = cell(pos, 0, cur.slot(i));
        sc[i] = score(i);
        pre[i] = load_record(m, cur.src(i));
      }
    }
    double vn = kNegInf, tn = 0.;
    if (hasNull) { vn = cell(pos, 1, cur.slot(kNull)); tn = score(kNull); pre[kNull] = load_record(m, cur.src(kNull)); }
#pragma unroll
    for (int i = 0; i < kRecEmit; ++i)
      if (i < nE) {
        offer(vD[i], sc[i] + m.delExtend, cur.src(i), pos, 1, cur.in(i), i);
        offer(vS[i], sc[i] + m.delOpen, cur.src(i), pos, 0, cur.in(i), i);
      }
    if (hasNull) offer(vn, tn, cur.src(kNull), pos, 1, cur.in(kNull), kNull);
  } else {
    const int k = w.mut - 2;
    const bool deeper = k < cur.mdl() - 1;
    const double vt = deeper ? dup_cell(m, rd, cur, subT, lenT, pos - 1, k + 1) : kNegInf;
    const double vs = cell(pos, 0, cur.ownSlot());
    if (deeper) offer(vt, subT[cur.ctx(k + 1) * 4 + x], w.state, pos - 1, w.mut + 1, 0, -1);
    offer(vs, m.tanDup + lenT[k], w.state, pos, 0, 0, -1);
  }
  if (adopt == 0) cur = pre[0];
  else if (adopt == 1) cur = pre[1];
  else if (adopt == 2) cur = pre[2];
  else if (adopt == kNull) cur = pre[kNull];
}

extern "C" __global__ void __launch_bounds__(256)
viterbi_traceback_kernel(DevModel m, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ readOff,
                         const int32_t* __restrict__ batchRead, const uint64_t* __restrict__ slotOff,
                         const double* __restrict__ arena, char* __restrict__ outSym,
                         const uint64_t* __restrict__ outOff, uint32_t* __restrict__ outLen,
                         uint8_t* __restrict__ outStatus, int nBatch,
                         unsigned long long* __restrict__ events, const uint64_t* __restrict__ evOff, uint32_t* __restrict__ evLen,
                         int readsPerWave) {
  // the model's small tables, indexed per lane: from LDS (a per-lane index into the kernel-argument block is a load from
  // wherever the runtime keeps kernel arguments -- host memory, as a rule -- in the middle of every step)
  __shared__ double subT[16], lenT[kMaxLen];
  if (threadIdx.x < 16) subT[threadIdx.x] = m.sub[threadIdx.x];
  if (threadIdx.x < kMaxLen) lenT[threadIdx.x] = m.len[threadIdx.x];
  __syncthreads();
  // readsPerWave of a wave's 64 lanes walk a read each: the lanes of a wave are at different places of different machines'
  // states, and a step costs the wave the union of what its lanes do -- fewer reads per wave, fewer paths per step
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (lane >= readsPerWave) return;
  const int b = wave * readsPerWave + lane;
  if (b >= nBatch) return;
  const TbRead rd = open_read(b, bases, readOff, batchRead, slotOff, arena, outSym, outOff, events, evOff);
  Walk w;
  if (!begin_walk(m, rd, w)) {
    outLen[rd.read] = 0;
    outStatus[rd.read] = 1;  // DNAS_READ_NO_PATH
    return;
  }
  const auto cells = [&](const TbCand& c) { return csr_cell(m, rd, c); };
  const TbStartStep first{m, rd.L};
  TbBest best;
  thread_gather(first.count(), [&](int c) { return first.at(c); }, cells, best);
  bool ok = accept(w, best);

  // States with more in-edges than a record holds, the local start column and the event log take the walk through the CSR arrays.
  const bool useRec = m.rec != nullptr && rd.ev == nullptr;
  bool haveRec = false;
  NodeRecord cur;            // the node record of w.state
  while (ok && w.pos >= 0 && w.state > 0) {
    const int stateWas = w.state;
    bool fromRec = false;
    best = TbBest();
    if (useRec) {
      if (!haveRec) { cur = load_record(m, w.state); haveRec = true; }
      if (cur.isInline() && !(w.mut == 0 && w.pos == 0 && m.local)) {
        fromRec = true;
        thread_record_step(m, rd, w, subT, lenT, cur, best);
      }
    }
    if (!fromRec) {
      const uint8_t* const ctx = m.ctx + (size_t)w.state * m.D;
      const auto ctxAt = [&](int q) { return (int)ctx[q]; };
      const auto s = tbCsrStep(m, subT, lenT, m.einPtr[w.state], m.einPtr[w.state + 1], m.ninPtr[w.state], m.ninPtr[w.state + 1], m.mdl[w.state],
                               slot_of(m, w.state), ctxAt, w.state, w.pos, w.mut, w.pos > 0 ? rd.seq[w.pos - 1] : 0);
      s.runs([&](int first, int n) { thread_gather(n, [&](int i) { return s.at(first + i); }, cells, best); });
      log_step(rd, w, best, true, ctxAt);
    }
    ok = accept(w, best);
    if (!ok) break;
    if (!fromRec && w.state != stateWas) haveRec = false;   // (a step from a record has brought the next state's record along)
    push_symbol(rd, w, true, best.in);
  }
  close_read(rd, w, true, outLen, outStatus, evLen);
}

// The same walk with one WAVE per read: the candidates of a step are dealt over the lanes, each lane fetches its
// candidate's cell, and the wave keeps the first strictly greater one.  From a node record every lane forms its candidate
// (the record is the same in all lanes), loads the candidate's cell AND the candidate state's record, and the winner's
// record goes to all lanes with its cell: one round of memory latency per step.  Through the CSR arrays it is three (the
// state's row pointers and context, the edge fields, the cells).  grid = ceil(nBatch / 4), block = 256.
extern "C" __global__ void __launch_bounds__(256)
viterbi_traceback_wave_kernel(DevModel m, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ readOff,
                              const int32_t* __restrict__ batchRead, const uint64_t* __restrict__ slotOff,
                              const double* __restrict__ arena, char* __restrict__ outSym,
                              const uint64_t* __restrict__ outOff, uint32_t* __restrict__ outLen,
                              uint8_t* __restrict__ outStatus, int nBatch,
                              unsigned long long* __restrict__ events, const uint64_t* __restrict__ evOff, uint32_t* __restrict__ evLen,
                              const int* __restrict__ colRange, TracebackWalk* __restrict__ walks) {
  // Bounded-memory decode (colRange / walks not null): the lattice holds columns colRange[2b] - (D + 1) .. colRange[2b + 1]
  // of read b only.  The walk runs while it stands on a column >= colRange[2b] (a step looks at most D columns back), is
  // then parked in walks[b] and picked up by the launch over the segment before.
  __shared__ double subT[16], lenT[kMaxLen];   // (as in the thread-per-read kernel: no per-lane index into the kernel-argument block)
  if (threadIdx.x < 16) subT[threadIdx.x] = m.sub[threadIdx.x];
  if (threadIdx.x < kMaxLen) lenT[threadIdx.x] = m.len[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const int ln = threadIdx.x & 63;
  if (b >= nBatch) return;
  const TbRead rd = open_read(b, bases, readOff, batchRead, slotOff, arena, outSym, outOff, events, evOff);
  const bool writes = ln == 0;
  TracebackWalk* const walk = walks ? walks + b : nullptr;
  const int stopBelow = colRange ? colRange[2 * b] : 0;
  const int phase = walk ? walk->phase : 0;      // 0: not started, 1: parked, 2: finished
  if (phase == 2) return;
  const auto csrCells = [&](const TbCand& c) { return csr_cell(m, rd, c); };
  Walk w;
  TbBest best;
  bool ok = true;
  if (phase == 1) {
    w = Walk{walk->state, walk->pos, walk->mut, walk->curCell, (long)walk->n, (long)walk->nEv, 0};
  } else {
    if (!begin_walk(m, rd, w)) {
      if (writes) { outLen[rd.read] = 0; outStatus[rd.read] = 1; if (walk) walk->phase = 2; }   // DNAS_READ_NO_PATH
      return;
    }
    wave_gather(TbStartStep{m, rd.L}, csrCells, ln, best);
    ok = accept(w, best);
  }

  const bool useRec = m.rec != nullptr && rd.ev == nullptr;
  bool haveRec = false;
  NodeRecord cur;            // the node record of w.state, the same in every lane
  while (ok && w.pos >= stopBelow && w.pos >= 0 && w.state > 0) {
    const int stateWas = w.state, x = w.pos > 0 ? rd.seq[w.pos - 1] : 0;
    bool fromRec = false;
    best = TbBest();
    if (useRec) {
      if (!haveRec) { cur = load_record(m, w.state); haveRec = true; }
      if (cur.isInline() && !(w.mut == 0 && w.pos == 0 && m.local)) {
        fromRec = true;
        const TbRecordStep s = tbRecordStep(m, subT, lenT, cur, w.state, w.pos, w.mut, x);
        const bool has = ln < s.count();
        const TbCand c = has ? s.at(ln) : TbCand{};
        NodeRecord next = {};
        double v = kNegInf;
        if (has) {
          if (c.other) next = load_record(m, c.state);
          v = c.lane < 2 ? stored_cell(m, rd.lat, c.slot, c.pos, c.lane) : dup_cell(m, rd, cur, subT, lenT, c.pos, c.lane - 2);
        }
        const int bi = wave_offer<false>(best, has, c, v, ln);
        if (bi >= 0 && best.other) {       // the next state's record, from the lane that fetched it
#pragma unroll
          for (int i = 0; i < 16; ++i) cur.w[i] = (uint32_t)__shfl((int)next.w[i], bi, 64);
        }
      }
    }
    if (!fromRec) {
      // round 1: what the step needs to know about the state, fetched by different lanes
      int meta = 0;
      if (ln == 0) meta = m.einPtr[w.state]; else if (ln == 1) meta = m.einPtr[w.state + 1];
      else if (ln == 2) meta = m.ninPtr[w.state]; else if (ln == 3) meta = m.ninPtr[w.state + 1];
      else if (ln == 4) meta = m.mdl[w.state]; else if (ln == 5) meta = slot_of(m, w.state);
      else if (ln >= 8 && ln < 8 + m.D) meta = m.ctx[(size_t)w.state * m.D + (ln - 8)];
      const auto ctxAt = [&](int q) { return __shfl(meta, 8 + q, 64); };   // (called by all lanes together)
      const auto s = tbCsrStep(m, subT, lenT, __shfl(meta, 0, 64), __shfl(meta, 1, 64), __shfl(meta, 2, 64), __shfl(meta, 3, 64),
                               __shfl(meta, 4, 64), __shfl(meta, 5, 64), ctxAt, w.state, w.pos, w.mut, x);
      wave_gather(s, csrCells, ln, best);
      log_step(rd, w, best, writes, ctxAt);
    }
    ok = accept(w, best);
    if (!ok) break;
    if (!fromRec && w.state != stateWas) haveRec = false;   // (a step from a record has brought the next state's record along)
    push_symbol(rd, w, writes, best.in);
  }

  if (walk && ok && w.pos >= 0 && w.state > 0) {   // the walk left this segment: park it
    if (writes) {
      walk->state = w.state; walk->pos = w.pos; walk->mut = w.mut; walk->curCell = w.curCell; walk->n = (long long)w.n; walk->nEv = (long long)w.nEv;
      walk->phase = 1;
    }
    return;
  }
  if (writes && walk) walk->phase = 2;
  __builtin_amdgcn_wave_barrier();
  close_read(rd, w, writes, outLen, outStatus, evLen);
}
