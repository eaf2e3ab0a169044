// Both-strand decode: the small kernels around the unchanged fill and traceback kernels.
//
// A call in mode "both" on n reads schedules 2n virtual reads: virtual read i is caller read i as written, virtual
// read n + 1 + i its reverse complement (index n is an empty read that is never scheduled: it makes the offset tables,
// the caller's prefix arrays written twice, bound slot i for both orientations).  The fill leaves one log-likelihood
// per virtual read; strand_pick_kernel keeps the larger one per caller read and lists the winners, the traceback
// kernels walk that list, and strand_gather_kernel brings what they wrote per virtual read to the caller's arrays.
// Plain loads and vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

// The reverse complement of every read: rcDst[off[r] + L - 1 - p] = 3 - src[off[r] + p]; with fwdDst also a copy of
// the read as written (mode "both": the two orientations then live in one buffer behind one offset table).
// off[] starts at 0 (src is the caller's buffer advanced to its first read).  grid = (reads, chunks): the work-groups
// blockIdx.y, blockIdx.y + gridDim.y, ... of a read take 256 bases each, so that a wave reads and writes 64
// neighbouring bytes whatever the read lengths are (check_bases_kernel has run: no code above 3 gets here).
extern "C" __global__ void __launch_bounds__(256)
revcomp_reads_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off, uint8_t* __restrict__ fwdDst,
                     uint8_t* __restrict__ rcDst) {
  const uint64_t a = off[blockIdx.x], L = off[blockIdx.x + 1] - a;
  for (uint64_t p = (uint64_t)blockIdx.y * 256u + threadIdx.x; p < L; p += (uint64_t)gridDim.y * 256u) {
    const uint8_t b = src[a + p];
    if (fwdDst) fwdDst[a + p] = b;
    rcDst[a + (L - 1 - p)] = (uint8_t)(3u - b);
  }
}

// One thread per caller read of a batch (or of a bounded-memory group).  pairRead[2k], pairRead[2k + 1] are the
// forward and the reverse virtual read of pair k, neighbours in the batch; ll[] holds what the fill wrote per virtual
// read.  The reverse strand wins iff its log-likelihood is strictly larger (fp64 compare): ties, and a pair of -inf,
// stay with the forward strand, whose lattice then tells the traceback kernels "no path".
//   winRead[k]   the winner's virtual read           (what the traceback launch takes as its batchRead)
//   winSlot[k]   = pairSlot[2k + w]                   (its lattice; pairSlot null: not written)
//   winRow[k]    = 2k + w                             (its row in the group's tables; null: not written)
//   counters     [0] reverse won, [1] ties (equal log-likelihoods, the -inf pairs among them), [2] both -inf
extern "C" __global__ void __launch_bounds__(256)
strand_pick_kernel(const int32_t* __restrict__ pairRead, const uint64_t* __restrict__ pairSlot, int nPairs,
                   const double* __restrict__ ll, double* __restrict__ outLoglike, uint8_t* __restrict__ outStrand,
                   int32_t* __restrict__ winRead, uint64_t* __restrict__ winSlot, int32_t* __restrict__ winRow,
                   unsigned long long* __restrict__ counters) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  bool rev = false, tie = false, none = false;
  if (k < nPairs) {
    const int vF = pairRead[2 * k], vR = pairRead[2 * k + 1];
    const double f = ll[vF], r = ll[vR];
    rev = r > f;
    tie = r == f;
    none = tie && !(f > -__builtin_inf());
    const int w = rev ? 1 : 0;
    outLoglike[vF] = rev ? r : f;          // the forward virtual read IS the caller's read index
    outStrand[vF] = (uint8_t)w;
    winRead[k] = rev ? vR : vF;
    if (pairSlot) winSlot[k] = pairSlot[2 * k + w];
    if (winRow) winRow[k] = 2 * k + w;
  }
  const unsigned long long mRev = __ballot(rev), mTie = __ballot(tie), mNone = __ballot(none);
  if ((threadIdx.x & 63) == 0) {
    if (mRev) atomicAdd(counters + 0, (unsigned long long)__popcll(mRev));
    if (mTie) atomicAdd(counters + 1, (unsigned long long)__popcll(mTie));
    if (mNone) atomicAdd(counters + 2, (unsigned long long)__popcll(mNone));
  }
}

// Bounded-memory decode: the winners' rows of a group's per-segment table.  tab[sg * nRows + row] -> out[sg * nWin + k]
// with row = winRow[k].  grid = (ceil(nWin / 256), segments).
extern "C" __global__ void __launch_bounds__(256)
strand_rows_kernel(const uint64_t* __restrict__ tab, int nRows, const int32_t* __restrict__ winRow, int nWin,
                   uint64_t* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k < nWin) out[(size_t)blockIdx.y * (size_t)nWin + k] = tab[(size_t)blockIdx.y * (size_t)nRows + winRow[k]];
}

// copy_rows_kernel for rows that are named by a list: row j of the launch is row rowOf[j] of src and dst.
extern "C" __global__ void strand_copy_rows_kernel(double* __restrict__ dst, const double* __restrict__ src, size_t dstStride,
                                                   size_t srcStride, size_t n, const int32_t* __restrict__ rowOf) {
  const size_t row = (size_t)rowOf[blockIdx.y];
  const double* s = src + row * srcStride;
  double* d = dst + row * dstStride;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// After the traceback of the winners: decoded length and status (and the length of the event log) from the winner's
// virtual read to the caller's read.  firstReverse = n + 1.
extern "C" __global__ void __launch_bounds__(256)
strand_gather_kernel(const int32_t* __restrict__ winRead, int nWin, int firstReverse, const uint32_t* __restrict__ vLen,
                     const uint8_t* __restrict__ vStatus, uint32_t* __restrict__ outLen, uint8_t* __restrict__ outStatus,
                     uint32_t* __restrict__ evLen) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= nWin) return;
  const int v = winRead[k], i = v >= firstReverse ? v - firstReverse : v;
  outLen[i] = vLen[v];
  outStatus[i] = vStatus[v];
  if (evLen && v != i) evLen[i] = evLen[v];
}
