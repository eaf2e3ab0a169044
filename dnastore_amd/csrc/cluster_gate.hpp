// The edit-distance gate of dnas_cluster_reads_gated and the kernels of dnas_edit_distances (include/dnastore_amd.h): what
// cluster_gate_kernels.hip offers cluster_kernels.hip, and the recurrence itself, stated once for the kernels and for a host
// program that wants to run it (the functions below are plain C++ over pointers and strides).  tools/bitvector_host_check.cpp is
// that program: gatePairWords<1|2|4|8>, gatePairLong and the primer search built on gateBlock (TrimSearch, host/trim.hpp) against
// a full-matrix dynamic program under ASan and UBSan, on homopolymers, short-period repeats and every length around a word
// boundary (tests/test_bitvector_cpu.py builds and runs it).  The host statements do not use the recurrence.
//
// Myers' bit-vector recurrence in Hyyro's block form, for the global distance.  A pattern of m rows is cut into words of 64 rows;
// column c of the dynamic program is held as the vertical differences Pv (+1) and Mv (-1) of every word, a word hands the
// horizontal difference of its last row (-1, 0, +1) to the next one, row 0 hands +1 to the first (D[0][c] = c), and the distance
// is D[m][0] = m plus the horizontal differences of row m, which are read off the word that holds it.  Rows above m in that word
// compute garbage that never reaches a lower bit: carries and shifts only go up.
#pragma once
#include <cstdint>

#include "host/cluster.hpp"

struct ClPair {
  int32_t i, j;
};

namespace dnas {

// One word, one column.  Eq: the rows of the word whose base is the column's.  rowBit: the bit of row m when this word holds it,
// else 0.  -> the horizontal difference below the word's last row.
DNAS_HD inline int gateBlock(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, uint64_t rowBit, int32_t& score) {
  const uint64_t hneg = hin < 0 ? 1u : 0u, hpos = hin > 0 ? 1u : 0u;
  const uint64_t Xv = Eq | Mv;
  Eq |= hneg;
  const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  uint64_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
  score += (int32_t)((Ph & rowBit) != 0) - (int32_t)((Mh & rowBit) != 0);
  const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
  Ph = Ph << 1 | hpos;
  Mh = Mh << 1 | hneg;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
  return hout;
}

// The match masks of the rows 64 w .. of pat[0..m): eq[b] has bit r set where pat[64 w + r] == b.
DNAS_HD inline void gateMasks(const int8_t* pat, int m, int w, uint64_t eq[4]) {
  eq[0] = eq[1] = eq[2] = eq[3] = 0;
  const int rows = m - 64 * w < 64 ? m - 64 * w : 64;
  for (int r = 0; r < rows; ++r) {
    const int b = pat[64 * w + r] & 3;
    const uint64_t bit = (uint64_t)1 << r;
    eq[0] |= b == 0 ? bit : 0;
    eq[1] |= b == 1 ? bit : 0;
    eq[2] |= b == 2 ? bit : 0;
    eq[3] |= b == 3 ? bit : 0;
  }
}

// e[0] = d(pat, txt), e[1] = d(pat, reverse complement of txt) for a pattern of at most 64 W rows: Pv, Mv and the scores of both
// orientations are locals (every loop over W is unrolled, no array is indexed by a run-time value), the masks go to
// peq[(b * W + w) * stride], which is the thread's column of the [base][word][thread] table.
template <int W>
DNAS_HD inline void gatePairWords(const int8_t* pat, int m, const int8_t* txt, int n, uint64_t* peq, int stride, int32_t* e) {
  if (m == 0) {
    e[0] = e[1] = n;
    return;
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {
    uint64_t eq[4];
    gateMasks(pat, m, w, eq);
#pragma unroll
    for (int b = 0; b < 4; ++b) peq[(b * W + w) * stride] = eq[b];
  }
  uint64_t Pv0[W], Mv0[W], Pv1[W], Mv1[W];
#pragma unroll
  for (int w = 0; w < W; ++w) Pv0[w] = Pv1[w] = ~(uint64_t)0, Mv0[w] = Mv1[w] = 0;
  int32_t s0 = m, s1 = m;
  const int last = (m - 1) >> 6;
  const uint64_t lastBit = (uint64_t)1 << ((m - 1) & 63);
  for (int c0 = 0; c0 < n; c0 += 16) {
    // 16 columns of the text from its front, and of its reverse complement, two bits each: the loads of a group go out together
    uint32_t fwd = 0, rev = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = c0 + u < n ? c0 + u : n - 1;
      fwd |= (uint32_t)(txt[c] & 3) << (2 * u);
      rev |= (uint32_t)(3 - (txt[n - 1 - c] & 3)) << (2 * u);
    }
    const int cols = n - c0 < 16 ? n - c0 : 16;
    for (int u = 0; u < cols; ++u) {
      const int bf = (int)(fwd >> (2 * u) & 3), br = (int)(rev >> (2 * u) & 3);
      int h0 = 1, h1 = 1;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const uint64_t rowBit = w == last ? lastBit : 0;
        h0 = gateBlock(Pv0[w], Mv0[w], peq[(bf * W + w) * stride], h0, rowBit, s0);
        h1 = gateBlock(Pv1[w], Mv1[w], peq[(br * W + w) * stride], h1, rowBit, s1);
      }
    }
  }
  e[0] = s0;
  e[1] = s1;
}

// The same for a pattern of any length, everything in memory: word x of the thread's slice is mem[x * stride].  With
// words = ceil(m / 64) the slice holds the masks [b * words + w], then Pv and Mv of the two orientations: 8 words in all.
DNAS_HD inline void gatePairLong(const int8_t* pat, int m, const int8_t* txt, int n, uint64_t* mem, int64_t stride, int32_t* e) {
  if (m == 0) {
    e[0] = e[1] = n;
    return;
  }
  const int words = (m + 63) >> 6;
  for (int w = 0; w < words; ++w) {
    uint64_t eq[4];
    gateMasks(pat, m, w, eq);
    for (int b = 0; b < 4; ++b) mem[(int64_t)(b * words + w) * stride] = eq[b];
    mem[(int64_t)(4 * words + w) * stride] = mem[(int64_t)(6 * words + w) * stride] = ~(uint64_t)0;
    mem[(int64_t)(5 * words + w) * stride] = mem[(int64_t)(7 * words + w) * stride] = 0;
  }
  int32_t s0 = m, s1 = m;
  const int last = words - 1;
  const uint64_t lastBit = (uint64_t)1 << ((m - 1) & 63);
  for (int c = 0; c < n; ++c) {
    const int bf = txt[c] & 3, br = 3 - (txt[n - 1 - c] & 3);
    int h0 = 1, h1 = 1;
    for (int w = 0; w < words; ++w) {
      const uint64_t rowBit = w == last ? lastBit : 0;
      uint64_t* const v = mem + (int64_t)(4 * words + w) * stride;
      const int64_t step = (int64_t)words * stride;
      uint64_t Pv = v[0], Mv = v[step];
      h0 = gateBlock(Pv, Mv, mem[(int64_t)(bf * words + w) * stride], h0, rowBit, s0);
      v[0] = Pv, v[step] = Mv;
      Pv = v[2 * step], Mv = v[3 * step];
      h1 = gateBlock(Pv, Mv, mem[(int64_t)(br * words + w) * stride], h1, rowBit, s1);
      v[2 * step] = Pv, v[3 * step] = Mv;
    }
  }
  e[0] = s0;
  e[1] = s1;
}

}  // namespace dnas

#if defined(__HIP__)
#include <hip/hip_runtime.h>

#include "device_buffer.hpp"

// The gate's launches on one device.  open() reads the testing aid and allocates what the longest pattern of the call needs
// on the current device (freed with the object, on the device that is current then);
// run() enqueues the kernels over list[0 .. pairs), whose longest pattern has at most boundWords words:
//   dist != null:  dist[2 q], dist[2 q + 1] = e[0], e[1] of pair q (no counts are kept);
//   dist == null:  the pairs that pass max_edit_permille are appended to surv in any order, counts[0] counts them, counts[1] the
//                  pairs of the long route and counts[2] the word steps (the caller zeroes counts, which is device memory).
struct ClGate {
  int cus = 256, regWords = 8, longWords = 0;
  unsigned longBlocks = 0;
  dnas::DevBuf<uint64_t> scratch;                        // the long route's slices, [word][thread]
  dnas::DevBuf<unsigned long long> counts;
  int open(int cus_, int64_t callBoundWords);
  void run(hipStream_t stream, int64_t pairs, const ClPair* list, const int8_t* readSeqs, const int64_t* readOff, int64_t boundWords,
           int32_t maxEditPermille, int32_t* dist, ClPair* surv) const;
};
#endif
