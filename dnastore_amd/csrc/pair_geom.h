// Where the pair-HMM wavefront stands, stated once for host and device: the band as host/pairalign.hpp defines it, where a
// cell's choice word (or parked value) lies, and what one lane knows about one stripe of 64 rows.  The walks of
// pair_align_device.h and pair_counts_device.h, the tracebacks that read what they filed, the host plans that size it and
// tools/pair_wavefront_host_check.cpp (a sanitizer build on the CPU) compile this text.
#pragma once
#include <stddef.h>

#if defined(__HIP__)
#define DNAS_GEOM_FN __host__ __device__ inline
#else
#define DNAS_GEOM_FN inline
#endif

// What fill and traceback agree on: the band, and that cell (ip, op) is filed under (stripe, step, lane).
struct PaGeom {
  int lo, hi, stepsMax, stripes;
  DNAS_GEOM_FN PaGeom(int I, int O, int band) {
    const int b = band < 0 || band > I + O + 1 ? I + O + 1 : band;
    lo = (O < I ? O - I : 0) - b;
    hi = (O > I ? O - I : 0) + b;
    // a stripe of rows r0 .. r0 + 63 runs from column c0 = rowLo(r0) to rowHi(r0 + 63), lane 63 another 63 steps behind
    const long w = (long)hi - lo + 1 + 126, f = (long)O + 64;
    stepsMax = (int)(w < f ? w : f);
    stripes = I / 64 + 1;
  }
  DNAS_GEOM_FN int rowLo(int ip) const { return ip + lo > 0 ? ip + lo : 0; }
  DNAS_GEOM_FN int rowHi(int ip, int O) const { return ip + hi < O ? ip + hi : O; }
  DNAS_GEOM_FN size_t words() const { return (size_t)stripes * (size_t)stepsMax * 64; }
  DNAS_GEOM_FN size_t wordAt(int ip, int op) const {
    const int s = ip >> 6, l = ip & 63;
    return ((size_t)s * (size_t)stepsMax + (size_t)(op - rowLo(s << 6) + l)) * 64 + (size_t)l;
  }
};

// The columns of one row inside the band.
struct PaSpan {
  int lo, hi;
  DNAS_GEOM_FN bool has(int op) const { return op >= lo && op <= hi; }
};

// Stripe s of a pair, as lane `lane` sees it: the lane owns row r = r0 + lane (row: the matrix has it) and is skewed one column
// per lane, at step t in 0 .. tmax it stands on column op(t), which is a cell iff active(op(t)).  last: the lane of the
// stripe's last row; kmax: the duplication lanes row r has.  Going forward the stripe's lane 0 reads the row above(g, O) it,
// going back its lane `last` the row below(g, O) it, g and O being what the stripe was made from.
struct PaStripe {
  int r0, r, lane, rlo, rhi, c0, last, tmax, kmax;
  bool row;
  DNAS_GEOM_FN PaStripe(const PaGeom& g, int I, int O, int P, int s, int lane_) {
    r0 = s << 6, r = r0 + lane_, lane = lane_;
    row = r <= I;
    rlo = row ? g.rowLo(r) : 1, rhi = row ? g.rowHi(r, O) : 0;
    c0 = g.rowLo(r0);
    last = I - r0 < 63 ? I - r0 : 63;
    tmax = g.rowHi(r0 + last, O) - c0 + last;
    kmax = row ? (r < P ? r : P) : 0;
  }
  DNAS_GEOM_FN int op(int t) const { return c0 + t - lane; }
  DNAS_GEOM_FN bool active(int op) const { return op >= rlo && op <= rhi; }
  DNAS_GEOM_FN PaSpan above(const PaGeom& g, int O) const { return PaSpan{g.rowLo(r0 - 1), g.rowHi(r0 - 1, O)}; }
  DNAS_GEOM_FN PaSpan below(const PaGeom& g, int O) const { return PaSpan{g.rowLo(r0 + 64), g.rowHi(r0 + 64, O)}; }
};
