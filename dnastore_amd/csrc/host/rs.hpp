// The outer code: Reed-Solomon over GF(2^8) across the strands of a block (include/dnastore_amd.h, "The outer code").  This file
// holds what the host statement (rs.cpp) and the kernels (rs_kernels.hip) share: the field's tables, a position's locator, and the
// solver of one column from its syndromes (erasure locator -> Forney syndromes -> Berlekamp-Massey -> root search over the n
// positions -> Forney values -> the re-check that makes FAILED follow the definition).  The statement runs the solver for every
// column; the kernels run it for the columns whose Forney syndromes are not all zero, and fill the others by a uniform path of
// their own.  Field arithmetic is exact, so the two agree byte for byte whatever the order of operations.
#pragma once
#include <cstdint>

#include "../../../include/dnastore_amd.h"

#ifndef DNAS_HD
#if defined(__HIPCC__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif
#endif

namespace dnas {

constexpr int kRsMaxN = 255, kRsMaxR = 64;

// GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1, alpha = 2: exp[i] = alpha^i for i = 0 .. 509 (so that exp[log a + log b] needs no
// reduction), log[alpha^i] = i, log[0] unused.
struct GfTables {
  uint8_t exp[512];
  uint8_t log[256];
};
constexpr GfTables makeGfTables() {
  GfTables t{};
  unsigned x = 1;
  for (int i = 0; i < 255; ++i) {
    t.exp[i] = (uint8_t)x;
    t.log[x] = (uint8_t)i;
    x <<= 1;
    if (x & 0x100) x ^= 0x11d;
  }
  for (int i = 255; i < 512; ++i) t.exp[i] = t.exp[i - 255];
  return t;
}

DNAS_HD inline uint8_t gfMul(const GfTables& gf, uint8_t a, uint8_t b) { return a && b ? gf.exp[gf.log[a] + gf.log[b]] : 0; }
DNAS_HD inline uint8_t gfDiv(const GfTables& gf, uint8_t a, uint8_t b) { return a ? gf.exp[gf.log[a] + 255 - gf.log[b]] : 0; }   // b != 0
// Position p of a word of n symbols is the coefficient of x^(n-1-p): its locator is X_p = alpha^(n-1-p).
DNAS_HD inline uint8_t rsLocator(const GfTables& gf, int n, int p) { return gf.exp[n - 1 - p]; }
DNAS_HD inline uint8_t rsLocatorInverse(const GfTables& gf, int n, int p) { return gf.exp[(255 - (n - 1 - p)) % 255]; }

// poly(x) of degree deg at the point x, coefficients ascending
DNAS_HD inline uint8_t gfEval(const GfTables& gf, const uint8_t* poly, int deg, uint8_t x) {
  uint8_t y = poly[deg];
  for (int i = deg - 1; i >= 0; --i) y = (uint8_t)(gfMul(gf, y, x) ^ poly[i]);
  return y;
}

// The erasure locator of f erased positions: gamma[0 .. f] = the coefficients of prod (1 - X_p x), ascending.
DNAS_HD inline void rsErasureLocator(const GfTables& gf, int n, int f, const uint8_t* erased, uint8_t* gamma) {
  gamma[0] = 1;
  for (int q = 0; q < f; ++q) {
    const uint8_t X = rsLocator(gf, n, erased[q]);
    gamma[q + 1] = 0;
    for (int i = q + 1; i >= 1; --i) gamma[i] = (uint8_t)(gamma[i] ^ gfMul(gf, X, gamma[i - 1]));
  }
}

// One column.  S[0 .. r-1]: its syndromes with the erased symbols read as 0; erased[0 .. f-1] (f <= r): the erased positions,
// gamma their locator; present[0 .. n-1].  -> DNAS_RS_OK, DNAS_RS_CORRECTED or DNAS_RS_FAILED.  Unless it failed, fixPos / fixVal
// [0 .. *nFix-1] are the positions to change and what to XOR into them (an erased symbol counts as 0): the f erased ones first, in
// the order of erased[], then the *nErr errors (a value may be 0 only at an erased position).
DNAS_HD inline int rsSolveColumn(const GfTables& gf, int n, int r, int f, const uint8_t* erased, const uint8_t* gamma, const uint8_t* present,
                                 const uint8_t* S, uint8_t* fixPos, uint8_t* fixVal, int* nFix, int* nErr) {
  *nFix = 0, *nErr = 0;
  const int rho = r - f;
  // Forney syndromes: the coefficients f .. r-1 of S(x) gamma(x)
  uint8_t T[kRsMaxR];
  for (int u = 0; u < rho; ++u) {
    uint8_t t = 0;
    for (int a = 0; a <= f; ++a) t = (uint8_t)(t ^ gfMul(gf, gamma[a], S[f + u - a]));
    T[u] = t;
  }
  // Berlekamp-Massey over T -> the error locator lam of degree len
  uint8_t lam[kRsMaxR + 1], prev[kRsMaxR + 1], tmp[kRsMaxR + 1];
  for (int i = 0; i <= kRsMaxR; ++i) lam[i] = prev[i] = 0;
  lam[0] = prev[0] = 1;
  int len = 0, shift = 1;
  uint8_t prevDelta = 1;
  for (int u = 0; u < rho; ++u) {
    uint8_t delta = T[u];
    for (int i = 1; i <= len; ++i) delta = (uint8_t)(delta ^ gfMul(gf, lam[i], T[u - i]));
    if (delta == 0) {
      ++shift;
      continue;
    }
    const uint8_t scale = gfDiv(gf, delta, prevDelta);
    if (2 * len <= u) {
      for (int i = 0; i <= kRsMaxR; ++i) tmp[i] = lam[i];
      for (int i = 0; i + shift <= kRsMaxR; ++i) lam[i + shift] = (uint8_t)(lam[i + shift] ^ gfMul(gf, scale, prev[i]));
      for (int i = 0; i <= kRsMaxR; ++i) prev[i] = tmp[i];
      len = u + 1 - len;
      prevDelta = delta;
      shift = 1;
    } else {
      for (int i = 0; i + shift <= kRsMaxR; ++i) lam[i + shift] = (uint8_t)(lam[i + shift] ^ gfMul(gf, scale, prev[i]));
      ++shift;
    }
  }
  if (2 * len > rho) return DNAS_RS_FAILED;
  int deg = len;
  while (deg > 0 && lam[deg] == 0) --deg;
  if (deg != len) return DNAS_RS_FAILED;
  // its roots among the present positions: as many as its degree, or there is no codeword within reach
  for (int q = 0; q < f; ++q) fixPos[q] = erased[q];
  int found = 0;
  if (len > 0)
    for (int p = 0; p < n; ++p) {
      if (!present[p]) continue;
      if (gfEval(gf, lam, len, rsLocatorInverse(gf, n, p)) != 0) continue;
      if (found == len) return DNAS_RS_FAILED;
      fixPos[f + found++] = (uint8_t)p;
    }
  if (found != len) return DNAS_RS_FAILED;
  // psi = lam gamma locates errors and erasures together; omega = S psi mod x^r; the value at X is X omega(1/X) / psi'(1/X)
  const int total = f + len;
  uint8_t psi[kRsMaxR + 1], omega[kRsMaxR];
  for (int i = 0; i <= total; ++i) {
    uint8_t c = 0;
    for (int a = 0; a <= len && a <= i; ++a)
      if (i - a <= f) c = (uint8_t)(c ^ gfMul(gf, lam[a], gamma[i - a]));
    psi[i] = c;
  }
  for (int t = 0; t < r; ++t) {
    uint8_t c = 0;
    for (int a = 0; a <= total && a <= t; ++a) c = (uint8_t)(c ^ gfMul(gf, psi[a], S[t - a]));
    omega[t] = c;
  }
  uint8_t check[kRsMaxR];
  for (int i = 0; i < r; ++i) check[i] = S[i];
  int errors = 0;
  for (int q = 0; q < total; ++q) {
    const int p = fixPos[q];
    const uint8_t X = rsLocator(gf, n, p), Xi = rsLocatorInverse(gf, n, p);
    uint8_t den = 0;                                     // psi'(1/X): the odd coefficients, x^(i-1)
    for (int i = (total - 1) | 1; i >= 1; i -= 2) {
      den = gfMul(gf, den, gfMul(gf, Xi, Xi));
      if (i <= total) den = (uint8_t)(den ^ psi[i]);
    }
    if (den == 0) return DNAS_RS_FAILED;
    const uint8_t v = gfDiv(gf, gfMul(gf, X, gfEval(gf, omega, r - 1, Xi)), den);
    fixVal[q] = v;
    if (q >= f) {
      if (v == 0) return DNAS_RS_FAILED;                 // (a located error changes its symbol)
      ++errors;
    }
    uint8_t pw = v;                                      // the corrected word's syndromes: S_i + v X^i
    for (int i = 0; i < r; ++i) {
      check[i] = (uint8_t)(check[i] ^ pw);
      pw = gfMul(gf, pw, X);
    }
  }
  for (int i = 0; i < r; ++i)
    if (check[i] != 0) return DNAS_RS_FAILED;
  if (2 * errors + f > r) return DNAS_RS_FAILED;
  *nFix = total, *nErr = errors;
  return errors ? DNAS_RS_CORRECTED : DNAS_RS_OK;
}

// DNAS_OK or the code, dnas_last_error set: what the entries of either side check.
int checkRsCode(int32_t n, int32_t k, int64_t L, int64_t B);

// The statement over blocks [first, last): one thread.  The arguments were checked.
void rsEncodeHost(int32_t n, int32_t k, int64_t L, int64_t first, int64_t last, const uint8_t* data, uint8_t* out_blocks);
void rsDecodeHost(int32_t n, int32_t k, int64_t L, int64_t first, int64_t last, const uint8_t* blocks, const uint8_t* present,
                  uint8_t* out_blocks, uint8_t* out_status, uint8_t* out_errors, int32_t* out_fixed);

// CRC-8 of the strand frame: polynomial 0x07, initial value 0, not reflected
uint8_t outerCrc8(const uint8_t* bytes, int64_t len, uint8_t crc = 0);

}  // namespace dnas
