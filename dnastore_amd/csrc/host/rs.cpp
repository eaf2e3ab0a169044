// dnas_rs_encode_host, dnas_rs_decode_host: the statement of include/dnastore_amd.h, "The outer code", as plain loops -- encoding
// by long division, decoding a column at a time with the solver of rs.hpp.  One thread; the CPU baseline of the kernels.
#include "rs.hpp"

#include <new>
#include <string>
#include <vector>

#include "../errors.hpp"

namespace dnas {

namespace {
constexpr GfTables kGf = makeGfTables();
}

int checkRsCode(int32_t n, int32_t k, int64_t L, int64_t B) {
  if (n < 2 || n > kRsMaxN || k < 1 || k >= n || n - k > kRsMaxR)
    return fail(DNAS_E_UNSUPPORTED, "reed-solomon: RS(" + std::to_string(n) + ", " + std::to_string(k) + ") needs 2 <= n <= 255, 1 <= k < n, n - k <= 64");
  if (L < 1) return fail(DNAS_E_INVALID, "reed-solomon: a strand has at least one byte");
  if (B < 0) return fail(DNAS_E_INVALID, "reed-solomon: bad argument");
  if (L > ((int64_t)1 << 24) || B > ((int64_t)1 << 40) / (n * L)) return fail(DNAS_E_UNSUPPORTED, "reed-solomon: strands beyond 2^24 bytes or a call beyond 2^40 bytes");
  return DNAS_OK;
}

uint8_t outerCrc8(const uint8_t* bytes, int64_t len, uint8_t crc) {
  for (int64_t i = 0; i < len; ++i) {
    crc = (uint8_t)(crc ^ bytes[i]);
    for (int b = 0; b < 8; ++b) crc = (uint8_t)(crc & 0x80 ? (crc << 1) ^ 0x07 : crc << 1);
  }
  return crc;
}

void rsEncodeHost(int32_t n, int32_t k, int64_t L, int64_t first, int64_t last, const uint8_t* data, uint8_t* out_blocks) {
  const int r = n - k;
  uint8_t g[kRsMaxR + 1] = {1};                          // g(x) = prod (x - alpha^i), descending: g[0] = 1 is x^r
  for (int i = 0; i < r; ++i) {
    g[i + 1] = 0;
    for (int j = i + 1; j >= 1; --j) g[j] = (uint8_t)(g[j] ^ gfMul(kGf, g[j - 1], kGf.exp[i]));
  }
  for (int64_t b = first; b < last; ++b) {
    const uint8_t* in = data + b * k * L;
    uint8_t* out = out_blocks + b * n * L;
    for (int64_t j = 0; j < L; ++j) {
      uint8_t rem[kRsMaxR] = {0};                        // the remainder so far, descending
      for (int p = 0; p < k; ++p) {
        const uint8_t d = in[p * L + j], fb = (uint8_t)(d ^ rem[0]);
        out[p * L + j] = d;
        for (int t = 0; t + 1 < r; ++t) rem[t] = (uint8_t)(rem[t + 1] ^ gfMul(kGf, fb, g[t + 1]));
        rem[r - 1] = gfMul(kGf, fb, g[r]);
      }
      for (int t = 0; t < r; ++t) out[(k + t) * L + j] = rem[t];
    }
  }
}

void rsDecodeHost(int32_t n, int32_t k, int64_t L, int64_t first, int64_t last, const uint8_t* blocks, const uint8_t* present,
                  uint8_t* out_blocks, uint8_t* out_status, uint8_t* out_errors, int32_t* out_fixed) {
  const int r = n - k;
  for (int64_t b = first; b < last; ++b) {
    const uint8_t *in = blocks + b * n * L, *pres = present + b * n;
    uint8_t* out = out_blocks + b * n * L;
    int32_t* fixed = out_fixed + b * n;
    uint8_t erased[kRsMaxN], gamma[kRsMaxR + 1];
    int f = 0;
    for (int p = 0; p < n; ++p) {
      fixed[p] = 0;
      if (!pres[p]) erased[f++] = (uint8_t)p;
    }
    for (int p = 0; p < n; ++p)
      for (int64_t j = 0; j < L; ++j) out[p * L + j] = pres[p] ? in[p * L + j] : 0;
    if (f > r) {
      for (int64_t j = 0; j < L; ++j) out_status[b * L + j] = DNAS_RS_FAILED, out_errors[b * L + j] = 0;
      continue;
    }
    rsErasureLocator(kGf, n, f, erased, gamma);
    for (int64_t j = 0; j < L; ++j) {
      uint8_t S[kRsMaxR], fixPos[kRsMaxR], fixVal[kRsMaxR];
      for (int i = 0; i < r; ++i) {
        uint8_t s = 0;
        for (int p = 0; p < n; ++p) s = (uint8_t)(gfMul(kGf, s, kGf.exp[i]) ^ out[p * L + j]);
        S[i] = s;
      }
      int nFix = 0, nErr = 0;
      const int status = rsSolveColumn(kGf, n, r, f, erased, gamma, pres, S, fixPos, fixVal, &nFix, &nErr);
      out_status[b * L + j] = (uint8_t)status;
      out_errors[b * L + j] = (uint8_t)nErr;
      for (int q = 0; q < nFix; ++q) {
        out[fixPos[q] * L + j] = (uint8_t)(out[fixPos[q] * L + j] ^ fixVal[q]);
        if (q >= f) ++fixed[fixPos[q]];
      }
    }
  }
}

}  // namespace dnas

namespace {

template <class F>
int rsGuarded(F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

}  // namespace

extern "C" {

int dnas_rs_encode_host(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t* data, uint8_t* out_blocks) {
  if (const int rc = dnas::checkRsCode(n, k, L, B)) return rc;
  if (B && (!data || !out_blocks)) return dnas::fail(DNAS_E_INVALID, "reed-solomon: null argument");
  return rsGuarded([&] {
    dnas::rsEncodeHost(n, k, L, 0, B, data, out_blocks);
    return (int)DNAS_OK;
  });
}

int dnas_rs_decode_host(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t* blocks, const uint8_t* present, uint8_t* out_blocks,
                        uint8_t* out_status, uint8_t* out_errors, int32_t* out_fixed) {
  if (const int rc = dnas::checkRsCode(n, k, L, B)) return rc;
  if (B && (!blocks || !present || !out_blocks || !out_status || !out_errors || !out_fixed))
    return dnas::fail(DNAS_E_INVALID, "reed-solomon: null argument");
  return rsGuarded([&] {
    dnas::rsDecodeHost(n, k, L, 0, B, blocks, present, out_blocks, out_status, out_errors, out_fixed);
    return (int)DNAS_OK;
  });
}

uint8_t dnas_outer_crc8(const uint8_t* bytes, int64_t len) { return bytes && len > 0 ? dnas::outerCrc8(bytes, len) : 0; }

}  // extern "C"
