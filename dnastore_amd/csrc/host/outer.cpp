// dnas_outer_encode, dnas_outer_decode (include/dnastore_amd.h, "The outer code"): the strand frame and the file layer over
// dnas_rs_encode / dnas_rs_decode.  A file becomes a stream (its length, the file, zeros), the stream the data strands of B blocks,
// every strand of a block a record (strand number, CRC-8, body); a pool of records becomes blocks with erasures, and the decoded
// blocks the file again.  Host code; the field arithmetic is behind the two calls.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../../include/dnastore_amd.h"
#include "../errors.hpp"
#include "rs.hpp"

namespace {

int checkOuter(int32_t n, int32_t k, int32_t L, int64_t B) {
  if (const int rc = dnas::checkRsCode(n, k, L, B)) return rc;
  if (B * n > ((int64_t)1 << 24)) return dnas::fail(DNAS_E_UNSUPPORTED, "outer code: a strand number has three bytes");
  return DNAS_OK;
}

template <class T>
T* handOut(const std::vector<T>& v) {
  T* p = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!p) throw std::bad_alloc();
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

template <class F>
int outerGuarded(F&& body) {
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

int64_t dnas_outer_blocks(int64_t file_len, int32_t k, int32_t L) {
  if (file_len < 0 || k < 1 || L < 1) return -1;
  const int64_t per = (int64_t)k * L;
  return (8 + file_len + per - 1) / per;
}

int dnas_outer_frame(int64_t strand, const uint8_t* body, int32_t L, uint8_t* out_record) {
  if (!body || !out_record || L < 1 || strand < 0 || strand >= ((int64_t)1 << 24)) return dnas::fail(DNAS_E_INVALID, "outer code: bad argument");
  out_record[0] = (uint8_t)(strand >> 16), out_record[1] = (uint8_t)(strand >> 8), out_record[2] = (uint8_t)strand;
  out_record[3] = dnas::outerCrc8(body, L, dnas::outerCrc8(out_record, 3));
  memmove(out_record + 4, body, (size_t)L);
  return DNAS_OK;
}

int dnas_outer_encode(const uint8_t* file, int64_t file_len, int32_t n, int32_t k, int32_t L, int device_id, int host, int64_t* out_n_blocks,
                      uint8_t** out_records) {
  if (!out_n_blocks || !out_records || file_len < 0 || (file_len && !file)) return dnas::fail(DNAS_E_INVALID, "outer code: bad argument");
  *out_records = nullptr;
  *out_n_blocks = 0;
  const int64_t B = dnas_outer_blocks(file_len, std::max(k, 1), std::max(L, 1));
  if (const int rc = checkOuter(n, k, L, B)) return rc;
  return outerGuarded([&] {
    std::vector<uint8_t> stream((size_t)(B * k * L), 0), blocks((size_t)(B * n * L));
    for (int b = 0; b < 8; ++b) stream[(size_t)b] = (uint8_t)((uint64_t)file_len >> (8 * b));
    if (file_len) memcpy(stream.data() + 8, file, (size_t)file_len);
    const int rc = host ? dnas_rs_encode_host(n, k, L, B, stream.data(), blocks.data())
                        : dnas_rs_encode(n, k, L, B, stream.data(), blocks.data(), nullptr, device_id);
    if (rc) return rc;
    const int64_t rec = 4 + (int64_t)L;
    std::vector<uint8_t> records((size_t)(B * n * rec));
    for (int64_t s = 0; s < B * n; ++s) dnas_outer_frame(s, blocks.data() + s * L, L, records.data() + s * rec);
    *out_records = handOut(records);
    *out_n_blocks = B;
    return (int)DNAS_OK;
  });
}

int dnas_outer_decode(int64_t n_records, const uint8_t* record_bytes, const int64_t* record_off, const double* weights, int32_t n, int32_t k,
                      int32_t L, int64_t B, int device_id, int host, uint8_t** out_data, int64_t* out_len, int32_t* out_status,
                      uint8_t* out_present, uint8_t* out_column_status, int32_t* out_fixed, int64_t** out_failed_ranges,
                      int64_t* out_n_ranges, dnas_outer_stats* out_stats) {
  if (out_stats) *out_stats = dnas_outer_stats{};
  if (!out_data || !out_len || !out_status || !out_failed_ranges || !out_n_ranges || n_records < 0 || (n_records && (!record_bytes || !record_off)))
    return dnas::fail(DNAS_E_INVALID, "outer code: bad argument");
  *out_data = nullptr, *out_failed_ranges = nullptr, *out_len = 0, *out_n_ranges = 0, *out_status = DNAS_OUTER_OK;
  if (const int rc = checkOuter(n, k, L, B)) return rc;
  if (B < 1 || !out_present || !out_column_status || !out_fixed) return dnas::fail(DNAS_E_INVALID, "outer code: bad argument");
  for (int64_t i = 0; i < n_records; ++i) {
    if (record_off[i + 1] < record_off[i]) return dnas::fail(DNAS_E_INVALID, "outer code: offsets must ascend");
    if (weights && !(weights[i] >= 0 && std::isfinite(weights[i]))) return dnas::fail(DNAS_E_INVALID, "outer code: a weight must be finite and at least 0");
  }
  return outerGuarded([&] {
    dnas_outer_stats st{};
    st.records = n_records;
    const int64_t rec = 4 + (int64_t)L, slots = B * n;
    // the valid records of every slot, in record order
    std::vector<int64_t> slotOf((size_t)n_records, -1), head((size_t)slots + 1, 0);
    for (int64_t i = 0; i < n_records; ++i) {
      const uint8_t* p = record_bytes + record_off[i];
      bool ok = record_off[i + 1] - record_off[i] == rec;
      if (ok) ok = dnas::outerCrc8(p + 4, L, dnas::outerCrc8(p, 3)) == p[3];
      const int64_t s = ok ? (int64_t)p[0] << 16 | (int64_t)p[1] << 8 | p[2] : -1;
      if (ok && s < slots) slotOf[(size_t)i] = s, ++head[(size_t)s + 1];
      else ++st.dropped;
    }
    for (int64_t s = 0; s < slots; ++s) head[(size_t)s + 1] += head[(size_t)s];
    std::vector<int64_t> order((size_t)head[(size_t)slots]), fill(head.begin(), head.end() - 1);
    for (int64_t i = 0; i < n_records; ++i)
      if (slotOf[(size_t)i] >= 0) order[(size_t)fill[(size_t)slotOf[(size_t)i]]++] = i;
    // per slot: identical records form a group, the heaviest group wins, a tie of the top two is an erasure
    std::vector<uint8_t> blocks((size_t)(slots * L), 0);
    struct Group {
      int64_t first;
      double weight;
    };
    std::vector<Group> groups;
    for (int64_t s = 0; s < slots; ++s) {
      groups.clear();
      for (int64_t at = head[(size_t)s]; at < head[(size_t)s + 1]; ++at) {
        const int64_t i = order[(size_t)at];
        const double w = weights ? weights[i] : 1.0;
        size_t g = 0;
        while (g < groups.size() && memcmp(record_bytes + record_off[groups[g].first], record_bytes + record_off[i], (size_t)rec) != 0) ++g;
        if (g == groups.size()) groups.push_back(Group{i, w});
        else groups[g].weight += w;
      }
      int64_t best = -1, second = -1;
      for (size_t g = 0; g < groups.size(); ++g) {
        if (best < 0 || groups[g].weight > groups[(size_t)best].weight) second = best, best = (int64_t)g;
        else if (second < 0 || groups[g].weight > groups[(size_t)second].weight) second = (int64_t)g;
      }
      if (groups.size() > 1) ++st.conflicts;
      const bool tie = second >= 0 && groups[(size_t)second].weight == groups[(size_t)best].weight;
      if (tie) ++st.ties;
      out_present[s] = best >= 0 && !tie;
      if (out_present[s]) memcpy(blocks.data() + s * L, record_bytes + record_off[groups[(size_t)best].first] + 4, (size_t)L);
      else ++st.erased;
    }
    std::vector<uint8_t> decoded((size_t)(slots * L)), errors((size_t)(B * L));
    const int rc = host ? dnas_rs_decode_host(n, k, L, B, blocks.data(), out_present, decoded.data(), out_column_status, errors.data(), out_fixed)
                        : dnas_rs_decode(n, k, L, B, blocks.data(), out_present, decoded.data(), out_column_status, errors.data(), out_fixed,
                                         &st.rs, device_id);
    if (rc) return rc;
    for (int64_t s = 0; s < slots; ++s) st.strands_fixed += out_fixed[s] != 0;
    // the stream, and which of its bytes lie in failed columns
    const int64_t streamLen = B * k * L;
    std::vector<uint8_t> stream((size_t)streamLen), lost((size_t)streamLen, 0);
    for (int64_t b = 0; b < B; ++b) {
      memcpy(stream.data() + b * k * L, decoded.data() + b * n * L, (size_t)k * L);
      for (int64_t j = 0; j < L; ++j) {
        const uint8_t cs = out_column_status[b * L + j];
        ++(cs == DNAS_RS_OK ? st.columns_ok : cs == DNAS_RS_CORRECTED ? st.columns_corrected : st.columns_failed);
        if (cs == DNAS_RS_FAILED)
          for (int64_t p = 0; p < k; ++p) lost[(size_t)((b * k + p) * L + j)] = 1;
      }
    }
    bool prefixLost = false;
    for (int64_t i = 0; i < 8 && i < streamLen; ++i) prefixLost = prefixLost || lost[(size_t)i];
    uint64_t len = 0;
    for (int b = 0; b < 8 && b < streamLen; ++b) len |= (uint64_t)stream[(size_t)b] << (8 * b);
    int64_t from = 8, to = 8 + (int64_t)len;
    if (prefixLost) *out_status = DNAS_OUTER_NO_LENGTH;
    else if (streamLen < 8 || len > (uint64_t)(streamLen - 8)) *out_status = DNAS_OUTER_BAD_LENGTH;
    if (*out_status != DNAS_OUTER_OK) from = 0, to = streamLen;      // the raw stream, ranges in its coordinates
    std::vector<int64_t> ranges;
    for (int64_t i = from; i < to; ++i)
      if (lost[(size_t)i]) {
        if (!ranges.empty() && ranges.back() == i - from) ranges.back() = i - from + 1;
        else ranges.push_back(i - from), ranges.push_back(i - from + 1);
      }
    if (*out_status == DNAS_OUTER_OK && !ranges.empty()) *out_status = DNAS_OUTER_DAMAGED;
    *out_data = handOut(std::vector<uint8_t>(stream.begin() + from, stream.begin() + to));
    *out_len = to - from;
    *out_failed_ranges = handOut(ranges);
    *out_n_ranges = (int64_t)ranges.size() / 2;
    if (out_stats) *out_stats = st;
    return (int)DNAS_OK;
  });
}

}  // extern "C"
