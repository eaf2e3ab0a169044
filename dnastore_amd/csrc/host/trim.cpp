// dnas_trim_reads_host: the statement of include/dnastore_amd.h, "Demultiplexing and trimming", as plain loops -- the two-row
// dynamic program of the search, every (pair, strand) of every read in (k, s) order, one thread.  No bit vectors.
#include "trim.hpp"

#include <algorithm>
#include <string>

#include "../errors.hpp"

namespace dnas {

int checkTrimArgs(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t n_reads, const int8_t* read_seqs,
                  const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors, int32_t min_payload,
                  const int32_t* out_pair, const uint8_t* out_strand, const int32_t* out_begin, const int32_t* out_end,
                  const int32_t* out_edits, const int32_t* out_second, const uint8_t* out_status) {
  if (n_pairs < 0 || n_reads < 0) return fail(DNAS_E_INVALID, "trim reads: bad argument");
  if (max_edit_permille < 0 || max_edit_permille > 1000) return fail(DNAS_E_INVALID, "trim reads: max_edit_permille must be 0 .. 1000");
  if (max_offset < -1) return fail(DNAS_E_INVALID, "trim reads: max_offset must be -1 (the whole read) or at least 0");
  if (anchors != DNAS_TRIM_BOTH && anchors != DNAS_TRIM_EITHER) return fail(DNAS_E_INVALID, "trim reads: anchors must be 0 (both) or 1 (either)");
  if (min_payload < 0) return fail(DNAS_E_INVALID, "trim reads: min_payload must be at least 0");
  if (n_pairs >= ((int64_t)1 << 30)) return fail(DNAS_E_UNSUPPORTED, "trim reads: 2^30 primer pairs or more");
  if (n_reads >= ((int64_t)1 << 31)) return fail(DNAS_E_UNSUPPORTED, "trim reads: 2^31 reads or more");
  if (n_pairs > 0) {
    if (!primer_seqs || !primer_off) return fail(DNAS_E_INVALID, "trim reads: null argument");
    if (primer_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
    for (int64_t q = 0; q < 2 * n_pairs; ++q) {
      const int64_t m = primer_off[q + 1] - primer_off[q];
      if (m < 1 || m > kTrimMaxPrimer)
        return fail(DNAS_E_INVALID, "trim reads: primer " + std::to_string(q) + " must have 1 .. " + std::to_string(kTrimMaxPrimer) + " bases");
    }
    for (int64_t j = 0; j < primer_off[2 * n_pairs]; ++j) if (primer_seqs[j] < 0 || primer_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  }
  if (n_reads == 0) return DNAS_OK;
  if (!read_seqs || !read_off || !out_pair || !out_strand || !out_begin || !out_end || !out_edits || !out_second || !out_status)
    return fail(DNAS_E_INVALID, "trim reads: null argument");
  if (read_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t n = read_off[i + 1] - read_off[i];
    if (n < 0) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": inconsistent offsets");
    if (n >= ((int64_t)1 << 30)) return fail(DNAS_E_UNSUPPORTED, "read " + std::to_string(i) + ": 2^30 bases or more");
  }
  int bad = 0;
  for (int64_t j = 0; j < read_off[n_reads]; ++j) bad |= read_seqs[j] & ~3;
  if (bad) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

TrimHit trimSearchHost(const int8_t* pat, int32_t m, bool patReversed, const int8_t* read, int32_t n, int32_t s, bool fromEnd,
                       int32_t maxOffset) {
  const int32_t w = trimWindow(m, n, maxOffset);
  // column by column, two columns of m + 1 rows: col[r] = D[r][c]
  int32_t cols[2][kTrimMaxPrimer + 1];
  int32_t *prev = cols[0], *cur = cols[1];
  for (int32_t r = 0; r <= m; ++r) prev[r] = r;
  TrimHit hit{m, 0};
  for (int32_t c = 1; c <= w; ++c) {
    const int32_t t = trimTextBase(read, n, s, fromEnd, c - 1);
    cur[0] = 0;
    for (int32_t r = 1; r <= m; ++r) {
      const int32_t p = pat[patReversed ? m - r : r - 1];
      cur[r] = std::min(prev[r - 1] + (p != t), std::min(prev[r], cur[r - 1]) + 1);
    }
    if (cur[m] <= hit.e) hit = TrimHit{cur[m], c};
    std::swap(prev, cur);
  }
  return hit;
}

void trimReadsHost(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t first, int64_t last,
                   const int8_t* read_seqs, const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors,
                   int32_t min_payload, int32_t* out_pair, uint8_t* out_strand, int32_t* out_begin, int32_t* out_end, int32_t* out_edits,
                   int32_t* out_second, uint8_t* out_status) {
  for (int64_t i = first; i < last; ++i) {
    const int8_t* read = read_seqs + read_off[i];
    const int32_t n = (int32_t)(read_off[i + 1] - read_off[i]);
    TrimBest best;
    for (int64_t k = 0; k < n_pairs; ++k) {
      const int8_t *F = primer_seqs + primer_off[2 * k], *R = primer_seqs + primer_off[2 * k + 1];
      const int32_t mF = (int32_t)(primer_off[2 * k + 1] - primer_off[2 * k]), mR = (int32_t)(primer_off[2 * k + 2] - primer_off[2 * k + 1]);
      for (int32_t s = 0; s < 2; ++s) {
        const TrimHit f = trimSearchHost(F, mF, false, read, n, s, false, max_offset);
        const TrimHit r = trimSearchHost(R, mR, true, read, n, s, true, max_offset);
        trimOffer(best, (int32_t)k, s, n, f, mF, r, mR, max_edit_permille, anchors, min_payload);
      }
    }
    trimFinish(best, n, out_pair + i, out_strand + i, out_begin + i, out_end + i, out_edits + 2 * i, out_second + i, out_status + i);
  }
}

}  // namespace dnas
