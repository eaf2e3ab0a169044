#include "assign.hpp"

#include <string>
#include <vector>

#include "../errors.hpp"

namespace dnas {

int checkAssignOriginals(const dnas_mutator_params* params, int32_t band, int64_t n_originals, const int8_t* orig_seqs,
                         const int64_t* orig_off) {
  if (!params || n_originals < 0) return fail(DNAS_E_INVALID, "assign reads: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "assign reads: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen) return fail(DNAS_E_UNSUPPORTED, "assign reads: more than 13 duplication lengths");
  if (n_originals == 0) return DNAS_OK;
  if (!orig_seqs || !orig_off) return fail(DNAS_E_INVALID, "assign reads: null argument");
  if (orig_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_originals; ++i) {
    const int64_t I = orig_off[i + 1] - orig_off[i];
    if (I < 0) return fail(DNAS_E_INVALID, "original " + std::to_string(i) + ": inconsistent offsets");
    if (I > kAlignMaxSeq) return fail(DNAS_E_UNSUPPORTED, "original " + std::to_string(i) + ": longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < orig_off[n_originals]; ++j) if (orig_seqs[j] < 0 || orig_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

int checkAssignReads(int64_t n_originals, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode,
                     const int64_t* cand_off, const int64_t* cand_idx, const int64_t* out_original, const uint8_t* out_strand,
                     const double* out_score, const double* out_second, const uint8_t* out_status) {
  if (n_reads < 0) return fail(DNAS_E_INVALID, "assign reads: bad argument");
  if (strand_mode != DNAS_STRAND_FORWARD && strand_mode != DNAS_STRAND_REVERSE && strand_mode != DNAS_STRAND_BOTH)
    return fail(DNAS_E_INVALID, "assign reads: strand_mode must be DNAS_STRAND_FORWARD, _REVERSE or _BOTH");
  if (n_reads == 0) return DNAS_OK;
  if (!read_seqs || !read_off || !out_original || !out_strand || !out_score || !out_second || !out_status)
    return fail(DNAS_E_INVALID, "assign reads: null argument");
  if (read_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t O = read_off[i + 1] - read_off[i];
    if (O < 0) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": inconsistent offsets");
    if (O > kAlignMaxSeq) return fail(DNAS_E_UNSUPPORTED, "read " + std::to_string(i) + ": longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < read_off[n_reads]; ++j) if (read_seqs[j] < 0 || read_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  if (cand_off) {
    if (cand_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
    for (int64_t i = 0; i < n_reads; ++i)
      if (cand_off[i + 1] < cand_off[i]) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": inconsistent candidate offsets");
    if (cand_off[n_reads] && !cand_idx) return fail(DNAS_E_INVALID, "assign reads: null argument");
    for (int64_t j = 0; j < cand_off[n_reads]; ++j)
      if (cand_idx[j] < 0 || cand_idx[j] >= n_originals)
        return fail(DNAS_E_INVALID, "candidate " + std::to_string(j) + ": original " + std::to_string(cand_idx[j]) + " of " + std::to_string(n_originals));
  }
  return DNAS_OK;
}

void assignReadsHost(const PairScores& sc, int64_t band, int64_t n_originals, const int8_t* orig_seqs, const int64_t* orig_off,
                     int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode, const int64_t* cand_off,
                     const int64_t* cand_idx, int64_t* out_original, uint8_t* out_strand, double* out_score, double* out_second,
                     uint8_t* out_status, double* out_item_scores) {
  const int strands = strandsOf(strand_mode);
  std::vector<int8_t> rc;
  for (int64_t r = 0; r < n_reads; ++r) {
    const int8_t* const b = read_seqs + read_off[r];
    const int64_t O = read_off[r + 1] - read_off[r];
    rc.resize((size_t)O);
    for (int64_t j = 0; j < O; ++j) rc[(size_t)j] = (int8_t)(3 - b[O - 1 - j]);
    const int64_t cands = cand_off ? cand_off[r + 1] - cand_off[r] : n_originals;
    AssignFold fold;
    for (int64_t c = 0; c < cands; ++c) {
      const int64_t orig = cand_off ? cand_idx[cand_off[r] + c] : c;
      for (int o = 0; o < strands; ++o) {
        const int st = strandAt(strand_mode, o);
        const double score = alignPairHost(sc, orig_seqs + orig_off[orig], orig_off[orig + 1] - orig_off[orig], st ? rc.data() : b, O, band, nullptr);
        fold.add(score, orig, st);
        if (out_item_scores) *out_item_scores++ = score;
      }
    }
    out_original[r] = fold.original;
    out_strand[r] = (uint8_t)fold.strand;
    out_score[r] = fold.best;
    out_second[r] = fold.second;
    out_status[r] = fold.status(cands * strands);
  }
}

}  // namespace dnas
