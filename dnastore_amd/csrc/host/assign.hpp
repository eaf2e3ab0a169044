// Read assignment (include/dnastore_amd.h, dnas_assign_reads): which original of a library, in which orientation, a read of
// a shuffled pool came from -- the one under which the pair-HMM Viterbi score S(I,O) of pairalign.hpp is largest.  This file
// holds what the host statement and the kernels (assign_kernels.hip) share: the fold of a read's item scores, stated once for
// both, the item arithmetic, and the argument checks.
#pragma once
#include <cstdint>

#include "pairalign.hpp"

#if defined(__HIP__)
#define DNAS_HD __host__ __device__
#else
#define DNAS_HD
#endif

namespace dnas {

// The fold over a read's items in item order.  best: the first item strictly greater than every earlier one (and than -inf);
// second: the largest score among the items whose original is not the winner's.  When the winner passes from original X to
// another original Y, every item seen so far scores at most X's best and X's best is not Y's: the runner-up is the old best.
struct AssignFold {
  double best, second;
  int64_t original;
  int32_t strand;
  DNAS_HD AssignFold() : best(-__builtin_huge_val()), second(-__builtin_huge_val()), original(-1), strand(0) {}
  DNAS_HD void add(double score, int64_t orig, int32_t st) {
    if (score > best) {
      if (orig != original) second = best;
      best = score;
      original = orig;
      strand = st;
    } else if (orig != original && score > second) {
      second = score;
    }
  }
  DNAS_HD uint8_t status(int64_t items) const {
    return items == 0 ? DNAS_ASSIGN_NO_CANDIDATES : (original < 0 ? DNAS_ASSIGN_NO_PATH : DNAS_ASSIGN_OK);
  }
};

// Orientations per candidate, and the strand of orientation o (0 .. strandsOf - 1) of a candidate.
DNAS_HD inline int strandsOf(int strand_mode) { return strand_mode == DNAS_STRAND_BOTH ? 2 : 1; }
DNAS_HD inline int strandAt(int strand_mode, int o) { return strand_mode == DNAS_STRAND_BOTH ? o : (strand_mode == DNAS_STRAND_REVERSE ? 1 : 0); }

// DNAS_OK or the code, dnas_last_error set: what dnas_assigner_create and dnas_assign_reads_host check of the originals ...
int checkAssignOriginals(const dnas_mutator_params* params, int32_t band, int64_t n_originals, const int8_t* orig_seqs,
                         const int64_t* orig_off);
// ... and what a run checks of the reads, the strand mode, the candidate lists and the outputs.
int checkAssignReads(int64_t n_originals, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode,
                     const int64_t* cand_off, const int64_t* cand_idx, const int64_t* out_original, const uint8_t* out_strand,
                     const double* out_score, const double* out_second, const uint8_t* out_status);

// The statement: one thread, alignPairHost per item, the fold above.  The arguments were checked.
void assignReadsHost(const PairScores& sc, int64_t band, int64_t n_originals, const int8_t* orig_seqs, const int64_t* orig_off,
                     int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode, const int64_t* cand_off,
                     const int64_t* cand_idx, int64_t* out_original, uint8_t* out_strand, double* out_score, double* out_second,
                     uint8_t* out_status, double* out_item_scores);

}  // namespace dnas
