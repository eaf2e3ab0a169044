#include "pairforward.hpp"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../errors.hpp"
#include "lsetable.hpp"
#include "pairforward_impl.hpp"

namespace dnas {
namespace {

template <class Lse>
double forwardPair(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                   const Lse& lse) {
  return forwardPairRows(sc, in, I, out, O, band, rev, lse, [](int64_t, int64_t, double, double, const double*, int) {});
}

}  // namespace

double forwardPairHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                       bool exactLse) {
  if (exactLse) return forwardPair(sc, in, I, out, O, band, rev, [](double a, double b) { return lseExactSum(a, b); });
  const double* tab = lseTable().data();
  return forwardPair(sc, in, I, out, O, band, rev, [tab](double a, double b) { return lseTableSum(tab, a, b); });
}

int checkForwardArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                     const int8_t* out_seqs, const int64_t* out_off, const double* out_ll) {
  if (!params || n_pairs < 0) return fail(DNAS_E_INVALID, "pair likelihoods: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "pair likelihoods: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen) return fail(DNAS_E_UNSUPPORTED, "pair likelihoods: more than 13 duplication lengths");
  if (n_pairs == 0) return DNAS_OK;
  if (!in_seqs || !in_off || !out_seqs || !out_off || !out_ll) return fail(DNAS_E_INVALID, "pair likelihoods: null argument");
  if (in_off[0] != 0 || out_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
    if (I < 0 || O < 0) return fail(DNAS_E_INVALID, "pair " + std::to_string(i) + ": inconsistent offsets");
    if (I > kAlignMaxSeq || O > kAlignMaxSeq)
      return fail(DNAS_E_UNSUPPORTED, "pair " + std::to_string(i) + ": sequences longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < in_off[n_pairs]; ++j) if (in_seqs[j] < 0 || in_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  for (int64_t j = 0; j < out_off[n_pairs]; ++j) if (out_seqs[j] < 0 || out_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

}  // namespace dnas
