// The EM loop of the error model (reference baumWelchParams, fwdback.cpp:211-230, with MutatorCounts::mlParams / logPrior,
// mutator.cpp:167-214), stated once for every fit: dnas_baum_welch over the guided E-step, dnas_baum_welch_pairs and its host
// twin over the marginal one.  The loop is a template on the E-step, so the fits cannot drift apart.
#pragma once
#include <cmath>
#include <vector>

#include "../../../include/dnastore_amd.h"

namespace dnas {

constexpr int kBaumWelchMaxIter = 100;          // BaumWelchMaxIter, fwdback.cpp:8
constexpr double kBaumWelchMinFracInc = .001;   // BaumWelchMinFracInc, fwdback.cpp:7,221

inline bool bwIsTransition(int x, int y) { return x != y && (x & 1) == (y & 1); }
inline double bwMatches(const double* c) { return c[5] + c[10] + c[15] + c[20]; }
inline double bwTransitions(const double* c) {
  double n = 0;
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) if (bwIsTransition(i, j)) n += c[5 + i * 4 + j];
  return n;
}
inline double bwTransversions(const double* c) {
  double n = 0;
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) if (i != j && !bwIsTransition(i, j)) n += c[5 + i * 4 + j];
  return n;
}
inline double logBetaPdfCounts(double prob, double yes, double no) {   // logsumexp.cpp:59-61,67-69
  const double al = yes + 1, be = no + 1;
  return std::lgamma(al + be) - std::lgamma(al) - std::lgamma(be) + (al - 1) * std::log(prob) + (be - 1) * std::log(1 - prob);
}
inline double logDirichletPdfCounts3(const double* prob, const double* count) {   // logsumexp.cpp:62-66,70-76
  double alpha[3];
  for (int n = 0; n < 3; ++n) alpha[n] = count[n] + 1;
  double ld = std::lgamma(0. + alpha[0] + alpha[1] + alpha[2]);
  for (int n = 0; n < 3; ++n) ld += (alpha[n] - 1) * std::log(prob[n]) - std::lgamma(alpha[n]);
  return ld;
}
inline double logPrior(const double* prior, const dnas_mutator_params& p) {   // MutatorCounts::logPrior, mutator.cpp:204-214
  const double pGap[3] = {p.p_del_open, p.p_tan_dup, 1. - p.p_del_open - p.p_tan_dup};
  const double nGap[3] = {prior[0], prior[1], prior[2]};
  const double pSub[3] = {p.p_transition, p.p_transversion, 1. - p.p_transition - p.p_transversion};
  const double nSub[3] = {bwTransitions(prior), bwTransversions(prior), bwMatches(prior)};
  return logBetaPdfCounts(p.p_del_extend, prior[3], prior[4]) + logDirichletPdfCounts3(pGap, nGap) + logDirichletPdfCounts3(pSub, nSub);
}

// MutatorCounts::mlParams (mutator.cpp:167-178) of counts that already hold the prior: pLen back to uniform, local from init.
inline void mlParams(const double* counts, const dnas_mutator_params& init, dnas_mutator_params* cur) {
  const int P = cur->n_len;
  for (int k = 0; k < P; ++k) cur->p_len[k] = 1. / (double)P;
  cur->p_del_open = counts[0] / (counts[0] + counts[1] + counts[2]);
  cur->p_tan_dup = counts[1] / (counts[0] + counts[1] + counts[2]);
  cur->p_del_extend = counts[3] / (counts[3] + counts[4]);
  const double ni = bwTransitions(counts), nv = bwTransversions(counts), nm = bwMatches(counts);
  cur->p_transition = ni / (ni + nv + nm);
  cur->p_transversion = nv / (ni + nv + nm);
  cur->local = init.local;
}

// estep(params, counts[21 + P], &ll) -> DNAS_OK or a code, which ends the fit; seen(params, ll + log prior) is told of every
// E-step, the one that stops the loop included.  maxIter <= 0: kBaumWelchMaxIter.  The Laplace prior is a count of 1 everywhere
// (prior.initLaplace(), dnastore.cpp:137-138).
template <class EStep, class Seen>
int baumWelchLoop(const dnas_mutator_params& init, int maxIter, EStep&& estep, Seen&& seen, dnas_mutator_params* out,
                  int32_t* outIterations) {
  dnas_mutator_params cur = init;
  const int nc = 21 + cur.n_len;
  if (maxIter <= 0) maxIter = kBaumWelchMaxIter;
  std::vector<double> counts(nc), prior(nc, 1.);
  double best = -INFINITY;
  int iter = 0;
  for (; iter < maxIter; ++iter) {
    double ll = 0;
    const int rc = estep(cur, counts.data(), &ll);
    if (rc != DNAS_OK) return rc;
    ll += logPrior(prior.data(), cur);
    seen(cur, ll);
    if ((ll - best) / std::fabs(best) < kBaumWelchMinFracInc) break;
    best = ll;
    for (int k = 0; k < nc; ++k) counts[k] += prior[k];   // counts.mlParams(prior), mutator.cpp:198-202
    mlParams(counts.data(), init, &cur);
  }
  *out = cur;
  if (outIterations) *outIterations = iter;
  return DNAS_OK;
}

}  // namespace dnas
