#include "pairforward.hpp"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../errors.hpp"
#include "lsetable.hpp"

namespace dnas {
namespace {

constexpr double kNegInf = -std::numeric_limits<double>::infinity();

template <class Lse>
double forwardPair(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                   const Lse& lse) {
  const PairBand bd(I, O, band);
  const int P = sc.P;
  // row ip holds the columns rowLo(ip) .. rowHi(ip), stored under the column itself; two rows of S and D roll
  std::vector<double> S[2], D[2];
  for (int h = 0; h < 2; ++h) {
    S[h].assign((size_t)O + 1, kNegInf);
    D[h].assign((size_t)O + 1, kNegInf);
  }
  auto inside = [&](int64_t ip, int64_t op) { return ip >= 0 && op >= bd.rowLo(ip) && op <= bd.rowHi(ip, O); };
  auto base = [&](int64_t j) { return rev ? 3 - (out[O - 1 - j] & 3) : out[j] & 3; };

  double T[2][kAlignMaxLen];
  for (int64_t ip = 0; ip <= I; ++ip) {
    const std::vector<double>&Sup = S[(ip + 1) & 1], &Dup = D[(ip + 1) & 1];
    std::vector<double>&Scur = S[ip & 1], &Dcur = D[ip & 1];
    const int lanes = (int)std::min<int64_t>(ip, P);
    for (int k = 0; k < kAlignMaxLen; ++k) T[0][k] = T[1][k] = kNegInf;
    for (int64_t op = bd.rowLo(ip); op <= bd.rowHi(ip, O); ++op) {
      const double* Tprev = T[(op + 1) & 1];   // the lanes of (ip, op - 1): -inf at the first column of the row
      double* Tcur = T[op & 1];
      const double sUp = inside(ip - 1, op) ? Sup[(size_t)op] : kNegInf, dUp = inside(ip - 1, op) ? Dup[(size_t)op] : kNegInf;
      const double d = lse(sUp + sc.delOpen, dUp + sc.delExtend);
      double s;
      if (ip == 0 && op == 0) {
        s = 0;
      } else {
        double s0 = kNegInf, s1 = kNegInf;
        if (ip > 0 && op > 0) {
          const double sub = sc.sub[in[ip - 1] * 4 + base(op - 1)];
          const double sDiag = inside(ip - 1, op - 1) ? Sup[(size_t)op - 1] : kNegInf;
          s0 = sDiag + sc.noGap + sub;
          if (P > 0) s1 = Tprev[0] + sub;
        }
        s = lse(lse(s0, s1), d + sc.delEnd);
      }
      for (int k = 0; k < lanes; ++k) {
        double t0 = kNegInf;
        if (op > 0 && k + 1 < lanes) t0 = Tprev[k + 1] + sc.sub[in[ip - 2 - k] * 4 + base(op - 1)];
        Tcur[k] = lse(t0, s + sc.tanDup + sc.len[k]);
      }
      for (int k = lanes; k < kAlignMaxLen; ++k) Tcur[k] = kNegInf;
      Scur[(size_t)op] = s;
      Dcur[(size_t)op] = d;
    }
  }
  return S[I & 1][(size_t)O];
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
