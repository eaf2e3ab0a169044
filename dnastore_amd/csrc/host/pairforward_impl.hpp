// The forward recurrence of host/pairforward.hpp as a template, so that forwardPairHost (which keeps two rows) and pairCountsHost
// (host/paircounts.cpp, which keeps every cell) run the same code: keep(ip, op, s, d, T, lanes) is called once per cell inside
// the band, in row order, with the cell's finished S, D and T_0 .. T_{lanes-1}.
#pragma once
#include <algorithm>
#include <limits>
#include <vector>

#include "pairalign.hpp"

namespace dnas {

template <class Lse, class Keep>
double forwardPairRows(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                       const Lse& lse, Keep&& keep) {
  constexpr double kNegInf = -std::numeric_limits<double>::infinity();
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
      keep(ip, op, s, d, Tcur, lanes);
    }
  }
  return S[I & 1][(size_t)O];
}

}  // namespace dnas
