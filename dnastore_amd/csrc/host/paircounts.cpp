#include "paircounts.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../errors.hpp"
#include "lsetable.hpp"
#include "pairforward.hpp"
#include "pairforward_impl.hpp"

namespace dnas {
namespace {

constexpr double kNegInf = -std::numeric_limits<double>::infinity();

// tree(v_0 .. v_{n-1}) of paircounts.hpp; v is overwritten.
template <class Lse>
double lseTree(double* v, int n, const Lse& lse) {
  while (n > 1) {
    const int h = n / 2;
    for (int i = 0; i < h; ++i) v[i] = lse(v[2 * i], v[2 * i + 1]);
    if (n & 1) v[h] = v[n - 1];
    n = (n + 1) / 2;
  }
  return v[0];
}

template <class Lse>
bool pairCounts(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                const Lse& lse, double* counts, double* ll, double* llBackward) {
  const PairBand bd(I, O, band);
  const int P = sc.P, nc = 21 + P;
  std::fill(counts, counts + nc, 0.);

  // pass 1: the forward code of forwardPairHost, every cell kept; row ip starts at rowStart[ip], column rowLo(ip) first
  std::vector<size_t> rowStart((size_t)I + 2, 0);
  for (int64_t ip = 0; ip <= I; ++ip) rowStart[(size_t)ip + 1] = rowStart[(size_t)ip] + (size_t)(bd.rowHi(ip, O) - bd.rowLo(ip) + 1);
  const size_t cells = rowStart[(size_t)I + 1];
  std::vector<double> FS(cells), FD(cells), FT(cells * (size_t)P);
  const auto cellAt = [&](int64_t ip, int64_t op) { return rowStart[(size_t)ip] + (size_t)(op - bd.rowLo(ip)); };
  const double Z = forwardPairRows(sc, in, I, out, O, band, rev, lse,
                                   [&](int64_t ip, int64_t op, double s, double d, const double* T, int) {
                                     const size_t c = cellAt(ip, op);
                                     FS[c] = s;
                                     FD[c] = d;
                                     for (int k = 0; k < P; ++k) FT[c * (size_t)P + (size_t)k] = T[k];
                                   });
  *ll = Z;
  if (!(Z > kNegInf)) {
    if (llBackward) *llBackward = kNegInf;
    return false;
  }

  // pass 2: rows last to first, columns right to left; two rows of B_S and B_D roll, two columns of the B_T lanes
  auto inside = [&](int64_t ip, int64_t op) { return ip <= I && op >= bd.rowLo(ip) && op <= bd.rowHi(ip, O); };
  auto base = [&](int64_t j) { return rev ? 3 - (out[O - 1 - j] & 3) : out[j] & 3; };
  std::vector<double> BS[2], BD[2];
  for (int h = 0; h < 2; ++h) {
    BS[h].assign((size_t)O + 2, kNegInf);
    BD[h].assign((size_t)O + 2, kNegInf);
  }
  double BT[2][kAlignMaxLen], v[kAlignMaxLen + 2];
  for (int64_t ip = I; ip >= 0; --ip) {
    const std::vector<double>&Sdn = BS[(ip + 1) & 1], &Ddn = BD[(ip + 1) & 1];
    std::vector<double>&Scur = BS[ip & 1], &Dcur = BD[ip & 1];
    const int lanes = (int)std::min<int64_t>(ip, P);
    for (int k = 0; k < kAlignMaxLen; ++k) BT[0][k] = BT[1][k] = kNegInf;
    for (int64_t op = bd.rowHi(ip, O); op >= bd.rowLo(ip); --op) {
      const double* Tnext = BT[(op + 1) & 1];   // the lanes of (ip, op + 1): -inf at the last column of the row
      double* Tcur = BT[op & 1];
      const int y = op < O ? base(op) : 0;
      const double sRight = inside(ip, op + 1) ? Scur[(size_t)op + 1] : kNegInf;
      const double sDiag = ip < I && op < O && inside(ip + 1, op + 1) ? Sdn[(size_t)op + 1] : kNegInf;
      const double dDn = ip < I && inside(ip + 1, op) ? Ddn[(size_t)op] : kNegInf;
      double target[kAlignMaxLen];
      for (int k = 0; k < lanes; ++k) {
        target[k] = k > 0 ? Tnext[k - 1] : sRight;
        Tcur[k] = op < O ? sc.sub[in[ip - 1 - k] * 4 + y] + target[k] : kNegInf;
      }
      for (int k = lanes; k < kAlignMaxLen; ++k) Tcur[k] = kNegInf;
      const double sub0 = ip < I && op < O ? sc.sub[in[ip] * 4 + y] : kNegInf;
      v[0] = (sc.noGap + sub0) + sDiag;
      v[1] = sc.delOpen + dDn;
      for (int k = 0; k < lanes; ++k) v[2 + k] = (sc.tanDup + sc.len[k]) + Tcur[k];
      const double bs = ip == I && op == O ? 0. : lseTree(v, 2 + lanes, lse);
      const double bdv = lse(sc.delExtend + dDn, sc.delEnd + bs);
      Scur[(size_t)op] = bs;
      Dcur[(size_t)op] = bdv;

      // the moves out of this cell
      const size_t c = cellAt(ip, op);
      const double fs = FS[c], fd = FD[c];
      double p;
      if (ip < I && op < O) {
        p = std::exp(fs + sc.noGap + sub0 + sDiag - Z);
        counts[2] += p;
        counts[5 + in[ip] * 4 + y] += p;
      }
      if (ip < I) counts[0] += std::exp(fs + sc.delOpen + dDn - Z);
      for (int k = 0; k < lanes; ++k) {
        p = std::exp(fs + sc.tanDup + sc.len[k] + Tcur[k] - Z);
        counts[1] += p;
        counts[21 + k] += p;
      }
      if (ip < I) counts[3] += std::exp(fd + sc.delExtend + dDn - Z);
      counts[4] += std::exp(fd + sc.delEnd + bs - Z);
      if (op < O)
        for (int k = 0; k < lanes; ++k) {
          const int x = in[ip - 1 - k];
          counts[5 + x * 4 + y] += std::exp(FT[c * (size_t)P + (size_t)k] + sc.sub[x * 4 + y] + target[k] - Z);
        }
    }
  }
  if (llBackward) *llBackward = BS[0][0];
  return true;
}

}  // namespace

bool pairCountsHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                    bool exactLse, double* counts, double* ll, double* llBackward) {
  if (exactLse)
    return pairCounts(sc, in, I, out, O, band, rev, [](double a, double b) { return lseExactSum(a, b); }, counts, ll, llBackward);
  const double* tab = lseTable().data();
  return pairCounts(sc, in, I, out, O, band, rev, [tab](double a, double b) { return lseTableSum(tab, a, b); }, counts, ll,
                    llBackward);
}

void pairCountsTotals(int64_t n, int nc, const double* pairCounts, const double* pairLl, const uint8_t* status, double* out_counts,
                      double* out_ll) {
  std::fill(out_counts, out_counts + nc, 0.);
  *out_ll = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (status[i] != DNAS_COUNTS_OK) continue;
    for (int k = 0; k < nc; ++k) out_counts[k] += pairCounts[(size_t)i * (size_t)nc + (size_t)k];
    *out_ll += pairLl[i];
  }
}

void pairCountsHostAll(const PairScores& sc, int64_t band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                       const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev, bool exactLse, double* out_counts,
                       double* out_ll, double* out_pair_counts, double* out_pair_ll, double* out_pair_ll_backward,
                       uint8_t* out_status) {
  const int nc = 21 + sc.P;
  std::vector<double> own;
  if (!out_pair_counts) {
    own.resize((size_t)std::max<int64_t>(n, 1) * (size_t)nc);
    out_pair_counts = own.data();
  }
  for (int64_t i = 0; i < n; ++i) {
    double back = 0;
    const bool ok = pairCountsHost(sc, in_seqs + in_off[i], in_off[i + 1] - in_off[i], out_seqs + out_off[i],
                                   out_off[i + 1] - out_off[i], band, out_rev != nullptr && out_rev[i] != 0, exactLse,
                                   out_pair_counts + (size_t)i * (size_t)nc, out_pair_ll + i, &back);
    if (out_pair_ll_backward) out_pair_ll_backward[i] = back;
    out_status[i] = ok ? DNAS_COUNTS_OK : DNAS_COUNTS_NO_PATH;
  }
  pairCountsTotals(n, nc, out_pair_counts, out_pair_ll, out_status, out_counts, out_ll);
}

int checkCountsArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                    const int8_t* out_seqs, const int64_t* out_off, const double* out_counts, const double* out_ll,
                    const double* out_pair_ll, const uint8_t* out_status) {
  if (!out_counts || !out_ll) return fail(DNAS_E_INVALID, "pair counts: null argument");
  if (const int rc = checkForwardArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_pair_ll)) return rc;
  if (n_pairs > 0 && !out_status) return fail(DNAS_E_INVALID, "pair counts: null argument");
  return DNAS_OK;
}

}  // namespace dnas
