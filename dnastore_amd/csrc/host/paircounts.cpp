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

// The keepers of the backward sweep: each is handed the posterior p of every move out of a cell, in the order of paircounts.hpp.
// kEveryMove = false: delEnd and the T_k emissions are not formed at all.

// MutatorCounts order, [21 + P].
struct KeepCounts {
  static constexpr bool kEveryMove = true;
  double* counts;
  void match(int64_t, int x, int y, double p) const {
    counts[2] += p;
    counts[5 + x * 4 + y] += p;
  }
  void delOpen(int64_t, double p) const { counts[0] += p; }
  void dup(int64_t, int k, double p) const {
    counts[1] += p;
    counts[21 + k] += p;
  }
  void delExtend(int64_t, double p) const { counts[3] += p; }
  void delEnd(double p) const { counts[4] += p; }
  void emit(int x, int y, double p) const { counts[5 + x * 4 + y] += p; }
};

// The moves that consume in[ip] or insert in front of it, filed by row: plane j of row ip at profile[j * rows + ip].
struct KeepProfile {
  static constexpr bool kEveryMove = false;
  double* profile;
  int64_t rows;
  void match(int64_t ip, int, int y, double p) const { profile[(DNAS_PROFILE_MATCH + y) * rows + ip] += p; }
  void delOpen(int64_t ip, double p) const { profile[DNAS_PROFILE_DEL_OPEN * rows + ip] += p; }
  void dup(int64_t ip, int k, double p) const { profile[(DNAS_PROFILE_DUP + k) * rows + ip] += p; }
  void delExtend(int64_t ip, double p) const { profile[DNAS_PROFILE_DEL_EXTEND * rows + ip] += p; }
  void delEnd(double) const {}
  void emit(int, int, double) const {}
};

// Both passes; what keep holds was zeroed by the caller.
template <class Lse, class Keep>
bool pairPosteriors(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                    const Lse& lse, const Keep& keep, double* ll, double* llBackward) {
  const PairBand bd(I, O, band);
  const int P = sc.P;

  // pass 1: the forward code of forwardPairHost, every cell kept; row ip starts at rowStart[ip], column rowLo(ip) first
  std::vector<size_t> rowStart((size_t)I + 2, 0);
  for (int64_t ip = 0; ip <= I; ++ip) rowStart[(size_t)ip + 1] = rowStart[(size_t)ip] + (size_t)(bd.rowHi(ip, O) - bd.rowLo(ip) + 1);
  const size_t cells = rowStart[(size_t)I + 1];
  const int kept = Keep::kEveryMove ? P : 0;                 // the T lanes are met again only by their emissions
  std::vector<double> FS(cells), FD(cells), FT(cells * (size_t)kept);
  const auto cellAt = [&](int64_t ip, int64_t op) { return rowStart[(size_t)ip] + (size_t)(op - bd.rowLo(ip)); };
  const double Z = forwardPairRows(sc, in, I, out, O, band, rev, lse,
                                   [&](int64_t ip, int64_t op, double s, double d, const double* T, int) {
                                     const size_t c = cellAt(ip, op);
                                     FS[c] = s;
                                     FD[c] = d;
                                     for (int k = 0; k < kept; ++k) FT[c * (size_t)P + (size_t)k] = T[k];
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
      if (ip < I && op < O) keep.match(ip, in[ip], y, std::exp(fs + sc.noGap + sub0 + sDiag - Z));
      if (ip < I) keep.delOpen(ip, std::exp(fs + sc.delOpen + dDn - Z));
      for (int k = 0; k < lanes; ++k) keep.dup(ip, k, std::exp(fs + sc.tanDup + sc.len[k] + Tcur[k] - Z));
      if (ip < I) keep.delExtend(ip, std::exp(fd + sc.delExtend + dDn - Z));
      if constexpr (Keep::kEveryMove) {
        keep.delEnd(std::exp(fd + sc.delEnd + bs - Z));
        if (op < O)
          for (int k = 0; k < lanes; ++k) {
            const int x = in[ip - 1 - k];
            keep.emit(x, y, std::exp(FT[c * (size_t)P + (size_t)k] + sc.sub[x * 4 + y] + target[k] - Z));
          }
      }
    }
  }
  if (llBackward) *llBackward = BS[0][0];
  return true;
}

template <class Keep>
bool pairPosteriorsHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                        bool exactLse, const Keep& keep, double* ll, double* llBackward) {
  if (exactLse)
    return pairPosteriors(sc, in, I, out, O, band, rev, [](double a, double b) { return lseExactSum(a, b); }, keep, ll, llBackward);
  const double* tab = lseTable().data();
  return pairPosteriors(sc, in, I, out, O, band, rev, [tab](double a, double b) { return lseTableSum(tab, a, b); }, keep, ll,
                        llBackward);
}

}  // namespace

bool pairCountsHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                    bool exactLse, double* counts, double* ll, double* llBackward) {
  std::fill(counts, counts + 21 + sc.P, 0.);
  return pairPosteriorsHost(sc, in, I, out, O, band, rev, exactLse, KeepCounts{counts}, ll, llBackward);
}

bool pairProfileHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band, bool rev,
                     bool exactLse, double* profile, double* ll) {
  std::fill(profile, profile + (size_t)(DNAS_PROFILE_DUP + sc.P) * (size_t)(I + 1), 0.);
  return pairPosteriorsHost(sc, in, I, out, O, band, rev, exactLse, KeepProfile{profile, I + 1}, ll, nullptr);
}

ProfileSum::ProfileSum(int P, int anchor, int64_t nPositions, double* profile, int64_t* coverage)
    : P_(P), anchor_(anchor), n_(nPositions), profile_(profile), coverage_(coverage) {
  std::fill(profile, profile + (size_t)(5 + P) * (size_t)nPositions, 0.);
  std::fill(coverage, coverage + nPositions, (int64_t)0);
}

void ProfileSum::add(const int8_t* in, int64_t I, const double* block) {
  const int64_t rows = I + 1;
  const auto at = [&](int plane, int64_t r) { return block[(size_t)plane * (size_t)rows + (size_t)r]; };
  for (int64_t r = 0; r <= I; ++r) {
    const int64_t p = anchor_ ? I - r : r;
    if (p >= n_) continue;
    ++coverage_[p];
    double* const col = profile_ + p;
    if (r < I) {
      const int x = in[r] & 3;
      for (int y = 0; y < 4; ++y) col[(y == x ? 0 : y == (x ^ 2) ? 1 : 2) * n_] += at(DNAS_PROFILE_MATCH + y, r);
      col[3 * n_] += at(DNAS_PROFILE_DEL_OPEN, r);
      col[4 * n_] += at(DNAS_PROFILE_DEL_EXTEND, r);
    }
    for (int k = 0; k < P_; ++k) col[(5 + k) * n_] += at(DNAS_PROFILE_DUP + k, r);
  }
}

void pairProfilesHostAll(const PairScores& sc, int64_t band, int64_t n, const int8_t* in_seqs, const int64_t* in_off,
                         const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev, bool exactLse, ProfileSum* sum,
                         double* out_pair_profiles, double* out_pair_ll, uint8_t* out_status) {
  const size_t W = (size_t)(DNAS_PROFILE_DUP + sc.P);
  std::vector<double> own;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t I = in_off[i + 1] - in_off[i];
    double* block;
    if (out_pair_profiles) {
      block = out_pair_profiles + W * (size_t)(in_off[i] + i);
    } else {
      own.resize(W * (size_t)(I + 1));
      block = own.data();
    }
    const bool ok = pairProfileHost(sc, in_seqs + in_off[i], I, out_seqs + out_off[i], out_off[i + 1] - out_off[i], band,
                                    out_rev != nullptr && out_rev[i] != 0, exactLse, block, out_pair_ll + i);
    out_status[i] = ok ? DNAS_COUNTS_OK : DNAS_COUNTS_NO_PATH;
    if (ok) sum->add(in_seqs + in_off[i], I, block);
  }
}

int checkProfileArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                     const int8_t* out_seqs, const int64_t* out_off, int32_t anchor, int64_t n_positions, const double* out_profile,
                     const int64_t* out_coverage, const double* out_pair_ll, const uint8_t* out_status) {
  if (anchor != DNAS_PROFILE_FROM_START && anchor != DNAS_PROFILE_FROM_END)
    return fail(DNAS_E_INVALID, "pair profiles: anchor must be DNAS_PROFILE_FROM_START (0) or DNAS_PROFILE_FROM_END (1)");
  if (n_positions < 0) return fail(DNAS_E_INVALID, "pair profiles: negative n_positions");
  if (n_positions > 0 && (!out_profile || !out_coverage)) return fail(DNAS_E_INVALID, "pair profiles: null argument");
  if (const int rc = checkForwardArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_pair_ll)) return rc;
  if (n_pairs > 0 && !out_status) return fail(DNAS_E_INVALID, "pair profiles: null argument");
  return DNAS_OK;
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
