#include "pairalign.hpp"

#include <cmath>
#include <limits>
#include <stdexcept>

#include "../errors.hpp"

namespace dnas {
namespace {

constexpr double kNegInf = -std::numeric_limits<double>::infinity();
bool isTransition(int x, int y) { return x != y && (x & 1) == (y & 1); }

}  // namespace

PairScores PairScores::from(const MutatorParams& p) {
  PairScores s{};
  s.delOpen = std::log(p.pDelOpen);
  s.tanDup = std::log(p.pTanDup);
  s.noGap = std::log(p.pNoGap());
  s.delExtend = std::log(p.pDelExtend);
  s.delEnd = std::log(p.pDelEnd());
  const double nullScore = std::log(1. / 4.);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      s.sub[i * 4 + j] = (i == j ? std::log(p.pMatch())
                                 : (isTransition(i, j) ? std::log(p.pTransition) : std::log(p.pTransversion / 2))) -
                         nullScore;
  s.P = (int)p.pLen.size();
  for (int k = 0; k < kAlignMaxLen; ++k) s.len[k] = k < s.P ? std::log(p.pLen[(size_t)k]) : kNegInf;
  return s;
}

// The matrices S, D and the choice words are kept for every cell of the band (row ip holds the columns rowLo(ip) .. rowHi(ip));
// the duplication lanes never cross a row and only ever look one column back, so two columns of them are.
double alignPairHost(const PairScores& sc, const int8_t* in, int64_t I, const int8_t* out, int64_t O, int64_t band,
                     std::vector<uint8_t>* ops) {
  const PairBand bd(I, O, band);
  const int P = sc.P;
  const int64_t width = std::min(O + 1, bd.hi - bd.lo + 1);
  std::vector<double> S((size_t)((I + 1) * width), kNegInf), D(S.size(), kNegInf);
  std::vector<uint16_t> choice(S.size(), 0);
  auto at = [&](int64_t ip, int64_t op) { return (size_t)(ip * width + (op - bd.rowLo(ip))); };
  auto inside = [&](int64_t ip, int64_t op) { return ip >= 0 && op >= bd.rowLo(ip) && op <= bd.rowHi(ip, O); };
  auto getS = [&](int64_t ip, int64_t op) { return inside(ip, op) ? S[at(ip, op)] : kNegInf; };
  auto getD = [&](int64_t ip, int64_t op) { return inside(ip, op) ? D[at(ip, op)] : kNegInf; };

  double T[2][kAlignMaxLen];
  for (int64_t ip = 0; ip <= I; ++ip) {
    const int lanes = (int)std::min<int64_t>(ip, P);
    for (int k = 0; k < kAlignMaxLen; ++k) T[0][k] = T[1][k] = kNegInf;
    for (int64_t op = bd.rowLo(ip); op <= bd.rowHi(ip, O); ++op) {
      double* Tprev = T[(op + 1) & 1];   // the lanes of (ip, op - 1): -inf at the first column of the row
      double* Tcur = T[op & 1];
      unsigned word = 0;
      double best, c;
      // D
      best = kNegInf;
      if (ip > 0) {
        c = getS(ip - 1, op) + sc.delOpen;
        if (c > best) { best = c; word &= ~4u; }
        c = getD(ip - 1, op) + sc.delExtend;
        if (c > best) { best = c; word |= 4u; }
      }
      const double d = best;
      // S
      best = kNegInf;
      if (ip == 0 && op == 0) {
        best = 0;
      } else {
        if (ip > 0 && op > 0) {
          const double sub = sc.sub[in[ip - 1] * 4 + out[op - 1]];
          c = getS(ip - 1, op - 1) + sc.noGap + sub;
          if (c > best) { best = c; word = (word & ~3u) | 0u; }
          if (P > 0) {
            c = Tprev[0] + sub;
            if (c > best) { best = c; word = (word & ~3u) | 1u; }
          }
        }
        c = d + sc.delEnd;
        if (c > best) { best = c; word = (word & ~3u) | 2u; }
      }
      const double s = best;
      // T_k
      for (int k = 0; k < lanes; ++k) {
        best = kNegInf;
        if (op > 0 && k + 1 < lanes) {
          c = Tprev[k + 1] + sc.sub[in[ip - 2 - k] * 4 + out[op - 1]];
          if (c > best) best = c;
        }
        c = s + sc.tanDup + sc.len[k];
        if (c > best) { best = c; word |= 8u << k; }
        Tcur[k] = best;
      }
      for (int k = lanes; k < kAlignMaxLen; ++k) Tcur[k] = kNegInf;
      S[at(ip, op)] = s;
      D[at(ip, op)] = d;
      choice[at(ip, op)] = (uint16_t)word;
    }
  }
  const double score = S[at(I, O)];
  if (ops) ops->clear();
  if (!ops || !(score > kNegInf)) return score;

  // traceback from (I, O, S) to (0, 0, S); state -1: S, -2: D, k >= 0: T_k
  std::vector<uint8_t>& rev = *ops;
  int64_t ip = I, op = O;
  int state = -1;
  while (!(ip == 0 && op == 0 && state == -1)) {
    if (!inside(ip, op)) throw std::logic_error("pair alignment traceback left the band");
    const unsigned w = choice[at(ip, op)];
    if (state == -1) {
      const unsigned c = w & 3u;
      if (c == 0) { rev.push_back(kOpMatch); --ip; --op; }
      else if (c == 1) { rev.push_back(kOpDup); --op; state = 0; }
      else state = -2;
    } else if (state == -2) {
      if (w & 4u) { rev.push_back(kOpDelete); --ip; }
      else { rev.push_back(kOpDelete | 1u << 2); --ip; state = -1; }
    } else {
      if (w & (8u << state)) { rev.back() |= (uint8_t)((state + 1) << 2); state = -1; }   // the column just written opened it
      else { rev.push_back(kOpDup); --op; ++state; }
    }
  }
  for (size_t a = 0, b = rev.size(); a + 1 < b; ++a, --b) std::swap(rev[a], rev[b - 1]);
  return score;
}

void expandAlignment(int nLen, const int8_t* in, int64_t I, const int8_t* out, int64_t O, const uint8_t* ops, int64_t nOps,
                     std::string* rowIn, std::string* rowOut, int32_t* cmIn, int32_t* cmOut, double* counts) {
  static const char kBase[] = "ACGT";
  auto bad = [](const std::string& what) { throw std::invalid_argument("alignment ops: " + what); };
  if (rowIn) rowIn->clear();
  if (rowOut) rowOut->clear();
  if (counts) for (int i = 0; i < 21 + nLen; ++i) counts[i] = 0;
  int64_t ip = 0, op = 0;
  int32_t matches = 0;
  if (cmIn) cmIn[0] = 0;
  if (cmOut) cmOut[0] = 0;
  int dupLeft = 0;                  // columns the open duplication still has to emit
  bool inDel = false;
  for (int64_t c = 0; c < nOps; ++c) {
    const unsigned kind = ops[c] & 3u, n = ops[c] >> 2;
    if (inDel && !(kind == kOpDelete && n == 0)) {
      if (counts) counts[4] += 1;   // nDelEnd
      inDel = false;
    }
    if (dupLeft > 0 && !(kind == kOpDup && n == 0)) bad("a duplication is cut short at column " + std::to_string(c));
    if (kind == kOpMatch) {
      if (n) bad("a match column with a length");
      if (ip >= I || op >= O) bad("more columns than bases");
      if (counts) { counts[2] += 1; counts[5 + in[ip] * 4 + out[op]] += 1; }
      if (rowIn) rowIn->push_back(kBase[in[ip] & 3]);
      if (rowOut) rowOut->push_back(kBase[out[op] & 3]);
      ++ip; ++op; ++matches;
      if (cmIn) cmIn[ip] = matches;
      if (cmOut) cmOut[op] = matches;
    } else if (kind == kOpDelete) {
      if (n > 1) bad("a deletion column with a length");
      if (n == 0 && !inDel) bad("a deletion is extended that was not opened");
      if (ip >= I) bad("more columns than bases");
      if (counts) counts[n ? 0 : 3] += 1;   // nDelOpen / nDelExtend
      inDel = true;
      if (rowIn) rowIn->push_back(kBase[in[ip] & 3]);
      if (rowOut) rowOut->push_back('-');
      ++ip;
      if (cmIn) cmIn[ip] = matches;
    } else if (kind == kOpDup) {
      if (n) {
        if ((int)n > nLen || (int64_t)n > ip) bad("a duplication longer than the model or the input so far allows");
        dupLeft = (int)n;
        if (counts) { counts[1] += 1; counts[21 + n - 1] += 1; }   // nTanDup, nLen[k]
      } else if (dupLeft == 0) {
        bad("a duplication column outside a duplication");
      }
      if (op >= O) bad("more columns than bases");
      const int8_t x = in[ip - dupLeft];      // the copy runs over in[ip - length .. ip)
      if (counts) counts[5 + x * 4 + out[op]] += 1;
      --dupLeft;
      if (rowIn) rowIn->push_back('-');
      if (rowOut) rowOut->push_back(kBase[out[op] & 3]);
      ++op;
      if (cmOut) cmOut[op] = matches;
    } else {
      bad("unknown column kind");
    }
  }
  if (inDel && counts) counts[4] += 1;
  if (dupLeft > 0) bad("a duplication is cut short at the end");
  if (ip != I || op != O) bad("the columns do not cover both sequences");
}

std::string writeStockholm(int64_t n, const char* const* namesIn, const char* const* namesOut, const char* const* rowsIn,
                           const char* const* rowsOut) {
  std::string text;
  for (int64_t i = 0; i < n; ++i) {
    const std::string a = namesIn[i], r1 = rowsIn[i], r2 = rowsOut[i];
    std::string b = namesOut[i];
    auto plain = [](const std::string& s) {
      if (s.empty() || s[0] == '#' || s.rfind("//", 0) == 0) return false;
      for (char c : s) if (c == ' ' || c == '\t' || c == '\n' || c == '\r') return false;
      return true;
    };
    if (!plain(a) || !plain(b)) throw std::invalid_argument("pair " + std::to_string(i) + ": a sequence name must be one word that starts with neither # nor //");
    if (r1.size() != r2.size()) throw std::invalid_argument("pair " + std::to_string(i) + ": rows differ in length");
    if (r1.empty()) throw std::invalid_argument("pair " + std::to_string(i) + ": an alignment without columns cannot be written");
    if (a == b) b += "/read";      // the reader merges rows of one name into one sequence
    const size_t w = std::max(a.size(), b.size());
    text += "# STOCKHOLM 1.0\n";
    text += a + std::string(w - a.size() + 1, ' ') + r1 + "\n";
    text += b + std::string(w - b.size() + 1, ' ') + r2 + "\n";
    text += "//\n";
  }
  return text;
}

int checkAlignArgs(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs, const int64_t* in_off,
                   const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_ops, const uint64_t* ops_off,
                   const uint32_t* out_n_ops, const double* out_score, const uint8_t* out_status) {
  if (!params || n_pairs < 0) return fail(DNAS_E_INVALID, "align pairs: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "align pairs: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen)
    return fail(DNAS_E_UNSUPPORTED, "align pairs: more than 13 duplication lengths (a cell's choices are a 16-bit word)");
  if (n_pairs == 0) return DNAS_OK;
  if (!in_seqs || !in_off || !out_seqs || !out_off || !out_ops || !ops_off || !out_n_ops || !out_score || !out_status)
    return fail(DNAS_E_INVALID, "align pairs: null argument");
  if (in_off[0] != 0 || out_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
    if (I < 0 || O < 0 || ops_off[i + 1] < ops_off[i]) return fail(DNAS_E_INVALID, "pair " + std::to_string(i) + ": inconsistent offsets");
    if (I > kAlignMaxSeq || O > kAlignMaxSeq)
      return fail(DNAS_E_UNSUPPORTED, "pair " + std::to_string(i) + ": sequences longer than " + std::to_string(kAlignMaxSeq));
    if (ops_off[i + 1] - ops_off[i] < (uint64_t)(I + O))
      return fail(DNAS_E_INVALID, "pair " + std::to_string(i) + ": the op slot is shorter than inLen + outLen");
  }
  for (int64_t j = 0; j < in_off[n_pairs]; ++j) if (in_seqs[j] < 0 || in_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  for (int64_t j = 0; j < out_off[n_pairs]; ++j) if (out_seqs[j] < 0 || out_seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

}  // namespace dnas
