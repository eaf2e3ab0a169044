// The host statement of the pair-HMM row profiles (pairProfileHost and ProfileSum of csrc/host/paircounts.cpp) as a program of
// its own for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_profile_host_check tools/pair_profile_host_check.cpp
// It runs pairProfileHost over every pair of lengths 0 .. 24, at bands 0, 1, 5 and -1 and with 0, 2, 6 and 13 duplication
// lengths, on sequences and profile blocks held in heap blocks of exactly their size, so that a read or write one element off is
// an error.  Z must be the bits of forwardPairHost, a pair must have a profile exactly when it has a path, no value may be NaN
// or negative, row I must hold nothing but duplications, every row r < I must sum to 1 within the table's bound, the sums over
// the rows must be the counts of pairCountsHost, and reading the read in place as its reverse complement must give the bits of
// the call on the reverse-complemented copy.  Every pair's block is then added to an aggregate of fewer positions than the
// longest original has rows, from either end, and the aggregate must hold what the blocks hold.  Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dnastore_amd/csrc/host/pairforward.cpp"
#include "../dnastore_amd/csrc/host/paircounts.cpp"

std::string& dnas::lastErrorSlot() {
  static thread_local std::string slot;
  return slot;
}

namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

dnas::PairScores scores(int P) {
  dnas::PairScores sc{};
  const double pDelOpen = .02, pTanDup = P ? .015 : 0., pDelExtend = .4;
  sc.delOpen = std::log(pDelOpen);
  sc.tanDup = std::log(pTanDup);
  sc.noGap = std::log(1 - pDelOpen - pTanDup);
  sc.delExtend = std::log(pDelExtend);
  sc.delEnd = std::log(1 - pDelExtend);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) sc.sub[i * 4 + j] = std::log(i == j ? .94 : .02) - std::log(.25);
  sc.P = P;
  for (int k = 0; k < dnas::kAlignMaxLen; ++k) sc.len[k] = k < P ? std::log(1. / P) : -std::numeric_limits<double>::infinity();
  return sc;
}

uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

}  // namespace

int main() {
  const int kMax = 24, kPositions = 17;
  const double kNeg = -std::numeric_limits<double>::infinity();
  uint32_t rng = 8765;
  auto next = [&] { rng = rng * 1664525u + 1013904223u; return (int8_t)(rng >> 30); };
  long pairs = 0;
  for (int P : {0, 2, 6, 13}) {
    const dnas::PairScores sc = scores(P);
    const int W = DNAS_PROFILE_DUP + P, nc = 21 + P;
    int depth = 1;
    while ((1 << depth) < P + 2) ++depth;
    for (int band : {0, 1, 5, -1})
      for (int anchor : {DNAS_PROFILE_FROM_START, DNAS_PROFILE_FROM_END}) {
        std::vector<double> aggregate((size_t)(5 + P) * kPositions), want((size_t)(5 + P) * kPositions, 0.);
        std::vector<int64_t> coverage((size_t)kPositions), wantCoverage((size_t)kPositions, 0);
        dnas::ProfileSum sum(P, anchor, kPositions, aggregate.data(), coverage.data());
        for (int I = 0; I <= kMax; ++I) {
          std::vector<int8_t> in((size_t)I);
          for (int8_t& x : in) x = next();
          for (int O = 0; O <= kMax; ++O) {
            std::vector<int8_t> out((size_t)O), rc((size_t)O);
            for (int8_t& x : out) x = next();
            for (int j = 0; j < O; ++j) rc[(size_t)j] = (int8_t)(3 - out[(size_t)(O - 1 - j)]);
            const bool rev = ((I + O) & 1) != 0;
            const size_t rows = (size_t)I + 1;
            std::vector<double> prof((size_t)W * rows, -1.), other((size_t)W * rows, -1.), counts((size_t)nc);   // exactly W (I + 1)
            double ll = 0, ll2 = 0, ll3 = 0;
            const bool ok = dnas::pairProfileHost(sc, in.data(), I, out.data(), O, band, rev, false, prof.data(), &ll);
            EXPECT(bits(ll) == bits(dnas::forwardPairHost(sc, in.data(), I, out.data(), O, band, rev, false)));
            const bool path = O <= I || (P > 0 && I > 0);
            EXPECT(ok == path && (ll > kNeg) == path);
            for (double v : prof) EXPECT(v == v && v >= 0 && (path || v == 0));
            if (rev) {
              dnas::pairProfileHost(sc, in.data(), I, rc.data(), O, band, false, false, other.data(), &ll2);
              EXPECT(bits(ll) == bits(ll2) && std::memcmp(prof.data(), other.data(), sizeof(double) * prof.size()) == 0);
            }
            dnas::pairCountsHost(sc, in.data(), I, out.data(), O, band, rev, false, counts.data(), &ll3, nullptr);
            EXPECT(bits(ll) == bits(ll3));
            if (path) {
              const double a = std::exp(-10.) + 1e-9, nF = 6. * (I + O + 1), nB = 3. * (I + O + 1) * depth;
              const double f = std::exp((2 * nF + nB) * a);
              for (int j = 0; j < DNAS_PROFILE_DUP; ++j) EXPECT(prof[(size_t)j * rows + (size_t)I] == 0);
              std::vector<double> plane((size_t)W, 0.);
              for (int r = 0; r <= I; ++r) {
                double one = 0;
                for (int j = 0; j < W; ++j) {
                  plane[(size_t)j] += prof[(size_t)j * rows + (size_t)r];
                  if (j < DNAS_PROFILE_DUP) one += prof[(size_t)j * rows + (size_t)r];
                }
                if (r < I) EXPECT(one >= 1 / f && one <= f);
              }
              // host sums over the same terms in another order
              EXPECT(close(plane[0] + plane[1] + plane[2] + plane[3], counts[2], 1e-12));
              EXPECT(close(plane[DNAS_PROFILE_DEL_OPEN], counts[0], 1e-12) && close(plane[DNAS_PROFILE_DEL_EXTEND], counts[3], 1e-12));
              for (int k = 0; k < P; ++k) EXPECT(close(plane[(size_t)(DNAS_PROFILE_DUP + k)], counts[(size_t)(21 + k)], 1e-12));
              sum.add(in.data(), I, prof.data());
              for (int r = 0; r <= I; ++r) {
                const int p = anchor == DNAS_PROFILE_FROM_END ? I - r : r;
                if (p >= kPositions) continue;
                ++wantCoverage[(size_t)p];
                for (int y = 0; y < 4 && r < I; ++y) {
                  const int x = in[(size_t)r], cls = y == x ? 0 : ((y ^ x) == 2 ? 1 : 2);
                  want[(size_t)cls * kPositions + (size_t)p] += prof[(size_t)y * rows + (size_t)r];
                }
                for (int j = DNAS_PROFILE_DEL_OPEN; j < W; ++j) want[(size_t)(j - 1) * kPositions + (size_t)p] += prof[(size_t)j * rows + (size_t)r];
              }
            }
            ++pairs;
          }
        }
        EXPECT(coverage == wantCoverage);
        for (size_t i = 0; i < want.size(); ++i) EXPECT(close(aggregate[i], want[i], 1e-12));
      }
  }
  if (failures) return 1;
  std::printf("pair profile host check: ok (%ld pairs)\n", pairs);
  return 0;
}
