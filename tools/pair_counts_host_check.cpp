// The host statement of the posterior move counts (csrc/host/paircounts.cpp) as a program of its own for a sanitizer build on
// the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_counts_host_check tools/pair_counts_host_check.cpp
// It runs pairCountsHost over every pair of lengths 0 .. 40, at bands 0, 1, 5 and -1 and with 0, 2, 6 and 13 duplication
// lengths, on sequences held in heap blocks of exactly their length, so that a read or write one element off is an error.  Z
// must be the bits of forwardPairHost, a pair must have counts exactly when it has a path, no count may be NaN or negative, the
// counts must add up to the sequences' lengths within the table's bound, B_S(0,0) must agree with Z within it, and reading the
// read in place as its reverse complement must give the bits of the call on the reverse-complemented copy.  Exit status 0: all
// held.
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

}  // namespace

int main() {
  const int kMax = 40;
  const double kNeg = -std::numeric_limits<double>::infinity();
  uint32_t rng = 4321;
  auto next = [&] { rng = rng * 1664525u + 1013904223u; return (int8_t)(rng >> 30); };
  long pairs = 0;
  for (int P : {0, 2, 6, 13}) {
    const dnas::PairScores sc = scores(P);
    const int nc = 21 + P;
    int depth = 1;
    while ((1 << depth) < P + 2) ++depth;
    for (int band : {0, 1, 5, -1})
      for (int I = 0; I <= kMax; ++I) {
        std::vector<int8_t> in((size_t)I);
        for (int8_t& x : in) x = next();
        for (int O = 0; O <= kMax; ++O) {
          std::vector<int8_t> out((size_t)O), rc((size_t)O);
          for (int8_t& x : out) x = next();
          for (int j = 0; j < O; ++j) rc[(size_t)j] = (int8_t)(3 - out[(size_t)(O - 1 - j)]);
          const bool rev = ((I + O) & 1) != 0;
          std::vector<double> counts((size_t)nc), other((size_t)nc);          // exactly 21 + P doubles
          double ll = 0, back = 0, ll2 = 0, back2 = 0;
          const bool ok = dnas::pairCountsHost(sc, in.data(), I, out.data(), O, band, rev, false, counts.data(), &ll, &back);
          EXPECT(bits(ll) == bits(dnas::forwardPairHost(sc, in.data(), I, out.data(), O, band, rev, false)));
          const bool path = O <= I || (P > 0 && I > 0);
          EXPECT(ok == path && (ll > kNeg) == path && (back > kNeg) == path);
          for (double c : counts) EXPECT(c == c && c >= 0 && (path || c == 0));
          if (rev) {
            dnas::pairCountsHost(sc, in.data(), I, rc.data(), O, band, false, false, other.data(), &ll2, &back2);
            EXPECT(bits(ll) == bits(ll2) && bits(back) == bits(back2));
            EXPECT(std::memcmp(counts.data(), other.data(), sizeof(double) * (size_t)nc) == 0);
          }
          if (path) {
            // the table's bound: 6 (I + O + 1) calls behind Z, 3 (I + O + 1) depth behind B_S(0,0), both behind every count
            const double a = std::exp(-10.) + 1e-9, nF = 6. * (I + O + 1), nB = 3. * (I + O + 1) * depth;
            EXPECT(std::fabs(back - ll) <= (nF + nB) * a);
            const double f = std::exp((2 * nF + nB) * a);
            double nSub = 0, nLen = 0;
            for (int k = 0; k < 16; ++k) nSub += counts[5 + (size_t)k];
            for (int k = 0; k < P; ++k) nLen += counts[21 + (size_t)k];
            EXPECT(nSub >= O / f && nSub <= O * f);
            const double rows = counts[2] + counts[0] + counts[3];
            EXPECT(rows >= I / f && rows <= I * f);
            EXPECT(counts[0] >= counts[4] / f && counts[0] <= counts[4] * f);
            EXPECT(counts[1] >= nLen / f && counts[1] <= nLen * f);
            if ((I * 41 + O) % 53 == 0) {
              const bool okExact = dnas::pairCountsHost(sc, in.data(), I, out.data(), O, band, rev, true, other.data(), &ll2, &back2);
              EXPECT(okExact && std::fabs(back2 - ll2) <= 1e-12 * std::fmax(1., std::fabs(ll2)));
              for (int k = 0; k < nc; ++k) EXPECT(counts[(size_t)k] >= other[(size_t)k] / f && counts[(size_t)k] <= other[(size_t)k] * f);
            }
          }
          ++pairs;
        }
      }
  }
  if (failures) return 1;
  std::printf("pair counts host check: ok (%ld pairs)\n", pairs);
  return 0;
}
