// The host statement of the forward pair-HMM score (csrc/host/pairforward.cpp) as a program of its own for a sanitizer build on
// the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_forward_host_check tools/pair_forward_host_check.cpp
// It runs forwardPairHost over every pair of lengths 0 .. 70, at bands 0, 1, 5 and -1 and with 0, 2, 6 and 13 duplication
// lengths, on sequences held in heap blocks of exactly their length, so that a read or write one element off is an error.  Every
// result must be finite or -inf, the pair (I, O) must have a path exactly when the model and the band leave one, and reading the
// read in place as its reverse complement must give the bits of the call on the reverse-complemented copy.  Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dnastore_amd/csrc/host/pairforward.cpp"

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
  const int kMax = 70;
  uint32_t rng = 12345;
  auto next = [&] { rng = rng * 1664525u + 1013904223u; return (int8_t)(rng >> 30); };
  long pairs = 0;
  for (int P : {0, 2, 6, 13}) {
    const dnas::PairScores sc = scores(P);
    for (int band : {0, 1, 5, -1})
      for (int I = 0; I <= kMax; ++I) {
        std::vector<int8_t> in((size_t)I);
        for (int8_t& x : in) x = next();
        for (int O = 0; O <= kMax; ++O) {
          std::vector<int8_t> out((size_t)O), rc((size_t)O);
          for (int8_t& x : out) x = next();
          for (int j = 0; j < O; ++j) rc[(size_t)j] = (int8_t)(3 - out[(size_t)(O - 1 - j)]);
          const bool rev = ((I + O) & 1) != 0;
          const double got = dnas::forwardPairHost(sc, in.data(), I, out.data(), O, band, rev, false);
          EXPECT(got == got && got <= O * std::log(4.));      // an output base scores log(p / (1/4)) at the most
          if (rev) EXPECT(bits(got) == bits(dnas::forwardPairHost(sc, in.data(), I, rc.data(), O, band, false, false)));
          // the band always holds the diagonal from (0,0) and the corner (I,O): a path of matches, then deletions (any I > O) or
          // duplications (O > I needs P > 0 and an input base to copy)
          const bool path = O <= I || (P > 0 && I > 0);
          EXPECT((got > -std::numeric_limits<double>::infinity()) == path);
          if ((I * 71 + O) % 97 == 0) {
            const double exact = dnas::forwardPairHost(sc, in.data(), I, out.data(), O, band, rev, true);
            EXPECT(exact == exact && (exact > -std::numeric_limits<double>::infinity()) == path);
            if (path) EXPECT(std::fabs(exact - got) <= 6. * (I + O + 1) * (std::exp(-10.) + 1e-9));
          }
          ++pairs;
        }
      }
  }
  if (failures) return 1;
  std::printf("pair forward host check: ok (%ld pairs)\n", pairs);
  return 0;
}
