// Where the pair-HMM wavefront stands (csrc/pair_geom.h: PaGeom, PaStripe) as a program of its own for a sanitizer build on the
// CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_wavefront_host_check tools/pair_wavefront_host_check.cpp
// For the shapes of tests/test_gpu_pair_align.py, bands 0, 1, 8, I+O, I+O+1, I+O+2, 2^31-1 and -1 and P of 2, 6 and 13 it
// enumerates (stripe, step, lane) the way paWalkForward does and holds the geometry to the band of host/pairalign.hpp:
//   - every cell of dnas::PairBand(I, O, band) is stood on exactly once, and nothing outside it is;
//   - PaGeom::wordAt(r, op) == (s * stepsMax + t) * 64 + lane with t < stepsMax: records and parked planes stay inside words();
//   - (r-1, op) was stood on by lane l-1 one step earlier, or by lane 63 of the stripe before when l == 0, which the row
//     above(g, O) says exactly then; (r-1, op-1) two steps earlier; (r, op-1) by the same lane one step earlier;
//   - the backward enumeration (stripes and steps descending, pcBackwardPair's) meets the same cell at the same (s, t, lane),
//     with (r+1, op) one step earlier on lane l+1, or on lane 0 of the stripe after, which the row below(g, O) says exactly then.
// Exit status 0: all held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dnastore_amd/csrc/host/pairalign.hpp"
#include "../dnastore_amd/csrc/pair_geom.h"

namespace {

long failures = 0;
#define EXPECT(cond)                                                                                      \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      if (++failures <= 20) std::fprintf(stderr, "%s:%d: %s does not hold (I %d O %d band %d P %d s %d t %d lane %d)\n", __FILE__, __LINE__, #cond, I, O, band, P, s, t, lane); \
    }                                                                                                     \
  } while (0)

struct At {
  int s = -1, t = -1, lane = -1;
  bool operator==(const At& o) const { return s == o.s && t == o.t && lane == o.lane; }
};

long checkCase(int I, int O, int band, int P) {
  const PaGeom g(I, O, band);
  const dnas::PairBand pb(I, O, band);
  const auto inBand = [&](int ip, int op) { return ip >= 0 && ip <= I && op >= pb.rowLo(ip) && op <= pb.rowHi(ip, O); };
  std::vector<At> fwd((size_t)(I + 1) * (size_t)(O + 1)), bwd(fwd.size());
  const auto at = [&](std::vector<At>& v, int ip, int op) -> At& { return v[(size_t)ip * (size_t)(O + 1) + (size_t)op]; };
  long cells = 0;

  for (int s = 0; s < g.stripes; ++s) {
    const int tmax = PaStripe(g, I, O, P, s, 0).tmax;
    for (int t = 0; t <= tmax; ++t)
      for (int lane = 0; lane < 64; ++lane) {
        const PaStripe st(g, I, O, P, s, lane);
        const int r = st.r, op = st.op(t);
        EXPECT(st.tmax == tmax && st.r0 == s * 64 && st.row == (r <= I));
        if (lane == 0 && s > 0 && op >= 0 && op <= O) EXPECT(st.above(g, O).has(op) == inBand(r - 1, op));
        if (lane == 0 && s > 0 && t == 0 && st.c0 >= 1) EXPECT(inBand(r - 1, st.c0 - 1) && at(fwd, r - 1, st.c0 - 1).lane == 63);
        if (!st.active(op)) continue;
        EXPECT(inBand(r, op));
        if (!inBand(r, op)) continue;
        EXPECT(at(fwd, r, op).s < 0);
        at(fwd, r, op) = At{s, t, lane};
        ++cells;
        EXPECT(t < g.stepsMax);
        EXPECT(g.wordAt(r, op) == ((size_t)s * (size_t)g.stepsMax + (size_t)t) * 64 + (size_t)lane && g.wordAt(r, op) < g.words());
        EXPECT(st.kmax == (r < P ? r : P));
        EXPECT(lane <= st.last);
        if (inBand(r - 1, op)) EXPECT(at(fwd, r - 1, op) == (lane > 0 ? At{s, t - 1, lane - 1} : At{s - 1, at(fwd, r - 1, op).t, 63}));
        if (inBand(r - 1, op - 1)) EXPECT(at(fwd, r - 1, op - 1) == (lane > 0 ? At{s, t - 2, lane - 1} : At{s - 1, at(fwd, r - 1, op - 1).t, 63}));
        if (inBand(r, op - 1)) EXPECT(at(fwd, r, op - 1) == (At{s, t - 1, lane}));
      }
  }
  {
    const int s = -1, t = -1, lane = -1;
    EXPECT(cells == pb.cells(I, O));
  }

  for (int s = g.stripes - 1; s >= 0; --s) {
    const int tmax = PaStripe(g, I, O, P, s, 0).tmax;
    for (int t = tmax; t >= 0; --t)
      for (int lane = 0; lane < 64; ++lane) {
        const PaStripe st(g, I, O, P, s, lane);
        const int r = st.r, op = st.op(t);
        const bool below = s < g.stripes - 1;
        if (lane == st.last && below && op >= 0 && op <= O) EXPECT(st.below(g, O).has(op) == inBand(r + 1, op));
        if (!st.active(op) || !inBand(r, op)) continue;
        EXPECT(at(fwd, r, op) == (At{s, t, lane}));
        at(bwd, r, op) = At{s, t, lane};
        if (inBand(r + 1, op)) EXPECT(at(bwd, r + 1, op) == (lane < st.last ? At{s, t + 1, lane + 1} : At{s + 1, at(fwd, r + 1, op).t, 0}));
        if (inBand(r + 1, op + 1)) EXPECT(at(bwd, r + 1, op + 1) == (lane < st.last ? At{s, t + 2, lane + 1} : At{s + 1, at(fwd, r + 1, op + 1).t, 0}));
        if (inBand(r, op + 1)) EXPECT(at(bwd, r, op + 1) == (At{s, t + 1, lane}));
      }
  }
  return cells;
}

}  // namespace

int main() {
  const int shapes[][2] = {{0, 0}, {0, 3}, {3, 0}, {1, 1}, {63, 63}, {64, 64}, {65, 60}, {129, 140}, {70, 40}, {40, 70}};
  long cases = 0, cells = 0;
  for (const auto& sh : shapes) {
    const int I = sh[0], O = sh[1];
    const int bands[] = {0, 1, 8, I + O, I + O + 1, I + O + 2, 2147483647, -1};
    for (int band : bands)
      for (int P : {2, 6, 13}) {
        cells += checkCase(I, O, band, P);
        ++cases;
      }
  }
  if (failures) {
    std::fprintf(stderr, "pair wavefront host check: %ld failures\n", failures);
    return 1;
  }
  std::printf("pair wavefront host check: ok (%ld cases, %ld cells)\n", cases, cells);
  return 0;
}
