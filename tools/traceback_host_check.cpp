// The traceback's step (csrc/traceback_step.h: the node record and the two sources of a step's candidates) as a program of its
// own for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o traceback_host_check tools/traceback_host_check.cpp
// The kernels (csrc/viterbi_kernels.hip) and the packer's caller (csrc/runtime.hip) compile the same text.
//
//   records  a few hundred random CSR models -- N = 2 .. 40 states, 0 .. 5 emit and 0 .. 2 null in-edges per state (so records
//            that hold their in-edges and records marked kNotInline both occur), mdl 0 .. D with D = 1 .. 4, identity and
//            permuted slotOf, 1 .. 300 distinct edge scores -- are packed, and every field is read back through the accessors.
//            A record names at most 4 in-edges, so 40 states cannot name more than 256 scores: a dozen models of 110 states,
//            every inline in-edge with a score of its own until 255, 256, 257 or 300 are out, meet the rule (the score table
//            of runtime.hip, restated here) from both sides: a 257th score, and the model gets no records.
//   sources  for every state whose record is inline, every mut = 0 .. mdl + 1, pos = 0, 1 and D + 1 + (0 .. 2), local and global
//            (but not mut == 0 && pos == 0 && local, which the record path declines): TbRecordStep and TbCsrStep enumerate the
//            same candidates -- as many, every field equal, the transition score as bits; the emitted base alone is the CSR
//            source's business (events are logged on that path only).
//   literal  five states of a model written out below, their candidates typed in from DESIGN 3.5's sentence (emit-in, null-in,
//            own D, own T1, local start; per in-edge D then S, then null-in, from D; T(k+1), then S from a duplication lane),
//            with parameters that are sums of powers of two, so that every expected score is a literal.
// Exit status 0: all held.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../dnastore_amd/csrc/traceback_step.h"

namespace {

int failures = 0;
std::string context;
#define EXPECT(cond)                                                                                                              \
  do {                                                                                                                            \
    if (!(cond)) {                                                                                                                \
      if (failures < 50) std::fprintf(stderr, "%s:%d: %s does not hold [%s]\n", __FILE__, __LINE__, #cond, context.c_str());     \
      ++failures;                                                                                                                 \
    }                                                                                                                             \
  } while (0)

uint32_t rngState = 20261020;
uint32_t rnd() {
  rngState = rngState * 1664525u + 1013904223u;
  return rngState >> 8;
}
int between(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

// A model in host memory, every array exactly as long as its contents, and the DevModel that points into it.
struct HostModel {
  int N = 0, D = 0;
  std::vector<int32_t> einPtr, einSrc, einSlot, ninPtr, ninSrc, ninSlot, slotOf;
  std::vector<double> einScore, ninScore;
  std::vector<uint8_t> einBase, einIn, ninIn, mdl, ctx;
  bool permuted = false;
  DevModel dev{};
  HostModel() = default;
  HostModel(HostModel&&) = default;     // (dev points into the vectors: a model moves, and is never copied)

  void addState(int stateMdl, const std::vector<uint8_t>& stateCtx) {
    if (einPtr.empty()) einPtr.push_back(0), ninPtr.push_back(0);
    einPtr.push_back((int32_t)einSrc.size());
    ninPtr.push_back((int32_t)ninSrc.size());
    mdl.push_back((uint8_t)stateMdl);
    ctx.insert(ctx.end(), stateCtx.begin(), stateCtx.end());
    ++N;
  }
  // (a state's in-edges first, then the addState() that closes its rows)
  void addEmit(int src, double score, int base, int in) { einSrc.push_back(src), einScore.push_back(score), einBase.push_back((uint8_t)base), einIn.push_back((uint8_t)in); }
  void addNull(int src, double score, int in) { ninSrc.push_back(src), ninScore.push_back(score), ninIn.push_back((uint8_t)in); }

  void finish(const std::vector<int32_t>& slots, bool local) {
    slotOf = slots;
    for (int32_t s : einSrc) einSlot.push_back(slotOf.empty() ? s : slotOf[(size_t)s]);
    for (int32_t s : ninSrc) ninSlot.push_back(slotOf.empty() ? s : slotOf[(size_t)s]);
    for (auto* v : {&einPtr, &einSrc, &einSlot, &ninPtr, &ninSrc, &ninSlot, &slotOf}) v->shrink_to_fit();
    for (auto* v : {&einScore, &ninScore}) v->shrink_to_fit();
    for (auto* v : {&einBase, &einIn, &ninIn, &mdl, &ctx}) v->shrink_to_fit();
    dev.N = N; dev.Npad = (N + 31) & ~31; dev.D = D; dev.P = kMaxLen; dev.local = local; dev.storedLanes = 2;
    dev.einPtr = einPtr.data(); dev.einSrc = einSrc.data(); dev.einScore = einScore.data(); dev.einBase = einBase.data(); dev.einIn = einIn.data();
    dev.ninPtr = ninPtr.data(); dev.ninSrc = ninSrc.data(); dev.ninScore = ninScore.data(); dev.ninIn = ninIn.data();
    dev.einSlot = einSlot.data(); dev.ninSlot = ninSlot.data();
    dev.slotOf = slotOf.empty() ? nullptr : slotOf.data();
    dev.mdl = mdl.data(); dev.ctx = ctx.data();
  }
};

// runtime.hip's table: an edge score is named by a byte, the 257th distinct one by nothing
struct ScoreTable {
  std::vector<double> scores;
  int operator()(double v) {
    for (size_t i = 0; i < scores.size(); ++i)
      if (std::memcmp(&scores[i], &v, sizeof v) == 0) return (int)i;
    if (scores.size() >= 256) return -1;
    scores.push_back(v);
    return (int)scores.size() - 1;
  }
};

// the records of a model, or none
bool packAll(const HostModel& hm, std::vector<NodeRecord>& rec, ScoreTable& table) {
  rec.assign((size_t)hm.N, NodeRecord{});
  for (int j = 0; j < hm.N; ++j)
    if (!NodeRecord::pack(hm.dev, j, table, rec[(size_t)j])) return false;
  return true;
}

// scores that no two draws share unless asked to: k / 1024 - 20
double scoreNo(int k) { return (double)k / 1024. - 20.; }

// nScores: how many distinct scores the edges draw from; freshInline: every in-edge a record holds takes a score of its own
// while there are any left (the models of the 256 rule)
HostModel randomModel(int N, int D, bool permuted, bool local, int nScores, bool freshInline) {
  HostModel hm;
  hm.D = D;
  hm.permuted = permuted;
  int nextFresh = 0;
  for (int j = 0; j < N; ++j) {
    const int ne = freshInline ? between(2, 3) : between(0, 5), nn = freshInline ? 1 : between(0, 2);
    const auto score = [&](bool inlineEdge) {
      if (freshInline && inlineEdge && nextFresh < nScores) return scoreNo(nextFresh++);
      return scoreNo(between(0, nScores - 1));
    };
    for (int i = 0; i < ne; ++i) hm.addEmit(between(0, N - 1), score(ne <= kRecEmit), between(0, 3), between(0, 255));
    for (int i = 0; i < nn; ++i) hm.addNull(between(0, N - 1), score(nn <= kRecNull), between(0, 255));
    std::vector<uint8_t> c((size_t)D);
    for (uint8_t& x : c) x = (uint8_t)between(0, 3);
    hm.addState(between(0, D), c);
  }
  std::vector<int32_t> slots;
  if (permuted) {
    for (int j = 0; j < N; ++j) slots.push_back(j);
    for (int j = N - 1; j > 0; --j) std::swap(slots[(size_t)j], slots[(size_t)between(0, j)]);
  }
  hm.finish(slots, local);
  DevModel& d = hm.dev;
  d.noGap = -(double)between(1, 999) / 512.; d.delOpen = -(double)between(1, 999) / 64.; d.delExtend = -(double)between(1, 999) / 256.;
  d.delEnd = -(double)between(1, 999) / 128.; d.tanDup = -(double)between(1, 999) / 32.;
  for (double& x : d.sub) x = -(double)between(0, 9999) / 777.;
  for (double& x : d.len) x = -(double)between(0, 9999) / 333.;
  return hm;
}

long recordsRead = 0, inlineRecords = 0;

// pack, then the accessors: every field of every record
void checkRecords(const HostModel& hm, const std::vector<NodeRecord>& rec, const ScoreTable& table) {
  const DevModel& d = hm.dev;
  for (int j = 0; j < hm.N; ++j) {
    context = "record of state " + std::to_string(j) + " of " + std::to_string(hm.N);
    const NodeRecord& r = rec[(size_t)j];
    const int e0 = d.einPtr[j], ne = d.einPtr[j + 1] - e0, n0 = d.ninPtr[j], nn = d.ninPtr[j + 1] - n0;
    EXPECT(r.emitCount() == (ne > kRecEmit ? NodeRecord::kNotInline : (unsigned)ne));
    EXPECT(r.nullCount() == (nn > kRecNull ? NodeRecord::kNotInline : (unsigned)nn));
    EXPECT(r.isInline() == (ne <= kRecEmit && nn <= kRecNull));
    EXPECT(r.mdl() == d.mdl[j]);
    for (int q = 0; q < d.D; ++q) EXPECT(r.ctx(q) == d.ctx[(size_t)j * d.D + q]);
    EXPECT(r.ownSlot() == (d.slotOf ? d.slotOf[j] : j));
    for (int i = 0; i < ne && ne <= kRecEmit; ++i) {
      EXPECT(r.src(i) == d.einSrc[e0 + i] && r.slot(i) == d.einSlot[e0 + i] && r.in(i) == d.einIn[e0 + i] && r.base(i) == d.einBase[e0 + i]);
      EXPECT(r.scoreIndex(i) < table.scores.size() && bits(table.scores[r.scoreIndex(i)]) == bits(d.einScore[e0 + i]));
    }
    if (nn == 1) {
      constexpr int e = NodeRecord::kNullEdge;
      EXPECT(r.src(e) == d.ninSrc[n0] && r.slot(e) == d.ninSlot[n0] && r.in(e) == d.ninIn[n0] && r.base(e) == 0);
      EXPECT(r.scoreIndex(e) < table.scores.size() && bits(table.scores[r.scoreIndex(e)]) == bits(d.ninScore[n0]));
    }
    ++recordsRead;
    inlineRecords += r.isInline();
  }
}

bool same(const TbCand& a, const TbCand& b, bool withEmit) {
  return a.state == b.state && a.slot == b.slot && a.pos == b.pos && a.lane == b.lane && bits(a.trans) == bits(b.trans) && a.in == b.in &&
         a.other == b.other && (!withEmit || a.emit == b.emit);
}

template <class Step>
std::vector<TbCand> listOf(const Step& s) {
  std::vector<TbCand> out;
  for (int c = 0; c < s.count(); ++c) out.push_back(s.at(c));
  return out;
}

std::vector<TbCand> csrList(const DevModel& d, int state, int pos, int mut, int x) {
  const uint8_t* ctx = d.ctx + (size_t)state * d.D;
  const auto ctxAt = [&](int q) { return (int)ctx[q]; };
  return listOf(tbCsrStep(d, d.sub, d.len, d.einPtr[state], d.einPtr[state + 1], d.ninPtr[state], d.ninPtr[state + 1], d.mdl[state],
                          d.slotOf ? d.slotOf[state] : state, ctxAt, state, pos, mut, x));
}

std::vector<TbCand> recordList(const DevModel& d, const NodeRecord& r, int state, int pos, int mut, int x) {
  return listOf(tbRecordStep(d, d.sub, d.len, r, state, pos, mut, x));
}

long stepsCompared = 0, candidatesCompared = 0;

// both sources, every state with an inline record, every lane, three kinds of column, local and global
void checkSources(HostModel& hm, const std::vector<NodeRecord>& rec) {
  DevModel& d = hm.dev;
  for (int local = 0; local < 2; ++local) {
    d.local = local;
    for (int j = 0; j < hm.N; ++j) {
      if (!rec[(size_t)j].isInline()) continue;
      for (int mut = 0; mut <= d.mdl[j] + 1; ++mut)
        for (int pos : {0, 1, d.D + 1 + between(0, 2)}) {
          if (mut == 0 && pos == 0 && local) continue;
          const int x = pos > 0 ? between(0, 3) : 0;
          context = "state " + std::to_string(j) + " of " + std::to_string(hm.N) + ", pos " + std::to_string(pos) + ", mut " + std::to_string(mut) +
                    (local ? ", local" : ", global");
          const std::vector<TbCand> a = recordList(d, rec[(size_t)j], j, pos, mut, x), b = csrList(d, j, pos, mut, x);
          EXPECT(a.size() == b.size());
          for (size_t c = 0; c < a.size() && c < b.size(); ++c) {
            EXPECT(same(a[c], b[c], false));
            EXPECT(a[c].emit == 0 || a[c].emit == b[c].emit);
            ++candidatesCompared;
          }
          ++stepsCompared;
        }
    }
  }
}

int modelsWithRecords = 0, modelsWithout = 0;

void checkModel(HostModel hm, int distinctInline) {
  std::vector<NodeRecord> rec;
  ScoreTable table;
  const bool packed = packAll(hm, rec, table);
  // how many distinct scores the records would have to name, counted apart from the table
  std::set<uint64_t> named;
  for (int j = 0; j < hm.N; ++j) {
    const int e0 = hm.einPtr[(size_t)j], ne = hm.einPtr[(size_t)j + 1] - e0, n0 = hm.ninPtr[(size_t)j], nn = hm.ninPtr[(size_t)j + 1] - n0;
    for (int i = 0; i < ne && ne <= kRecEmit; ++i) named.insert(bits(hm.einScore[(size_t)(e0 + i)]));
    for (int i = 0; i < nn && nn <= kRecNull; ++i) named.insert(bits(hm.ninScore[(size_t)(n0 + i)]));
  }
  context = "model of " + std::to_string(hm.N) + " states naming " + std::to_string(named.size()) + " scores";
  EXPECT(packed == (named.size() <= 256));
  if (distinctInline >= 0) EXPECT((int)named.size() == distinctInline);
  if (!packed) { ++modelsWithout; return; }
  ++modelsWithRecords;
  EXPECT(table.scores.size() == named.size());
  hm.dev.recScore = table.scores.data();
  checkRecords(hm, rec, table);
  checkSources(hm, rec);
}

void randomModels() {
  for (int k = 0; k < 320; ++k) {
    const int N = between(2, 40), D = 1 + k % 4;
    checkModel(randomModel(N, D, (k >> 2) & 1, false, k % 5 == 0 ? between(1, 4) : between(1, 300), false), -1);
  }
  // 110 states of 2 or 3 emit in-edges and a null one name 330 scores if there are as many
  for (int distinct : {255, 256, 257, 300})
    for (int k = 0; k < 3; ++k) checkModel(randomModel(110, 1 + k, k == 1, false, distinct, true), distinct);
}

// ------------------------------------------------------------------------------------------------------------ the literal lists
// Parameters: noGap -1/8, delOpen -3, delExtend -1, delEnd -1/2, tanDup -4, sub[a][b] = -(4 a + b + 1) / 4, len[k] = -(k + 1) / 16.
// State j lives in lattice slot 2 j + 1.  D = 2.
//   state 3   emit in-edges from 1 (score -1, emits T, decodes 1) and from 2 (score -2, emits A, decodes 2), a null in-edge
//             from 0 (score -1/2), mdl 2, context G C
//   state 4   no emit in-edge, a null in-edge from 3 (score -1/4, decodes 3), mdl 0
//   state 5   emit in-edges from 1, 2, 3, 4 (scores -1, -2, -3, -4, emitting A C G T, decoding 11 .. 14), mdl 1, context T A
HostModel literalModel(bool local) {
  HostModel hm;
  hm.D = 2;
  hm.addState(0, {0, 0});
  hm.addState(0, {0, 0});
  hm.addState(0, {0, 0});
  hm.addEmit(1, -1., 3, 1), hm.addEmit(2, -2., 0, 2), hm.addNull(0, -.5, 0);
  hm.addState(2, {2, 1});
  hm.addNull(3, -.25, 3);
  hm.addState(0, {0, 0});
  for (int i = 0; i < 4; ++i) hm.addEmit(1 + i, -1. - i, i, 11 + i);
  hm.addState(1, {3, 0});
  hm.finish({1, 3, 5, 7, 9, 11}, local);
  DevModel& d = hm.dev;
  d.noGap = -.125; d.delOpen = -3.; d.delExtend = -1.; d.delEnd = -.5; d.tanDup = -4.;
  for (int i = 0; i < 16; ++i) d.sub[i] = -(i + 1) / 4.;
  for (int k = 0; k < kMaxLen; ++k) d.len[k] = -(k + 1) / 16.;
  return hm;
}

int literalLists = 0;

// the CSR source, and the record source where the state's record is inline and the step is one it takes
void expectList(HostModel& hm, const std::vector<NodeRecord>& rec, const char* what, int state, int pos, int mut, int x, const std::vector<TbCand>& want) {
  context = what;
  const DevModel& d = hm.dev;
  const std::vector<TbCand> csr = csrList(d, state, pos, mut, x);
  EXPECT(csr.size() == want.size());
  for (size_t c = 0; c < csr.size() && c < want.size(); ++c) EXPECT(same(csr[c], want[c], true));
  if (rec[(size_t)state].isInline() && !(mut == 0 && pos == 0 && d.local)) {
    const std::vector<TbCand> r = recordList(d, rec[(size_t)state], state, pos, mut, x);
    EXPECT(r.size() == want.size());
    for (size_t c = 0; c < r.size() && c < want.size(); ++c) EXPECT(same(r[c], want[c], false));
  }
  ++literalLists;
}

void literalStates() {
  for (int local = 0; local < 2; ++local) {
    HostModel hm = literalModel(local != 0);
    std::vector<NodeRecord> rec;
    ScoreTable table;
    context = "the literal model";
    EXPECT(packAll(hm, rec, table));
    hm.dev.recScore = table.scores.data();
    EXPECT(rec[3].isInline() && rec[4].isInline() && !rec[5].isInline());
    // {state, slot, pos, lane, trans, in, emit, other}
    if (!local) {
      // 2 emit + 1 null, mdl 2, from S at column 5 behind a C: emit-in (one column back), null-in, own D, own T1
      expectList(hm, rec, "state 3 from S", 3, 5, 0, 1,
                 {{1, 3, 4, 0, -4.625, 1, 4, true},      // (-1 - 1/8) + sub[T][C] = -9/8 - 14/4
                  {2, 5, 4, 0, -2.625, 2, 1, true},      // (-2 - 1/8) + sub[A][C] = -17/8 - 2/4
                  {0, 1, 5, 0, -.5, 0, 0, true},
                  {3, 7, 5, 1, -.5, 0, 0, false},        // delEnd
                  {3, 7, 4, 2, -2.5, 0, 0, false}});     // sub[G][C] = -10/4
      // ... from D: per in-edge D (score + delExtend) then S (score + delOpen), then the null in-edge's D
      expectList(hm, rec, "state 3 from D", 3, 5, 1, 1,
                 {{1, 3, 5, 1, -2., 1, 4, true}, {1, 3, 5, 0, -4., 1, 4, true}, {2, 5, 5, 1, -3., 2, 1, true}, {2, 5, 5, 0, -5., 2, 1, true},
                  {0, 1, 5, 1, -.5, 0, 0, true}});
      // the first column has none before it: no emit in-edge, no T1
      expectList(hm, rec, "state 3 from S in column 0", 3, 0, 0, 0, {{0, 1, 0, 0, -.5, 0, 0, true}, {3, 7, 0, 1, -.5, 0, 0, false}});
      // no emit in-edge, mdl 0
      expectList(hm, rec, "state 4 from S", 4, 3, 0, 2, {{3, 7, 3, 0, -.25, 3, 0, true}, {4, 9, 3, 1, -.5, 0, 0, false}});
      expectList(hm, rec, "state 4 from D", 4, 3, 1, 2, {{3, 7, 3, 1, -.25, 3, 0, true}});
      // 4 emit in-edges (more than a record holds), mdl 1, behind a G
      expectList(hm, rec, "state 5 from S", 5, 2, 0, 2,
                 {{1, 3, 1, 0, -1.875, 11, 1, true},     // (-1 - 1/8) + sub[A][G] = -9/8 - 3/4
                  {2, 5, 1, 0, -3.875, 12, 2, true},     // -17/8 - 7/4
                  {3, 7, 1, 0, -5.875, 13, 3, true},     // -25/8 - 11/4
                  {4, 9, 1, 0, -7.875, 14, 4, true},     // -33/8 - 15/4
                  {5, 11, 2, 1, -.5, 0, 0, false},
                  {5, 11, 1, 2, -3.75, 0, 0, false}});   // sub[T][G] = -15/4
      // a duplication lane with a deeper one: T(k+1) one column back (sub[context[1] = C][C] = -6/4), then S (tanDup + len[0])
      expectList(hm, rec, "state 3 from T1", 3, 5, 2, 1, {{3, 7, 4, 3, -1.5, 0, 0, false}, {3, 7, 5, 0, -4.0625, 0, 0, false}});
      // ... and the deepest: S alone (tanDup + len[1])
      expectList(hm, rec, "state 3 from T2", 3, 5, 3, 1, {{3, 7, 5, 0, -4.125, 0, 0, false}});
    } else {
      // the local start: S of state 0 in column 0, last
      expectList(hm, rec, "state 3 from S in column 0, local", 3, 0, 0, 0,
                 {{0, 1, 0, 0, -.5, 0, 0, true}, {3, 7, 0, 1, -.5, 0, 0, false}, {0, 1, 0, 0, 0., 0, 0, true}});
    }
  }
}

}  // namespace

int main() {
  randomModels();
  const int inModels = failures;
  literalStates();
  if (failures) {
    std::fprintf(stderr, "traceback host check: %d checks failed (random models %d, literal lists %d)\n", failures, inModels, failures - inModels);
    return 1;
  }
  std::printf("traceback host check: ok (%d models with records, %d beyond 256 scores; %ld records read back, %ld inline; "
              "%ld steps and %ld candidates on both sources; %d literal lists)\n",
              modelsWithRecords, modelsWithout, recordsRead, inlineRecords, stepsCompared, candidatesCompared, literalLists);
  return 0;
}
