// Myers' bit-vector recurrence (gateBlock, csrc/cluster_gate.hpp) and everything built on it -- gatePairWords<1|2|4|8>, gatePairLong
// and the primer search TrimSearch (csrc/host/trim.hpp) -- as a program of its own for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bitvector_host_check tools/bitvector_host_check.cpp
// The kernels run this text and nothing else does: the host statements (editDistanceHost, trimSearchHost) are two-row dynamic
// programs.  Here the kernels' text runs on the CPU against a full-matrix dynamic program written below (ColumnDp: the global
// distance, and the search with its free first row), and the host statements are held to the same matrix.
//
// Memory: every pattern and every text lives in a heap block of exactly its length; the mask table peq is used at stride 3 and the
// long route's slice mem at stride 2, in blocks of exactly 4 W and 8 words columns that were filled with a canary, and the
// columns of the other "threads" must hold the canary afterwards -- the [base][word][thread] indexing of the kernels.
//
//   tails    all pattern tails x text tails of up to 3 bases over ACGT and of up to 5 over {A, C}, behind a common prefix of
//            0, 29..32, 61..64 or 125..128 bases that is a homopolymer, a period-2 repeat or random: exhaustive on each side of
//            bit 31/32 and of the first and second word boundary, through every gatePairWords<W> that holds the pattern and
//            through gatePairLong, both orientations.  (The matrix is filled column by column, and the columns of the prefix,
//            which do not depend on what follows them, once per text: the text is its rows, the pattern its columns.  One case
//            in 64 fills it afresh the other way round and asks editDistanceHost as well.  Sized for a sanitizer run of about
//            40 s: behind the random prefix the tails are one base shorter, and the tails of 4 and 5 bases meet only tails
//            over {A, C}.)
//   ladder   m in {1, 2, 31, 32, 33} and 64 k - 1, 64 k, 64 k + 1 for k = 1 .. 10, n = m + {0, 1, 15, 16, 17, 40}: homopolymers
//            (with their closed forms), a homopolymer against a period-2 repeat, a period-2 and a period-3 repeat against
//            themselves at a shifted phase (d((AC)^k, (CA)^k) = 2), tandem duplications, three substitutions, unrelated.
//   primers  every primer length 1 .. 64, reads of ten lengths around it, max_offset -1, 0 and 8, both strands, both anchors
//            (the pattern reversed for the end anchor), five kinds of primer, planted in a read made of the primer's own repeat
//            unit (nearly every column ties) and not planted: TrimSearch, trimSearchHost and the matrix name the same (e, c).
//   loop     the window packing of trim_pack_kernel and the column loop of trim_search_kernel, restated, on every
//            (mF, mR) in {1, 7, 8, 9, 31, 32, 33, 63, 64}^2 with reads across the 16-column groups: the four hits of the one
//            loop are the four separate trimSearchHost calls.
// Exit status 0: all held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../dnastore_amd/csrc/cluster_gate.hpp"
#include "../dnastore_amd/csrc/host/cluster.cpp"
#include "../dnastore_amd/csrc/host/pairalign.cpp"
#include "../dnastore_amd/csrc/host/trim.cpp"

std::string& dnas::lastErrorSlot() {
  static thread_local std::string slot;
  return slot;
}

namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures < 50) std::fprintf(stderr, "%s:%d: %s does not hold [%s]\n", __FILE__, __LINE__, #cond, describe().c_str()); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

typedef std::vector<int8_t> Seq;

// what the case at hand is, spelled out only when a check fails
struct Context {
  const char* what = "";
  const Seq *a = nullptr, *b = nullptr;
  int x = 0, y = 0, z = 0;
} context;
std::string describe();

uint32_t rngState = 20240229;
uint32_t rnd() {
  rngState = rngState * 1664525u + 1013904223u;
  return rngState >> 8;
}
int8_t rndBase() { return (int8_t)(rnd() & 3); }

Seq randomSeq(int n) {
  Seq s((size_t)n);
  for (int8_t& x : s) x = rndBase();
  return s;
}

// unit repeated from phase to n bases
Seq repeatSeq(const Seq& unit, int n, int phase = 0) {
  Seq s((size_t)n);
  for (int q = 0; q < n; ++q) s[(size_t)q] = unit[(size_t)(q + phase) % unit.size()];
  return s;
}

Seq operator+(const Seq& a, const Seq& b) {
  Seq s(a);
  s.insert(s.end(), b.begin(), b.end());
  return s;
}

Seq reversed(const Seq& a) { return Seq(a.rbegin(), a.rend()); }

Seq reverseComplement(const Seq& a) {
  Seq s = reversed(a);
  for (int8_t& x : s) x = (int8_t)(3 - x);
  return s;
}

std::string text(const Seq& a) {
  std::string s;
  for (int8_t x : a) s += "ACGT"[x & 3];
  return s.size() > 80 ? s.substr(0, 38) + ".." + s.substr(s.size() - 38) + "(" + std::to_string(s.size()) + ")" : s;
}

std::string describe() {
  return std::string(context.what) + " " + (context.a ? text(*context.a) : "") + " / " + (context.b ? text(*context.b) : "") + " (" +
         std::to_string(context.x) + ", " + std::to_string(context.y) + ", " + std::to_string(context.z) + ")";
}

// A heap block of exactly the sequence's length (of no byte for an empty one).
struct Block {
  std::unique_ptr<int8_t[]> p;
  int n;
  explicit Block(const Seq& s) : p(new int8_t[s.size()]), n((int)s.size()) { std::copy(s.begin(), s.end(), p.get()); }
  const int8_t* get() const { return p.get(); }
};

// The full matrix of the global distance, rows = a sequence fixed at the start, one column per base pushed: col[j][i] = D[i][j],
// the cost of turning rows[0..i) into the j bases pushed so far.  A column depends on the bases before it alone, so truncate()
// goes back to a shared prefix and other bases follow.
struct ColumnDp {
  Seq rows;
  std::vector<int32_t> cells;                            // column j is cells[j * (rows + 1) ..]
  size_t used = 1;
  ColumnDp(const Seq& r, size_t maxColumns) : rows(r), cells((maxColumns + 1) * (r.size() + 1)) {
    for (size_t i = 0; i <= r.size(); ++i) cells[i] = (int32_t)i;
  }
  void truncate(size_t columns) { used = columns + 1; }
  void push(int8_t x) {
    const size_t n = rows.size();
    if ((used + 1) * (n + 1) > cells.size()) abort();
    const int32_t* const prev = cells.data() + (used - 1) * (n + 1);
    int32_t* const cur = cells.data() + used * (n + 1);
    const int8_t* const r = rows.data();
    cur[0] = (int32_t)used;
    for (size_t i = 1; i <= n; ++i) {
      const int32_t diag = prev[i - 1] + (r[i - 1] != x ? 1 : 0), left = prev[i] + 1, up = cur[i - 1] + 1;
      const int32_t side = left < up ? left : up;
      cur[i] = diag < side ? diag : side;
    }
    ++used;
  }
  int32_t distance() const { return cells[used * (rows.size() + 1) - 1]; }
};

int32_t distanceMatrix(const Seq& a, const Seq& b) {
  ColumnDp dp(a, b.size());
  for (int8_t x : b) dp.push(x);
  return dp.distance();
}

// search(p, t[0..w)): D[0][c] = 0, D[r][0] = r, the smallest D[m][c] over c = 0 .. w and the largest c that attains it.
dnas::TrimHit searchMatrix(const Seq& p, const Seq& t, int w) {
  const size_t m = p.size(), width = (size_t)w + 1;
  std::vector<int32_t> matrix((m + 1) * width, 0);       // D[r][c] = matrix[r * width + c]
  const int8_t* const text = t.data();
  for (size_t r = 1; r <= m; ++r) {
    const int32_t* const above = matrix.data() + (r - 1) * width;
    int32_t* const here = matrix.data() + r * width;
    const int8_t x = p[r - 1];
    here[0] = (int32_t)r;
    for (size_t c = 1; c < width; ++c) {
      const int32_t diag = above[c - 1] + (x != text[c - 1] ? 1 : 0), up = above[c] + 1, left = here[c - 1] + 1;
      const int32_t side = left < up ? left : up;
      here[c] = diag < side ? diag : side;
    }
  }
  const int32_t* const last = matrix.data() + m * width;
  dnas::TrimHit hit{last[0], 0};
  for (int c = 1; c <= w; ++c)
    if (last[c] <= hit.e) hit = dnas::TrimHit{last[c], c};
  return hit;
}

// ------------------------------------------------------------------------------------------------------------- the gate
constexpr uint64_t kCanary = 0xC0FFEE0DDBA11AD5ull;
long gateCases = 0, gateRuns = 0, hostCalls = 0;

template <int W>
void runWords(const Block& pat, const Block& txt, int32_t want0, int32_t want1) {
  if (pat.n > 64 * W) return;
  const int stride = 3, lane = (int)(gateRuns % stride);
  const size_t words = (size_t)4 * W * stride;
  std::unique_ptr<uint64_t[]> peq(new uint64_t[words]);
  std::fill(peq.get(), peq.get() + words, kCanary);
  int32_t e[2] = {-7, -7};
  dnas::gatePairWords<W>(pat.get(), pat.n, txt.get(), txt.n, peq.get() + lane, stride, e);
  EXPECT(e[0] == want0);
  EXPECT(e[1] == want1);
  bool clean = true;
  for (size_t x = 0; x < words; ++x) clean = clean && ((int)(x % stride) == lane || peq[x] == kCanary);
  EXPECT(clean);
  ++gateRuns;
}

void runLong(const Block& pat, const Block& txt, int32_t want0, int32_t want1) {
  const int64_t stride = 2;
  const size_t words = (size_t)8 * (size_t)((pat.n + 63) / 64) * (size_t)stride;
  const int lane = words ? (int)(gateRuns % stride) : 0;
  std::unique_ptr<uint64_t[]> mem(new uint64_t[words]);
  std::fill(mem.get(), mem.get() + words, kCanary);
  int32_t e[2] = {-7, -7};
  dnas::gatePairLong(pat.get(), pat.n, txt.get(), txt.n, mem.get() + lane, stride, e);
  EXPECT(e[0] == want0);
  EXPECT(e[1] == want1);
  bool clean = true;
  for (size_t x = 0; x < words; ++x) clean = clean && ((int)(x % (size_t)stride) == lane || mem[x] == kCanary);
  EXPECT(clean);
  ++gateRuns;
}

// every instance that holds the pattern, and the long route, against e[0], e[1] of the matrix; the host statement as well
void gateCase(const Seq& p, const Seq& t, int32_t want0, int32_t want1, bool withHost) {
  context = Context{"gate: pattern / text (want e[0], e[1])", &p, &t, want0, want1, 0};
  const Block pat(p), txt(t);
  runWords<1>(pat, txt, want0, want1);
  runWords<2>(pat, txt, want0, want1);
  runWords<4>(pat, txt, want0, want1);
  runWords<8>(pat, txt, want0, want1);
  runLong(pat, txt, want0, want1);
  if (withHost) {
    EXPECT(dnas::editDistanceHost(pat.get(), pat.n, txt.get(), txt.n, false) == want0);
    EXPECT(dnas::editDistanceHost(pat.get(), pat.n, txt.get(), txt.n, true) == want1);
    ++hostCalls;
  }
  ++gateCases;
}

struct Edits {
  int32_t e0, e1;
};

// ... against the matrix filled for this pair -> what the matrix said.  The host statement, whose two rows are the slowest part
// of a sanitizer build, runs on every pattern of up to 129 rows and on every third case beyond.
Edits gateCase(const Seq& p, const Seq& t) {
  const Edits want{distanceMatrix(p, t), distanceMatrix(p, reverseComplement(t))};
  gateCase(p, t, want.e0, want.e1, p.size() <= 129 || gateCases % 3 == 0);
  return want;
}

std::vector<Seq> tails() {
  std::vector<Seq> out;
  for (int alphabet : {4, 2})
    for (int len = alphabet == 4 ? 0 : 4; len <= (alphabet == 4 ? 3 : 5); ++len) {   // {A, C} up to 3 is within ACGT up to 3
      int count = 1;
      for (int q = 0; q < len; ++q) count *= alphabet;
      for (int code = 0; code < count; ++code) {
        Seq s((size_t)len);
        for (int q = 0, c = code; q < len; ++q, c /= alphabet) s[(size_t)q] = (int8_t)(c % alphabet);
        out.push_back(s);
      }
    }
  return out;
}

bool overTwo(const Seq& s) {
  for (int8_t x : s) if (x > 1) return false;
  return true;
}

long tailCases = 0;
void exhaustiveTails() {
  const std::vector<Seq> all = tails();                  // 85 over ACGT, then 48 of 4 and 5 bases over {A, C}
  for (int kind = 0; kind < 3; ++kind)
    for (int len : {0, 29, 30, 31, 32, 61, 62, 63, 64, 125, 126, 127, 128}) {
      if (len == 0 && kind > 0) continue;                // no prefix is of no kind
      const Seq prefix = kind == 0 ? repeatSeq(Seq{0}, len) : kind == 1 ? repeatSeq(Seq{0, 1}, len) : randomSeq(len);
      // the size of the run: behind a random prefix, whose carries end within a few bits whatever follows, the tails are one
      // base shorter (up to 2 over ACGT, up to 4 over {A, C})
      const size_t longest = kind == 2 ? 4 : 5, longest4 = kind == 2 ? 2 : 3;
      const auto sized = [&](const Seq& s) { return s.size() <= (overTwo(s) ? longest : longest4); };
      for (const Seq& tt : all) {
        if (!sized(tt)) continue;
        // the text and its reverse complement are the rows; the pattern's bases are pushed: first the prefix, once
        const Seq t = prefix + tt, turned = reverseComplement(t);
        ColumnDp fwd(t, prefix.size() + 5), rev(turned, prefix.size() + 5);
        for (int8_t x : prefix) fwd.push(x), rev.push(x);
        for (const Seq& pt : all) {
          if (!sized(pt)) continue;
          if (overTwo(tt) != overTwo(pt) && (tt.size() > 3 || pt.size() > 3)) continue;   // the long tails pair over {A, C} only
          fwd.truncate(prefix.size()), rev.truncate(prefix.size());
          for (int8_t x : pt) fwd.push(x), rev.push(x);
          // one case in 64 (and every one without a prefix) also asks the matrix filled afresh, pattern as rows, and the host
          const bool afresh = len == 0 || tailCases % 64 == 0;
          const Seq p = prefix + pt;
          if (afresh) {
            context = Context{"the matrix afresh: pattern / text", &p, &t, fwd.distance(), rev.distance(), 0};
            EXPECT(distanceMatrix(p, t) == fwd.distance());
            EXPECT(distanceMatrix(p, turned) == rev.distance());
          }
          gateCase(p, t, fwd.distance(), rev.distance(), afresh);
          ++tailCases;
        }
      }
    }
}

// a copy of src grown to n bases by tandem duplications of 1 .. 3 bases
Seq withDuplications(const Seq& src, int n) {
  Seq s(src);
  while ((int)s.size() < n) {
    const int at = (int)(rnd() % s.size());
    const int k = std::min<int>(1 + (int)(rnd() % 3), std::min(at + 1, n - (int)s.size()));
    const Seq copy(s.begin() + at + 1 - k, s.begin() + at + 1);
    s.insert(s.begin() + at + 1, copy.begin(), copy.end());
  }
  return s;
}

long ladderCases = 0, closedForms = 0;
void ladder() {
  std::vector<int> lengths = {1, 2, 31, 32, 33};
  for (int k = 1; k <= 10; ++k) lengths.insert(lengths.end(), {64 * k - 1, 64 * k, 64 * k + 1});
  for (int m : lengths)
    for (int d : {0, 1, 15, 16, 17, 40}) {
      const int n = m + d;
      const long before = gateCases;
      // homopolymers: (A^m, A^n) -> (n - m, n); (A^m, C^n) -> (n, n), as rc(C^n) = G^n; (A^m, T^n) -> (n, n - m)
      const int8_t b = (int8_t)((m + d) & 3), other = (int8_t)(b ^ 1);
      const Seq hp = repeatSeq(Seq{b}, m);
      const Edits same = gateCase(hp, repeatSeq(Seq{b}, n));
      const Edits different = gateCase(hp, repeatSeq(Seq{other}, n));
      const Edits complement = gateCase(hp, repeatSeq(Seq{(int8_t)(3 - b)}, n));
      context = Context{"closed forms of homopolymers (m, n)", nullptr, nullptr, m, n, 0};
      EXPECT(same.e0 == n - m && same.e1 == n);
      EXPECT(different.e0 == n && different.e1 == n);
      EXPECT(complement.e0 == n && complement.e1 == n - m);
      closedForms += 6;
      // a homopolymer against a period-2 repeat that holds its base, either way round
      gateCase(hp, repeatSeq(Seq{b, other}, n, m & 1));
      gateCase(repeatSeq(Seq{other, b}, m), repeatSeq(Seq{b}, n));
      // the same repeat at a shifted phase: d((AC)^k, (CA)^k) = 2
      const Seq two = {b, other}, three = {b, other, (int8_t)(b ^ 2)};
      const Edits shifted = gateCase(repeatSeq(two, m), repeatSeq(two, n, 1));
      if (d == 0 && m % 2 == 0) {
        context = Context{"closed form of a shifted period 2 (m, n)", nullptr, nullptr, m, n, 0};
        EXPECT(shifted.e0 == 2);
        ++closedForms;
      }
      gateCase(repeatSeq(three, m), repeatSeq(three, n, 1 + (m & 1)));
      // a copy with tandem duplications; a copy with three substitutions, extended; unrelated
      const Seq src = randomSeq(m);
      gateCase(src, withDuplications(src, n));
      Seq subs = src + randomSeq(d);
      for (int q = 0; q < 3; ++q) {
        int8_t& x = subs[rnd() % subs.size()];
        x = (int8_t)((x + 1 + (int)(rnd() % 3)) & 3);
      }
      gateCase(src, subs);
      gateCase(src, randomSeq(n));
      ladderCases += gateCases - before;
    }
}

// --------------------------------------------------------------------------------------------------------- the primer search
long trimSearches = 0;

// the text of the search of strand s from the front or from the end, spelled out
Seq searchText(const Seq& read, int s, bool fromEnd) {
  const Seq v = s ? reverseComplement(read) : read;
  return fromEnd ? reversed(v) : v;
}

// TrimSearch as trim_search_kernel drives it, one search on its own
dnas::TrimHit searchBits(const Block& pattern, const Block& txt, int w) {
  uint64_t eq[4];
  dnas::gateMasks(pattern.get(), pattern.n, 0, eq);
  dnas::TrimSearch search(pattern.n);
  const uint64_t bit = (uint64_t)1 << (pattern.n - 1);
  for (int c = 1; c <= w; ++c) search.step(eq, txt.get()[c - 1], bit, c, w);
  return search.hit;
}

void searchCase(const Seq& primer, const Seq& read, int maxOffset) {
  const Block prim(primer), rd(read);
  for (int s = 0; s < 2; ++s)
    for (int fromEnd = 0; fromEnd < 2; ++fromEnd) {
      context = Context{"search: primer / read (strand, from the end, max_offset)", &primer, &read, s, fromEnd, maxOffset};
      const Seq p = fromEnd ? reversed(primer) : primer, t = searchText(read, s, fromEnd != 0);
      const int w = dnas::trimWindow((int32_t)p.size(), (int32_t)t.size(), maxOffset);
      const dnas::TrimHit want = searchMatrix(p, t, w);
      const dnas::TrimHit host = dnas::trimSearchHost(prim.get(), prim.n, fromEnd != 0, rd.get(), rd.n, s, fromEnd != 0, maxOffset);
      const dnas::TrimHit bits = searchBits(Block(p), Block(Seq(t.begin(), t.begin() + w)), w);
      EXPECT(host.e == want.e && host.c == want.c);
      EXPECT(bits.e == want.e && bits.c == want.c);
      ++trimSearches;
    }
}

// the five kinds of primer, and the repeat unit a read around it is made of
Seq primerOfKind(int kind, int m, Seq* unit) {
  const int8_t b = (int8_t)(m & 3);
  switch (kind) {
    case 0: *unit = randomSeq(3); return randomSeq(m);
    case 1: *unit = Seq{b}; return repeatSeq(*unit, m);
    case 2: *unit = Seq{b, (int8_t)(b ^ 1)}; return repeatSeq(*unit, m);
    case 3: *unit = Seq{b, (int8_t)(b ^ 2), (int8_t)(b ^ 3)}; return repeatSeq(*unit, m);
    default: {
      *unit = Seq{b, (int8_t)(b ^ 1)};
      Seq p = repeatSeq(*unit, m);
      p[(size_t)(m / 2)] = (int8_t)(b ^ 2);                // the odd base
      return p;
    }
  }
}

void everyPrimerLength() {
  for (int m = 1; m <= 64; ++m)
    for (int kind = 0; kind < 5; ++kind) {
      Seq unit;
      const Seq primer = primerOfKind(kind, m, &unit);
      std::vector<int> lengths = {0, 1, m - 1, m, m + 1, m + 7, m + 8, m + 9, m + 30, 2 * m + 3};
      std::sort(lengths.begin(), lengths.end());
      lengths.erase(std::unique(lengths.begin(), lengths.end()), lengths.end());
      for (int n : lengths)
        for (int planted = 0; planted < 2; ++planted) {
          Seq front, end;                                // the primer near the front of one read and near the end of the other
          if (planted) {
            const int junk = (m + n) % 3;
            const Seq body = repeatSeq(unit, junk) + primer + repeatSeq(unit, n, junk + m);
            front = Seq(body.begin(), body.begin() + n);
            const Seq tail = repeatSeq(unit, n) + primer + repeatSeq(unit, junk);
            end = Seq(tail.end() - n, tail.end());
          } else {
            front = kind == 0 ? randomSeq(n) : repeatSeq(unit, n, 1);
            end = reversed(front);
          }
          for (int maxOffset : {-1, 0, 8}) {
            searchCase(primer, front, maxOffset);
            searchCase(primer, end, maxOffset);
          }
        }
    }
}

// The windows of one read as trim_pack_kernel packs them: G dwords each, 16 bases to a dword, the end window backwards.
struct Packed {
  std::unique_ptr<uint32_t[]> front, end;
  int64_t G;
  Packed(const Block& read, int32_t W) : G(std::max<int64_t>(1, (W + 15) / 16)) {
    front.reset(new uint32_t[(size_t)G]);
    end.reset(new uint32_t[(size_t)G]);
    const int64_t n = read.n, lim = n < W ? n : W;
    for (int64_t g = 0; g < G; ++g) {
      uint32_t f = 0, e = 0;
      for (int u = 0; u < 16; ++u) {
        const int64_t c = 16 * g + u;
        if (c < lim) {
          f |= (uint32_t)(read.get()[c] & 3) << (2 * u);
          e |= (uint32_t)(read.get()[n - 1 - c] & 3) << (2 * u);
        }
      }
      front[(size_t)g] = f;
      end[(size_t)g] = e;
    }
  }
};

long loopCases = 0;
// the column loop of trim_search_kernel for one read and one pair, the windows packed for a call whose longest primer is maxM
void fourInOne(const Seq& F, const Seq& R, const Seq& read, int maxOffset, int maxM) {
  context = Context{"loop: F / read (length of R, max_offset, longest primer)", &F, &read, (int)R.size(), maxOffset, maxM};
  const Block f(F), r(R), rev(reversed(R)), rd(read);
  const int32_t n = rd.n, mF = f.n, mR = r.n;
  const Packed win(rd, dnas::trimWindow(maxM, n, maxOffset));
  uint64_t eqF[4], eqR[4];
  dnas::gateMasks(f.get(), mF, 0, eqF);
  dnas::gateMasks(rev.get(), mR, 0, eqR);
  const int32_t wF = dnas::trimWindow(mF, n, maxOffset), wR = dnas::trimWindow(mR, n, maxOffset);
  const int32_t wmax = wF > wR ? wF : wR;
  const uint64_t bitF = (uint64_t)1 << (mF - 1), bitR = (uint64_t)1 << (mR - 1);
  dnas::TrimSearch f0(mF), r0(mR), f1(mF), r1(mR);
  for (int32_t c0 = 0; c0 < wmax; c0 += 16) {
    const uint32_t fw = win.front[(size_t)(c0 >> 4)], ew = win.end[(size_t)(c0 >> 4)];
    const int32_t cols = wmax - c0 < 16 ? wmax - c0 : 16;
    for (int32_t u = 0; u < cols; ++u) {
      const int bf = (int)(fw >> (2 * u) & 3), be = (int)(ew >> (2 * u) & 3);
      const int32_t c = c0 + u + 1;
      f0.step(eqF, bf, bitF, c, wF);
      r0.step(eqR, be, bitR, c, wR);
      f1.step(eqF, 3 - be, bitF, c, wF);
      r1.step(eqR, 3 - bf, bitR, c, wR);
    }
  }
  const dnas::TrimHit wantF0 = dnas::trimSearchHost(f.get(), mF, false, rd.get(), n, 0, false, maxOffset);
  const dnas::TrimHit wantR0 = dnas::trimSearchHost(r.get(), mR, true, rd.get(), n, 0, true, maxOffset);
  const dnas::TrimHit wantF1 = dnas::trimSearchHost(f.get(), mF, false, rd.get(), n, 1, false, maxOffset);
  const dnas::TrimHit wantR1 = dnas::trimSearchHost(r.get(), mR, true, rd.get(), n, 1, true, maxOffset);
  EXPECT(f0.hit.e == wantF0.e && f0.hit.c == wantF0.c);
  EXPECT(r0.hit.e == wantR0.e && r0.hit.c == wantR0.c);
  EXPECT(f1.hit.e == wantF1.e && f1.hit.c == wantF1.c);
  EXPECT(r1.hit.e == wantR1.e && r1.hit.c == wantR1.c);
  ++loopCases;
}

void theFourInOneLoop() {
  const int lengths[] = {1, 7, 8, 9, 31, 32, 33, 63, 64};
  int at = 0;
  for (int mF : lengths)
    for (int mR : lengths) {
      const int kind = at++ % 5;
      Seq unit, unitR;
      const Seq F = primerOfKind(kind, mF, &unit), R = primerOfKind(kind, mR, &unitR);
      // reads whose windows end on each side of the 16-column groups, the primers planted in their own repeat unit
      for (int n : {0, 1, 15, 16, 17, 31, 32, 33, 40, 47, 48, 49, 64, 65, 72, 73, 80, 97, 140}) {
        const int junk = n % 3;
        const Seq whole = repeatSeq(unit, junk) + F + repeatSeq(unit, std::max(0, n - junk - mF - mR - 1)) + R + repeatSeq(unit, 1);
        Seq read(whole.begin(), whole.begin() + std::min<int>(n, (int)whole.size()));
        read = read + repeatSeq(unit, n - (int)read.size());
        for (int maxOffset : {-1, 0, 8}) {
          fourInOne(F, R, read, maxOffset, std::max(mF, mR));
          fourInOne(F, R, reverseComplement(read), maxOffset, 64);   // a call whose longest primer has 64 bases packs wider windows
        }
      }
    }
}

}  // namespace

int main() {
  exhaustiveTails();
  const int inTails = failures;
  ladder();
  const int inLadder = failures - inTails;
  everyPrimerLength();
  const int inPrimers = failures - inTails - inLadder;
  theFourInOneLoop();
  if (failures) {
    std::fprintf(stderr, "bit-vector host check: %d checks failed (tails %d, ladder %d, primers %d, loop %d)\n", failures, inTails, inLadder,
                 inPrimers, failures - inTails - inLadder - inPrimers);
    return 1;
  }
  std::printf("bit-vector host check: ok (%ld gate cases: %ld tails, %ld ladder; %ld kernel-text runs, %ld host pairs, %ld closed forms; "
              "%ld trim searches, %ld four-in-one loops)\n",
              gateCases, tailCases, ladderCases, gateRuns, hostCalls, closedForms, trimSearches, loopCases);
  return 0;
}
