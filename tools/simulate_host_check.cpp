// The read sampler's host statement (csrc/host/simulate.cpp) and the text it shares with the kernels (csrc/host/simulate.hpp:
// the generator, simExtend, simPosition, simEntryBits) as a program of its own for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o simulate_host_check tools/simulate_host_check.cpp
//
//   list     the CPU tests' list -- strands of 0, 1, 2, 5, 64, 65, 130 and the chunk edges 63 .. 300, P = 0, 1, 3, 13, 32, the six
//            parameter sets, reverse_prob 0, .5, 1 -- through checkSimulateArgs, simulateReadHost and simulateHandOut.  Every strand
//            lives in a heap block of exactly its length.
//   lanes    the kernels' way, restated: every position's S loop on its own (64 "lanes" a chunk), the entry bits from
//            simEntryBits with the carry from chunk to chunk, swallowed positions one op and no base, places from the running
//            sums -- the read and the ops this gives are the statement's.
//   carries  simEntryBits against the bit-by-bit recurrence on random masks.
// Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../dnastore_amd/csrc/host/simulate.cpp"

std::string& dnas::lastErrorSlot() {
  static thread_local std::string slot;
  return slot;
}

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}

uint64_t nextRandom(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 11;
}

dnas_mutator_params paramsOf(const double v[5], int P, bool zerosInFront) {
  dnas_mutator_params p{};
  p.p_del_open = v[0], p.p_del_extend = v[1], p.p_tan_dup = v[2], p.p_transition = v[3], p.p_transversion = v[4];
  p.n_len = P;
  const int z = zerosInFront && P > 1 ? P / 2 : 0;
  for (int k = z; k < P; ++k) p.p_len[k] = 1.0 / (P - z);
  return p;
}

// One read the kernels' way.
void lanesRead(const dnas::SimThresholds& th, uint64_t seed, uint64_t index, const int8_t* in, int64_t I, std::vector<int8_t>* seq,
               std::vector<uint8_t>* ops) {
  unsigned carry = 0;
  for (int64_t c0 = 0; c0 <= I; c0 += 64) {
    uint64_t gen = 0, ext = 0;
    std::vector<int8_t> laneSeq[64];
    std::vector<uint8_t> laneOps[64];
    for (int lane = 0; lane < 64 && c0 + lane <= I; ++lane) {
      const int64_t ip = c0 + lane;
      dnas::SimDraws d(seed, index, (uint32_t)ip);
      if (dnas::simExtend(th, d, ip, I)) ext |= (uint64_t)1 << lane;
      const bool opens = dnas::simPosition(th, d, in, ip, I, [&](int base, uint8_t op) {
        if (base >= 0) laneSeq[lane].push_back((int8_t)base);
        laneOps[lane].push_back(op);
      });
      if (opens) gen |= (uint64_t)1 << lane;
    }
    unsigned carryOut;
    const uint64_t inD = dnas::simEntryBits(gen, ext, carry, &carryOut);
    carry = carryOut;
    for (int lane = 0; lane < 64 && c0 + lane <= I; ++lane) {
      if ((ext & inD) >> lane & 1) {
        ops->push_back(dnas::kSimOpDelete);
        continue;
      }
      seq->insert(seq->end(), laneSeq[lane].begin(), laneSeq[lane].end());
      ops->insert(ops->end(), laneOps[lane].begin(), laneOps[lane].end());
    }
  }
}

}  // namespace

int main() {
  const double sets[6][5] = {{.001, .01, .001, .01 * 10 / 11, .01 / 11}, {.15, .3, .1, .1, .1}, {1, .3, 0, .1, .1},
                             {.15, 1, .1, .1, .1},                       {.05, .3, .9, .1, .1}, {.15, .3, 0, .1, .1}};
  const int lengths[] = {0, 1, 2, 5, 64, 65, 130, 63, 127, 128, 129, 191, 192, 300}, dupLengths[] = {0, 1, 3, 13, 32};
  const double reverseProbs[] = {0, .5, 1};
  uint64_t rng = 12345, checksum = 0;
  int64_t reads = 0;
  for (const auto& v : sets)
    for (int P : dupLengths)
      for (int zeros = 0; zeros < (P == 3 || P == 13 ? 2 : 1); ++zeros) {
        const dnas_mutator_params p = paramsOf(v, P, zeros != 0);
        for (double reverseProb : reverseProbs) {
          const dnas::SimThresholds th = dnas::SimThresholds::from(p, reverseProb);
          for (int I : lengths) {
            std::unique_ptr<int8_t[]> strand(new int8_t[(size_t)I]);       // exactly I bytes: a read past the end is seen
            for (int c = 0; c < I; ++c) strand[c] = (int8_t)(nextRandom(rng) & 3);
            const int64_t off[2] = {0, I}, readStrand[2] = {0, 0};
            int8_t* outSeqs = nullptr;
            int64_t *outOff = nullptr, *outOpsOff = nullptr;
            uint8_t *outRev = nullptr, *outOps = nullptr, status[2];
            expect(dnas::checkSimulateArgs(&p, 1, strand.get(), off, 2, readStrand, reverseProb, 1, &outSeqs, &outOff, &outRev, &outOps,
                                           &outOpsOff, status) == DNAS_OK, "arguments");
            std::vector<int8_t> seqs;
            std::vector<uint8_t> ops, rev;
            std::vector<int64_t> seqOff(1, 0), opsOff(1, 0);
            for (uint64_t r = 0; r < 2; ++r) {
              const uint64_t index = ((uint64_t)1 << 32) - 1 + r;
              const size_t s0 = seqs.size(), o0 = ops.size();
              rev.push_back(dnas::simulateReadHost(th, 77, index, strand.get(), I, &seqs, &ops));
              seqOff.push_back((int64_t)seqs.size()), opsOff.push_back((int64_t)ops.size());
              std::vector<int8_t> laneSeq;
              std::vector<uint8_t> laneOps;
              lanesRead(th, 77, index, strand.get(), I, &laneSeq, &laneOps);
              if (rev.back())
                for (size_t a = 0, b = laneSeq.size(); a < b; ++a, --b) {
                  const int8_t x = laneSeq[a], y = laneSeq[b - 1];
                  laneSeq[a] = (int8_t)(3 - y);
                  if (a != b - 1) laneSeq[b - 1] = (int8_t)(3 - x);
                }
              expect(std::vector<int8_t>(seqs.begin() + (long)s0, seqs.end()) == laneSeq, "lanes: the read");
              expect(std::vector<uint8_t>(ops.begin() + (long)o0, ops.end()) == laneOps, "lanes: the ops");
              ++reads;
            }
            expect(dnas::simulateHandOut(2, seqs, seqOff, rev, 1, ops, opsOff, &outSeqs, &outOff, &outRev, &outOps, &outOpsOff) == DNAS_OK, "hand out");
            for (int64_t c = 0; c < outOff[2]; ++c) checksum = checksum * 31 + (uint64_t)outSeqs[c];
            for (int64_t c = 0; c < outOpsOff[2]; ++c) checksum = checksum * 31 + outOps[c];
            free(outSeqs), free(outOff), free(outRev), free(outOps), free(outOpsOff);
          }
        }
      }
  for (int trial = 0; trial < 100000; ++trial) {
    const uint64_t gen = nextRandom(rng) << 11 ^ nextRandom(rng), ext = (nextRandom(rng) << 11 ^ nextRandom(rng)) | (trial & 1 ? ~(uint64_t)0 << 7 : 0);
    const unsigned carry = trial >> 1 & 1;
    unsigned state = carry, carryOut;
    uint64_t want = 0;
    for (int i = 0; i < 64; ++i) {
      want |= (uint64_t)state << i;
      state = (gen >> i & 1) | ((ext >> i & 1) & state);
    }
    expect(dnas::simEntryBits(gen, ext, carry, &carryOut) == want && carryOut == state, "carries");
  }
  printf("%lld reads, checksum %016llx, %d failures\n", (long long)reads, (unsigned long long)checksum, failures);
  return failures ? 1 : 0;
}
