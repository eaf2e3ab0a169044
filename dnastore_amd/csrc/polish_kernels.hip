// dnas_cluster_consensus: the reads of a cluster aligned to a template, the alignments' columns voted into integer counters, a
// new template emitted from them, round after round (include/dnastore_amd.h), equal to clusterConsensusHost (host/polish.cpp).
//
// Fill.  paWalkForward of pair_align_device.h under the Viterbi cell with its choice words recorded, as dnas_align_pairs runs
// it: a wave owns a pair and walks the batch with the grid's stride.  A pair is (active cluster, read): its template is the
// cluster's, read where the last round left it, its read is taken in place, reverse-complemented where read_strand says so.
//
// Vote.  The traceback of pair_align_traceback_kernel, which adds to the cluster's table (host/polish.hpp) instead of writing op
// bytes.  It walks backwards, so a run of duplication columns is voted when the walk leaves it: its bases are then known from
// its first.  Two routes.  A template of up to kPolishLdsPositions bases has its table in LDS: one work-group of one wave per
// cluster clears it, walks the cluster's pairs (a lane per pair, LDS atomics), and emits.  A longer one has it in HBM: a thread
// per pair with global atomics, then a wave per cluster emits.
//
// Emit.  A lane per gap evaluates polishEmitGap -- the one statement of step 3, shared with the host --, a wave scan gives the
// places, and the bases go to the cluster's slot in the other of two template buffers; the lanes compare them with the old
// template on the way, which gives the changed flag.  A slot holds polishCapacity bases, a bound no round can exceed.
//
// The host reads back, per round, the new lengths, the changed flags, the voters and the new templates, drops the clusters that
// are done, and plans the next round's records from the new lengths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/pairalign.hpp"
#include "host/polish.hpp"
#include "pair_align_device.h"

namespace {

// template bases whose table fits the 64 KiB of LDS a work-group may have: 4 x (1 + 25 x 651) = 65 104 bytes
constexpr int kPolishLdsPositions = 650;
constexpr uint64_t kPlInLds = ~0ull;

// What the kernels of a round read and write.  a counts the round's active clusters, q its pairs: the pairs of a are
// pairBegin[a] .. pairBegin[a+1] - 1 and stand for the reads readBegin[a] + (q - pairBegin[a]).
struct PlRound {
  const int8_t* cur;                 // the templates: cluster a's is cur[curOff[a] .. + curLen[a])
  int8_t* next;                      // the new ones: next[nextOff[a] .. + newLen[a]), a slot of nextCap[a] bases
  const int64_t *curOff, *nextOff;
  const int32_t *curLen, *nextCap;
  const int64_t *readBegin, *pairBegin;
  const int32_t* pairAct;            // a of pair q
  const uint64_t* recOff;            // where pair q's choice words start in the arena
  const uint64_t* tabOff;            // where a's table starts in tab; kPlInLds: it lives in LDS
  uint32_t* tab;
  const int8_t* reads;
  const int64_t* readOff;
  const uint8_t* strand;
  double* score;                     // S(I,O) of pair q
  int32_t *newLen, *voters;
  uint8_t* changed;
  int* fail;                         // bit 0: a traceback left its record, bit 1: a slot overflowed -- defects, never inputs
};

template <int KP>
__global__ __launch_bounds__(64 * kPaWavesPerBlock) void polish_fill_kernel(PaScores sc, const double* __restrict__ subTable, int band,
                                                                            int64_t first, int64_t count, PlRound r,
                                                                            uint16_t* __restrict__ arena, double* bndScratch,
                                                                            int64_t bndStride) {
  __shared__ double lds[kPaWavesPerBlock][kPaLdsDoubles];
  const PaWave w = paWaveBegin(&lds[0][0], kPaLdsDoubles, subTable, bndScratch, bndStride);

  for (int64_t p = w.wave; p < count; p += w.nWaves) {
    const int64_t q = first + p;
    const int a = r.pairAct[q];
    const int64_t i = r.readBegin[a] + (q - r.pairBegin[a]);
    const int I = r.curLen[a], O = (int)(r.readOff[i + 1] - r.readOff[i]);
    PaViterbiCell<true> cell{arena + r.recOff[q] + w.lane, PaGeom(I, O, band).stepsMax};
    paWalkForward<KP>(sc, w.lds, PaBoundary(w.lds + 16, kPaLdsCols, w.bndMem, O), w.lane, band,
                      PaItem{r.cur + r.curOff[a], r.reads + r.readOff[i], I, O, r.strand != nullptr && r.strand[i] != 0}, r.score + q,
                      cell);
  }
}

// The traceback of one pair, voting into tab (LDS or HBM).  false: the recorded choices do not lead back to (0,0).
__device__ __forceinline__ bool plVotePair(uint32_t* tab, int band, const int8_t* b, int I, int O, bool rev, const uint16_t* rec) {
  const PaGeom g(I, O, band);
  const int cap = I + O;
  int ip = I, op = O, state = -1;      // state -1: S, -2: D, k >= 0: T_k
  int runEnd = -1;                     // the read position after the run of duplication columns the walk is in; -1: in none
  for (int moves = 0; !(ip == 0 && op == 0 && state == -1); ++moves) {
    if (ip < 0 || op < g.rowLo(ip) || op > g.rowHi(ip, O) || moves > 2 * cap + 2) return false;
    const unsigned w = rec[g.wordAt(ip, op)];
    bool column = false;               // a match or deletion column: the run, if any, ends (it stands at gap ip)
    if (state == -1) {
      const unsigned c = w & 3u;
      if (c == 0) column = true;
      else if (c == 1) {
        if (op == 0) return false;
        if (runEnd < 0) runEnd = op;
        --op;
        state = 0;
      } else state = -2;
    } else if (state == -2) {
      column = true;
    } else {
      if (w & (8u << state)) state = -1;
      else {
        if (op == 0) return false;
        --op;
        ++state;
      }
    }
    if (!column) continue;
    if (ip == 0) return false;
    if (runEnd >= 0) {
      const int L = runEnd - op < DNAS_POLISH_MAX_INSERT ? runEnd - op : DNAS_POLISH_MAX_INSERT;
      for (int k = 0; k < L; ++k) {
        const int j = op + k, y = rev ? 3 - ((int)b[O - 1 - j] & 3) : (int)b[j] & 3;
        atomicAdd(tab + dnas::polishN(ip, k), 1u);
        atomicAdd(tab + dnas::polishB(ip, k, y), 1u);
      }
      runEnd = -1;
    }
    if (state == -1) {                 // match
      if (op == 0) return false;
      const int j = op - 1, y = rev ? 3 - ((int)b[O - 1 - j] & 3) : (int)b[j] & 3;
      atomicAdd(tab + dnas::polishM(ip - 1, y), 1u);
      --ip;
      --op;
    } else {                           // deletion; d0 goes back to S
      atomicAdd(tab + dnas::polishD(ip - 1), 1u);
      --ip;
      if (!(w & 4u)) state = -1;
    }
  }
  if (runEnd >= 0) {                   // (a duplication needs a template base before it: the model has no run at gap 0)
    const int L = runEnd - op < DNAS_POLISH_MAX_INSERT ? runEnd - op : DNAS_POLISH_MAX_INSERT;
    for (int k = 0; k < L; ++k) {
      const int j = op + k, y = rev ? 3 - ((int)b[O - 1 - j] & 3) : (int)b[j] & 3;
      atomicAdd(tab + dnas::polishN(ip, k), 1u);
      atomicAdd(tab + dnas::polishB(ip, k, y), 1u);
    }
  }
  return true;
}

// Pair q of the round votes into tab, its cluster's table.
__device__ __forceinline__ void plVote(const PlRound& r, int band, const uint16_t* arena, int a, int64_t q, uint32_t* tab) {
  if (!(r.score[q] > paNegInf())) return;
  const int64_t i = r.readBegin[a] + (q - r.pairBegin[a]);
  const int O = (int)(r.readOff[i + 1] - r.readOff[i]);
  if (plVotePair(tab, band, r.reads + r.readOff[i], r.curLen[a], O, r.strand != nullptr && r.strand[i] != 0, arena + r.recOff[q]))
    atomicAdd(tab, 1u);
  else
    atomicOr(r.fail, 1);
}

// One wave emits cluster a's new template from its table.
__device__ __forceinline__ void plEmit(const PlRound& r, int a, const uint32_t* tab, int lane) {
  const int I = r.curLen[a], cap = r.nextCap[a];
  const int8_t* const t = r.cur + r.curOff[a];
  int8_t* const out = r.next + r.nextOff[a];
  int base = 0;
  bool differs = false, overflow = false;
  for (int g0 = 0; g0 <= I; g0 += 64) {
    const int g = g0 + lane;
    dnas::PolishGap e{0, 0};
    if (g <= I) e = dnas::polishEmitGap(tab, g, I, t);
    int incl = e.n;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int at = base + incl - e.n;
    for (int j = 0; j < e.n; ++j) {
      const int y = (int)((e.bases >> (2 * j)) & 3u), p = at + j;
      if (p >= cap) { overflow = true; break; }
      out[p] = (int8_t)y;
      if (p >= I || ((int)t[p] & 3) != y) differs = true;
    }
    base += __shfl(incl, 63);
  }
  differs = __any(differs) || base != I;
  overflow = __any(overflow);
  if (lane == 0) {
    r.newLen[a] = overflow ? 0 : base;
    r.changed[a] = differs ? 1 : 0;
    r.voters[a] = (int32_t)tab[0];
    if (overflow) atomicOr(r.fail, 2);
  }
}

// The LDS route: work-group b serves cluster list[b].
__global__ __launch_bounds__(64) void polish_vote_lds_kernel(int band, const int32_t* __restrict__ list, PlRound r,
                                                             const uint16_t* __restrict__ arena) {
  extern __shared__ uint32_t ldsTab[];
  const int lane = threadIdx.x, a = list[blockIdx.x];
  const int words = (int)dnas::polishWords(r.curLen[a]);
  for (int w = lane; w < words; w += 64) ldsTab[w] = 0;
  __syncthreads();
  for (int64_t q = r.pairBegin[a] + lane; q < r.pairBegin[a + 1]; q += 64) plVote(r, band, arena, a, q, ldsTab);
  __syncthreads();
  plEmit(r, a, ldsTab, lane);
}

// The HBM route: a thread per pair of the batch, the pairs of LDS clusters stepped over; then a wave per cluster emits.
__global__ __launch_bounds__(64) void polish_vote_hbm_kernel(int band, int64_t first, int64_t count, PlRound r,
                                                             const uint16_t* __restrict__ arena) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= count) return;
  const int64_t q = first + w;
  const int a = r.pairAct[q];
  if (r.tabOff[a] == kPlInLds) return;
  plVote(r, band, arena, a, q, r.tab + r.tabOff[a]);
}

__global__ __launch_bounds__(64) void polish_emit_hbm_kernel(const int32_t* __restrict__ list, PlRound r) {
  const int a = list[blockIdx.x];
  plEmit(r, a, r.tab + r.tabOff[a], threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct PlInputs {
  int64_t nClusters, nReads;
  const int8_t* tmplSeqs;
  const int64_t* tmplOff;
  const int8_t* readSeqs;
  const int64_t* readOff;
  const uint8_t* readStrand;
  const int64_t* clusterReadOff;
};

// Device memory that grows from round to round (the templates may), to exactly what the round needs: what it held is not kept.
template <class T>
int plNeed(dnas::DevBuf<T>& b, size_t n) {
  DNAS_HIP_TRY(b.reserve(n, dnas::growExact(n)));
  return DNAS_OK;
}

template <class T>
int plSend(T* dst, const std::vector<T>& src) {
  if (!src.empty()) DNAS_HIP_TRY(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return DNAS_OK;
}

// One device.  The arguments were checked; seqs[c] receives cluster c's consensus read.
int plRunOnDevice(int device, const dnas::PairScores& hs, int band, const PlInputs& in, int32_t roundsMax, size_t arena_bytes,
                  std::vector<std::vector<int8_t>>* seqs, int32_t* out_rounds, uint8_t* out_converged, int32_t* out_voters,
                  uint8_t* out_status, dnas_polish_stats* stats) {
  *stats = dnas_polish_stats{};
  const int64_t nc = in.nClusters;
  seqs->assign((size_t)nc, {});
  std::vector<dnas::PolishCluster> state((size_t)nc);
  std::vector<int64_t> active, curOff((size_t)nc), clMaxO((size_t)nc, 0);
  std::vector<int32_t> curLen((size_t)nc);
  int64_t maxO = 0, pairs0 = 0;
  for (int64_t c = 0; c < nc; ++c) {
    curOff[(size_t)c] = in.tmplOff[c];
    curLen[(size_t)c] = (int32_t)(in.tmplOff[c + 1] - in.tmplOff[c]);
    (*seqs)[(size_t)c].assign(in.tmplSeqs + in.tmplOff[c], in.tmplSeqs + in.tmplOff[c + 1]);
    const int64_t r0 = in.clusterReadOff[c], r1 = in.clusterReadOff[c + 1];
    for (int64_t i = r0; i < r1; ++i) clMaxO[(size_t)c] = std::max(clMaxO[(size_t)c], in.readOff[i + 1] - in.readOff[i]);
    maxO = std::max(maxO, clMaxO[(size_t)c]);
    if (r1 == r0) { state[(size_t)c].status = DNAS_POLISH_NO_READS; state[(size_t)c].active = false; }
    if (roundsMax == 0) state[(size_t)c].active = false;
    if (state[(size_t)c].active) { active.push_back(c); pairs0 += r1 - r0; }
  }
  const auto finish = [&] {
    for (int64_t c = 0; c < nc; ++c) {
      out_rounds[c] = state[(size_t)c].rounds;
      out_converged[c] = state[(size_t)c].converged;
      out_voters[c] = state[(size_t)c].voters;
      out_status[c] = state[(size_t)c].status;
    }
    return DNAS_OK;
  };
  if (active.empty()) return finish();

  DNAS_HIP_TRY(hipSetDevice(device));
  PaBuffers bufs;
  int rc;
  if ((rc = bufs.open())) return rc;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  size_t freeB = 0, totalB = 0;
  DNAS_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
  const size_t arenaLimit = arena_bytes ? arena_bytes / 2 : freeB / 2 / 2;
  int ldsPositions = kPolishLdsPositions;
  if (const char* s = getenv("DNAS_POLISH_LDS_POSITIONS")) ldsPositions = std::max(0, std::min(ldsPositions, atoi(s)));

  const PaScores sc = PaScores::from(hs);
  PaLaunchPlan plan;
  plan.cut(cus, 2, (int)maxO, pairs0);                     // 64 KiB of static LDS per work-group: two of them share a CU

  const size_t nA0 = active.size(), nP0 = (size_t)pairs0;
  int8_t* dReads = nullptr;
  int64_t *dReadOff = nullptr, *dCurOff = nullptr, *dNextOff = nullptr, *dReadBegin = nullptr, *dPairBegin = nullptr;
  int32_t *dCurLen = nullptr, *dNextCap = nullptr, *dPairAct = nullptr, *dNewLen = nullptr, *dVoters = nullptr, *dLdsList = nullptr,
          *dHbmList = nullptr;
  uint64_t *dRecOff = nullptr, *dTabOff = nullptr;
  uint8_t *dStrand = nullptr, *dChanged = nullptr;
  double *dSub = nullptr, *dScore = nullptr, *dBnd = nullptr;
  int* dFail = nullptr;
  if ((rc = paUpload(bufs, &dReads, in.readSeqs, (size_t)in.readOff[in.nReads]))) return rc;
  if ((rc = paUpload(bufs, &dReadOff, in.readOff, (size_t)in.nReads + 1))) return rc;
  if (in.readStrand && (rc = paUpload(bufs, &dStrand, in.readStrand, (size_t)in.nReads))) return rc;
  if ((rc = paUpload(bufs, &dSub, hs.sub, 16))) return rc;
  if ((rc = paAlloc(bufs, &dCurOff, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dNextOff, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dReadBegin, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dPairBegin, nA0 + 1))) return rc;
  if ((rc = paAlloc(bufs, &dCurLen, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dNextCap, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dNewLen, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dVoters, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dChanged, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dLdsList, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dHbmList, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dTabOff, nA0))) return rc;
  if ((rc = paAlloc(bufs, &dPairAct, nP0))) return rc;
  if ((rc = paAlloc(bufs, &dRecOff, nP0))) return rc;
  if ((rc = paAlloc(bufs, &dScore, nP0))) return rc;
  if ((rc = paAlloc(bufs, &dBnd, plan.bndDoubles()))) return rc;
  if ((rc = paAlloc(bufs, &dFail, 1))) return rc;
  DNAS_HIP_TRY(hipMemset(dFail, 0, sizeof(int)));
  dnas::DevBuf<int8_t> tmpl[2];
  dnas::DevBuf<uint16_t> arena;
  dnas::DevBuf<uint32_t> table;
  if ((rc = plNeed(tmpl[0], (size_t)in.tmplOff[nc]))) return rc;
  if (in.tmplOff[nc]) DNAS_HIP_TRY(hipMemcpy(tmpl[0].get(), in.tmplSeqs, (size_t)in.tmplOff[nc], hipMemcpyHostToDevice));

  struct Batch { int64_t pairFirst, pairEnd, ldsFirst, ldsEnd, hbmFirst, hbmEnd; };
  std::vector<int64_t> hCurOff, hNextOff, hReadBegin, hPairBegin;
  std::vector<int32_t> hCurLen, hNextCap, hPairAct, hLdsList, hHbmList, hNewLen, hVoters;
  std::vector<uint64_t> hRecOff, hTabOff;
  std::vector<uint8_t> hChanged;
  std::vector<int8_t> hNext;
  std::vector<Batch> batches;

  for (int32_t run = 1; !active.empty(); ++run) {
    const size_t nA = active.size();
    const int from = (run - 1) & 1, to = run & 1;
    hCurOff.assign(nA, 0); hNextOff.assign(nA, 0); hReadBegin.assign(nA, 0); hPairBegin.assign(nA + 1, 0);
    hCurLen.assign(nA, 0); hNextCap.assign(nA, 0); hTabOff.assign(nA, kPlInLds);
    hPairAct.clear(); hRecOff.clear(); hLdsList.clear(); hHbmList.clear(); batches.clear();
    int64_t nextTotal = 0, maxI = 0, ldsMaxI = 0;
    size_t tabWords = 0, used = 0, roundWords = 0, largest = 0;
    for (size_t a = 0; a < nA; ++a) maxI = std::max<int64_t>(maxI, curLen[(size_t)active[a]]);
    PaCellMemo memo(maxI, maxO, band);
    Batch bt{0, 0, 0, 0, 0, 0};
    for (size_t a = 0; a < nA; ++a) {
      const int64_t c = active[a], I = curLen[(size_t)c], r0 = in.clusterReadOff[c], r1 = in.clusterReadOff[c + 1];
      hCurOff[a] = curOff[(size_t)c];
      hCurLen[a] = (int32_t)I;
      hNextOff[a] = nextTotal;
      hNextCap[a] = (int32_t)dnas::polishCapacity(I, clMaxO[(size_t)c]);
      nextTotal += hNextCap[a];
      hReadBegin[a] = r0;
      size_t mine = 0;
      for (int64_t i = r0; i < r1; ++i) mine += PaGeom((int)I, (int)(in.readOff[i + 1] - in.readOff[i]), band).words();
      largest = std::max(largest, mine);
      if (used + mine > arenaLimit && used) {             // the batch is full: this cluster opens the next one
        batches.push_back(bt);
        bt = Batch{(int64_t)hPairAct.size(), 0, (int64_t)hLdsList.size(), 0, (int64_t)hHbmList.size(), 0};
        used = 0;
      }
      for (int64_t i = r0; i < r1; ++i) {
        const int64_t O = in.readOff[i + 1] - in.readOff[i];
        hPairAct.push_back((int32_t)a);
        hRecOff.push_back(used);
        used += PaGeom((int)I, (int)O, band).words();
        stats->cells += memo.cells(I, O);
      }
      roundWords = std::max(roundWords, used);
      hPairBegin[a + 1] = (int64_t)hPairAct.size();
      if (I <= ldsPositions) {
        hLdsList.push_back((int32_t)a);
        ldsMaxI = std::max(ldsMaxI, I);
      } else {
        hHbmList.push_back((int32_t)a);
        hTabOff[a] = tabWords;
        tabWords += dnas::polishWords(I);
      }
      bt.pairEnd = (int64_t)hPairAct.size(); bt.ldsEnd = (int64_t)hLdsList.size(); bt.hbmEnd = (int64_t)hHbmList.size();
    }
    batches.push_back(bt);
    if (largest > arenaLimit)
      return dnas::fail(DNAS_E_INVALID, "cluster consensus: the arena (" + std::to_string(arenaLimit * 2) + " bytes) is smaller than one cluster's records (" + std::to_string(largest * 2) + " bytes)");
    if ((rc = plNeed(arena, roundWords))) return rc;
    if ((rc = plNeed(tmpl[to], (size_t)nextTotal))) return rc;
    if ((rc = plNeed(table, tabWords))) return rc;
    if (tabWords) DNAS_HIP_TRY(hipMemsetAsync(table.get(), 0, tabWords * sizeof(uint32_t), bufs.stream));
    if ((rc = plSend(dCurOff, hCurOff)) || (rc = plSend(dNextOff, hNextOff)) || (rc = plSend(dReadBegin, hReadBegin)) ||
        (rc = plSend(dPairBegin, hPairBegin)) || (rc = plSend(dCurLen, hCurLen)) || (rc = plSend(dNextCap, hNextCap)) ||
        (rc = plSend(dTabOff, hTabOff)) || (rc = plSend(dPairAct, hPairAct)) || (rc = plSend(dRecOff, hRecOff)) ||
        (rc = plSend(dLdsList, hLdsList)) || (rc = plSend(dHbmList, hHbmList)))
      return rc;
    const PlRound r{tmpl[from].get(), tmpl[to].get(), dCurOff, dNextOff, dCurLen, dNextCap, dReadBegin, dPairBegin, dPairAct, dRecOff, dTabOff,
                    table.get(), dReads, dReadOff, dStrand, dScore, dNewLen, dVoters, dChanged, dFail};
    const size_t ldsBytes = dnas::polishWords(ldsMaxI) * sizeof(uint32_t);

    for (const Batch& b : batches) {
      const int64_t count = b.pairEnd - b.pairFirst, nLds = b.ldsEnd - b.ldsFirst, nHbm = b.hbmEnd - b.hbmFirst;
      if (count == 0) continue;
      DNAS_HIP_TRY(hipEventRecord(bufs.ev[0], bufs.stream));
      paDispatchKP(sc.P, [&](auto kp) {
        hipLaunchKernelGGL(polish_fill_kernel<decltype(kp)::value>, dim3(plan.blocks(count)), dim3(64 * kPaWavesPerBlock), 0, bufs.stream,
                           sc, dSub, band, b.pairFirst, count, r, arena.get(), dBnd, plan.bndStride);
      });
      DNAS_HIP_TRY(hipGetLastError());
      DNAS_HIP_TRY(hipEventRecord(bufs.ev[1], bufs.stream));
      if (nLds) {
        hipLaunchKernelGGL(polish_vote_lds_kernel, dim3((unsigned)nLds), dim3(64), ldsBytes, bufs.stream, band, dLdsList + b.ldsFirst, r,
                           arena.get());
        DNAS_HIP_TRY(hipGetLastError());
      }
      if (nHbm) {
        hipLaunchKernelGGL(polish_vote_hbm_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, bufs.stream, band, b.pairFirst, count,
                           r, arena.get());
        DNAS_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(polish_emit_hbm_kernel, dim3((unsigned)nHbm), dim3(64), 0, bufs.stream, dHbmList + b.hbmFirst, r);
        DNAS_HIP_TRY(hipGetLastError());
      }
      DNAS_HIP_TRY(hipEventRecord(bufs.ev[2], bufs.stream));
      DNAS_HIP_TRY(hipStreamSynchronize(bufs.stream));
      float fill = 0, vote = 0;
      DNAS_HIP_TRY(hipEventElapsedTime(&fill, bufs.ev[0], bufs.ev[1]));
      DNAS_HIP_TRY(hipEventElapsedTime(&vote, bufs.ev[1], bufs.ev[2]));
      stats->fill_ms += fill;
      stats->vote_ms += vote;
      ++stats->batches;
    }
    ++stats->rounds;
    stats->pairs += (int64_t)hPairAct.size();
    stats->lds_clusters += (int64_t)hLdsList.size();
    stats->hbm_clusters += (int64_t)hHbmList.size();

    int failed = 0;
    hNewLen.resize(nA); hVoters.resize(nA); hChanged.resize(nA); hNext.resize((size_t)std::max<int64_t>(nextTotal, 1));
    DNAS_HIP_TRY(hipMemcpy(&failed, dFail, sizeof(int), hipMemcpyDeviceToHost));
    if (failed) return dnas::fail(DNAS_E_DEVICE, failed & 1 ? "cluster consensus: a traceback left its record" : "cluster consensus: a new template left its slot");
    DNAS_HIP_TRY(hipMemcpy(hNewLen.data(), dNewLen, nA * sizeof(int32_t), hipMemcpyDeviceToHost));
    DNAS_HIP_TRY(hipMemcpy(hVoters.data(), dVoters, nA * sizeof(int32_t), hipMemcpyDeviceToHost));
    DNAS_HIP_TRY(hipMemcpy(hChanged.data(), dChanged, nA, hipMemcpyDeviceToHost));
    if (nextTotal) DNAS_HIP_TRY(hipMemcpy(hNext.data(), tmpl[to].get(), (size_t)nextTotal, hipMemcpyDeviceToHost));
    std::vector<int64_t> still;
    for (size_t a = 0; a < nA; ++a) {
      const int64_t c = active[a];
      state[(size_t)c].after(hVoters[a], hChanged[a] != 0, run, roundsMax);
      curOff[(size_t)c] = hNextOff[a];
      curLen[(size_t)c] = hNewLen[a];
      if (state[(size_t)c].active) still.push_back(c);
      else (*seqs)[(size_t)c].assign(hNext.begin() + hNextOff[a], hNext.begin() + hNextOff[a] + hNewLen[a]);
    }
    active.swap(still);
  }
  return finish();
}

}  // namespace

extern "C" int dnas_cluster_consensus(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, const int8_t* tmpl_seqs,
                                      const int64_t* tmpl_off, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                      const uint8_t* read_strand, const int64_t* cluster_read_off, int32_t rounds_max, int device_id,
                                      size_t arena_bytes, int8_t** out_seqs, int64_t* out_off, int32_t* out_rounds,
                                      uint8_t* out_converged, int32_t* out_voters, uint8_t* out_status, dnas_polish_stats* out_stats) {
  if (const int rc = dnas::checkPolishArgs(params, band, n_clusters, tmpl_seqs, tmpl_off, n_reads, read_seqs, read_off, read_strand,
                                           cluster_read_off, rounds_max, out_seqs, out_off, out_rounds, out_converged, out_voters, out_status))
    return rc;
  *out_seqs = nullptr;
  dnas_polish_stats total{};
  if (out_stats) *out_stats = total;
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  try {
    const dnas::PairScores hs = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    const int64_t zero = 0;
    const int8_t none = 0;
    const PlInputs all{n_clusters, n_reads, n_clusters ? tmpl_seqs : &none, n_clusters ? tmpl_off : &zero, n_reads ? read_seqs : &none,
                       n_reads ? read_off : &zero, read_strand, cluster_read_off};
    const std::vector<int> devices = dnas::pickDevices(device_id);
    const size_t W = devices.size();
    std::vector<std::vector<int8_t>> seqs;
    if (W == 1 || n_clusters == 0) {
      const int rc = plRunOnDevice(devices[0], hs, band, all, rounds_max, arena_bytes, &seqs, out_rounds, out_converged, out_voters,
                                   out_status, &total);
      if (rc != DNAS_OK) return rc;
      if (out_stats) *out_stats = total;
      return dnas::polishExport(seqs, out_seqs, out_off);
    }
    // every GPU of the node: the clusters dealt by (template length + 1) x the sum of their reads' lengths, one host thread per
    // device, every device's templates, reads and offsets gathered for it, results scattered back under the caller's indices
    std::vector<int64_t> cost((size_t)n_clusters);
    for (int64_t c = 0; c < n_clusters; ++c) {
      const int64_t r0 = cluster_read_off[c], r1 = cluster_read_off[c + 1];
      cost[(size_t)c] = (tmpl_off[c + 1] - tmpl_off[c] + 1) * (r1 > r0 ? read_off[r1] - read_off[r0] : 0);
    }
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(cost, W);
    std::vector<dnas_polish_stats> stats(W);
    seqs.assign((size_t)n_clusters, {});
    const int rc = dnas::forEachDevice(devices, [&](size_t k) {
      const std::vector<int64_t>& mine = shard[k];
      const size_t m = mine.size();
      std::vector<int64_t> readIds, clReadOff(1, 0), tmplOff, readOff;
      for (int64_t c : mine) {
        for (int64_t i = cluster_read_off[c]; i < cluster_read_off[c + 1]; ++i) readIds.push_back(i);
        clReadOff.push_back((int64_t)readIds.size());
      }
      std::vector<int8_t> tmpls, reads;
      dnas::gatherShard(mine, all.tmplSeqs, all.tmplOff, &tmpls, &tmplOff);
      dnas::gatherShard(readIds, all.readSeqs, all.readOff, &reads, &readOff);
      std::vector<uint8_t> strand(readIds.size() + 1);
      if (read_strand) for (size_t q = 0; q < readIds.size(); ++q) strand[q] = read_strand[readIds[q]];
      const PlInputs part{(int64_t)m, (int64_t)readIds.size(), tmpls.data(), tmplOff.data(), reads.data(), readOff.data(),
                          read_strand ? strand.data() : nullptr, clReadOff.data()};
      std::vector<std::vector<int8_t>> got;
      std::vector<int32_t> rounds(m + 1), voters(m + 1);
      std::vector<uint8_t> converged(m + 1), status(m + 1);
      const int rc = plRunOnDevice(devices[k], hs, band, part, rounds_max, arena_bytes, &got, rounds.data(), converged.data(), voters.data(),
                                   status.data(), &stats[k]);
      if (rc != DNAS_OK) return rc;
      for (size_t q = 0; q < m; ++q) {
        const int64_t c = mine[q];
        seqs[(size_t)c].swap(got[q]);
        out_rounds[c] = rounds[q];
        out_converged[c] = converged[q];
        out_voters[c] = voters[q];
        out_status[c] = status[q];
      }
      return DNAS_OK;
    });
    if (rc != DNAS_OK) return rc;
    for (size_t k = 0; k < W; ++k) {
      total.fill_ms = std::max(total.fill_ms, stats[k].fill_ms);
      total.vote_ms = std::max(total.vote_ms, stats[k].vote_ms);
      total.rounds = std::max(total.rounds, stats[k].rounds);
      total.pairs += stats[k].pairs;
      total.cells += stats[k].cells;
      total.batches += stats[k].batches;
      total.lds_clusters += stats[k].lds_clusters;
      total.hbm_clusters += stats[k].hbm_clusters;
    }
    if (out_stats) *out_stats = total;
    return dnas::polishExport(seqs, out_seqs, out_off);
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}
