// Device runtime behind the C ABI: model upload, lattice arena, batch scheduling and
// kernel launches for the Viterbi path (include/dnastore_amd.h, "device side").
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "device_buffer.hpp"
#include "device_model.h"
#include "traceback_step.h"
#include "errors.hpp"
#include "host/plan.hpp"
#include <cmath>

#include "jit.hpp"

extern "C" __global__ void copy_rows_kernel(double*, const double*, size_t, size_t, size_t);
extern "C" __global__ void viterbi_fill_kernel(DevModel, const uint8_t*, const uint64_t*, const int32_t*,
                                               const uint64_t*, double*, double*, unsigned long long*, int, const int*);
extern "C" __global__ void expand_lattice_kernel(DevModel, const uint8_t*, const double*, double*);
extern "C" __global__ void viterbi_traceback_wave_kernel(DevModel, const uint8_t*, const uint64_t*, const int32_t*,
                                                         const uint64_t*, const double*, char*, const uint64_t*,
                                                         uint32_t*, uint8_t*, int, unsigned long long*, const uint64_t*, uint32_t*,
                                                         const int*, TracebackWalk*);
extern "C" __global__ void fill_neginf_kernel(double*, size_t);
extern "C" __global__ void sync_latency_kernel(unsigned*, int, int, int, unsigned long long*, unsigned*);
extern "C" __global__ void xcc_probe_kernel(unsigned*);
extern "C" __global__ void check_bases_kernel(const uint8_t*, size_t, unsigned long long*);
extern "C" __global__ void viterbi_traceback_kernel(DevModel, const uint8_t*, const uint64_t*, const int32_t*,
                                                    const uint64_t*, const double*, char*, const uint64_t*,
                                                    uint32_t*, uint8_t*, int, unsigned long long*, const uint64_t*, uint32_t*, int);
// strand_kernels.hip
extern "C" __global__ void revcomp_reads_kernel(const uint8_t*, const uint64_t*, uint8_t*, uint8_t*);
extern "C" __global__ void strand_pick_kernel(const int32_t*, const uint64_t*, int, const double*, double*, uint8_t*, int32_t*,
                                              uint64_t*, int32_t*, unsigned long long*);
extern "C" __global__ void strand_rows_kernel(const uint64_t*, int, const int32_t*, int, uint64_t*);
extern "C" __global__ void strand_copy_rows_kernel(double*, const double*, size_t, size_t, size_t, const int32_t*);
extern "C" __global__ void strand_gather_kernel(const int32_t*, int, int, const uint32_t*, const uint8_t*, uint32_t*, uint8_t*,
                                                uint32_t*);

using dnas::DevBuf;

// kernel-argument block of viterbi_fill_tiera (must mirror csrc/viterbi_tiera.hip)
struct TierAArgs {
  int N, local;
  double noGap, delOpen, delExtend, delEnd, tanDup;
  double sub[16];
  double len[8];
  double score[4];
};
struct TierALaunch {
  TierAArgs a;
  const unsigned* entTab;
  const unsigned* metaTab;
  const uint8_t* bases;
  const uint64_t* readOff;
  const int32_t* batchRead;
  const uint64_t* slotOff;
  double* arena;
  double* outLoglike;
  unsigned long long* roundsTotal;
  // tier C (a cluster of work-groups per read): exchange buffers, sync blocks, clusters in this launch, reads in this launch
  double* xbuf;
  unsigned* syncWords;
  const unsigned* foldTab;
  int nClusters;
  int nReads;
  unsigned long long timeoutTicks;
  unsigned long long arriveTicks;
  const int* colRange;          // bounded-memory decode: [nReads][2] first and last column of this launch (null: whole reads)
  int spread;                   // tier C: 1 = a cluster's members are neighbouring blocks (dealt over the XCDs; option cluster_spread)
};

struct dnas_model {
  int device = 0;
  int tier = 0;                 // 1 = tier A (register/LDS-resident JIT kernel, one work-group per read), 2 = tier C (the same
                                // kernel, a cluster of work-groups per read), 0 = tier B (global-memory kernel)
  // bounded-memory decode: reads whose lattice does not fit the arena (checkpoint=auto), or every read (always), are
  // filled in segments of `segmentCols` columns (0: chosen from the arena) from checkpoints, twice -- see DESIGN.md 3.7
  int checkpointMode = 0;       // 0 auto, 1 always, 2 never
  int segmentCols = 0;
  int64_t lastCheckpointed = 0; // reads (in sorted order: the longest) of the last call that went that way
  DevBuf<int> dColRange;         // the per-segment tables and the parked walks of the last call that had segmented reads
  DevBuf<uint64_t> dSegSlot;
  DevBuf<TracebackWalk> dWalks;
  bool waveTraceback = true;    // one wave per read for batches of up to 256 reads (option traceback=thread: never)
  int tbThreads = kTraceThreads;     // threads per block of the thread-per-read traceback (option tb_threads)
  int tbLanes = kTraceLanes;         // reads per wave there (option tb_lanes): the other lanes idle
  int maxClusters = 1;          // tier C: clusters that fit the GPU at once
  DevBuf<double> dXbuf;         // tier C: exchange buffers, one per cluster
  unsigned* dSync = nullptr;    // tier C: sync blocks (64 u32 per cluster), inside dSyncBase
  DevBuf<unsigned> dSyncBase;   // ... the allocation they sit in: the blocks are placed inside it by measured latency
  std::string syncPlaceNote;
  std::vector<double> syncLat;     // [8 XCCs][syncCand] measured round trips (ticks), by the XCC id the measuring block ran on; empty: not measured
  int syncCand = 0;
  size_t syncOffNow = 0;           // where the blocks sit in their window right now
  DevBuf<unsigned, dnas::PinnedMem> xccProbe;   // pinned host word the probe kernel writes
  DevBuf<unsigned> dFoldTab;    // tier C: inbox slot -> LDS cells, per member
  size_t xStride = 0;           // doubles per cluster in dXbuf
  unsigned long long timeoutTicks = 0, arriveTicks = 0;
  int clusterSpread = 0;        // members of a cluster dealt over the XCDs (option cluster_spread; default: when that fits a quarter more clusters)
  DevBuf<unsigned, dnas::PinnedMem> syncCheck;   // pinned host copies of the sync blocks of every launch of the last call (watchdog, placement census)
  size_t syncCheckWords = 0;
  size_t syncLaunches = 0;
  unsigned clustersSeen = 0, clustersSplit = 0;   // last call: clusters that ran, clusters whose members sat on more than one XCD
  std::string tierNote;
  dnas::TierAPlan plan;
  hipModule_t module = nullptr;
  hipFunction_t fillA = nullptr;
  hipModule_t moduleSeg = nullptr;  // the same kernel built with -DDNAS_SEGMENTS=1 (bounded-memory decode), compiled at first use
  hipFunction_t fillSeg = nullptr;
  std::string jitDefs;
  TierAArgs argsA{};
  DevBuf<unsigned> dEntTab, dMetaTab;
  DevBuf<int32_t> dSlotOf;
  hipStream_t stream = nullptr;     // fill kernels
  hipStream_t stream2 = nullptr;    // traceback kernels (batch i traces back while batch i+1 fills)
  hipStream_t stream3 = nullptr;    // tier A, ring of arena slices: the fills of the odd batches (viterbi_call)
  hipEvent_t ringHead = nullptr, ringTail = nullptr;   // the call's prologue on `stream` -> stream3; the tail of stream3 -> `stream`
  int fillOverlap = 1;              // option fill_overlap: 0 never, 1 the default rule (plan_call), 2 also re-cut an explicit arena
  bool arenaGiven = false;          // the caller named arena_bytes
  int lastSlices = 0;               // batches whose lattices the last call kept side by side (1, 2 or kRingSlices)
  std::vector<hipEvent_t> sync;     // 2 per batch: fill done, traceback done
  DevModel dm{};
  dnas::DevPool tables;       // the device copies of the machine's tables (dm points into them)
  DevBuf<double> arena;       // the lattices of a call: replaced when a call needs more (viterbi_call)
  size_t arenaCap = 0;
  int maxSlots = 512;
  DevBuf<unsigned long long> dRounds;
  // per-call scheduling arrays (device), grown on demand to exactly what a call needs
  DevBuf<int32_t> dBatchRead;
  DevBuf<uint64_t> dSlotOff, dReadOff, dOutOff;
  size_t halfDoubles = 0;              // size of one arena half (doubles)
  std::vector<uint64_t> lastSlotOff;   // host copy, sorted-batch order of the last call
  std::vector<int32_t> lastBatchRead;
  std::vector<int64_t> lastBatchStart; // first read (sorted order) of every batch of the last call, + n_reads
  std::vector<uint64_t> lastReadOff;   // host copy of the last call's read offsets
  const uint8_t* lastBases = nullptr;  // device pointer of the last call's bases (valid while the caller keeps it)
  // dnas_viterbi_batch's device copies of the caller's host arrays: only ever grown (an allocation or a free per call is what
  // another tenant of the card can hold up for seconds: tools/alloc_probe.py); the bases stay valid until the next call
  // (lattice export)
  DevBuf<uint8_t> ioBases; DevBuf<char> ioSym;                                          // growQuarter256
  DevBuf<uint32_t> ioLen; DevBuf<double> ioLL; DevBuf<uint8_t> ioSt, ioStrand;          // per read: growQuarter64
  std::vector<hipEvent_t> events;      // 4 per batch: fill start/end (the batch's fill stream), traceback start/end (stream2)
  dnas_batch_stats stats{};
  bool statsPending = false;
  // optional traceback event log (the reference's level-3 messages): device buffers of the last call
  bool eventLog = false;
  DevBuf<unsigned long long> dEvents;
  DevBuf<uint64_t> dEvOff;
  DevBuf<uint32_t> dEvLen;
  std::vector<uint64_t> evOff;
  std::vector<uint64_t> evWant;        // the call in hand runs again because a read's log was full: events per caller read to make room for
  // both-strand decode (strand_kernels.hip): buffers per VIRTUAL read (2n + 2 of them: caller read i as written,
  // n + 1 + i reverse-complemented), only ever grown, like the io buffers
  DevBuf<uint8_t> sBases;                                   // the reads as written, behind them their reverse complements (growQuarter256)
  DevBuf<uint64_t> sOff;                                    // mode "reverse": the read offsets the reverse-complement kernel reads (growQuarter256)
  DevBuf<double> sLL; DevBuf<uint32_t> sLen; DevBuf<uint8_t> sSt;               // what fill and traceback write per virtual read (growQuarter64)
  DevBuf<int32_t> sWinRead, sWinRow; DevBuf<uint64_t> sWinSlot;                 // per caller read: the winner, sorted order (growQuarter64)
  DevBuf<uint64_t> dWinSegSlot; DevBuf<int> dWinColRange;   // bounded-memory decode: the winners' per-segment tables (growQuarter256)
  bool lastBoth = false;            // the last call was a DNAS_STRAND_BOTH call
  int64_t lastSegColumns = 0;       // columns of the reads of the last call that went through segments
  dnas_strand_stats strandStats{};
};

// Tier A: the slices of the lattice arena a call's batches go round when their fills overlap (viterbi_call): two fills in flight
// on two fill streams and a third batch under traceback.  Four slices measured no better than three on the bench workload, and
// a third fill stream measured faster in one process layout and slower than no ring in another (profiles/EXPERIMENTS.md).
constexpr int kRingSlices = 3;

constexpr size_t kSyncWindow = 64 * 1024, kSyncStep = 1024;   // the sync blocks of a tier-C model sit somewhere in a window this much longer than they are

// Where in their window the sync blocks serve a launch best, given the measured round trips (m->syncLat) and the XCC the launch's
// block 0 -- cluster 0 -- is expected on: cluster c of a launch runs on the XCC c after it (whole clusters per XCD), the clusters of
// a spread plan on all of them.  The first cluster counts four times: a launch of ONE cluster is what latency is asked of.
static size_t place_sync_words(const dnas_model* m, unsigned firstXcc) {
  if (m->syncLat.empty()) return 0;
  const int first = std::min(8, m->maxClusters), nC = m->syncCand;
  double best = -1;
  size_t at = 0;
  for (size_t off = 0; off <= kSyncWindow; off += kSyncStep) {
    double cost = 0;
    for (int c = 0; c < first; ++c) {
      const size_t k = (off + (size_t)c * 256) / kSyncStep;
      if ((int)k >= nC) { cost = -1; break; }
      double t = 0;
      if (m->clusterSpread) { for (int x = 0; x < 8; ++x) t += m->syncLat[(size_t)x * nC + k] / 8; }
      else t = m->syncLat[(size_t)((firstXcc + (unsigned)c) & 7u) * nC + k];
      cost += (c == 0 ? 4.0 : 1.0) * t;
    }
    if (cost >= 0 && (best < 0 || cost < best)) { best = cost; at = off; }
  }
  return at;
}

namespace {

// roctx ranges around the phases of a call (visible in rocprofv3 --marker-trace): the marker library is looked up at run
// time, so that the shared library does not depend on it
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* lib : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      if (void* h = dlopen(lib, RTLD_LAZY | RTLD_LOCAL)) {
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() { static Roctx r; return r; }
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~RoctxRange() { if (on) roctx().pop(); }
};

template <class T>
int upload(dnas_model* m, const T* host, size_t n, const T** out) {
  DNAS_HIP_TRY(m->tables.upload(host, n, const_cast<T**>(out)));     // (the model reads what it uploaded, and only reads)
  return DNAS_OK;
}

int collect_stats(dnas_model* m) {
  if (!m->statsPending) return DNAS_OK;
  m->stats.fill_ms = m->stats.traceback_ms = 0;
  // fill_ms: the time during which at least one fill launch of the call ran.  Launches that go down one stream are apart, and
  // that time is the sum of their durations; the launches of a ring call overlap, and it is the length of the union of their
  // intervals, taken against the call's first event.  The tracebacks are serial either way.
  const bool overlapped = m->lastSlices >= kRingSlices;
  std::vector<std::pair<double, double>> spans;
  for (size_t i = 0; i + 4 <= m->events.size(); i += 4) {
    float a = 0, b = 0;
    DNAS_HIP_TRY(hipEventElapsedTime(&a, m->events[i], m->events[i + 1]));
    DNAS_HIP_TRY(hipEventElapsedTime(&b, m->events[i + 2], m->events[i + 3]));
    if (overlapped) {
      float at = 0;
      if (i > 0) DNAS_HIP_TRY(hipEventElapsedTime(&at, m->events[0], m->events[i]));
      spans.emplace_back((double)at, (double)at + (double)a);
    } else {
      m->stats.fill_ms += a;
    }
    m->stats.traceback_ms += b;
  }
  if (overlapped) {
    std::sort(spans.begin(), spans.end());
    double from = 0, to = 0;
    bool open = false;
    for (const auto& sp : spans) {
      if (open && sp.first <= to) { to = std::max(to, sp.second); continue; }
      if (open) m->stats.fill_ms += to - from;
      from = sp.first; to = sp.second; open = true;
    }
    if (open) m->stats.fill_ms += to - from;
  }
  unsigned long long r = 0;
  DNAS_HIP_TRY(hipMemcpy(&r, m->dRounds.get(), sizeof r, hipMemcpyDeviceToHost));
  m->stats.rounds = (int64_t)r;
  if (m->lastBoth) {           // what strand_pick_kernel counted (words 12-14 of the rounds buffer)
    unsigned long long c[3] = {0, 0, 0};
    DNAS_HIP_TRY(hipMemcpy(c, m->dRounds.get() + 12, sizeof c, hipMemcpyDeviceToHost));
    m->strandStats.reverse_won = (int64_t)c[0]; m->strandStats.ties = (int64_t)c[1]; m->strandStats.both_no_path = (int64_t)c[2];
  }
  m->statsPending = false;
  if (m->tier == 2) {
    unsigned xccMixed = 0, clusters = 0;
    for (size_t c = 0; c * 64 < m->syncCheckWords; ++c) {
      const unsigned* w = m->syncCheck.get() + c * 64;
      if (w[1]) return dnas::fail(DNAS_E_DEVICE, "tier C: a cluster did not agree on a lattice column within the watchdog time, or its work-groups were "
                                                 "not all started within the arrival time (launch aborted; options cluster_timeout_s, cluster_arrive_s)");
      if (w[40]) { ++clusters; if (w[40] & (w[40] - 1)) ++xccMixed; }
      if (c == 0 && getenv("DNAS_SYNC_DEBUG")) fprintf(stderr, "sync debug: cluster 0 ran on XCC mask 0x%x, its epoch word counted %u bumps\n", w[40], w[0]);
    }
    m->clustersSeen = clusters; m->clustersSplit = xccMixed;
  }
  return DNAS_OK;
}

}  // namespace

namespace {

// Which row program serves a machine fastest?  The planner can deal the states breadth first or by longest-path level
// (host/plan.hpp: PlanChoice); which is best depends on the machine and the plan's cost model does not predict it, so it is
// measured and RECORDED: dnastore_amd/tune/ ships the verdicts of the fixture and bench machines (tools/make_tune_records.sh:
// bench-like reads), and a model follows its machine's record.  The record's name hashes the machine's graph (not the error
// model: the row programs do not depend on it), the work-group shape and the planner version; the kernel source it was
// measured with is named INSIDE the record ("kernel=<hash>"), so that an edit of the kernel leaves the records in force and
// tests/test_tune_records.py says which ones to measure again.
std::string tune_record_name(const dnas_flat_model* fm, int members, int threads) {
  std::string graph((const char*)&fm->n_states, sizeof fm->n_states);
  auto add = [&](const void* ptr, size_t bytes) { graph.append((const char*)ptr, bytes); };
  add(&fm->max_dup_len, sizeof fm->max_dup_len); add(&threads, sizeof threads); add(&members, sizeof members);
  add(&dnas::kPlanVersion, sizeof dnas::kPlanVersion);
  add(fm->ein_ptr, ((size_t)fm->n_states + 1) * sizeof(int32_t)); add(fm->ein_src, (size_t)fm->n_emit * sizeof(int32_t));
  add(fm->ein_score, (size_t)fm->n_emit * sizeof(double)); add(fm->ein_base, (size_t)fm->n_emit);
  add(fm->nin_ptr, ((size_t)fm->n_states + 1) * sizeof(int32_t)); add(fm->nin_src, (size_t)fm->n_null * sizeof(int32_t));
  add(fm->nin_score, (size_t)fm->n_null * sizeof(double));
  char name[64];
  snprintf(name, sizeof name, "tune_%016llx.txt", dnas::textHash(graph));
  return name;
}

// "order=<o> slack=<s> kernel=<hash> ..." -> the choice a record names (false: no record / not readable)
bool parse_plan_record(const std::string& note, dnas::PlanChoice* choice, std::string* kernel = nullptr) {
  int o = -1, sl = 0;
  char k[32] = "";
  if (sscanf(note.c_str(), "order=%d slack=%d kernel=%31s", &o, &sl, k) < 2 || o < 0 || o > 2 || sl < 0 || sl > 8) return false;
  choice->order = o;
  choice->slack = sl;
  if (kernel) *kernel = k;
  return true;
}

// the record of a machine, if there is one: the choice, and a note for dnas_model_tier ("record tune_x.txt" / "... stale: measured
// with another kernel source")
bool follow_plan_record(const dnas_flat_model* fm, int members, int threads, dnas::PlanChoice* choice, std::string* note) {
  const std::string name = tune_record_name(fm, members, threads);
  std::string kernel;
  if (!parse_plan_record(dnas::cacheNoteRead(name), choice, &kernel)) { *note = "no tuning record (default row program)"; return false; }
  char now[32];
  snprintf(now, sizeof now, "%016llx", dnas::kernelSourceHash());
  *note = "record " + name + " order=" + std::to_string(choice->order) + " slack=" + std::to_string(choice->slack) +
          (kernel == now ? "" : " (stale: measured with kernel " + kernel + ", this is " + now + ")");
  return true;
}

// The choice a model of this machine would be planned with when nothing is forced by an option: the environment (DNAS_PLAN_ORDER,
// DNAS_PLAN_SLACK: left to the planner), else the machine's tuning record unless DNAS_RECORDS=0, else the default.  The
// precompile and analysis entry points use it, so that what they compile or describe is the program a model runs.
dnas::PlanChoice env_or_recorded_choice(const dnas_flat_model* fm, int members, int threads) {
  dnas::PlanChoice choice;
  if (!getenv("DNAS_PLAN_ORDER") && !getenv("DNAS_PLAN_SLACK") && !(getenv("DNAS_RECORDS") && atoi(getenv("DNAS_RECORDS")) == 0))
    (void)parse_plan_record(dnas::cacheNoteRead(tune_record_name(fm, members, threads)), &choice);
  return choice;
}
int env_threads(int fallback) { return getenv("DNAS_THREADS") && atoi(getenv("DNAS_THREADS")) > 0 ? atoi(getenv("DNAS_THREADS")) : fallback; }

// autotune=1 and no record: time the candidate programs on synthetic reads once (one launch each), keep the verdict in the
// kernel cache.  The reads are what a random walk through the machine emits (a code word sequence) with one base in a hundred
// substituted; the lattice arena of the timing models is the caller's (at most 8 GiB).
int tune_row_program(const dnas_flat_model* fm, int device_id, int threads, size_t arena_bytes, dnas::PlanChoice* choice) {
  *choice = dnas::PlanChoice{1, 0};
  const std::string name = tune_record_name(fm, 1, threads);
  const size_t arena = std::min<size_t>(arena_bytes ? arena_bytes : (size_t)8 << 30, (size_t)8 << 30);
  const int L = 480;
  // a read's lattice: (L + 1) columns of 2 lanes of (about) n_states doubles; half the arena holds a launch
  const int nReads = (int)std::max<size_t>(4, std::min<size_t>(240, arena / 2 / ((size_t)(L + 1) * 2 * 8 * ((size_t)fm->n_states + 2048))));
  std::vector<uint8_t> bases((size_t)L * nReads);
  {
    // (destination, emitted base or -1); the walk stays inside one message: it does not take an edge that reads the
    // end-of-message symbol '$' while another one is there
    std::vector<std::vector<std::pair<int, int>>> out((size_t)fm->n_states), outEnd((size_t)fm->n_states);
    for (int j = 0; j < fm->n_states; ++j) {
      for (int e = fm->ein_ptr[j]; e < fm->ein_ptr[j + 1]; ++e) (fm->ein_in[e] == '$' ? outEnd : out)[(size_t)fm->ein_src[e]].emplace_back(j, (int)fm->ein_base[e]);
      for (int e = fm->nin_ptr[j]; e < fm->nin_ptr[j + 1]; ++e) (fm->nin_in[e] == '$' ? outEnd : out)[(size_t)fm->nin_src[e]].emplace_back(j, -1);
    }
    for (int j = 0; j < fm->n_states; ++j) if (out[(size_t)j].empty()) out[(size_t)j] = outEnd[(size_t)j];
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int r = 0; r < nReads; ++r) {
      int state = 0, got = 0;
      for (long steps = 0; got < L && steps < 64l * L; ++steps) {
        if (out[(size_t)state].empty()) { state = 0; continue; }
        const std::pair<int, int>& e = out[(size_t)state][rnd() % out[(size_t)state].size()];
        state = e.first;
        if (e.second >= 0) bases[(size_t)r * L + got++] = (uint8_t)((rnd() % 100 == 0) ? (e.second + 1 + rnd() % 3) & 3 : e.second);
      }
      for (; got < L; ++got) bases[(size_t)r * L + got] = (uint8_t)(rnd() & 3);       // (a machine that emits too little)
    }
  }
  std::vector<uint64_t> readOff(nReads + 1), outOff(nReads + 1);
  const size_t cap = 4 * (size_t)L + 64;
  for (int r = 0; r <= nReads; ++r) { readOff[(size_t)r] = (uint64_t)r * L; outOff[(size_t)r] = (uint64_t)r * cap; }
  std::vector<char> sym(cap * nReads);
  std::vector<uint32_t> len(nReads);
  std::vector<double> ll(nReads);
  std::vector<uint8_t> st(nReads);
  // the default first: another candidate has to beat it by 1.5 % (run-to-run differences of one program stay below 0.5 %)
  const dnas::PlanChoice candidates[] = {{1, 0}, {2, 0}, {2, 8}};
  double best = 0;
  std::string report;
  for (const dnas::PlanChoice& c : candidates) {
    dnas_model* t = nullptr;
    const std::string options = "tier=A,autotune=0,plan_order=" + std::to_string(c.order) + ",plan_slack=" + std::to_string(c.slack) + ",threads=" + std::to_string(threads);
    int rc = dnas_model_create_ex(fm, device_id, arena, options.c_str(), &t);
    if (rc != DNAS_OK) { if (c.order == 1) return DNAS_OK; continue; }   // (the creation that asked reports what is wrong)
    dnas_batch_stats s{};
    double fastest = 0;
    for (int rep = 0; rep < 3 && rc == DNAS_OK; ++rep) {          // the first run warms up; the faster of the other two counts
      rc = dnas_viterbi_batch(t, nReads, readOff.data(), bases.data(), sym.data(), outOff.data(), len.data(), ll.data(), st.data());
      if (rc == DNAS_OK) rc = dnas_model_last_stats(t, &s);
      if (rc == DNAS_OK && rep > 0 && (fastest == 0 || s.fill_ms < fastest)) fastest = s.fill_ms;
    }
    dnas_model_destroy(t);
    s.fill_ms = fastest;
    if (rc != DNAS_OK || !(s.fill_ms > 0)) continue;
    char item[96];
    snprintf(item, sizeof item, "  %d/%d: %.3f ms", c.order, c.slack, s.fill_ms);
    report += item;
    if (best == 0 || s.fill_ms < 0.985 * best) { if (best == 0 || s.fill_ms < best) best = s.fill_ms; *choice = c; }
  }
  if (best == 0) return DNAS_OK;
  char head[200];
  snprintf(head, sizeof head, "order=%d slack=%d kernel=%016llx   (fill of %d synthetic reads of %d bases;", choice->order, choice->slack,
           dnas::kernelSourceHash(), nReads, L);
  dnas::cacheNoteWrite(name, std::string(head) + report + ")\n");
  return DNAS_OK;
}

}  // namespace

extern "C" int dnas_has_device_code(void) { return 1; }

extern "C" int dnas_debug_alloc_stats(int64_t out[5], int reset) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "dnas_debug_alloc_stats: out is null");
  dnas::debugAllocStats(out, reset != 0);
  return DNAS_OK;
}

extern "C" int dnas_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

extern "C" int dnas_model_create(const dnas_flat_model* fm, int device_id, size_t arena_bytes, dnas_model** out) {
  return dnas_model_create_ex(fm, device_id, arena_bytes, nullptr, out);
}

// options: "key=value,key=value"; keys tier (A|B|C), cluster (work-groups per read), threads (512 | 1024 per work-group),
// max_clusters, max_slots, fill_overlap (tier A: 0 | 1 | 2, plan_call), cluster_timeout_s, traceback, arena_fraction, checkpoint, segment, plan_order (dealing order: 0 depth
// first, 1 breadth first, 2 longest-path levels), plan_slack, records (0: ignore the machine's tuning record), autotune (1: a
// tier-A machine without a record is timed once and the verdict kept in the kernel cache).  A key that is absent falls back to
// the environment variable DNAS_<KEY>.
extern "C" int dnas_model_create_ex(const dnas_flat_model* fm, int device_id, size_t arena_bytes, const char* options,
                                    dnas_model** out) {
  if (!fm || !out) return dnas::fail(DNAS_E_INVALID, "dnas_model_create: null argument");
  *out = nullptr;
  const std::string optStr = options ? options : "";
  std::string optHold;
  auto opt = [&](const char* key) -> const char* {
    const std::string k = std::string(key) + "=";
    size_t at = 0;
    while (at < optStr.size()) {
      size_t end = optStr.find(',', at);
      if (end == std::string::npos) end = optStr.size();
      if (optStr.compare(at, k.size(), k) == 0) { optHold = optStr.substr(at + k.size(), end - at - k.size()); return optHold.c_str(); }
      at = end + 1;
    }
    std::string env = "DNAS_" + std::string(key);
    for (char& c : env) c = (char)toupper((unsigned char)c);
    return getenv(env.c_str());
  };
  if (fm->n_len > kMaxLen) return dnas::fail(DNAS_E_UNSUPPORTED, "pLen longer than 32 entries");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return dnas::fail(DNAS_E_DEVICE, "no HIP device available");
  if (device_id < 0 || device_id >= count) return dnas::fail(DNAS_E_INVALID, "device_id out of range");
  DNAS_HIP_TRY(hipSetDevice(device_id));
  dnas_model* m = new dnas_model();
  m->device = device_id;
  auto bail = [&](int rc) { dnas_model_destroy(m); return rc; };
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&m->stream3, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&m->ringHead, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->ringTail, hipEventDisableTiming) != hipSuccess)
    return bail(dnas::fail(DNAS_E_DEVICE, "hipStreamCreate failed"));
  const int N = fm->n_states, D = fm->max_dup_len;
  DevModel& d = m->dm;
  d.N = N;
  d.Npad = (N + 31) & ~31;  // 256-byte aligned rows
  d.D = D;
  d.P = fm->n_len;
  d.local = fm->local;
  d.storedLanes = D + 2;
  int rc;
#define UP(field, src, n) if ((rc = upload(m, src, (size_t)(n), &d.field)) != DNAS_OK) return bail(rc)
  UP(einPtr, fm->ein_ptr, N + 1); UP(einSrc, fm->ein_src, fm->n_emit); UP(einScore, fm->ein_score, fm->n_emit);
  UP(einBase, fm->ein_base, fm->n_emit); UP(einIn, fm->ein_in, fm->n_emit);
  UP(ninPtr, fm->nin_ptr, N + 1); UP(ninSrc, fm->nin_src, fm->n_null); UP(ninScore, fm->nin_score, fm->n_null);
  UP(ninIn, fm->nin_in, fm->n_null);
  UP(eoutPtr, fm->eout_ptr, N + 1); UP(eoutDst, fm->eout_dst, fm->n_emit);
  UP(noutPtr, fm->nout_ptr, N + 1); UP(noutDst, fm->nout_dst, fm->n_null);
  UP(mdl, fm->mdl, N); UP(ctx, fm->ctx, (size_t)N * (D ? D : 1));
#undef UP
  d.noGap = fm->no_gap; d.delOpen = fm->del_open; d.delExtend = fm->del_extend; d.delEnd = fm->del_end;
  d.tanDup = fm->tan_dup;
  memcpy(d.sub, fm->sub, sizeof d.sub);
  for (int k = 0; k < kMaxLen; ++k) d.len[k] = k < fm->n_len ? fm->len[k] : 0.;
  d.slotOf = nullptr;
  if (m->dRounds.assign(16).error != hipSuccess) return bail(dnas::fail(DNAS_E_DEVICE, "allocating the 128-byte rounds buffer failed"));
  // ---- tier A: specialise the register/LDS-resident kernel for this machine
  auto uploadEdgeSlots = [&](const int32_t* slotOf) -> int {   // after the tier (and with it the slot map) is known
    std::vector<int32_t> es((size_t)std::max(fm->n_emit, 1)), ns((size_t)std::max(fm->n_null, 1));
    for (int e = 0; e < fm->n_emit; ++e) es[(size_t)e] = slotOf ? slotOf[fm->ein_src[e]] : fm->ein_src[e];
    for (int e = 0; e < fm->n_null; ++e) ns[(size_t)e] = slotOf ? slotOf[fm->nin_src[e]] : fm->nin_src[e];
    int r = upload(m, es.data(), es.size(), &d.einSlot);
    if (r == DNAS_OK) r = upload(m, ns.data(), ns.size(), &d.ninSlot);
    if (r != DNAS_OK) return r;
    // node records (traceback_step.h): only when the machine's edge scores are few enough to be named by a byte
    d.rec = nullptr; d.recScore = nullptr;
    if (D > 4 || getenv("DNAS_NO_NODE_RECORDS")) return DNAS_OK;
    std::vector<double> scores;
    auto scoreIndex = [&](double v) -> int {
      for (size_t i = 0; i < scores.size(); ++i) if (memcmp(&scores[i], &v, sizeof v) == 0) return (int)i;
      if (scores.size() >= 256) return -1;
      scores.push_back(v);
      return (int)scores.size() - 1;
    };
    DevModel h = d;          // the model by host pointers, for the packer
    h.einPtr = fm->ein_ptr;   h.ninPtr = fm->nin_ptr;
    h.einSrc = fm->ein_src;   h.ninSrc = fm->nin_src;
    h.einSlot = es.data();    h.ninSlot = ns.data();
    h.einScore = fm->ein_score; h.ninScore = fm->nin_score;
    h.einIn = fm->ein_in;     h.ninIn = fm->nin_in;
    h.einBase = fm->ein_base;
    h.mdl = fm->mdl; h.ctx = fm->ctx; h.slotOf = slotOf;
    std::vector<NodeRecord> rec((size_t)N);
    for (int j = 0; j < N; ++j)
      if (!NodeRecord::pack(h, j, scoreIndex, rec[(size_t)j])) return DNAS_OK;
    if (scores.empty()) scores.push_back(0.);
    r = upload(m, scores.data(), scores.size(), &d.recScore);
    if (r == DNAS_OK) r = upload(m, reinterpret_cast<const uint32_t*>(rec.data()), rec.size() * 16, &d.rec);
    if (r != DNAS_OK) { d.rec = nullptr; d.recScore = nullptr; }
    return r;
  };
  {
    // DNAS_TIER=A|B|C forces a tier (and makes its failure an error); DNAS_CLUSTER=<G> forces the cluster size
    const char* forceOpt = opt("tier");
    const std::string force = forceOpt ? forceOpt : "";
    const char want = !force.empty() ? (char)(force[0] & ~0x20) : 0;
    int wantG = 0, wantT = 0;
    dnas::PlanChoice want_;               // -1: not said
    bool autotune = false, records = true;
    std::string recordNote = "row program forced by option";
    if (const char* s = opt("cluster")) wantG = atoi(s);
    if (const char* s = opt("threads")) wantT = atoi(s);
    if (const char* s = opt("plan_order")) want_.order = std::max(0, std::min(2, atoi(s)));
    if (const char* s = opt("plan_slack")) want_.slack = std::max(0, std::min(8, atoi(s)));
    if (const char* s = opt("autotune")) autotune = atoi(s) != 0;
    if (const char* s = opt("records")) records = atoi(s) != 0;
    const bool free_ = want_.order < 0 && want_.slack < 0;     // nothing forced: the record decides
    if (want == 'B') {
      m->tierNote = "tier B forced by DNAS_TIER";
    } else {
      std::string whyNotA;
      if (want != 'C' && wantG < 2) {
        const int threadsA = wantT ? wantT : dnas::kTierAThreads;
        dnas::PlanChoice choiceA = want_;
        if (free_ && !records) recordNote = "tuning records off (default row program)";
        if (free_ && records && !follow_plan_record(fm, 1, threadsA, &choiceA, &recordNote) && autotune) {
          // no record for this machine: time the candidates once (if the machine fits one work-group at all)
          if (dnas::buildTierAPlan(*fm, threadsA, choiceA).ok) {
            int rcTune = tune_row_program(fm, device_id, threadsA, arena_bytes, &choiceA);
            if (rcTune != DNAS_OK) return bail(rcTune);
            if (hipSetDevice(device_id) != hipSuccess) return bail(dnas::fail(DNAS_E_DEVICE, "hipSetDevice failed"));
            recordNote = "timed at model creation: order=" + std::to_string(choiceA.order) + " slack=" + std::to_string(choiceA.slack);
          }
        }
        m->plan = dnas::buildTierAPlan(*fm, threadsA, choiceA);
        if (!m->plan.ok) whyNotA = m->plan.whyNot;
      } else {
        m->plan.ok = false;
        whyNotA = "cluster forced";
      }
      if (!m->plan.ok && want != 'A') {
        // (clusters are not timed here -- planning a 258 538-state machine takes seconds per candidate -- but a recorded
        //  verdict is followed: tools/make_tune_records.py times the dealing orders for the bench machines)
        dnas::PlanChoice choiceC = want_;
        if (free_ && !records) recordNote = "tuning records off (default row program)";
        if (free_ && records) (void)follow_plan_record(fm, wantG >= 2 ? wantG : 0, wantT, &choiceC, &recordNote);
        m->plan = dnas::chooseClusterPlan(*fm, wantG, wantT, choiceC);
        if (!m->plan.ok) m->plan.whyNot = "one work-group: " + whyNotA + "; cluster: " + m->plan.whyNot;
      }
      if (!m->plan.ok) {
        m->tierNote = "tier B: " + m->plan.whyNot;
        if (want) return bail(dnas::fail(DNAS_E_UNSUPPORTED, "tier " + force + " was asked for: " + m->plan.whyNot));
      } else {
        try {
          std::string defs = m->plan.defines;
          if (const char* extra = getenv("DNAS_TIERA_DEFS")) {      // diagnostics, e.g. -DDNAS_STAMP; several: separated by ':', ' ' or newlines
            std::string more = extra;
            for (char& c : more) if (c == ':' || c == ' ') c = '\n';
            defs += "\n" + more;
          }
          m->jitDefs = defs;
          const std::vector<char> code = dnas::jitCompile(defs, m->plan.key);
          if (hipModuleLoadData(&m->module, code.data()) != hipSuccess ||
              hipModuleGetFunction(&m->fillA, m->module, "viterbi_fill_tiera") != hipSuccess)
            throw std::runtime_error("hipModuleLoadData/GetFunction failed");
          const dnas::TierAPlan& p = m->plan;
          if (m->dEntTab.assign(p.entTab.size()).error != hipSuccess || m->dMetaTab.assign(p.metaTab.size()).error != hipSuccess ||
              m->dSlotOf.assign(p.slotOf.size()).error != hipSuccess ||
              hipMemcpy(m->dEntTab.get(), p.entTab.data(), p.entTab.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(m->dMetaTab.get(), p.metaTab.data(), p.metaTab.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(m->dSlotOf.get(), p.slotOf.data(), p.slotOf.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("tier A table upload failed (" + std::to_string((p.entTab.size() + p.metaTab.size() + p.slotOf.size()) * 4) + " bytes in three tables)");
          TierAArgs& a = m->argsA;
          a.N = N; a.local = fm->local;
          a.noGap = fm->no_gap; a.delOpen = fm->del_open; a.delExtend = fm->del_extend; a.delEnd = fm->del_end;
          a.tanDup = fm->tan_dup;
          memcpy(a.sub, fm->sub, sizeof a.sub);
          for (int k = 0; k < 8; ++k) a.len[k] = k < fm->n_len ? fm->len[k] : 0.;
          memcpy(a.score, p.score, sizeof a.score);
          d.slotOf = m->dSlotOf.get();
          d.Npad = p.NS;          // lattice row stride = slots
          d.storedLanes = 2;      // tier A keeps S and D in HBM; T lanes are recomputed where needed
          if (p.G == 1) {
            m->tier = 1;
            m->tierNote = "tier A: " + p.key + "; " + recordNote;
          } else {
            // a cluster lives on one XCD (32 CUs): floor(32 / G) clusters per XCD.  Every cluster owns an exchange
            // buffer (3 arrays of G * GROWS * T cells + the end-of-read reduction cells) and a sync block.
            // The members of a cluster wait for each other, so all of them must be resident together: the grid is sized
            // from what the device says it can hold of THIS kernel (one work-group per CU is what the plan aims at; were it
            // none, the launch could never finish).  Work-groups are dispatched in index order and a cluster's members are
            // neighbours in it (groups of 8 clusters), so whatever else holds CUs -- another process, this model's traceback --
            // delays at most the last clusters of a launch until CUs come free; the kernel gives late members time (below).
            int cus = 256, perCu = 0;
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id);
            if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, m->fillA, p.T, p.ldsBytes) != hipSuccess || perCu < 1)
              throw std::runtime_error("the cluster kernel cannot be resident on this device (occupancy " + std::to_string(perCu) + ")");
            const int xcds = std::max(1, cus / 32);
            m->maxClusters = std::max(1, xcds * ((cus / xcds) / p.G));      // one work-group per CU, whole clusters per XCD
            // Whole clusters per XCD leave CUs idle when a cluster is large (21 members: one cluster and 11 idle CUs per XCD).
            // Dealt over the XCDs instead (block b = member b % G of cluster b / G) half as many clusters again fit, and the
            // exchange through memory (write-through stores, the loads find them there) costs 2 %: measured 12 clusters of
            // 21 at 152 ms per read against 8 at 144 -- taken when it buys a quarter more clusters.
            if (const char* s = opt("cluster_spread")) m->clusterSpread = atoi(s) != 0;
            else if ((cus / p.G) * 4 >= m->maxClusters * 5) m->clusterSpread = 1;
            if (m->clusterSpread) m->maxClusters = std::max(1, cus / p.G);
            if (const char* s = opt("max_clusters")) m->maxClusters = std::max(1, atoi(s));
            m->xStride = (size_t)p.exchangeStride();
            // the sync blocks sit in a window of 64 KB more than they need: their place in it is chosen below
            size_t syncOff = kSyncWindow;
            if (m->dXbuf.assign(m->xStride * (size_t)m->maxClusters).error != hipSuccess ||
                m->dSyncBase.assign((size_t)m->maxClusters * 64 + syncOff / sizeof(unsigned)).error != hipSuccess ||
                m->dFoldTab.assign(p.foldTab.size()).error != hipSuccess ||
                hipMemcpy(m->dFoldTab.get(), p.foldTab.data(), p.foldTab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
              throw std::runtime_error("tier C exchange buffer allocation failed (" + std::to_string(m->xStride * (size_t)m->maxClusters * sizeof(double)) + " bytes, and the sync blocks and fold table)");
            // WHERE in the window: the members of a cluster agree on every column through device-scope atomics on their sync block,
            // performed at the memory side -- the round trip from an XCD depends on the memory channel the address belongs to (one
            // read alone on 16 work-groups: 41.6 ms or 54 ms with the block 4 KB apart; a full launch of 64 clusters does not care,
            // its blocks spread over the channels).  sync_latency_kernel times the round trip from every XCD to a candidate
            // every KB; the offset is taken that serves the first clusters of a launch best (cluster c runs on the XCD of block
            // c % 8; the clusters of a spread plan on all of them), the first one -- a single read's -- above all.
            // DNAS_SYNC_OFFSET=<bytes> forces a place (experiments), sync_place=0 takes the start of the window.
            syncOff = 0;
            if (const char* e = getenv("DNAS_SYNC_OFFSET")) syncOff = std::min((size_t)atol(e) & ~(size_t)255, kSyncWindow);
            else if (!(opt("sync_place") && atoi(opt("sync_place")) == 0)) {
              const int nCand = (int)(kSyncWindow / kSyncStep) + 16, reps = 12;    // (the blocks of the first clusters reach past the offset)
              DevBuf<unsigned long long> dLat;
              DevBuf<unsigned> dXcc;
              std::vector<unsigned long long> lat((size_t)8 * nCand, 0ull);
              if (dLat.assign(lat.size()).error == hipSuccess && dXcc.assign(8).error == hipSuccess &&
                  hipMemsetAsync(m->dSyncBase.get(), 0, (size_t)m->maxClusters * 64 * sizeof(unsigned) + kSyncWindow, m->stream) == hipSuccess) {
                const int candAvail = (int)std::min<size_t>((size_t)nCand, ((size_t)m->maxClusters * 64 * sizeof(unsigned) + kSyncWindow) / kSyncStep);
                hipLaunchKernelGGL(sync_latency_kernel, dim3(8), dim3(64), 0, m->stream, m->dSyncBase.get(), candAvail, (int)(kSyncStep / sizeof(unsigned)), reps, dLat.get(), dXcc.get());
                if (hipGetLastError() == hipSuccess &&
                    hipMemcpyAsync(lat.data(), dLat.get(), (size_t)8 * candAvail * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream) == hipSuccess &&
                    hipStreamSynchronize(m->stream) == hipSuccess) {
                  std::vector<unsigned> xcc(8, 0);
                  (void)hipMemcpy(xcc.data(), dXcc.get(), 8 * sizeof(unsigned), hipMemcpyDeviceToHost);
                  m->syncCand = candAvail;
                  m->syncLat.assign((size_t)8 * candAvail, 0.);
                  for (int b = 0; b < 8; ++b)
                    for (int k = 0; k < candAvail; ++k) m->syncLat[(size_t)(xcc[(size_t)b] & 7u) * candAvail + k] = (double)lat[(size_t)b * candAvail + k];
                  syncOff = place_sync_words(m, 0);
                  m->syncPlaceNote = "sync words at +" + std::to_string(syncOff) + " B";
                  if (getenv("DNAS_SYNC_DEBUG")) {
                    fprintf(stderr, "sync debug: calibration blocks ran on XCCs");
                    for (int b = 0; b < 8; ++b) fprintf(stderr, " %u", xcc[(size_t)b]);
                    fprintf(stderr, "; offset %zu; block 0 ticks per candidate:", syncOff);
                    for (int k = 0; k < candAvail; k += 4) fprintf(stderr, " %llu", lat[(size_t)k]);
                    fprintf(stderr, "\n");
                  }
                }
              }
            }
            m->syncOffNow = syncOff;
            m->dSync = m->dSyncBase.get() + syncOff / sizeof(unsigned);
            // watchdog per lattice column.  A column takes tens of microseconds, but the clock keeps running while the device's
            // scheduler lets another queue's kernel run: the limit only has to turn a protocol failure into an error instead
            // of a hung GPU.  (Two cluster launches at once on one card take turns launch by launch; the stalls of 2-6 s once
            // seen beside them were hipMalloc / hipFree of the arenas: tools/alloc_probe.py)
            double seconds = 30.0;
            if (const char* s = opt("cluster_timeout_s")) seconds = std::max(0.001, atof(s));
            m->timeoutTicks = (unsigned long long)(seconds * 1e8);   // s_memrealtime counts at 100 MHz
            double arrive = 120.0;  // ... and for the work-groups of a cluster to have all been started (CUs held by others)
            if (const char* s = opt("cluster_arrive_s")) arrive = std::max(0.001, atof(s));
            m->arriveTicks = (unsigned long long)(arrive * 1e8);
            m->tier = 2;
            m->tierNote = "tier C: " + std::to_string(p.G) + " work-groups per read, " + std::to_string(m->maxClusters) +
                          (m->clusterSpread ? " clusters dealt over the XCDs, exchange edges " : " clusters, exchange edges ") + std::to_string(p.crossEdges) + ", " + p.key + "; " + recordNote +
                          (m->syncPlaceNote.empty() ? "" : "; " + m->syncPlaceNote);
          }
        } catch (const std::exception& e) {
          m->tier = 0;
          m->tierNote = std::string("tier B: tier A/C unavailable: ") + e.what();
          // no silent fallback: a machine the register/LDS kernel can serve is served by it or not at all,
          // unless the caller asked for the fallback explicitly (DNAS_ALLOW_TIER_B_FALLBACK=1)
          if (!getenv("DNAS_ALLOW_TIER_B_FALLBACK")) return bail(dnas::fail(DNAS_E_DEVICE, m->tierNote));
        }
      }
    }
  }
  // the general kernel is compiled for every width: its note says which one this model runs (tiers A and C: D<d> in the key)
  if (m->tier == 0) m->tierNote += " (D" + std::to_string(D) + ")";
  if ((rc = uploadEdgeSlots(m->tier >= 1 ? m->plan.slotOf.data() : nullptr)) != DNAS_OK) return bail(rc);
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return bail(dnas::fail(DNAS_E_DEVICE, "hipMemGetInfo failed"));
  m->arenaCap = arena_bytes ? arena_bytes : (size_t)((double)freeB * 0.6);
  m->arenaGiven = arena_bytes != 0;
  if (m->tier == 1) {
    // A tier-A work-group owns a whole CU (all of its vector registers and nearly all of its LDS), so
    // a launch runs in rounds of one read per CU -- per XCD: work-groups are dealt round-robin to the
    // XCDs (32 CUs each), and an XCD that gets one work-group more than rounds x its free CUs adds a
    // whole round to the launch.  The traceback of the previous batch runs beside the fill (blocks of
    // 512 reads, one CU each), and a round with a few CUs of an XCD idle is faster than a full one
    // (the XCD's 4 MB L2 holds the S history of ~17 work-groups).  Measured on MI355X with the bench
    // workload: three rounds of 30 work-groups per XCD (720 reads) per launch, 48.8 ms, is the best
    // point; 2 x 255 = 510 reads cost 48 ms (a third round on the traceback's XCD), 500 reads 37 ms.
    // (Round 2 measured persistent work-groups that pull reads from a queue: a round takes 16.0-16.4 ms for any number
    // from 208 to 240 and 18 ms at 248, with or without the queue -- 3 x 240 stays the best point; the queue is gone.)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 1) {
      const int xcds = std::max(1, cus / 32);
      m->maxSlots = std::max(1, 3 * (cus - 2 * xcds));
      // A small row program is compiled so that two work-groups share a CU (plan.cpp, wavesPerSimd): what the device says it holds
      // of this kernel decides, and a launch is then ONE round of two reads per CU (measured on water64.1*l4c4, ~1050-nt reads:
      // 480 reads per launch 0.565 of the roofline, 448: 0.53, 512: 0.51; one work-group per CU, 695 per launch: 0.41)
      int perCu = 1;
      if (m->plan.wavesPerSimd && hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, m->fillA, m->plan.T, m->plan.ldsBytes) == hipSuccess && perCu >= 2) {
        m->maxSlots = std::max(1, 2 * (cus - 2 * xcds));
        m->tierNote += "; 2 work-groups per CU";
      }
    }
  }
  if (m->tier == 2) m->maxSlots = 1 << 20;   // persistent clusters walk any number of reads: a launch is bounded by the arena only
  if (const char* s = opt("max_slots")) m->maxSlots = std::max(1, atoi(s));
  if (const char* s = opt("fill_overlap")) m->fillOverlap = std::max(0, std::min(2, atoi(s)));
  if (const char* s = opt("traceback")) m->waveTraceback = !(s[0] == 't' || s[0] == 'T');
  if (const char* s = opt("tb_threads")) m->tbThreads = std::max(64, std::min(256, atoi(s) / 64 * 64));
  if (const char* s = opt("tb_lanes")) m->tbLanes = std::max(1, std::min(64, atoi(s)));
  if (const char* s = opt("checkpoint")) m->checkpointMode = (s[0] == 'a' && s[1] == 'l') ? 1 : (s[0] == 'n' ? 2 : 0);   // auto | always | never
  if (const char* s = opt("segment")) m->segmentCols = std::max(0, atoi(s));
  if (const char* s = opt("arena_fraction")) {
    const double f = atof(s);
    if (f > 0.05 && f < 0.95 && !arena_bytes) m->arenaCap = (size_t)((double)freeB * f);
  }
  *out = m;
  return DNAS_OK;
}

extern "C" void dnas_model_destroy(dnas_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->stream2) (void)hipStreamSynchronize(m->stream2);
  if (m->stream3) (void)hipStreamSynchronize(m->stream3);   // (`stream` waited for its tail: drained already)
  for (hipEvent_t e : m->sync) (void)hipEventDestroy(e);
  if (m->ringHead) (void)hipEventDestroy(m->ringHead);
  if (m->ringTail) (void)hipEventDestroy(m->ringTail);
  if (m->stream2) (void)hipStreamDestroy(m->stream2);
  if (m->stream3) (void)hipStreamDestroy(m->stream3);
  if (m->module) (void)hipModuleUnload(m->module);
  if (m->moduleSeg) (void)hipModuleUnload(m->moduleSeg);
  for (hipEvent_t e : m->events) (void)hipEventDestroy(e);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;                      // the device and pinned memory: every owner frees its own, this device current
}

extern "C" int dnas_model_sync(dnas_model* m) {
  if (!m) return dnas::fail(DNAS_E_INVALID, "null model");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  return collect_stats(m);
}

extern "C" int dnas_model_device(const dnas_model* m) { return m ? m->device : -1; }

extern "C" int dnas_model_last_stats(const dnas_model* m, dnas_batch_stats* out) {
  if (!m || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  if (m->statsPending) return dnas::fail(DNAS_E_INVALID, "call dnas_model_sync first");
  *out = m->stats;
  return DNAS_OK;
}

extern "C" int dnas_model_last_arena_slices(const dnas_model* m, int64_t* out) {
  if (!m || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  if (m->statsPending) return dnas::fail(DNAS_E_INVALID, "call dnas_model_sync first");
  *out = m->lastSlices;
  return DNAS_OK;
}

namespace {

// ---- one call of dnas_viterbi_batch_device, planned on the host -----------------------------------------------------------
// Bounded-memory decode (the reference holds every read's whole lattice, viterbi.h:48-50): the reads whose lattice does not
// fit half the arena -- the longest, first in sorted order -- are decoded in groups, in segments of C columns:
//   pass 1  fill segment after segment into a work buffer of H + C + 1 columns per read, keeping of every segment only its
//           last H columns and the hand-over lane (what the fill of the next segment and a traceback step look back at)
//   pass 2  from the last segment to the first: restore the checkpoint in front of the segment, fill it again (the last one
//           is still there), and let the traceback walk it; a walk that leaves the segment is parked until the next launch
// Fill work doubles; memory per read drops from L + 1 columns to about 2 sqrt((L + 1)(H + 1)).
struct SegmentGroup {
  int64_t first, n;          // reads [first, first + n) of the sorted order
  int64_t C, nSeg;           // columns per segment, segments of the longest read
  size_t workStride, ckStride;   // doubles per read: work buffer (H + C + 1 columns + a spare cell), checkpoint store
  size_t tabAt;              // where the group's per-segment tables start (entries of n reads per segment)
};
struct CallPlan {
  std::vector<int32_t> order;        // reads, longest first
  std::vector<uint64_t> slotOff;     // lattice of read i of the sorted order inside its arena half (or slice of the ring)
  std::vector<int64_t> batchStart;   // whole-lattice batches: first read of each, + n_reads
  std::vector<SegmentGroup> groups;  // reads [0, nSegmented) in groups
  int64_t nSegmented = 0, columns = 0, segColumns = 0;   // columns: sum of L + 1 over the reads; segColumns: over [0, nSegmented)
  size_t peak = 0;                   // doubles of the largest batch
  int slices = 1;                    // batches whose lattices lie side by side: 1, 2 halves in turn, or a ring of kRingSlices
  size_t groupPeak = 0, tabEntries = 0, groupLaunches = 0;
};

// pairs > 0 (both-strand decode): n_reads = 2 * pairs virtual reads behind an offset table of 2 * pairs + 2 entries -- caller
// read i as written is virtual read i, its reverse complement virtual read pairs + 1 + i.  The two are neighbours in the
// sorted order (the CALLER's reads are sorted, then each expands into its pair: sorting the virtual reads would separate pairs of
// equal length) and no cut -- batch, arena half, round of clusters, bounded-memory group -- falls between them: `unit` below.
int plan_call(const dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, CallPlan* cp, int64_t pairs = 0) {
  const DevModel& d = m->dm;
  const size_t colDoubles = (size_t)d.storedLanes * (size_t)d.Npad;
  const int64_t unit = pairs > 0 ? 2 : 1;
  // longest reads first: a batch's work-groups then finish together
  cp->order.resize((size_t)(pairs > 0 ? pairs : n_reads));
  std::iota(cp->order.begin(), cp->order.end(), 0);
  std::stable_sort(cp->order.begin(), cp->order.end(), [&](int32_t a, int32_t b) {
    return read_offsets[a + 1] - read_offsets[a] > read_offsets[b + 1] - read_offsets[b];
  });
  if (pairs > 0) {
    std::vector<int32_t> both((size_t)n_reads);
    for (int64_t i = 0; i < pairs; ++i) { both[2 * (size_t)i] = cp->order[(size_t)i]; both[2 * (size_t)i + 1] = (int32_t)(pairs + 1) + cp->order[(size_t)i]; }
    cp->order.swap(both);
  }
  auto lenOf = [&](int64_t i) { return (int64_t)(read_offsets[cp->order[(size_t)i] + 1] - read_offsets[cp->order[(size_t)i]]); };
  for (int64_t i = 0; i < n_reads; ++i)
    if (lenOf(i) > 0x7ffffff0ll) return dnas::fail(DNAS_E_UNSUPPORTED, "read too long");
  // two arena halves: batch i fills half (i & 1) while the traceback of batch i-1 still reads the other
  const size_t arenaCapDoubles = m->arenaCap / sizeof(double) / 2;

  // ---- the reads that go through segments, and their groups
  const size_t H = (size_t)d.D + 1;
  int64_t nSeg = 0;
  if (m->checkpointMode == 1) nSeg = n_reads;
  else if (m->checkpointMode == 0)
    while (nSeg < n_reads && (size_t)unit * (colDoubles * (size_t)(lenOf(nSeg) + 1) + 8) > arenaCapDoubles) ++nSeg;
  cp->nSegmented = nSeg;
  const size_t budget = m->arenaCap / sizeof(double);
  // (pairs: whole pairs per group -- an odd number of clusters leaves one idle rather than split a pair; one cluster walks both)
  const int64_t groupMax = std::max<int64_t>(unit, (m->tier == 2 ? m->maxClusters : m->maxSlots) / unit * unit);
  for (int64_t g0 = 0; g0 < nSeg;) {
    const int64_t Lmax = lenOf(g0);
    int64_t nG = std::min(nSeg - g0, groupMax), C = 0;
    auto perRead = [&](int64_t c) {
      return (H + (size_t)c + 1) * colDoubles + 8 + (size_t)(Lmax / c + 1) * (H + 1) * colDoubles;
    };
    const int64_t cMin = (int64_t)H + 1;
    for (;;) {
      const size_t per = budget / (size_t)nG;
      if (m->segmentCols > 0) {
        C = std::max<int64_t>(cMin, m->segmentCols);
        if (perRead(C) <= per) break;
      } else {
        C = std::max<int64_t>(cMin, (int64_t)std::ceil(std::sqrt((double)(Lmax + 1) * (double)(H + 1))));
        if (perRead(C) <= per) {
          while (C < Lmax + 1 && perRead(std::min(2 * C, Lmax + 1)) <= per) C = std::min(2 * C, Lmax + 1);
          break;
        }
      }
      if (nG == unit)
        return dnas::fail(DNAS_E_NOMEM, "a read of " + std::to_string(Lmax) + " bases needs " + std::to_string(perRead(C) * 8 * (size_t)unit) +
                                            " bytes of lattice segments and checkpoints; the lattice arena has " + std::to_string(m->arenaCap));
      nG = (nG / unit + 1) / 2 * unit;
    }
    SegmentGroup g{g0, nG, C, Lmax / C + 1, (H + (size_t)C + 1) * colDoubles + 8, (size_t)(Lmax / C + 1) * (H + 1) * colDoubles, cp->tabEntries};
    cp->groupPeak = std::max(cp->groupPeak, (size_t)nG * (g.workStride + g.ckStride));
    cp->tabEntries += (size_t)g.nSeg * (size_t)nG;
    cp->groupLaunches += 2 * (size_t)g.nSeg;
    cp->groups.push_back(g);
    g0 += nG;
  }

  // ---- the other reads, in whole-lattice batches
  for (int64_t i = 0; i < nSeg; ++i) cp->columns += lenOf(i) + 1;
  cp->segColumns = cp->columns;
  // one work-group per read: equal batches rather than full ones and a remainder.  A launch that has the chip to itself costs
  // whole rounds of work-groups, and the CUs its last round leaves free idle until the next launch.  (Where the fills of a call
  // overlap -- the ring below -- the next batch's work-groups take those CUs and only the call as a whole pays for a last round:
  // the size of a batch then matters little, and the arena may cut it.)
  const int64_t nPlain = n_reads - nSeg;
  const int64_t nFull = std::max<int64_t>(1, (nPlain + m->maxSlots - 1) / m->maxSlots);
  int64_t perBatch = (nPlain + nFull - 1) / nFull;
  // clusters: a launch runs whole rounds of maxClusters reads -- a batch that the arena cuts at 14 reads on 12 clusters would
  // take two rounds for 14; it is cut at 12, and the other two open the next batch
  int64_t round = m->tier == 2 ? std::max(1, m->maxClusters) : 1;
  if (unit > 1) {                      // whole pairs: an odd round of clusters is cut at every second one
    perBatch = (perBatch + unit - 1) / unit * unit;
    if (perBatch > m->maxSlots && perBatch > unit) perBatch -= unit;
    if (round > 1 && round % unit) round *= unit;
  }
  if (round > 1 && perBatch > round) perBatch = (perBatch + round - 1) / round * round;
  auto needOf = [&](int64_t i) { return colDoubles * (size_t)((uint64_t)lenOf(i) + 1) + 8; };   // + a spare cell (tier A, local mode: S(N-1, L) before its overwrite)
  // the cut, with `arenaCapDoubles` for the lattices of a batch
  auto cutBatches = [&](const size_t arenaCapDoubles) -> int {
  cp->slotOff.assign((size_t)n_reads, 0);
  cp->batchStart.assign(1, nSeg);
  cp->peak = 0;
  cp->columns = cp->segColumns;
  size_t used = 0;
  for (int64_t i = nSeg; i < n_reads; ++i) {
    const uint64_t L = (uint64_t)lenOf(i);
    const size_t need = needOf(i);
    if (need > arenaCapDoubles)
      return dnas::fail(DNAS_E_NOMEM, "a single read's lattice (" + std::to_string(need * 8) +
                                          " bytes) exceeds the lattice arena (" + std::to_string(m->arenaCap) + ") and checkpoint=never");
    if (unit > 1 && unit * need > arenaCapDoubles)
      return dnas::fail(DNAS_E_NOMEM, "the lattices of a read and of its reverse complement (" + std::to_string(unit * need * 8) +
                                          " bytes) exceed the lattice arena (" + std::to_string(m->arenaCap) + ") and checkpoint=never");
    // (pairs: a cut is considered in front of a pair only, with the room both of its lattices take -- they are equally long)
    if ((i - nSeg) % unit == 0 && (i - cp->batchStart.back() >= perBatch || used + unit * need > arenaCapDoubles)) {
      const int64_t start = cp->batchStart.back(), count = i - start;
      const int64_t cut = (round > 1 && count > round && count % round) ? start + count / round * round : i;
      cp->batchStart.push_back(cut);
      used = 0;
      for (int64_t t = cut; t < i; ++t) { cp->slotOff[(size_t)t] = used; used += needOf(t); }   // the reads that moved on
    }
    cp->slotOff[(size_t)i] = used;
    used += need;
    cp->peak = std::max(cp->peak, used);
    cp->columns += (int64_t)L + 1;
  }
  if (nPlain > 0) cp->batchStart.push_back(n_reads);
  return DNAS_OK;
  };
  int rc = cutBatches(arenaCapDoubles);
  if (rc != DNAS_OK) return rc;
  const size_t nBatches = cp->batchStart.size() - 1;
  cp->slices = nBatches > 1 ? 2 : 1;
  // ---- tier A: a ring of kRingSlices arena slices instead of the two halves, so that two fills can be in flight while a third
  // batch is traced back (viterbi_call).  Used from kRingSlices batches on, when (a) that many slices of the cut above fit the
  // arena: the cut stays -- or (b) they do not, and the arena is the library's own choice (or fill_overlap=2 says to): the
  // batches are cut again with a slice of the arena as the cap and no more reads each than before.  An arena the caller sized --
  // for two batches, say -- is otherwise served as it always was, and so is a call whose longest whole-lattice read (pair of
  // reads) does not fit a slice.
  if (m->tier == 1 && m->fillOverlap > 0 && nBatches >= (size_t)kRingSlices) {
    const size_t sliceCapDoubles = m->arenaCap / sizeof(double) / (size_t)kRingSlices;
    if (cp->peak <= sliceCapDoubles) {
      cp->slices = kRingSlices;
    } else if ((!m->arenaGiven || m->fillOverlap == 2) && (size_t)unit * needOf(nSeg) <= sliceCapDoubles) {
      if ((rc = cutBatches(sliceCapDoubles)) != DNAS_OK) return rc;
      cp->slices = kRingSlices;
    }
  }
  return DNAS_OK;
}

// the kernels index their substitution tables with the base codes: anything but 0..3 must not reach them
int check_device_bases(dnas_model* m, const uint8_t* d_bases, size_t nBases) {
  if (!nBases) return DNAS_OK;
  DNAS_HIP_TRY(hipMemsetAsync(m->dRounds.get() + 8, 0, sizeof(unsigned long long), m->stream));
  hipLaunchKernelGGL(check_bases_kernel, dim3((unsigned)std::min<size_t>((nBases + 255) / 256, 4096)), dim3(256), 0, m->stream,
                     d_bases, nBases, m->dRounds.get() + 8);
  DNAS_HIP_TRY(hipGetLastError());
  unsigned long long bad = 0;
  DNAS_HIP_TRY(hipMemcpyAsync(&bad, m->dRounds.get() + 8, sizeof bad, hipMemcpyDeviceToHost, m->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  if (bad) return dnas::fail(DNAS_E_BAD_BASE, "base code > 3 in the device buffer (bases are 0..3 = ACGT)");
  return DNAS_OK;
}

// One fill launch over nB reads (their indices at batchRead, their lattices at arena + slots[.]) on stream `st`, one of the
// model's fill streams; colRange: the columns to fill per read (segments), or null for whole reads.
// Launches of one tier-A model may run side by side (the ring of viterbi_call) once their lattices are apart: the launch
// keeps no scratch of its own -- the argument block goes by value, the tables are read only, every read writes its own lattice
// and log-likelihood, and word 0 of dRounds is only added to atomically (words 1-7 are stamps of a diagnostic build: whichever
// launch wrote them last).  Tiers B and C do keep per-launch state (dXbuf, dSync, syncCheck): their launches stay on one stream.
struct FillLauncher {
  dnas_model* m;
  const uint8_t* d_bases;
  double* d_out_loglike;
  size_t syncAt = 0, launches = 0;

  int operator()(hipStream_t st, const int32_t* batchRead, const uint64_t* slots, int nB, const int* colRange) {
    ++launches;
    RoctxRange fillRange(m->tier == 2 ? "viterbi fill (tier C)" : (m->tier == 1 ? "viterbi fill (tier A)" : "viterbi fill (tier B)"));
    if (m->tier == 0) {
      const int maskWords = (m->dm.N + 31) / 32 + 1;
      hipLaunchKernelGGL(viterbi_fill_kernel, dim3(nB), dim3(kFillThreads), 2 * (size_t)maskWords * sizeof(unsigned), st, m->dm, d_bases,
                         (const uint64_t*)m->dReadOff.get(), batchRead, slots, m->arena.get(), d_out_loglike, m->dRounds.get(), maskWords, colRange);
      DNAS_HIP_TRY(hipGetLastError());
      return DNAS_OK;
    }
    TierALaunch la{m->argsA, m->dEntTab.get(), m->dMetaTab.get(), d_bases, m->dReadOff.get(), batchRead, slots,
                   m->arena.get(), d_out_loglike, m->dRounds.get(), nullptr, nullptr, nullptr, 0, nB, 0ull, 0ull, colRange, m->clusterSpread};
    unsigned grid = (unsigned)nB;
    int nClusters = 0;
    if (m->tier == 2) {
      // a cluster of G work-groups per read, persistent over the reads of the launch.  Blocks b and b + 8 share
      // an XCD (observed dispatch order; the kernel is correct under any placement): the members of a cluster are
      // 8 blocks apart, cluster = (b / 8 / G) * 8 + b % 8.
      const int G = m->plan.G;
      nClusters = std::min(nB, m->maxClusters);
      la.xbuf = m->dXbuf.get(); la.syncWords = m->dSync; la.foldTab = m->dFoldTab.get(); la.nClusters = nClusters; la.timeoutTicks = m->timeoutTicks; la.arriveTicks = m->arriveTicks;
      grid = m->clusterSpread ? (unsigned)(G * nClusters) : (unsigned)(8 * G * ((nClusters + 7) / 8));
      const size_t nX = m->xStride * (size_t)nClusters;
      hipLaunchKernelGGL(fill_neginf_kernel, dim3((unsigned)((nX + 255) / 256)), dim3(256), 0, st, m->dXbuf.get(), nX);
      DNAS_HIP_TRY(hipGetLastError());
      if (!m->syncLat.empty() && !m->clusterSpread && nClusters <= 8) {
        // A launch of a few clusters -- one read alone -- is a latency matter, and which XCD its first block goes to is not fixed:
        // the dispatcher deals the work-groups of successive kernels round the XCDs in one sequence.  A one-block probe says where
        // that sequence stands right now (the fill is the next kernel: its block 0 goes where the probe's one block went -- observed
        // over and over, `DNAS_SYNC_DEBUG=1` prints both), and the
        // sync blocks move to the place in their window that this XCD reaches soonest.  Speed only: a wrong guess costs what a
        // badly placed block costs, 42 against 54 ms for a ~980-nt read of the 46 670-state machine on 16 work-groups.
        DNAS_HIP_TRY(m->xccProbe.reserve(1, 1));
        DNAS_HIP_TRY(hipMemsetAsync(m->dSyncBase.get(), 0, (size_t)m->maxClusters * 64 * sizeof(unsigned) + kSyncWindow, st));
        *m->xccProbe.get() = 0xffu;
        hipLaunchKernelGGL(xcc_probe_kernel, dim3(1), dim3(64), 0, st, m->xccProbe.get());
        DNAS_HIP_TRY(hipGetLastError());
        DNAS_HIP_TRY(hipStreamSynchronize(st));
        if (*m->xccProbe.get() < 8u) {
          m->syncOffNow = place_sync_words(m, *m->xccProbe.get() & 7u);
          m->dSync = m->dSyncBase.get() + m->syncOffNow / sizeof(unsigned);
          la.syncWords = m->dSync;
          if (getenv("DNAS_SYNC_DEBUG")) fprintf(stderr, "sync debug: probe on XCC %u, sync words at +%zu\n", *m->xccProbe.get(), m->syncOffNow);
        }
      } else {
        DNAS_HIP_TRY(hipMemsetAsync(m->dSync, 0, (size_t)nClusters * 64 * sizeof(unsigned), st));
      }
    }
    size_t laSize = sizeof la;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &la, HIP_LAUNCH_PARAM_BUFFER_SIZE, &laSize, HIP_LAUNCH_PARAM_END};
    DNAS_HIP_TRY(hipModuleLaunchKernel(colRange ? m->fillSeg : m->fillA, grid, 1, 1, (unsigned)m->plan.T, 1, 1, (unsigned)m->plan.ldsBytes,
                                  st, nullptr, config));
    if (m->tier == 2) {
      // the watchdog words of this launch: [1] of every sync block (checked in dnas_model_sync)
      DNAS_HIP_TRY(hipMemcpyAsync(m->syncCheck.get() + syncAt * (size_t)m->maxClusters * 64, m->dSync,
                             (size_t)nClusters * 64 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      ++syncAt;
    }
    return DNAS_OK;
  }
};

// the register/LDS kernel built with -DDNAS_SEGMENTS=1, compiled when a call first needs it
int ensure_segment_kernel(dnas_model* m) {
  if (m->tier == 0 || m->fillSeg) return DNAS_OK;
  try {
    const std::vector<char> code = dnas::jitCompile(m->jitDefs + "\n-DDNAS_SEGMENTS=1", m->plan.key + "+segments");
    if (hipModuleLoadData(&m->moduleSeg, code.data()) != hipSuccess ||
        hipModuleGetFunction(&m->fillSeg, m->moduleSeg, "viterbi_fill_tiera") != hipSuccess)
      throw std::runtime_error("hipModuleLoadData/GetFunction failed");
  } catch (const std::exception& e) {
    m->fillSeg = nullptr;
    return dnas::fail(DNAS_E_DEVICE, std::string("bounded-memory decode: the segment kernel is unavailable: ") + e.what());
  }
  return DNAS_OK;
}

// A DNAS_STRAND_BOTH call: the caller's arrays -- fill and traceback write per virtual read into the model's own.
struct StrandCall {
  int64_t n;                  // the caller's reads; virtual read n + 1 + i is the reverse complement of read i
  double* outLoglike; uint8_t* outStrand; uint32_t* outLen; uint8_t* outStatus;
  int64_t tracebacks = 0;     // reads a traceback kernel was launched over
};

// After the fill of nPairs pairs (batchRead[2k], batchRead[2k + 1]; first = their place in the sorted order), on its stream:
// the winners.
int pick_strands(dnas_model* m, hipStream_t st, const StrandCall& sc, int64_t first, int nPairs, const uint64_t* pairSlot, bool rows) {
  hipLaunchKernelGGL(strand_pick_kernel, dim3((unsigned)((nPairs + 255) / 256)), dim3(256), 0, st,
                     (const int32_t*)(m->dBatchRead.get() + first), pairSlot, nPairs, (const double*)m->sLL.get(), sc.outLoglike, sc.outStrand,
                     m->sWinRead.get() + first / 2, m->sWinSlot.get() + first / 2, rows ? m->sWinRow.get() + first / 2 : (int32_t*)nullptr, m->dRounds.get() + 12);
  DNAS_HIP_TRY(hipGetLastError());
  return DNAS_OK;
}
// After their traceback: length, status and event count from the winner's virtual read to the caller's read.
int gather_winners(dnas_model* m, const StrandCall& sc, int64_t first, int nWin, hipStream_t stream) {
  hipLaunchKernelGGL(strand_gather_kernel, dim3((unsigned)((nWin + 255) / 256)), dim3(256), 0, stream, (const int32_t*)(m->sWinRead.get() + first / 2),
                     nWin, (int)(sc.n + 1), (const uint32_t*)m->sLen.get(), (const uint8_t*)m->sSt.get(), sc.outLen, sc.outStatus, m->dEvLen.get());
  DNAS_HIP_TRY(hipGetLastError());
  return DNAS_OK;
}

// The groups of the bounded-memory decode, everything in order on the fill stream.  events: 4 per group (pass 1, pass 2).
// sc (both-strand decode): pass 1 runs over the group's pairs, the strands are picked between the passes, and pass 2 -- the
// second fill of every segment and the resumable traceback -- runs over the winners only: their rows of the group's tables
// (strand_rows_kernel), their checkpoints (strand_copy_rows_kernel), walks[] per winner.
int run_segment_groups(dnas_model* m, const CallPlan& cp, const uint64_t* read_offsets, FillLauncher& fill, const uint8_t* d_bases,
                       char* d_out_sym, uint32_t* d_out_len, uint8_t* d_out_status, StrandCall* sc = nullptr) {
  const DevModel& d = m->dm;
  const size_t colDoubles = (size_t)d.storedLanes * (size_t)d.Npad, H = (size_t)d.D + 1;
  auto lenOf = [&](int64_t i) { return (int64_t)(read_offsets[cp.order[(size_t)i] + 1] - read_offsets[cp.order[(size_t)i]]); };
  // per group and segment: the column range and the (virtual) lattice origin of every read
  std::vector<int> ranges(2 * cp.tabEntries);
  std::vector<uint64_t> segSlot(cp.tabEntries);
  for (const SegmentGroup& g : cp.groups)
    for (int64_t sg = 0; sg < g.nSeg; ++sg)
      for (int64_t j = 0; j < g.n; ++j) {
        const size_t at = g.tabAt + (size_t)sg * (size_t)g.n + (size_t)j;
        const int64_t L = lenOf(g.first + j), c0 = sg * g.C;
        ranges[2 * at] = (int)c0;
        ranges[2 * at + 1] = (int)std::min(L, c0 + g.C - 1);
        // column c of the segment sits at work(j) + (c - c0 + H) columns: the origin the kernels add c * column to
        segSlot[at] = (uint64_t)((size_t)j * g.workStride + H * colDoubles) - (uint64_t)((size_t)c0 * colDoubles);
      }
  m->dColRange.reset(); m->dSegSlot.reset(); m->dWalks.reset();
  DNAS_HIP_TRY(m->dColRange.assign(ranges.size()));
  DNAS_HIP_TRY(m->dSegSlot.assign(segSlot.size()));
  DNAS_HIP_TRY(m->dWalks.assign((size_t)cp.nSegmented));
  DNAS_HIP_TRY(hipMemcpy(m->dColRange.get(), ranges.data(), ranges.size() * sizeof(int), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemcpy(m->dSegSlot.get(), segSlot.data(), segSlot.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemset(m->dWalks.get(), 0, (size_t)cp.nSegmented * sizeof(TracebackWalk)));
  const int64_t unit = sc ? 2 : 1;
  if (sc) {
    // the winners' column ranges are those of their pair (row 2k of the group); their lattice origins are picked on the device
    std::vector<int> winRanges(cp.tabEntries);
    for (const SegmentGroup& g : cp.groups)
      for (int64_t sg = 0; sg < g.nSeg; ++sg)
        for (int64_t k = 0; k < g.n / 2; ++k) {
          const size_t at = g.tabAt + (size_t)sg * (size_t)g.n + 2 * (size_t)k, atW = g.tabAt / 2 + (size_t)sg * (size_t)(g.n / 2) + (size_t)k;
          winRanges[2 * atW] = ranges[2 * at];
          winRanges[2 * atW + 1] = ranges[2 * at + 1];
        }
    DNAS_HIP_TRY(m->dWinSegSlot.reserve(cp.tabEntries / 2, dnas::growQuarter256(cp.tabEntries / 2)));
    DNAS_HIP_TRY(m->dWinColRange.reserve(cp.tabEntries, dnas::growQuarter256(cp.tabEntries)));
    DNAS_HIP_TRY(hipMemcpy(m->dWinColRange.get(), winRanges.data(), winRanges.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  const size_t headDoubles = (H + 1) * colDoubles;
  for (size_t gi = 0; gi < cp.groups.size(); ++gi) {
    const SegmentGroup& g = cp.groups[gi];
    RoctxRange groupRange("viterbi bounded-memory group");
    double* const work = m->arena.get();
    double* const ckpt = m->arena.get() + (size_t)g.n * g.workStride;
    // reads of the group that reach segment sg (sorted longest first: a prefix)
    auto reach = [&](int64_t sg) {
      int64_t k = 0;
      while (k < g.n && lenOf(g.first + k) >= sg * g.C) ++k;
      return (int)k;
    };
    auto copyRows = [&](double* dst, size_t dstStride, const double* src, size_t srcStride, int rows) -> int {
      hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)std::min<size_t>((headDoubles + 255) / 256, 256), (unsigned)rows), dim3(256), 0,
                         m->stream, dst, src, dstStride, srcStride, headDoubles);
      DNAS_HIP_TRY(hipGetLastError());
      return DNAS_OK;
    };
    int rc;
    DNAS_HIP_TRY(hipEventRecord(m->events[4 * gi], m->stream));
    for (int64_t sg = 0; sg < g.nSeg; ++sg) {            // pass 1
      const int nAct = reach(sg);
      if (nAct == 0) break;
      if (sg > 0) {
        // the last H columns of the segment before and the hand-over lane behind them: kept, and moved to the front
        if ((rc = copyRows(ckpt + (size_t)sg * headDoubles, g.ckStride, work + (size_t)g.C * colDoubles, g.workStride, nAct)) != DNAS_OK) return rc;
        if ((rc = copyRows(work, g.workStride, ckpt + (size_t)sg * headDoubles, g.ckStride, nAct)) != DNAS_OK) return rc;
      }
      const size_t at = g.tabAt + (size_t)sg * (size_t)g.n;
      if ((rc = fill(m->stream, m->dBatchRead.get() + g.first, m->dSegSlot.get() + at, nAct, m->dColRange.get() + 2 * at)) != DNAS_OK) return rc;
    }
    DNAS_HIP_TRY(hipEventRecord(m->events[4 * gi + 1], m->stream));
    // pass 2 walks a list of reads with their per-segment tables: the group's own, or -- both-strand decode -- the winners'
    const int nList = (int)(g.n / unit);
    const int32_t* listRead = m->dBatchRead.get() + g.first;
    const uint64_t* listSlot = m->dSegSlot.get() + g.tabAt;
    const int* listRange = m->dColRange.get() + 2 * g.tabAt;
    TracebackWalk* listWalk = m->dWalks.get() + g.first;
    if (sc) {
      if ((rc = pick_strands(m, m->stream, *sc, g.first, nList, nullptr, true)) != DNAS_OK) return rc;
      for (int64_t s0 = 0; s0 < g.nSeg; s0 += 65535) {       // (a grid's second dimension holds 65 535 segments)
        hipLaunchKernelGGL(strand_rows_kernel, dim3((unsigned)((nList + 255) / 256), (unsigned)std::min<int64_t>(g.nSeg - s0, 65535)), dim3(256), 0, m->stream,
                           (const uint64_t*)(m->dSegSlot.get() + g.tabAt + (size_t)s0 * (size_t)g.n), (int)g.n, (const int32_t*)(m->sWinRow.get() + g.first / 2), nList,
                           m->dWinSegSlot.get() + g.tabAt / 2 + (size_t)s0 * (size_t)nList);
        DNAS_HIP_TRY(hipGetLastError());
      }
      listRead = m->sWinRead.get() + g.first / 2; listSlot = m->dWinSegSlot.get() + g.tabAt / 2; listRange = m->dWinColRange.get() + g.tabAt;
      listWalk = m->dWalks.get() + g.first / 2;
      sc->tracebacks += nList;
    }
    DNAS_HIP_TRY(hipEventRecord(m->events[4 * gi + 2], m->stream));
    for (int64_t sg = g.nSeg - 1; sg >= 0; --sg) {        // pass 2
      const int nAct = reach(sg) / (int)unit, nAgain = sg + 1 < g.nSeg ? reach(sg + 1) / (int)unit : 0;
      if (nAct == 0) continue;
      const size_t at = (size_t)sg * (size_t)nList;
      if (nAgain > 0) {
        if (sg > 0 && !sc && (rc = copyRows(work, g.workStride, ckpt + (size_t)sg * headDoubles, g.ckStride, nAgain)) != DNAS_OK) return rc;
        if (sg > 0 && sc) {
          hipLaunchKernelGGL(strand_copy_rows_kernel, dim3((unsigned)std::min<size_t>((headDoubles + 255) / 256, 256), (unsigned)nAgain), dim3(256), 0,
                             m->stream, work, (const double*)(ckpt + (size_t)sg * headDoubles), g.workStride, g.ckStride, headDoubles,
                             (const int32_t*)(m->sWinRow.get() + g.first / 2));
          DNAS_HIP_TRY(hipGetLastError());
        }
        if ((rc = fill(m->stream, listRead, listSlot + at, nAgain, listRange + 2 * at)) != DNAS_OK) return rc;
      }
      hipLaunchKernelGGL(viterbi_traceback_wave_kernel, dim3((nAct + 3) / 4), dim3(256), 0, m->stream, d, d_bases,
                         (const uint64_t*)m->dReadOff.get(), listRead, listSlot + at,
                         (const double*)m->arena.get(), d_out_sym, (const uint64_t*)m->dOutOff.get(), d_out_len, d_out_status, nAct, m->dEvents.get(),
                         (const uint64_t*)m->dEvOff.get(), m->dEvLen.get(), listRange + 2 * at, listWalk);
      DNAS_HIP_TRY(hipGetLastError());
    }
    if (sc && (rc = gather_winners(m, *sc, g.first, nList, m->stream)) != DNAS_OK) return rc;
    DNAS_HIP_TRY(hipEventRecord(m->events[4 * gi + 3], m->stream));
  }
  return DNAS_OK;
}

// The n reads at src, bounded by off[0] = 0 .. off[n] (host; dOff: the same words on the device), reverse-complemented read by
// read into rcDst and copied into fwdDst, if given.  On the fill stream.
int launch_revcomp(dnas_model* m, int64_t n, const uint64_t* off, const uint64_t* dOff, const uint8_t* src, uint8_t* fwdDst, uint8_t* rcDst) {
  uint64_t longest = 0;
  for (int64_t i = 0; i < n; ++i) longest = std::max(longest, off[i + 1] - off[i]);
  if (!longest) return DNAS_OK;
  hipLaunchKernelGGL(revcomp_reads_kernel, dim3((unsigned)n, (unsigned)std::min<uint64_t>((longest + 255) / 256, 64)), dim3(256), 0, m->stream,
                     src, dOff, fwdDst, rcDst);
  DNAS_HIP_TRY(hipGetLastError());
  return DNAS_OK;
}

// dnas_viterbi_batch_device, and -- out_strand given -- the same call in mode DNAS_STRAND_BOTH: 2n virtual reads (plan_call),
// fill and traceback writing per virtual read into the model's own arrays, a pick between the fill and the traceback of every
// batch, the traceback over the winners, a gather behind it.  With out_strand null nothing of that runs.
int viterbi_call_once(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* d_bases, char* d_out_sym,
                      const uint64_t* out_offsets, uint32_t* d_out_len, double* d_out_loglike, uint8_t* d_out_status, uint8_t* d_out_strand,
                      bool basesChecked) {
  const bool both = d_out_strand != nullptr;
  if (n_reads > (both ? 0x3ffffff0ll : 0x7fffffffll)) return dnas::fail(DNAS_E_UNSUPPORTED, both ? "more than 2^30-16 reads in one both-strand call" : "more than 2^31-1 reads in one call");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  // the previous call's events/stat buffers are about to be reused
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  m->stats = dnas_batch_stats{};
  m->statsPending = false;
  m->strandStats = dnas_strand_stats{};
  m->lastBoth = false;
  m->lastSegColumns = 0;
  m->lastSlices = 0;
  if (n_reads == 0) {
    // an empty call is the last call too: nothing of the call before it stays readable (lattices, events, census)
    m->lastSlotOff.clear(); m->lastBatchRead.clear(); m->lastBatchStart.clear(); m->lastReadOff.clear();
    m->lastBases = nullptr;
    m->lastCheckpointed = 0;
    m->clustersSeen = m->clustersSplit = 0;
    m->dEvents.reset(); m->dEvOff.reset(); m->dEvLen.reset();
    m->evOff.clear();
    return DNAS_OK;
  }
  int rc = basesChecked ? DNAS_OK : check_device_bases(m, d_bases + read_offsets[0], (size_t)(read_offsets[n_reads] - read_offsets[0]));
  if (rc != DNAS_OK) return rc;
  const DevModel& d = m->dm;
  // both strands: the virtual reads and their tables.  Virtual read i = caller read i, n + 1 + i = its reverse complement; the
  // offset tables hold the caller's prefix arrays twice (2n + 2 entries), so that [v], [v + 1] bound read i's bases -- in the
  // model's copy: the reads as written, behind them the reverse complements -- and read i's OUTPUT slot for both orientations
  const int64_t nCaller = n_reads;
  const uint64_t* const callerOff = read_offsets;
  const size_t nTab = both ? 2 * (size_t)nCaller + 2 : (size_t)nCaller + 1;     // entries of an offset table
  std::vector<uint64_t> vReadOff, vOutOff;
  StrandCall sc{nCaller, d_out_loglike, d_out_strand, d_out_len, d_out_status};
  if (both) {
    const uint64_t nBases = read_offsets[nCaller] - read_offsets[0];
    vReadOff.resize(nTab); vOutOff.resize(nTab);
    for (int64_t i = 0; i <= nCaller; ++i) {
      vReadOff[(size_t)i] = read_offsets[i] - read_offsets[0];
      vReadOff[(size_t)(nCaller + 1 + i)] = nBases + vReadOff[(size_t)i];
      vOutOff[(size_t)i] = vOutOff[(size_t)(nCaller + 1 + i)] = out_offsets[i];
    }
    DNAS_HIP_TRY(m->sBases.reserve(2 * (size_t)nBases, dnas::growQuarter256(2 * (size_t)nBases)));
    const size_t want = dnas::growQuarter64(nTab);
    DNAS_HIP_TRY(m->sLL.reserve(nTab, want));
    DNAS_HIP_TRY(m->sLen.reserve(nTab, want));
    DNAS_HIP_TRY(m->sSt.reserve(nTab, want));
    DNAS_HIP_TRY(m->sWinRead.reserve(nTab, want));      // (n entries are used)
    DNAS_HIP_TRY(m->sWinSlot.reserve(nTab, want));
    DNAS_HIP_TRY(m->sWinRow.reserve(nTab, want));
    // from here on the call is today's call on the virtual reads
    n_reads = 2 * nCaller;
    read_offsets = vReadOff.data();
    out_offsets = vOutOff.data();
  }
  const uint8_t* const callerBases = d_bases;
  uint32_t* const tbLen = both ? m->sLen.get() : d_out_len;         // where the traceback kernels write per (virtual) read
  uint8_t* const tbStatus = both ? m->sSt.get() : d_out_status;
  if (both) { d_bases = m->sBases.get(); d_out_loglike = m->sLL.get(); }

  // plan the call against the arena cap; if the device cannot give that much any more (the cap was taken from the free memory
  // when the model was created -- another process may have come since), plan once more against what is free now: smaller
  // batches, or segments for the reads that no longer fit
  CallPlan cp;
  for (int attempt = 0;; ++attempt) {
    cp = CallPlan();
    if ((rc = plan_call(m, n_reads, read_offsets, &cp, both ? nCaller : 0)) != DNAS_OK) return rc;
    const size_t need = std::max((size_t)cp.slices * cp.peak, cp.groupPeak) * sizeof(double);
    if (need <= m->arena.capacity() * sizeof(double)) break;
    const hipError_t e = m->arena.assign(need / sizeof(double)).error;     // frees first
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    size_t freeB = 0, totalB = 0;
    if (attempt > 0 || e != hipErrorOutOfMemory || hipMemGetInfo(&freeB, &totalB) != hipSuccess || freeB / 10 * 8 >= m->arenaCap)
      return dnas::fail(DNAS_E_DEVICE, "hipMalloc of the lattice arena (" + std::to_string(need) + " bytes): " + hipGetErrorString(e));
    m->arenaCap = freeB / 10 * 8;
  }
  std::vector<uint64_t>& slotOff = cp.slotOff;
  const std::vector<int64_t>& batchStart = cp.batchStart;
  const size_t nBatches = batchStart.size() - 1, nGroups = cp.groups.size();
  m->lastCheckpointed = cp.nSegmented;
  m->lastBatchStart = batchStart;
  const size_t nSlices = (size_t)cp.slices;
  const bool ring = cp.slices >= kRingSlices;
  m->lastSlices = cp.slices;
  m->halfDoubles = cp.peak;
  DNAS_HIP_TRY(m->dBatchRead.reserve(nTab, dnas::growExact(nTab)));
  DNAS_HIP_TRY(m->dSlotOff.reserve(nTab, dnas::growExact(nTab)));
  DNAS_HIP_TRY(m->dReadOff.reserve(nTab, dnas::growExact(nTab)));
  DNAS_HIP_TRY(m->dOutOff.reserve(nTab, dnas::growExact(nTab)));
  // the slot offsets of batch b point into half (b & 1), or into slice b % kRingSlices of the ring
  for (size_t b = 1; b < nBatches; ++b)
    for (int64_t i = batchStart[b]; i < batchStart[b + 1]; ++i) slotOff[(size_t)i] += (b % nSlices) * m->halfDoubles;
  m->lastSlotOff = slotOff;
  m->lastBatchRead = cp.order;
  m->lastReadOff.assign(read_offsets, read_offsets + nTab);
  m->lastBases = d_bases;
  m->lastBoth = both;
  // host vectors stay alive until the copies complete (synchronous copies keep this simple)
  DNAS_HIP_TRY(hipMemcpy(m->dBatchRead.get(), cp.order.data(), (size_t)n_reads * sizeof(int32_t), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemcpy(m->dSlotOff.get(), slotOff.data(), (size_t)n_reads * sizeof(uint64_t), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemcpy(m->dReadOff.get(), read_offsets, nTab * sizeof(uint64_t), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemcpy(m->dOutOff.get(), out_offsets, nTab * sizeof(uint64_t), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemsetAsync(m->dRounds.get(), 0, 8 * sizeof(unsigned long long), m->stream));
  if (both) {
    DNAS_HIP_TRY(hipMemsetAsync(m->dRounds.get() + 12, 0, 3 * sizeof(unsigned long long), m->stream));
    // the two orientations of every read into the model's buffer (the offsets it reads are the first half of the table above)
    const uint64_t nBases = callerOff[nCaller] - callerOff[0];
    if ((rc = launch_revcomp(m, nCaller, read_offsets, m->dReadOff.get(), callerBases + callerOff[0], m->sBases.get(), m->sBases.get() + nBases)) != DNAS_OK) return rc;
  }

  m->dEvents.reset(); m->dEvOff.reset(); m->dEvLen.reset();
  if (m->eventLog) {
    // at most one event per traceback step.  3 L + 64 events is a guess: a walk logs one deletion per state it passes without a
    // base of the read, however short the read.  The kernels count every event they meet, viterbi_call compares the counts with
    // these capacities and runs the call once more with the room it then knows (evWant)
    // (both strands: one log per CALLER read, the offset table twice like the others -- the winner's traceback writes it)
    m->evOff.assign((size_t)nCaller + 1, 0);
    for (int64_t i = 0; i < nCaller; ++i)
      m->evOff[(size_t)i + 1] = m->evOff[(size_t)i] + (m->evWant.empty() ? 3 * (read_offsets[i + 1] - read_offsets[i]) + 64 : m->evWant[(size_t)i]);
    DNAS_HIP_TRY(m->dEvents.assign(m->evOff.back()));
    DNAS_HIP_TRY(m->dEvOff.assign(nTab));
    DNAS_HIP_TRY(m->dEvLen.assign(nTab));
    DNAS_HIP_TRY(hipMemcpy(m->dEvOff.get(), m->evOff.data(), ((size_t)nCaller + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (both) DNAS_HIP_TRY(hipMemcpy(m->dEvOff.get() + nCaller + 1, m->evOff.data(), ((size_t)nCaller + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    DNAS_HIP_TRY(hipMemset(m->dEvLen.get(), 0, nTab * sizeof(uint32_t)));
  }
  const size_t nTimed = nBatches + nGroups;              // 4 timing events each: the groups first, then the batches
  while (m->events.size() < 4 * nTimed) {
    hipEvent_t e;
    DNAS_HIP_TRY(hipEventCreate(&e));
    m->events.push_back(e);
  }
  while (m->sync.size() < 2 * nBatches) {
    hipEvent_t e;
    DNAS_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    m->sync.push_back(e);
  }
  if (m->tier == 2) {
    const size_t wantWords = (nBatches + cp.groupLaunches) * (size_t)m->maxClusters * 64;
    m->syncCheckWords = 0;
    DNAS_HIP_TRY(m->syncCheck.reserve(wantWords, dnas::growExact(wantWords)));   // pinned: the copies after each fill stay asynchronous
    m->syncCheckWords = wantWords;
    memset(m->syncCheck.get(), 0, m->syncCheckWords * sizeof(unsigned));
    m->syncLaunches = nBatches + cp.groupLaunches;
  }

  FillLauncher fill{m, d_bases, d_out_loglike};
  if (nGroups) {
    if ((rc = ensure_segment_kernel(m)) != DNAS_OK) return rc;
    if ((rc = run_segment_groups(m, cp, read_offsets, fill, d_bases, d_out_sym, tbLen, tbStatus, both ? &sc : nullptr)) != DNAS_OK) return rc;
  }

  // Tier A with a ring of slices: the fills of the even batches go down `stream`, those of the odd ones down stream3, so that
  // the work-groups of batch b + 1 take the CUs that the last round of batch b leaves free -- the call is then one stream of
  // work-groups instead of launches of whole rounds.  Two fills are in flight while a third batch is traced back.  What this
  // call put on `stream` so far (the rounds counters' memset, the reverse complements, the segment groups) is ahead of the
  // first fill on stream3; the call before was drained on entry.
  if (ring) {
    DNAS_HIP_TRY(hipEventRecord(m->ringHead, m->stream));
    DNAS_HIP_TRY(hipStreamWaitEvent(m->stream3, m->ringHead, 0));
  }
  for (size_t b = 0; b < nBatches; ++b) {
    const int64_t s = batchStart[b];
    const int nB = (int)(batchStart[b + 1] - s);
    const size_t ev = 4 * (nGroups + b);
    const hipStream_t fs = ring && (b & 1) ? m->stream3 : m->stream;
    // the half (slice) this batch fills was last read by the traceback of batch b - 2 (b - kRingSlices)
    if (b >= nSlices) DNAS_HIP_TRY(hipStreamWaitEvent(fs, m->sync[2 * (b - nSlices) + 1], 0));
    DNAS_HIP_TRY(hipEventRecord(m->events[ev], fs));
    if ((rc = fill(fs, m->dBatchRead.get() + s, m->dSlotOff.get() + s, nB, nullptr)) != DNAS_OK) return rc;
    DNAS_HIP_TRY(hipEventRecord(m->events[ev + 1], fs));
    // both strands: the batch holds whole pairs; the traceback walks the winners, half as many
    const int nT = both ? nB / 2 : nB;
    const int32_t* const tbReads = both ? m->sWinRead.get() + s / 2 : m->dBatchRead.get() + s;
    const uint64_t* const tbSlots = both ? m->sWinSlot.get() + s / 2 : m->dSlotOff.get() + s;
    if (both) {
      if ((rc = pick_strands(m, fs, sc, s, nT, m->dSlotOff.get() + s, false)) != DNAS_OK) return rc;
      sc.tracebacks += nT;
    }
    DNAS_HIP_TRY(hipEventRecord(m->sync[2 * b], fs));
    RoctxRange tbRange("viterbi traceback");
    DNAS_HIP_TRY(hipStreamWaitEvent(m->stream2, m->sync[2 * b], 0));
    DNAS_HIP_TRY(hipEventRecord(m->events[ev + 2], m->stream2));
    // one wave per read finishes a read 4-5x sooner but costs about three times the CU time: for batches small enough
    // that the traceback is what the caller waits for (tier C, short jobs); large batches trace back thread-per-read in
    // blocks of 128 threads, 16 reads per wave (round 4; ~9 ms beside the next batch's fill.  Round 3: 128 reads per block, six CUs
    // for ~18 ms; as two blocks of 512 it held its CUs for 22-37 ms,
    // and every fifth fill launch paid a fourth round of work-groups on the shader engine it sat on: 51 ms instead of 43.  Also
    // tried: a wave per read launched when the next fill opens its last round -- the work-group that opens it bumped a signal
    // word the traceback stream waited on --: its 180 blocks then crowd the forty idle CUs and every launch took 48 ms) --
    // except the last batch of a call, which has the GPU to itself
    if (m->waveTraceback && (nT <= 256 || b + 1 == nBatches))
      hipLaunchKernelGGL(viterbi_traceback_wave_kernel, dim3((nT + 3) / 4), dim3(256), 0, m->stream2, d, d_bases,
                         (const uint64_t*)m->dReadOff.get(), tbReads, tbSlots,
                         (const double*)m->arena.get(), d_out_sym, (const uint64_t*)m->dOutOff.get(), tbLen, tbStatus, nT, m->dEvents.get(),
                         (const uint64_t*)m->dEvOff.get(), m->dEvLen.get(), (const int*)nullptr, (TracebackWalk*)nullptr);
    else
    {
      const int perBlock = (m->tbThreads / 64) * m->tbLanes;     // reads a block walks: tbLanes of every wave's 64 lanes
      hipLaunchKernelGGL(viterbi_traceback_kernel, dim3((nT + perBlock - 1) / perBlock), dim3(m->tbThreads), 0,
                         m->stream2, d, d_bases, (const uint64_t*)m->dReadOff.get(), tbReads,
                         tbSlots, (const double*)m->arena.get(), d_out_sym,
                         (const uint64_t*)m->dOutOff.get(), tbLen, tbStatus, nT, m->dEvents.get(), (const uint64_t*)m->dEvOff.get(), m->dEvLen.get(),
                         m->tbLanes);
    }
    DNAS_HIP_TRY(hipGetLastError());
    if (both && (rc = gather_winners(m, sc, s, nT, m->stream2)) != DNAS_OK) return rc;
    DNAS_HIP_TRY(hipEventRecord(m->events[ev + 3], m->stream2));
    DNAS_HIP_TRY(hipEventRecord(m->sync[2 * b + 1], m->stream2));
  }
  // "stream and stream2 drained" keeps meaning "the call is done": `stream` takes the tail of stream3 behind it
  if (ring) {
    DNAS_HIP_TRY(hipEventRecord(m->ringTail, m->stream3));
    DNAS_HIP_TRY(hipStreamWaitEvent(m->stream, m->ringTail, 0));
  }
  // trim so collect_stats sees exactly this call's events
  while (m->events.size() > 4 * nTimed) {
    (void)hipEventDestroy(m->events.back());
    m->events.pop_back();
  }
  m->stats.fill_launches = (int64_t)fill.launches;
  m->stats.checkpointed_reads = cp.nSegmented;
  m->stats.columns = cp.columns;
  m->stats.lattice_bytes = (int64_t)(8 * ((size_t)d.D + 2) * (size_t)d.N) * cp.columns;
  m->lastSegColumns = cp.segColumns;
  if (both) {
    m->strandStats.reads = nCaller;
    m->strandStats.tracebacks = sc.tracebacks;
    m->strandStats.fill_columns = cp.columns;              // both orientations of every read
    m->strandStats.pass2_columns = cp.segColumns / 2;      // the winners of the reads that went through segments
  }
  m->statsPending = true;
  return DNAS_OK;
}

// viterbi_call_once, and -- with the event log on -- the check that every read's log held every event.  The log is the model's
// own buffer, so a full one is the model's to mend: the call waits for its tracebacks, reads the counts, and where one exceeds
// its log runs once more with logs of the counted sizes (the same walks: they fit).  A call without the log is the one call,
// nothing added; with the log on a device call has finished when it returns.
int viterbi_call(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* d_bases, char* d_out_sym,
                 const uint64_t* out_offsets, uint32_t* d_out_len, double* d_out_loglike, uint8_t* d_out_status, uint8_t* d_out_strand,
                 bool basesChecked = false) {
  int rc = viterbi_call_once(m, n_reads, read_offsets, d_bases, d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, d_out_strand, basesChecked);
  if (rc != DNAS_OK || !m->eventLog || n_reads == 0) return rc;
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  std::vector<uint32_t> met((size_t)n_reads);
  DNAS_HIP_TRY(hipMemcpy(met.data(), m->dEvLen.get(), (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint64_t> want((size_t)n_reads);
  bool full = false;
  for (size_t i = 0; i < (size_t)n_reads; ++i) {
    const uint64_t room = m->evOff[i + 1] - m->evOff[i];
    want[i] = std::max<uint64_t>(room, met[i]);
    full = full || met[i] > room;
  }
  if (!full) return DNAS_OK;
  m->evWant.swap(want);
  rc = viterbi_call_once(m, n_reads, read_offsets, d_bases, d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, d_out_strand, basesChecked);
  m->evWant.clear();
  return rc;
}

}  // namespace

extern "C" int dnas_viterbi_batch_device(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets,
                                         const uint8_t* d_bases, char* d_out_sym, const uint64_t* out_offsets,
                                         uint32_t* d_out_len, double* d_out_loglike, uint8_t* d_out_status) {
  if (!m || n_reads < 0 || (n_reads > 0 && (!read_offsets || !d_bases || !d_out_sym || !out_offsets || !d_out_len ||
                                            !d_out_loglike || !d_out_status)))
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_batch_device: bad argument");
  RoctxRange callRange("dnas_viterbi_batch_device");
  return viterbi_call(m, n_reads, read_offsets, d_bases, d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, nullptr);
}

// Argument checks shared by the two strand entry points: the mode and out_strand first, then the device (as every device entry
// point answers DNAS_E_DEVICE where there is none), then the model.
static int check_strand_call(const dnas_model* m, int64_t n_reads, int strand_mode, const void* out_strand, const char* who) {
  if (strand_mode < DNAS_STRAND_FORWARD || strand_mode > DNAS_STRAND_BOTH)
    return dnas::fail(DNAS_E_INVALID, std::string(who) + ": strand_mode must be DNAS_STRAND_FORWARD, _REVERSE or _BOTH");
  if (!out_strand) return dnas::fail(DNAS_E_INVALID, std::string(who) + ": out_strand is null");
  if (!m) {            // (a model proves a device; without one, say which of the two is missing)
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return dnas::fail(DNAS_E_DEVICE, "no HIP device available");
  }
  if (!m || n_reads < 0) return dnas::fail(DNAS_E_INVALID, std::string(who) + ": bad argument");
  return DNAS_OK;
}

extern "C" int dnas_viterbi_batch_strands_device(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* d_bases,
                                                 int strand_mode, char* d_out_sym, const uint64_t* out_offsets, uint32_t* d_out_len,
                                                 double* d_out_loglike, uint8_t* d_out_status, uint8_t* d_out_strand) {
  int rc = check_strand_call(m, n_reads, strand_mode, d_out_strand, "dnas_viterbi_batch_strands_device");
  if (rc != DNAS_OK) return rc;
  if (n_reads > 0 && (!read_offsets || !d_bases || !d_out_sym || !out_offsets || !d_out_len || !d_out_loglike || !d_out_status))
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_batch_strands_device: null argument");
  RoctxRange callRange("dnas_viterbi_batch_strands_device");
  if (strand_mode == DNAS_STRAND_BOTH)
    return viterbi_call(m, n_reads, read_offsets, d_bases, d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, d_out_strand);
  if (strand_mode == DNAS_STRAND_FORWARD) {      // today's call, and zeros
    rc = viterbi_call(m, n_reads, read_offsets, d_bases, d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, nullptr);
    if (rc == DNAS_OK && n_reads > 0) DNAS_HIP_TRY(hipMemsetAsync(d_out_strand, 0, (size_t)n_reads, m->stream));
    return rc;
  }
  // DNAS_STRAND_REVERSE: today's call on the reverse complements, kept in the model's buffer until the next call
  if (n_reads == 0) return viterbi_call(m, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  DNAS_HIP_TRY(hipSetDevice(m->device));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));          // (the buffers below may still serve the call before)
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  const size_t nBases = (size_t)(read_offsets[n_reads] - read_offsets[0]);
  if ((rc = check_device_bases(m, d_bases + read_offsets[0], nBases)) != DNAS_OK) return rc;
  DNAS_HIP_TRY(m->sBases.reserve(nBases, dnas::growQuarter256(nBases)));
  DNAS_HIP_TRY(m->sOff.reserve((size_t)n_reads + 1, dnas::growQuarter256((size_t)n_reads + 1)));
  std::vector<uint64_t> off((size_t)n_reads + 1);
  for (int64_t i = 0; i <= n_reads; ++i) off[(size_t)i] = read_offsets[i] - read_offsets[0];
  DNAS_HIP_TRY(hipMemcpy(m->sOff.get(), off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  if ((rc = launch_revcomp(m, n_reads, off.data(), m->sOff.get(), d_bases + read_offsets[0], nullptr, m->sBases.get())) != DNAS_OK) return rc;
  rc = viterbi_call(m, n_reads, off.data(), m->sBases.get(), d_out_sym, out_offsets, d_out_len, d_out_loglike, d_out_status, nullptr, true);
  if (rc != DNAS_OK) return rc;
  DNAS_HIP_TRY(hipMemsetAsync(d_out_strand, 1, (size_t)n_reads, m->stream));
  m->strandStats.reads = m->strandStats.tracebacks = n_reads;
  m->strandStats.fill_columns = m->stats.columns;
  m->strandStats.pass2_columns = m->lastSegColumns;
  return DNAS_OK;
}

extern "C" int dnas_model_last_strand_stats(const dnas_model* m, dnas_strand_stats* out) {
  if (!m || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  if (m->statsPending) return dnas::fail(DNAS_E_INVALID, "call dnas_model_sync first");
  *out = m->strandStats;
  return DNAS_OK;
}

// dnas_viterbi_batch (out_strand null) and dnas_viterbi_batch_strands: host arrays in, the device call, host arrays out.
static int viterbi_host_call(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases, int strand_mode,
                             char* out_sym, const uint64_t* out_offsets, uint32_t* out_len, double* out_loglike,
                             uint8_t* out_status, uint8_t* out_strand) {
  if (!m || n_reads < 0) return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_batch: bad argument");
  // nothing to copy in or out; the device call resets the stats and drops the call before's lattices and events
  if (n_reads == 0) return dnas_viterbi_batch_device(m, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (!read_offsets || !bases || !out_sym || !out_offsets || !out_len || !out_loglike || !out_status)
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_batch: null argument");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  const size_t nBases = (size_t)(read_offsets[n_reads] - read_offsets[0]);
  if (read_offsets[0] != 0) return dnas::fail(DNAS_E_INVALID, "read_offsets[0] must be 0");
  for (size_t i = 0; i < nBases; ++i)
    if (bases[i] > 3) return dnas::fail(DNAS_E_BAD_BASE, "base code > 3 at offset " + std::to_string(i));
  const size_t nOut = (size_t)out_offsets[n_reads];
  // (the streams are idle: the call before was synchronised before it returned its results)
  int rc;
  m->lastBases = nullptr;
  DNAS_HIP_TRY(m->ioBases.reserve(nBases, dnas::growQuarter256(nBases)));
  DNAS_HIP_TRY(m->ioSym.reserve(nOut, dnas::growQuarter256(nOut)));
  const size_t wantReads = dnas::growQuarter64((size_t)n_reads);
  DNAS_HIP_TRY(m->ioLen.reserve((size_t)n_reads, wantReads));
  DNAS_HIP_TRY(m->ioLL.reserve((size_t)n_reads, wantReads));
  DNAS_HIP_TRY(m->ioSt.reserve((size_t)n_reads, wantReads));
  DNAS_HIP_TRY(m->ioStrand.reserve((size_t)n_reads, wantReads));
  if (nBases) DNAS_HIP_TRY(hipMemcpy(m->ioBases.get(), bases, nBases, hipMemcpyHostToDevice));
  if (out_strand)
    rc = dnas_viterbi_batch_strands_device(m, n_reads, read_offsets, m->ioBases.get(), strand_mode, m->ioSym.get(), out_offsets, m->ioLen.get(), m->ioLL.get(), m->ioSt.get(), m->ioStrand.get());
  else
    rc = dnas_viterbi_batch_device(m, n_reads, read_offsets, m->ioBases.get(), m->ioSym.get(), out_offsets, m->ioLen.get(), m->ioLL.get(), m->ioSt.get());
  if (rc == DNAS_OK) rc = dnas_model_sync(m);
  if (rc != DNAS_OK) return rc;
  if (nOut) DNAS_HIP_TRY(hipMemcpy(out_sym, m->ioSym.get(), nOut, hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_len, m->ioLen.get(), (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_loglike, m->ioLL.get(), (size_t)n_reads * sizeof(double), hipMemcpyDeviceToHost));
  DNAS_HIP_TRY(hipMemcpy(out_status, m->ioSt.get(), (size_t)n_reads, hipMemcpyDeviceToHost));
  if (out_strand) DNAS_HIP_TRY(hipMemcpy(out_strand, m->ioStrand.get(), (size_t)n_reads, hipMemcpyDeviceToHost));
  return DNAS_OK;
}

extern "C" int dnas_viterbi_batch(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases,
                                  char* out_sym, const uint64_t* out_offsets, uint32_t* out_len, double* out_loglike,
                                  uint8_t* out_status) {
  return viterbi_host_call(m, n_reads, read_offsets, bases, DNAS_STRAND_FORWARD, out_sym, out_offsets, out_len, out_loglike, out_status, nullptr);
}

extern "C" int dnas_viterbi_batch_strands(dnas_model* m, int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases,
                                          int strand_mode, char* out_sym, const uint64_t* out_offsets, uint32_t* out_len,
                                          double* out_loglike, uint8_t* out_status, uint8_t* out_strand) {
  const int rc = check_strand_call(m, n_reads, strand_mode, out_strand, "dnas_viterbi_batch_strands");
  if (rc != DNAS_OK) return rc;
  return viterbi_host_call(m, n_reads, read_offsets, bases, strand_mode, out_sym, out_offsets, out_len, out_loglike, out_status, out_strand);
}

extern "C" int dnas_model_read_lattice(dnas_model* m, int64_t slot, int64_t len, double* out) {
  if (!m || !out || slot < 0 || len < 0 || m->lastReadOff.empty() || (size_t)slot + 1 >= m->lastReadOff.size())
    return dnas::fail(DNAS_E_INVALID, "dnas_model_read_lattice: bad argument");
  if (m->lastBoth) return dnas::fail(DNAS_E_UNSUPPORTED, "dnas_model_read_lattice: the last call decoded both strands (a single-read testing aid: call one orientation)");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  if (!m->lastBases) return dnas::fail(DNAS_E_INVALID, "dnas_model_read_lattice: the read bases of the last call are gone");
  const DevModel& d = m->dm;
  const size_t lanes = (size_t)d.D + 2;
  // `slot` indexes the caller's read order; find its arena slot.  The arena has two halves that the batches of a call
  // use in turn: only the lattices of the last two batches still exist.  (A ring of three slices still holds a third batch;
  // the rule is kept as callers know it: the last two.)
  size_t pos = 0;
  for (; pos < m->lastBatchRead.size(); ++pos)
    if (m->lastBatchRead[pos] == (int32_t)slot) break;
  if (pos == m->lastBatchRead.size()) return dnas::fail(DNAS_E_INVALID, "no such read in the last call");
  if ((int64_t)pos < m->lastCheckpointed)
    return dnas::fail(DNAS_E_INVALID, "dnas_model_read_lattice: that read was decoded in segments (bounded-memory decode); its lattice was never whole");
  {
    size_t batchOf = 0;
    while (batchOf + 1 < m->lastBatchStart.size() && (int64_t)pos >= m->lastBatchStart[batchOf + 1]) ++batchOf;
    const size_t nB = m->lastBatchStart.size() - 1;
    if (batchOf + 2 < nB) return dnas::fail(DNAS_E_INVALID, "dnas_model_read_lattice: that read's lattice has been overwritten by a later batch of the call");
  }
  if ((uint64_t)len != m->lastReadOff[slot + 1] - m->lastReadOff[slot]) return dnas::fail(DNAS_E_INVALID, "length mismatch");
  const size_t n = (size_t)(len + 1) * lanes * (size_t)d.N;
  DevBuf<double> dOut;
  DNAS_HIP_TRY(dOut.assign(n));
  hipLaunchKernelGGL(expand_lattice_kernel, dim3((unsigned)(len + 1)), dim3(256), 0, m->stream, d,
                     m->lastBases + m->lastReadOff[slot], (const double*)(m->arena.get() + m->lastSlotOff[pos]), dOut.get());
  hipError_t e = hipStreamSynchronize(m->stream);
  if (e == hipSuccess) e = hipMemcpy(out, dOut.get(), n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return dnas::fail(DNAS_E_DEVICE, hipGetErrorString(e));
  return DNAS_OK;
}

// Analysis / test aid: the tier-A tables of a machine exactly as the kernel receives them (no GPU
// needed): row shapes [K][2] = {out-edge entries, S stripe or -1}, the entry table [n_entries][T]
// and the meta table [K][T].  Either output may be NULL; *n_entries / *n_s_rows are always set.
extern "C" int dnas_tiera_plan_tables(const dnas_flat_model* fm, int32_t* row_shapes, uint32_t* entries, size_t entries_cap,
                                      uint32_t* meta, int32_t* n_entries, int32_t* n_s_rows) {
  if (!fm) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    const int threads = env_threads(dnas::kTierAThreads);
    const dnas::TierAPlan p = dnas::buildTierAPlan(*fm, threads, env_or_recorded_choice(fm, 1, threads));
    if (!p.ok) return dnas::fail(DNAS_E_UNSUPPORTED, p.whyNot);
    if (n_entries) *n_entries = p.nEntries;
    if (n_s_rows) *n_s_rows = p.nSRows;
    if (row_shapes) for (int k = 0; k < p.K; ++k) { row_shapes[2 * k] = p.rows[k].nOut; row_shapes[2 * k + 1] = p.rows[k].sIdx; }
    if (entries) {
      if (entries_cap < p.entTab.size()) return dnas::fail(DNAS_E_INVALID, "entry buffer too small");
      memcpy(entries, p.entTab.data(), p.entTab.size() * sizeof(uint32_t));
    }
    if (meta) memcpy(meta, p.metaTab.data(), p.metaTab.size() * sizeof(uint32_t));
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

// Build-time helper: specialise and compile the tier-A kernel for a machine without touching
// a GPU (fills dnastore_amd/kcache so that the GPU box finds the code object ready).
extern "C" int dnas_tiera_precompile(const dnas_flat_model* fm, char* note, size_t note_cap) {
  if (!fm) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    // the row program a model of this machine will run: as the environment says, else as its tuning record says, else the
    // default one
    const int threads = env_threads(dnas::kTierAThreads);   // as dnas_model_create_ex reads it
    const dnas::TierAPlan p = dnas::buildTierAPlan(*fm, threads, env_or_recorded_choice(fm, 1, threads));
    std::string msg;
    if (!p.ok) {
      msg = "tier B: " + p.whyNot;
    } else {
      (void)dnas::jitCompile(p.defines, p.key);
      msg = "tier A: " + p.key + " lds=" + std::to_string(p.ldsBytes) + " fill=" + std::to_string(p.fillRatio) +
            " reads=" + std::to_string(p.sweepReads) + " entries=" + std::to_string(p.nEntries) + " back=" +
            std::to_string(p.backEdgesOnWalk) + " sameWave=" + std::to_string(p.sameWave);
    }
    if (note && note_cap) { strncpy(note, msg.c_str(), note_cap - 1); note[note_cap - 1] = 0; }
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

extern "C" const char* dnas_model_tier(const dnas_model* m) { return m ? m->tierNote.c_str() : ""; }

extern "C" int dnas_model_set_event_log(dnas_model* m, int on) {
  if (!m) return dnas::fail(DNAS_E_INVALID, "null model");
  if (on && m->dm.D > 13)     // a duplication event carries its bases in 26 bits (viterbi_kernels.hip)
    return dnas::fail(DNAS_E_UNSUPPORTED, "the traceback event log holds at most 13 duplicated bases per event; this model has " + std::to_string(m->dm.D) + " duplication lanes");
  m->eventLog = on != 0;
  return DNAS_OK;
}

// The traceback events of read `read_index` of the last call, in the order the traceback met them.
extern "C" int dnas_model_read_events(dnas_model* m, int64_t read_index, uint64_t* out, int64_t cap, int64_t* n_events) {
  if (!m || !n_events || read_index < 0) return dnas::fail(DNAS_E_INVALID, "dnas_model_read_events: bad argument");
  *n_events = 0;
  if (!m->dEvents.get() || (size_t)read_index + 1 >= m->evOff.size()) return dnas::fail(DNAS_E_INVALID, "no event log for that read (dnas_model_set_event_log before the call)");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream2));
  uint32_t n = 0;
  DNAS_HIP_TRY(hipMemcpy(&n, m->dEvLen.get() + read_index, sizeof n, hipMemcpyDeviceToHost));
  // (the kernels count every event they meet; viterbi_call has made the log hold them all: a short list is never handed out as whole)
  if ((uint64_t)n > m->evOff[(size_t)read_index + 1] - m->evOff[(size_t)read_index])
    return dnas::fail(DNAS_E_DEVICE, "the traceback met " + std::to_string(n) + " events of read " + std::to_string(read_index) + ", more than its event log holds");
  *n_events = n;
  if (out && cap > 0) {
    const size_t take = (size_t)std::min<int64_t>(cap, n);
    if (take) DNAS_HIP_TRY(hipMemcpy(out, m->dEvents.get() + m->evOff[(size_t)read_index], take * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return DNAS_OK;
}

// Tier C: compile the cluster kernel for a machine ahead of time (members = 0: the smallest cluster that fits).
extern "C" int dnas_tierc_precompile(const dnas_flat_model* fm, int32_t members, char* note, size_t note_cap) {
  if (!fm) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    const int threads = env_threads(0);   // (the same thread count names the record and shapes the plan)
    const dnas::TierAPlan p = dnas::chooseClusterPlan(*fm, members, threads, env_or_recorded_choice(fm, members >= 2 ? members : 0, threads));
    if (!p.ok) return dnas::fail(DNAS_E_UNSUPPORTED, p.whyNot);
    (void)dnas::jitCompile(p.defines, p.key);
    const std::string msg = "tier C: G=" + std::to_string(p.G) + " K=" + std::to_string(p.K) + " inbox rows " + std::to_string(p.nGRows) +
                            " exchange edges " + std::to_string(p.crossEdges) + " lds=" + std::to_string(p.ldsBytes) + " entries=" +
                            std::to_string(p.nEntries) + " back=" + std::to_string(p.backEdgesOnWalk) + " " + p.key;
    if (note && note_cap) { strncpy(note, msg.c_str(), note_cap - 1); note[note_cap - 1] = 0; }
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

namespace {
// members = 1: the tier-A plan, else the cluster plan -- under the row program a model of this machine follows (record, environment)
dnas::TierAPlan plan_as_a_model_would(const dnas_flat_model* fm, int members) {
  if (members == 1) {
    const int threads = env_threads(dnas::kTierAThreads);
    return dnas::buildTierAPlan(*fm, threads, env_or_recorded_choice(fm, 1, threads));
  }
  const int threads = env_threads(0);
  return dnas::chooseClusterPlan(*fm, members, threads, env_or_recorded_choice(fm, members >= 2 ? members : 0, threads));
}
}  // namespace

// Analysis / test aid: the tier-C tables of a machine exactly as the kernel receives them (no GPU needed).
// info[8] = {G, K, T, entries per member, S stripes, exchange rows, proxies, 0}; every other output may be NULL:
// row_shapes[K][6], entries[G][n_entries][T], meta[G][K][T], member_of[N], lds_index[N] = row*T + lane inside
// the member, lattice_slot[N], fold[G][inbox rows][T].
extern "C" int dnas_tierc_plan(const dnas_flat_model* fm, int32_t members, int32_t* info, int32_t* row_shapes, uint32_t* entries,
                               size_t entries_cap, uint32_t* meta, int32_t* member_of, int32_t* lds_index, int32_t* lattice_slot,
                               uint32_t* fold) {
  if (!fm || !info) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    const dnas::TierAPlan p = plan_as_a_model_would(fm, members);
    if (!p.ok) return dnas::fail(DNAS_E_UNSUPPORTED, p.whyNot);
    info[0] = p.G; info[1] = p.K; info[2] = p.T; info[3] = p.nEntries; info[4] = p.nSRows; info[5] = p.nGRows; info[6] = (int32_t)p.proxyMember.size(); info[7] = 0;
    if (row_shapes)
      for (int k = 0; k < p.K; ++k) {
        const dnas::RowShape& r = p.rows[k];
        const int v[6] = {r.nOut, r.sIdx, r.kind, r.cls, r.full, r.gOut};
        memcpy(row_shapes + 6 * k, v, sizeof v);
      }
    if (entries) {
      if (entries_cap < p.entTab.size()) return dnas::fail(DNAS_E_INVALID, "entry buffer too small");
      memcpy(entries, p.entTab.data(), p.entTab.size() * sizeof(uint32_t));
    }
    if (meta) memcpy(meta, p.metaTab.data(), p.metaTab.size() * sizeof(uint32_t));
    if (member_of) memcpy(member_of, p.memberOf.data(), (size_t)p.N * sizeof(int32_t));
    if (lds_index)
      for (size_t idx = 0; idx < p.stateOf.size(); ++idx)
        if (p.stateOf[idx] >= 0) lds_index[p.stateOf[idx]] = (int32_t)(idx % ((size_t)p.K * p.T));
    if (lattice_slot) memcpy(lattice_slot, p.slotOf.data(), (size_t)p.N * sizeof(int32_t));
    if (fold && !p.foldTab.empty()) memcpy(fold, p.foldTab.data(), p.foldTab.size() * sizeof(uint32_t));
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

// ... and the places of its proxies (plan.cpp: extra places that combine a member's null edges into one state of another
// member): member and row*T + lane of each, info[6] of them.
extern "C" int dnas_tierc_plan_proxies(const dnas_flat_model* fm, int32_t members, int32_t* proxy_member, int32_t* proxy_lds_index, size_t cap) {
  if (!fm || !proxy_member || !proxy_lds_index) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    const dnas::TierAPlan p = plan_as_a_model_would(fm, members);
    if (!p.ok) return dnas::fail(DNAS_E_UNSUPPORTED, p.whyNot);
    if (cap < p.proxyMember.size()) return dnas::fail(DNAS_E_INVALID, "proxy buffer too small");
    if (!p.proxyMember.empty()) {
      memcpy(proxy_member, p.proxyMember.data(), p.proxyMember.size() * sizeof(int32_t));
      memcpy(proxy_lds_index, p.proxyLds.data(), p.proxyLds.size() * sizeof(int32_t));
    }
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

// The name of the tuning record of a tier-A machine (tune_row_program above; tools/make_tune_records.py writes the records
// that ship with the library from bench-like reads).
extern "C" int dnas_tune_record_name(const dnas_flat_model* fm, int32_t members, int32_t threads, char* out, size_t cap) {
  if (!fm || !out || cap < 40) return dnas::fail(DNAS_E_INVALID, "dnas_tune_record_name: bad argument");
  // members 1: tier A (threads 0 = 1024); 0 or >= 2: tier C with the smallest / that cluster (threads 0 = chosen by the planner)
  const std::string name = tune_record_name(fm, members, members == 1 && threads <= 0 ? dnas::kTierAThreads : threads);
  strncpy(out, name.c_str(), cap - 1);
  out[cap - 1] = 0;
  return DNAS_OK;
}

// The hash of the fill kernel's source as this library carries it (what a tuning record names as "kernel=").
extern "C" int dnas_kernel_source_hash(char* out, size_t cap) {
  if (!out || cap < 17) return dnas::fail(DNAS_E_INVALID, "dnas_kernel_source_hash: bad argument");
  snprintf(out, cap, "%016llx", dnas::kernelSourceHash());
  return DNAS_OK;
}

extern "C" int dnas_model_cluster_census(dnas_model* m, int32_t* clusters, int32_t* split) {
  if (!m || !clusters || !split) return dnas::fail(DNAS_E_INVALID, "null argument");
  if (m->statsPending) return dnas::fail(DNAS_E_INVALID, "call dnas_model_sync first");
  *clusters = (int32_t)m->clustersSeen; *split = (int32_t)m->clustersSplit;
  return DNAS_OK;
}

// Diagnostic: the 8 words of the rounds/stamps buffer of the last call (word 0 = total rounds).
extern "C" int dnas_model_debug_words(dnas_model* m, unsigned long long* out8) {
  if (!m || !out8) return dnas::fail(DNAS_E_INVALID, "null argument");
  DNAS_HIP_TRY(hipSetDevice(m->device));
  DNAS_HIP_TRY(hipStreamSynchronize(m->stream));
  DNAS_HIP_TRY(hipMemcpy(out8, m->dRounds.get(), 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return DNAS_OK;
}

// Analysis / test aid: the tier-A placement of a machine (no GPU needed).  lds_index[N] receives
// row*T + lane of every state; returns T in *threads and K in *rows; DNAS_E_UNSUPPORTED when the
// machine does not fit tier A.
extern "C" int dnas_tiera_plan_slots(const dnas_flat_model* fm, int32_t* lds_index, int32_t* lattice_slot, int32_t* threads,
                                     int32_t* rows) {
  if (!fm) return dnas::fail(DNAS_E_INVALID, "null argument");
  try {
    const dnas::TierAPlan p = plan_as_a_model_would(fm, 1);
    if (!p.ok) return dnas::fail(DNAS_E_UNSUPPORTED, p.whyNot);
    if (threads) *threads = p.T;
    if (rows) *rows = p.K;
    for (int slot = 0; slot < p.NS; ++slot)
      if (p.stateOf[slot] >= 0 && lds_index) lds_index[p.stateOf[slot]] = slot;
    if (lattice_slot) for (int j = 0; j < p.N; ++j) lattice_slot[j] = p.slotOf[j];
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}
