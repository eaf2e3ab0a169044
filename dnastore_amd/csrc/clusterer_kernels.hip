// dnas_clusterer_*: a pool of reads that grows by batches (include/dnastore_amd.h), bit-identical to clusterReadsHost
// (host/cluster.cpp) on the concatenation of the batches.
//
// The handle keeps the reads, their offsets and signatures, one band's buffers and the gate's on its device; the edges found so
// far live on the host.  An add uploads and sketches the new reads only, compares their signatures with those of every read in
// front of them, and sends the candidates down the one-shot call's path (cluster_device.h): gate, score, pick.
//
// Filter.  The one-shot filter owns rows and walks to the end of the pool; an add is the other shape, few new columns j against
// many rows i < j.  A work-group owns a tile of 64 new reads j, staged once in LDS (row stride m + 1 words, so that lane l reading
// the signature of column l stands on its own bank) and copied into registers, a column per lane.  The row tiles of the pool pass
// by from read 0 to the tile that holds the work-group's last column; each is staged in LDS, a wave takes 16 of its rows as
// broadcasts and builds, per lane, a 16-bit mask of the rows that are candidates of the lane's column.  So that a small batch
// fills the chip the row tiles of a column tile are cut into S segments, one work-group each: the grid is column tiles x S.
// The count pass leaves count[jLocal * S + s]; the host's prefix sum over them in that order is where every (column, segment)
// starts in the add's list, which therefore is in (j, i) order.  The emit pass walks the same tiles and files a candidate at
//   off[jLocal * S + s] + the column's candidates in earlier tiles of the segment + those in the lower waves' rows of this tile
//   (exchanged through 4 x 64 words of LDS) + those below its row in the wave's own mask:
// no atomic decides a place.  Positions in [lo, hi) go to list[pos - lo], so a band may begin and end inside a column, and a
// work-group whose columns have nothing in the band leaves at once.
#include "cluster_device.h"
#include "host/clusterer.hpp"

namespace {

constexpr int kCrTile = (int)dnas::kClustererTile;       // columns of a work-group, rows of a row tile
constexpr int kCrWaves = 4;                              // waves of a work-group
constexpr int kCrRowsPerWave = kCrTile / kCrWaves;
static_assert(kCrTile == 64 && kCrRowsPerWave <= 32, "a column per lane, a row mask in one word");

// Segment blockIdx.y of column tile tileFirst + blockIdx.x of an add that found n0 reads and leaves n1.  EMIT = false:
// count[jLocal * S + s].  EMIT = true: off[jLocal * S + s] (S * columns + 1 entries), [lo, hi), list as above.
template <int M, bool EMIT>
__device__ __forceinline__ void clustererFilterBody(int64_t n0, int64_t n1, const uint32_t* __restrict__ sig,
                                                    const int64_t* __restrict__ readOff, int minShared, int64_t tileFirst,
                                                    int tilesPerSegment, int64_t* __restrict__ count, const int64_t* __restrict__ off,
                                                    int64_t lo, int64_t hi, ClPair* __restrict__ list) {
  constexpr int kStride = M + 1;
  __shared__ uint32_t rowSig[kCrTile * kStride], colSig[kCrTile * kStride];
  __shared__ uint8_t rowFull[kCrTile], colFull[kCrTile];   // the read is not empty
  __shared__ int waveCnt[kCrWaves * kCrTile];              // [wave][column]: the wave's candidates of the column in this tile
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t S = gridDim.y, s = blockIdx.y;
  const int64_t j0 = n0 + (tileFirst + blockIdx.x) * kCrTile, j = j0 + lane;
  if (j0 >= n1) return;
  const int64_t jLast = (j0 + kCrTile < n1 ? j0 + kCrTile : n1) - 1, need = jLast / kCrTile + 1;
  const int64_t tBegin = s * tilesPerSegment < need ? s * tilesPerSegment : need;
  const int64_t tEnd = tBegin + tilesPerSegment < need ? tBegin + tilesPerSegment : need;
  const int64_t slot = (j - n0) * S + s;

  int64_t base = 0;
  if (EMIT) {
    // what the band holds of this column's segment: nothing for every column of the tile, and the work-group is done
    int64_t end = 0;
    if (j < n1) base = off[slot], end = off[slot + 1];
    if (!__syncthreads_or(end > base && base < hi && end > lo)) return;
  }

  for (int idx = tid; idx < kCrTile * M; idx += 64 * kCrWaves) {
    const int r = idx / M, t = idx % M;
    colSig[r * kStride + t] = j0 + r < n1 ? sig[(j0 + r) * M + t] : dnas::kClusterNoSig;
  }
  if (tid < kCrTile) colFull[tid] = j0 + tid < n1 && readOff[j0 + tid + 1] > readOff[j0 + tid];
  __syncthreads();
  uint32_t col[M];
  if (minShared > 0) {
#pragma unroll
    for (int t = 0; t < M; ++t) col[t] = colSig[lane * kStride + t];
  }
  const bool full = colFull[lane];

  int run = 0;                                           // EMIT: the column's candidates in earlier tiles; else this wave's so far
  for (int64_t tile = tBegin; tile < tEnd; ++tile) {
    const int64_t i0 = tile * kCrTile;
    __syncthreads();                                     // the last row tile and its counts have been read
    for (int idx = tid; idx < kCrTile * M; idx += 64 * kCrWaves) {
      const int r = idx / M, t = idx % M;
      rowSig[r * kStride + t] = i0 + r < n1 ? sig[(i0 + r) * M + t] : dnas::kClusterNoSig;
    }
    if (tid < kCrTile) rowFull[tid] = i0 + tid < n1 && readOff[i0 + tid + 1] > readOff[i0 + tid];
    __syncthreads();
    uint32_t mask = 0;                                   // bit rr: row wv * 16 + rr of the tile is a candidate of column j
#pragma unroll
    for (int rr = 0; rr < kCrRowsPerWave; ++rr) {
      const int r = wv * kCrRowsPerWave + rr;
      const int64_t i = i0 + r;
      int shared = 0;
      if (minShared > 0) {
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const uint32_t a = rowSig[r * kStride + t];
          shared += a == col[t] && a != dnas::kClusterNoSig;
        }
      }
      const bool cand = j < n1 && i < j && dnas::clusterCandidate(shared, minShared, rowFull[r], full);
      mask |= (uint32_t)cand << rr;
    }
    if (!EMIT) {
      run += __popc(mask);
      continue;                                          // (uniform)
    }
    waveCnt[wv * kCrTile + lane] = __popc(mask);
    __syncthreads();
    int below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCrWaves; ++w) {
      const int c = waveCnt[w * kCrTile + lane];
      below += w < wv ? c : 0;
      all += c;
    }
    int before = 0;
    while (mask) {
      const int rr = __ffs((int)mask) - 1;
      mask &= mask - 1;
      const int64_t pos = base + run + below + before++;
      if (pos >= lo && pos < hi) list[pos - lo] = ClPair{(int32_t)(i0 + wv * kCrRowsPerWave + rr), (int32_t)j};
    }
    run += all;
  }
  if (!EMIT) {
    waveCnt[wv * kCrTile + lane] = run;                  // (the count pass has not used it so far)
    __syncthreads();
    if (wv == 0 && j < n1) {
      int64_t all = 0;
#pragma unroll
      for (int w = 0; w < kCrWaves; ++w) all += waveCnt[w * kCrTile + lane];
      count[slot] = all;
    }
  }
}

template <int M>
__global__ __launch_bounds__(64 * kCrWaves) void clusterer_filter_count_kernel(int64_t n0, int64_t n1, const uint32_t* __restrict__ sig,
                                                                              const int64_t* __restrict__ readOff, int minShared,
                                                                              int tilesPerSegment, int64_t* __restrict__ count) {
  clustererFilterBody<M, false>(n0, n1, sig, readOff, minShared, 0, tilesPerSegment, count, nullptr, 0, 0, nullptr);
}

// The band [lo, hi) of the add's list, whose candidates lie in the column tiles tileFirst .. tileFirst + gridDim.x - 1.
template <int M>
__global__ __launch_bounds__(64 * kCrWaves) void clusterer_filter_emit_kernel(int64_t n0, int64_t n1, const uint32_t* __restrict__ sig,
                                                                             const int64_t* __restrict__ readOff, int minShared,
                                                                             int64_t tileFirst, int tilesPerSegment,
                                                                             const int64_t* __restrict__ off, int64_t lo, int64_t hi,
                                                                             ClPair* __restrict__ list) {
  clustererFilterBody<M, true>(n0, n1, sig, readOff, minShared, tileFirst, tilesPerSegment, nullptr, off, lo, hi, list);
}

// ---------------------------------------------------------------------------------------------------------------- host side

// A buffer of the handle grows to max(needed, 2 x capacity) (clustererGrowTo), the first `keep` elements copied device to device
// on the stream (an empty buffer has nothing to keep).
template <class T>
int clGrow(dnas::DevBuf<T>& b, int64_t needed, int64_t keep, hipStream_t stream) {
  DNAS_HIP_TRY(b.reserveKeep((size_t)needed, (size_t)dnas::clustererGrowTo(needed, (int64_t)b.capacity()), (size_t)keep, stream));
  return DNAS_OK;
}

}  // namespace

struct dnas_clusterer {
  dnas::PairScores hs;
  int band, k, m, minShared;
  double minScorePerNt;
  int32_t maxEditPermille;
  bool opened = false, poisoned = false;
  // host
  std::vector<int64_t> readOff{0};
  int64_t longest = 0;                                   // among the reads held
  std::vector<dnas::ClusterEdge> edges;                  // in the order found
  dnas_cluster_stats stats{};
  dnas_cluster_gate_stats gate{};
  // device
  ClDevice d;
  dnas::DevBuf<int8_t> reads;
  dnas::DevBuf<int64_t> off, count, slotOff;
  dnas::DevBuf<uint32_t> sig;
  dnas::DevBuf<ClPair> list, surv;
  dnas::DevBuf<double> chunk, bnd;
  dnas::DevBuf<dnas::ClusterEdge> bandEdges;
  unsigned long long* edgeCount = nullptr;               // (freed with d's buffers)
  std::unique_ptr<ClGate> gateBufs;
  int64_t gateWordsOpen = -1;                            // what gateBufs was opened for

  int64_t n() const { return (int64_t)readOff.size() - 1; }
};

namespace {

int clustererOpen(dnas_clusterer& h) {
  if (h.opened) return DNAS_OK;
  int rc;
  if ((rc = h.d.bufs.open())) return rc;
  for (hipEvent_t& e : h.d.ev) DNAS_HIP_TRY(hipEventCreate(&e));
  (void)hipDeviceGetAttribute(&h.d.cus, hipDeviceAttributeMultiprocessorCount, h.d.device);
  if ((rc = paUpload(h.d.bufs, &h.d.dSub, h.hs.sub, 16))) return rc;
  if ((rc = paAlloc(h.d.bufs, &h.edgeCount, 1))) return rc;
  h.opened = true;
  return DNAS_OK;
}

// The add proper, the arguments checked and nNew > 0.  The host's offsets are already those of the grown pool.
int clustererAddOn(dnas_clusterer& h, int64_t n0, int64_t nNew, const int8_t* seqs, const int64_t* readOffNew) {
  DNAS_HIP_TRY(hipSetDevice(h.d.device));
  int rc;
  if ((rc = clustererOpen(h))) return rc;
  ClDevice& d = h.d;
  hipStream_t stream = d.bufs.stream;
  const int64_t n1 = n0 + nNew, bases0 = h.readOff[(size_t)n0], bases1 = h.readOff[(size_t)n1];

  if ((rc = clGrow(h.reads, std::max<int64_t>(bases1, 1), bases0, stream))) return rc;
  if ((rc = clGrow(h.off, n1 + 1, n0 + 1, stream))) return rc;
  if ((rc = clGrow(h.sig, n1 * h.m, n0 * h.m, stream))) return rc;
  if (bases1 > bases0) DNAS_HIP_TRY(hipMemcpy(h.reads.get() + bases0, seqs, (size_t)(bases1 - bases0), hipMemcpyHostToDevice));
  DNAS_HIP_TRY(hipMemcpy(h.off.get() + n0, h.readOff.data() + n0, (size_t)(nNew + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  d.dReads = h.reads.get(), d.dReadOff = h.off.get(), d.dSig = h.sig.get();

  const unsigned sketchBlocks = (unsigned)std::min<int64_t>((nNew + 3) / 4, (int64_t)d.cus * 8);
  rc = d.timed(&d.stats.sketch_ms, [&] {
    clDispatchM(h.m, [&](auto mm) {
      hipLaunchKernelGGL(cluster_sketch_kernel<decltype(mm)::value>, dim3(sketchBlocks), dim3(256), 0, stream, nNew, d.dReads,
                         d.dReadOff + n0, h.k, d.dSig + n0 * h.m);
    });
  });
  if (rc) return rc;

  int64_t forced = 0;
  if (const char* s = getenv("DNAS_CLUSTERER_SEGMENTS")) forced = std::max<int64_t>(0, atoll(s));
  const dnas::ClustererGrid g = dnas::clustererGrid(n0, n1, d.cus, forced);
  const int64_t slots = nNew * g.segments;
  if ((rc = clGrow(h.count, slots, 0, stream))) return rc;
  if ((rc = clGrow(h.slotOff, slots + 1, 0, stream))) return rc;
  rc = d.timed(&d.stats.filter_ms, [&] {
    clDispatchM(h.m, [&](auto mm) {
      hipLaunchKernelGGL(clusterer_filter_count_kernel<decltype(mm)::value>, dim3((unsigned)g.colTiles, (unsigned)g.segments),
                         dim3(64 * kCrWaves), 0, stream, n0, n1, d.dSig, d.dReadOff, h.minShared, (int)g.tilesPerSegment, h.count.get());
    });
  });
  if (rc) return rc;
  std::vector<int64_t> count((size_t)slots);
  DNAS_HIP_TRY(hipMemcpy(count.data(), h.count.get(), (size_t)slots * sizeof(int64_t), hipMemcpyDeviceToHost));
  const std::vector<int64_t> slotOff = dnas::clustererPrefix(count);
  const int64_t total = slotOff.back();
  if (total == 0) return DNAS_OK;
  DNAS_HIP_TRY(hipMemcpy(h.slotOff.get(), slotOff.data(), slotOff.size() * sizeof(int64_t), hipMemcpyHostToDevice));

  // the bands: as the one-shot call cuts them, but no buffer is larger than the add's list
  int64_t capPairs = (int64_t)1 << 21;
  if (const char* s = getenv("DNAS_CLUSTER_CHUNK")) capPairs = std::min<int64_t>(capPairs, atoll(s));
  capPairs = std::min(std::max<int64_t>(capPairs, 1), total);
  int maxO = (int)h.longest;
  for (int64_t q = 0; q < nNew; ++q) maxO = std::max(maxO, (int)(readOffNew[q + 1] - readOffNew[q]));
  const bool gated = h.maxEditPermille >= 0;
  std::vector<int64_t> gateWords;                        // per new read j: words of the longest pattern a pair (i < j, j) can have
  if (gated) {
    gateWords.resize((size_t)nNew);
    int64_t longest = h.longest;                         // among the reads in front of j
    for (int64_t q = 0; q < nNew; ++q) {
      const int64_t len = readOffNew[q + 1] - readOffNew[q];
      gateWords[(size_t)q] = dnas::clusterGateWords(len, longest);
      longest = std::max(longest, len);
    }
  }

  const PaScores sc = PaScores::from(h.hs);
  ClBand bd;
  bd.hs = &h.hs, bd.band = h.band, bd.minScorePerNt = h.minScorePerNt, bd.maxEditPermille = h.maxEditPermille;
  bd.readOff = h.readOff.data();
  if ((rc = paPlanScore(sc.P, clScoreKernelOf(), d.cus, maxO, "DNAS_CLUSTER_CHUNK", 2 * capPairs, &bd.plan))) return rc;
  bd.plan.chunkItems = 2 * capPairs;                     // a band is one chunk, as in the one-shot call
  if ((rc = clGrow(h.list, capPairs, 0, stream))) return rc;
  if ((rc = clGrow(h.chunk, 2 * capPairs, 0, stream))) return rc;
  if ((rc = clGrow(h.bnd, std::max<int64_t>((int64_t)bd.plan.bndDoubles(), 1), 0, stream))) return rc;
  if ((rc = clGrow(h.bandEdges, capPairs, 0, stream))) return rc;
  bd.dList = h.list.get(), bd.dChunk = h.chunk.get(), bd.dBnd = h.bnd.get(), bd.dEdges = h.bandEdges.get();
  bd.dEdgeCount = h.edgeCount;
  if (gated) {
    const int64_t words = *std::max_element(gateWords.begin(), gateWords.end());
    if (!h.gateBufs || words > h.gateWordsOpen) {        // (the gate sizes its long route by the longest pattern it was opened for)
      h.gateBufs.reset();
      h.gateBufs.reset(new ClGate);
      if ((rc = h.gateBufs->open(d.cus, words))) return rc;
      h.gateWordsOpen = words;
    }
    if ((rc = clGrow(h.surv, capPairs, 0, stream))) return rc;
    bd.dSurv = h.surv.get(), bd.gate = h.gateBufs.get();
  }

  PaCellMemo memo(maxO, maxO, h.band);
  for (int64_t lo = 0; lo < total; lo += capPairs) {
    const int64_t hi = std::min(total, lo + capPairs);
    int64_t colFirst, colEnd;
    dnas::clustererBandColumns(slotOff, g.segments, lo, hi, &colFirst, &colEnd);
    const int64_t tileFirst = colFirst / kCrTile, tiles = (colEnd - 1) / kCrTile - tileFirst + 1;
    rc = d.timed(&d.stats.filter_ms, [&] {
      clDispatchM(h.m, [&](auto mm) {
        hipLaunchKernelGGL(clusterer_filter_emit_kernel<decltype(mm)::value>, dim3((unsigned)tiles, (unsigned)g.segments),
                           dim3(64 * kCrWaves), 0, stream, n0, n1, d.dSig, d.dReadOff, h.minShared, tileFirst, (int)g.tilesPerSegment,
                           h.slotOff.get(), lo, hi, bd.dList);
      });
    });
    if (rc) return rc;
    const int64_t boundWords = gated ? *std::max_element(gateWords.begin() + colFirst, gateWords.begin() + colEnd) : 0;
    if ((rc = clRunBand(d, bd, memo, hi - lo, boundWords))) return rc;
  }
  return DNAS_OK;
}

// The checks of an add: nothing of the handle changes here.
int clustererCheckAdd(const dnas_clusterer& h, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off) {
  if (n_reads < 0) return dnas::fail(DNAS_E_INVALID, "clusterer add: bad argument");
  if (n_reads >= ((int64_t)1 << 31) - h.n()) return dnas::fail(DNAS_E_UNSUPPORTED, "clusterer add: 2^31 reads or more");
  if (n_reads == 0) return DNAS_OK;
  if (!read_seqs || !read_off) return dnas::fail(DNAS_E_INVALID, "clusterer add: null argument");
  if (read_off[0] != 0) return dnas::fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t O = read_off[i + 1] - read_off[i];
    if (O < 0) return dnas::fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": inconsistent offsets");
    if (O > dnas::kAlignMaxSeq)
      return dnas::fail(DNAS_E_UNSUPPORTED, "read " + std::to_string(i) + ": longer than " + std::to_string(dnas::kAlignMaxSeq));
  }
  for (int64_t q = 0; q < read_off[n_reads]; ++q)
    if (read_seqs[q] < 0 || read_seqs[q] > 3) return dnas::fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

template <class F>
int clustererGuarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

}  // namespace

extern "C" int dnas_clusterer_create(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                     double min_score_per_nt, int32_t max_edit_permille, int device_id, dnas_clusterer** out) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "clusterer create: null argument");
  *out = nullptr;
  if (const int rc = dnas::checkClusterArgs(params, band, k, m, min_shared, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (min_shared > m) return dnas::fail(DNAS_E_INVALID, "clusterer create: min_shared exceeds the sketch's positions");
  if (const int rc = dnas::checkClusterGate(max_edit_permille)) return rc;
  if (device_id == -1) return dnas::fail(DNAS_E_UNSUPPORTED, "clusterer create: a handle lives on one device, device_id = -1 is not supported");
  if (const int rc = dnas::checkDeviceId(device_id)) return rc;
  return clustererGuarded([&] {
    std::unique_ptr<dnas_clusterer> h(new dnas_clusterer{dnas::PairScores::from(dnas::MutatorParams::fromC(*params)), band, k, m, min_shared,
                                                         min_score_per_nt, max_edit_permille});
    h->d.device = device_id;
    *out = h.release();
    return (int)DNAS_OK;
  });
}

extern "C" int dnas_clusterer_add(dnas_clusterer* h, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                  dnas_cluster_stats* out_stats, dnas_cluster_gate_stats* out_gate) {
  if (out_stats) *out_stats = dnas_cluster_stats{};
  if (out_gate) *out_gate = dnas_cluster_gate_stats{};
  if (!h) return dnas::fail(DNAS_E_INVALID, "clusterer add: null handle");
  if (h->poisoned) return dnas::fail(DNAS_E_DEVICE, "clusterer: an earlier device error left the handle unusable");
  if (const int rc = clustererCheckAdd(*h, n_reads, read_seqs, read_off)) return rc;
  if (n_reads == 0) return DNAS_OK;
  const int64_t n0 = h->n();
  h->poisoned = true;                                    // until the add is complete
  const int rc = clustererGuarded([&] {
    h->readOff.reserve((size_t)(n0 + n_reads) + 1);
    const int64_t bases0 = h->readOff.back();
    for (int64_t q = 0; q < n_reads; ++q) h->readOff.push_back(bases0 + read_off[q + 1]);
    h->d.stats = dnas_cluster_stats{};
    h->d.gate = dnas_cluster_gate_stats{};
    h->d.edges.clear();
    if (const int rc = clustererAddOn(*h, n0, n_reads, read_seqs, read_off)) return rc;
    h->edges.insert(h->edges.end(), h->d.edges.begin(), h->d.edges.end());
    for (int64_t q = 0; q < n_reads; ++q) h->longest = std::max(h->longest, read_off[q + 1] - read_off[q]);
    dnas_cluster_stats& a = h->d.stats;
    a.pairs = dnas::clustererAddPairs(n0, n_reads);
    a.edges = (int64_t)h->d.edges.size();
    dnas_cluster_stats& t = h->stats;
    t.sketch_ms += a.sketch_ms, t.filter_ms += a.filter_ms, t.score_ms += a.score_ms, t.fold_ms += a.fold_ms;
    t.pairs += a.pairs, t.candidates += a.candidates, t.items += a.items, t.cells += a.cells, t.edges += a.edges, t.chunks += a.chunks;
    const dnas_cluster_gate_stats& ga = h->d.gate;
    dnas_cluster_gate_stats& gt = h->gate;
    gt.gate_ms += ga.gate_ms, gt.tested += ga.tested, gt.passed += ga.passed, gt.long_pairs += ga.long_pairs, gt.word_steps += ga.word_steps;
    if (out_stats) *out_stats = a;
    if (out_gate) *out_gate = ga;
    return (int)DNAS_OK;
  });
  if (rc == DNAS_OK) h->poisoned = false;
  return rc;
}

extern "C" int64_t dnas_clusterer_reads(const dnas_clusterer* h) { return h ? h->n() : 0; }

extern "C" int dnas_clusterer_result(dnas_clusterer* h, int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand, uint8_t* out_status,
                                     int64_t** out_edge_ij, double** out_edge_score, uint8_t** out_edge_strand, int64_t* out_n_edges,
                                     dnas_cluster_stats* out_stats, dnas_cluster_gate_stats* out_gate) {
  if (out_stats) *out_stats = dnas_cluster_stats{};
  if (out_gate) *out_gate = dnas_cluster_gate_stats{};
  if (!h) return dnas::fail(DNAS_E_INVALID, "clusterer result: null handle");
  if (h->poisoned) return dnas::fail(DNAS_E_DEVICE, "clusterer: an earlier device error left the handle unusable");
  const int64_t n = h->n();
  if (n > 0 && (!out_root || !out_cluster || !out_strand || !out_status)) return dnas::fail(DNAS_E_INVALID, "clusterer result: null argument");
  return clustererGuarded([&] {
    std::vector<dnas::ClusterEdge> edges = h->edges;
    if (n == 0) return dnas::clusterExportEdges(edges, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges);
    std::sort(edges.begin(), edges.end(), dnas::clusterEdgeLess);
    dnas_cluster_stats total = h->stats;
    total.pairs = n * (n - 1) / 2;
    total.clusters = dnas::clusterComponents(n, h->readOff.data(), h->k, h->minShared, edges, out_root, out_cluster, out_strand, out_status,
                                             &total.strand_conflicts);
    if (out_stats) *out_stats = total;
    if (out_gate) *out_gate = h->gate;
    return dnas::clusterExportEdges(edges, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges);
  });
}

extern "C" void dnas_clusterer_destroy(dnas_clusterer* h) {
  if (!h) return;
  if (h->opened) (void)hipSetDevice(h->d.device);
  delete h;
}
