"""Measures dnas_consensus_score (consensus by rescoring, csrc/consensus_kernels.hip) against the route the library offered for
the same job before it, and where the time of ViterbiDecoder.decode_clusters goes.

rescore   20 000 clusters x 10 reads x 4 candidates of 150 nt, band 16, the error model with the rates below (P = 6).  A
          cluster's candidates are its strand and three near copies of it (what reads with an error or two decode to), its reads
          the strand after substitutions, deletions and tandem copies at those rates.  A few hundred distinct clusters are
          tiled to that number (making them all in Python would take longer than the measurement).
            consensus_*  dnas_consensus_score: items/s over the host clock around the call -- copies in, kernels, copies out --
                         and band cells/s over score_ms of dnas_consensus_stats (HIP events around the score kernel);
            assign_*     the other arm: dnas_assign_reads with the cluster's candidates as every read's candidate list and
                         out_item_scores, which copies one score per (read, candidate) to the host, plus the sums in read
                         order and the pick in numpy; cells/s over score_ms of dnas_assign_stats.
          The arms are timed alternately, --calls times after a warm-up call; medians.  Winners, totals and runners-up of the two
          arms are compared bit for bit.  The condition of record: per item the new call is not slower than the old route by
          more than the larger of the two arms' spreads, (max - min) / median of their timed calls, and neither is the score
          kernel's cells/s against assign_score_kernel's.
decode    ViterbiDecoder.decode_clusters on the headline machine (s16h74l4c4.json, 29-byte payloads, reads of about 490 nt
          with 1 % substitutions, every other one reverse-complemented), clusters of 5 reads, both strands, band 32: the
          share of the call's wall time spent in the Viterbi decode, in making the candidates (encode and dedup) and in
          rescoring, from dnas_consensus_stats.  No condition.

    python bench_consensus.py [--parts rd] [--calls 5] [--scale 1.0] [--decode-clusters 400]

prints one JSON line per part and, after rescore, a line with the verdict."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

RESCORE = dict(clusters=20000, reads=10, candidates=4, nt=150, band=16, distinct=250)
RATES = dict(sub=.03, dup=.02, del_open=.02, del_ext=.2)


def mutate(rng, src, p_del=.02, p_sub=.03, p_dup=.02):
    out = []
    for i, c in enumerate(src):
        r = rng.random()
        if r < p_del:
            continue
        out.append(int(rng.choice([b for b in range(4) if b != c])) if rng.random() < p_sub else int(c))
        if r < p_del + p_dup and i >= 3:
            out.extend(int(b) for b in src[i + 1 - rng.randint(1, 3):i + 1])
    return np.array(out, np.int8)


def make_clusters(n):
    """-> (candidates, reads): per cluster RESCORE['candidates'] strands and RESCORE['reads'] reads, as int8 arrays."""
    cfg = RESCORE
    rng = random.Random("bench-consensus/rescore")
    uniq = []
    for _ in range(min(n, cfg["distinct"])):
        a = np.array([rng.randrange(4) for _ in range(cfg["nt"])], np.int8)
        cands = [a] + [mutate(rng, a, .005, .01, .005) for _ in range(cfg["candidates"] - 1)]
        rng.shuffle(cands)
        uniq.append((cands, [mutate(rng, a) for _ in range(cfg["reads"])]))
    return [uniq[i % len(uniq)][0] for i in range(n)], [uniq[i % len(uniq)][1] for i in range(n)]


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


class ConsensusArm:
    def __init__(self, params, cands, reads, band):
        from dnastore_amd import lib as _l
        self.L, self.params, self.band = _l.lib(), params, band
        self.nc = len(cands)
        self.cl_cand = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
        self.cl_read = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        self.cand, self.cand_off = concat([x for c in cands for x in c])
        self.reads, self.read_off = concat([x for r in reads for x in r])
        self.n_cand, self.n_reads = len(self.cand_off) - 1, len(self.read_off) - 1
        self.winner, self.status = np.zeros(self.nc, np.int64), np.zeros(self.nc, np.uint8)
        self.total, self.second = np.zeros(self.nc), np.zeros(self.nc)
        self.stats = _l.ConsensusStatsC()

    def call(self):
        from dnastore_amd import lib as _l
        _l.check(self.L.dnas_consensus_score(ctypes.byref(self.params.c), self.band, self.nc, self.n_cand, self.cand.ctypes.data,
                                             self.cand_off.ctypes.data, self.cl_cand.ctypes.data, self.n_reads, self.reads.ctypes.data,
                                             self.read_off.ctypes.data, None, self.cl_read.ctypes.data, 0, self.winner.ctypes.data,
                                             self.total.ctypes.data, self.second.ctypes.data, self.status.ctypes.data, None,
                                             ctypes.byref(self.stats)))


class AssignArm:
    """The route before dnas_consensus_score: every candidate an original, every read with its cluster's candidates as its list,
    the item scores copied out, summed per candidate in read order and picked in numpy."""

    def __init__(self, new, n_per_cluster_cands, n_per_cluster_reads):
        from dnastore_amd import lib as _l
        self.L, self.new = _l.lib(), new
        self.C, self.R = n_per_cluster_cands, n_per_cluster_reads
        n = new.n_reads
        self.cand_off = (np.arange(n + 1, dtype=np.int64) * self.C)
        cluster_of_read = np.repeat(np.arange(new.nc, dtype=np.int64), self.R)
        self.cand_idx = np.ascontiguousarray((cluster_of_read[:, None] * self.C + np.arange(self.C, dtype=np.int64)[None, :]).reshape(-1))
        self.original, self.strand, self.status = np.zeros(n, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.score, self.second_read = np.zeros(n), np.zeros(n)
        self.items = np.zeros(n * self.C)
        self.stats = _l.AssignStatsC()

    def call(self):
        from dnastore_amd import lib as _l
        new = self.new
        _l.check(self.L.dnas_assign_reads(ctypes.byref(new.params.c), new.band, new.n_cand, new.cand.ctypes.data, new.cand_off.ctypes.data,
                                          new.n_reads, new.reads.ctypes.data, new.read_off.ctypes.data, _l.STRAND_FORWARD,
                                          self.cand_off.ctypes.data, self.cand_idx.ctypes.data, 0, self.original.ctypes.data,
                                          self.strand.ctypes.data, self.score.ctypes.data, self.second_read.ctypes.data,
                                          self.status.ctypes.data, self.items.ctypes.data, ctypes.byref(self.stats)))
        sc = self.items.reshape(new.nc, self.R, self.C)
        totals = np.zeros((new.nc, self.C))
        for i in range(self.R):                                         # left to right in read order, from 0.0
            totals += sc[:, i, :]
        first = np.argmax(totals, axis=1)                               # the first of equal maxima: the first strictly greater
        rows = np.arange(new.nc)
        self.total = totals[rows, first]
        self.winner = np.where(self.total > -np.inf, first + rows * self.C, -1)
        others = totals.copy()
        others[rows, first] = -np.inf
        self.second = np.where(self.winner >= 0, others.max(axis=1), -np.inf)


def run_rescore(calls, scale):
    import dnastore_amd as da
    cfg = RESCORE
    n = max(8, int(cfg["clusters"] * scale))
    params = da.MutatorParams.fromFlags(**RATES)
    cands, reads = make_clusters(n)
    new = ConsensusArm(params, cands, reads, cfg["band"])
    old = AssignArm(new, cfg["candidates"], cfg["reads"])
    new.call()                                                          # warm-up: code objects, the allocator
    old.call()
    t_new, t_old, new_ms, new_fold, old_ms, old_fold = [], [], [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        new.call()
        t_new.append(time.perf_counter() - t0)
        new_ms.append(new.stats.score_ms)
        new_fold.append(new.stats.fold_ms)
        t0 = time.perf_counter()
        old.call()
        t_old.append(time.perf_counter() - t0)
        old_ms.append(old.stats.score_ms)
        old_fold.append(old.stats.fold_ms)
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    same = bool(np.array_equal(new.winner, old.winner) and np.array_equal(bits(new.total), bits(old.total)) and
                np.array_equal(bits(new.second), bits(old.second)))
    items, cells = int(new.stats.items), int(new.stats.cells)
    med = statistics.median
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)
    margin = max(spread(t_new), spread(t_old))
    k_margin = max(spread(new_ms), spread(old_ms))
    out = dict(part="rescore", clusters=n, reads_per_cluster=cfg["reads"], candidates_per_cluster=cfg["candidates"], nt=cfg["nt"],
               band=cfg["band"], calls=calls, items=items, band_cells=cells, chunks=int(new.stats.chunks),
               assign_items=int(old.stats.items), assign_band_cells=int(old.stats.cells),
               consensus_call_s=med(t_new), consensus_call_items_per_s=items / med(t_new), consensus_call_spread=spread(t_new),
               consensus_score_ms=med(new_ms), consensus_fold_ms=med(new_fold), consensus_score_cells_per_s=cells / (med(new_ms) / 1e3),
               consensus_score_spread=spread(new_ms),
               assign_call_s=med(t_old), assign_call_items_per_s=int(old.stats.items) / med(t_old), assign_call_spread=spread(t_old),
               assign_score_ms=med(old_ms), assign_fold_ms=med(old_fold),
               assign_score_cells_per_s=int(old.stats.cells) / (med(old_ms) / 1e3), assign_score_spread=spread(old_ms),
               results_equal=same)
    out["call_ratio"] = out["consensus_call_items_per_s"] / out["assign_call_items_per_s"]
    out["kernel_cells_ratio"] = out["consensus_score_cells_per_s"] / out["assign_score_cells_per_s"]
    out["call_not_slower"] = bool(out["call_ratio"] >= 1 - margin)
    out["kernel_not_slower"] = bool(out["kernel_cells_ratio"] >= 1 - k_margin)
    return out


def run_decode(n_clusters, calls):
    import dnastore_amd as da
    machine = da.Machine.fromFile(os.path.join(ROOT, "tests", "golden", "ref_data", "s16h74l4c4.json"))
    params = da.MutatorParams.fromFlags(global_=True)
    rng = random.Random("bench-consensus/decode")
    nrng = np.random.default_rng(20261017)
    reads, labels, strands = [], [], []
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    for k in range(n_clusters):
        dna = np.frombuffer(machine.encodeBytes(bytes(rng.randrange(256) for _ in range(29))).encode(), dtype=np.uint8)
        strands.append(dna.tobytes().decode())
        for i in range(5):
            b = dna.copy()
            hit = nrng.random(len(b)) < .01
            cur = np.array([code[int(c)] for c in b[hit]], dtype=np.int64)
            b[hit] = letters[(cur + nrng.integers(1, 4, size=cur.size)) % 4]
            r = b.tobytes().decode()
            reads.append(da.reverse_complement(r) if i % 2 else r)
            labels.append(k)
    dec = da.ViterbiDecoder(machine, params, device=0)
    dec.decode_clusters(reads, labels, strands="both", band=32)         # warm-up
    walls, parts = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = dec.decode_clusters(reads, labels, strands="both", band=32)
        walls.append(time.perf_counter() - t0)
        parts.append(res.stats)
    right = sum(machine.encodeSymbols(s) == strands[k] if s else False for k, s in enumerate(res.symbols))
    single = sum(machine.encodeSymbols(s) == strands[i // 5] if s else False for i, s in enumerate(res.per_read[0]))
    dec.close()
    med = statistics.median
    d, c, r = (med([p[k] for p in parts]) for k in ("decode_wall_ms", "candidates_wall_ms", "rescore_wall_ms"))
    return dict(part="decode", machine="s16h74l4c4.json", clusters=n_clusters, reads=len(reads), mean_read_nt=sum(map(len, reads)) / len(reads),
                calls=calls, call_s=med(walls), clusters_per_s=n_clusters / med(walls), decode_wall_ms=d, candidates_wall_ms=c,
                rescore_wall_ms=r, decode_share=d / (d + c + r), candidates_share=c / (d + c + r), rescore_share=r / (d + c + r),
                candidates=int(res.stats["candidates"]), items=int(res.stats["items"]), score_ms=med([p["score_ms"] for p in parts]),
                clusters_right=int(right), single_reads_right=int(single))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="rd", help="r = rescore, d = decode")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the rescore part's clusters (a rehearsal)")
    ap.add_argument("--decode-clusters", type=int, default=400)
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    ok = True
    if "r" in args.parts:
        line = run_rescore(args.calls, args.scale)
        print(json.dumps(line), flush=True)
        verdict = dict(condition="per item dnas_consensus_score is not slower than dnas_assign_reads + item scores + numpy sums by more than "
                                 "the larger spread of the two arms' timed calls, and consensus_score_kernel's cells/s not lower than "
                                 "assign_score_kernel's by more than the larger spread of the two kernels' times",
                       met=bool(line["call_not_slower"] and line["kernel_not_slower"]), call_ratio=line["call_ratio"],
                       kernel_cells_ratio=line["kernel_cells_ratio"], results_equal=line["results_equal"])
        print(json.dumps(verdict), flush=True)
        ok = line["results_equal"]
    if "d" in args.parts:
        print(json.dumps(run_decode(args.decode_clusters, args.calls)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
