"""Measures dnas_cluster_reads (clustering a pool of reads, csrc/cluster_kernels.hip).

Seeded pools made like pool A of tests/test_cluster_cpu.py, ten reads per cluster: per cluster a random 16-byte payload encoded
on h74l4c4.json, per read synth.mutate(strand, sub=.01, dele=.005, dup=.005), reverse-complemented with probability 1/2; reads
of 205 - 235 nt, shuffled.  The CLI's default error model, band 32.  After a warm-up call, the median of --calls timed calls,
the arms of a case alternated, every call returning with its results in host memory.

  (a) N = 4 000.  clusterReads with the defaults against the only route the library offered before: assignReads(params, reads,
      reads, strands="both") with every item's score, then the floor and a union on the host.  Condition: the slowest new call is
      faster than the fastest call of the other arm.
  (b) N = 1 000, min_shared = 0 (every pair is scored).  cluster_score_kernel's band cells per second (cells / score_ms) against
      assign_score_kernel's in the same run, on the same items: assignReads(params, reads, reads, strands="both") with read j's
      candidates the reads i < j.  (Against all N x N x 2 items the assign kernel has twice as many items per wave, and the
      uneven last round of the grid-stride loop and the tail of the launch weigh half as much: 0.25 % against 0.5 % here.)  The
      cell body is shared; condition: not below it by more than the larger (max - min) / median spread of the two.
      Measured with the assign arm over all 2 M items, before it was given the same items: 113.80 against 114.57 G cells/s,
      ratio 0.9933 with spreads of 0.21 % -- the condition missed; with the same items: not measured yet.
  (c) N = 20 000 and 100 000 (--large), reported only: sketch_ms, filter_ms, score_ms, fold_ms, candidates per read, clusters found
      against those planted -- where the N^2 filter starts to dominate.

    python bench_cluster.py [--cases ab] [--large 20000,100000] [--calls 5] [--scale 1.0]

prints one JSON line per case and a last line with the verdict."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MACHINE = os.path.join(ROOT, "tests", "golden", "ref_data", "h74l4c4.json")
PER_CLUSTER = 10
BAND = 32


def make_pool(da, n):
    """-> (reads, planted cluster of every read)."""
    import synth
    machine = da.Machine.fromFile(MACHINE)
    rng = random.Random("bench-cluster/%d" % n)
    reads, truth = [], []
    for c in range((n + PER_CLUSTER - 1) // PER_CLUSTER):
        strand = machine.encodeBytes(bytes(rng.randrange(256) for _ in range(16)))
        for _ in range(PER_CLUSTER):
            read = synth.mutate(strand, rng, sub=.01, dele=.005, dup=.005)
            reads.append(da.reverse_complement(read) if rng.random() < .5 else read)
            truth.append(c)
    order = list(range(len(reads)))
    rng.shuffle(order)
    order = order[:n]
    return [da.tokenize(reads[i]).astype(np.int8) for i in order], [truth[i] for i in order]


def partition(labels):
    groups = {}
    for i, lab in enumerate(labels):
        groups.setdefault(int(lab), []).append(i)
    return sorted(groups.values())


def union_of_assign(res, n, lens, floor=0.0):
    """The other arm's second half: every (i, j, strand) score of assignReads(reads, reads) -> edges i < j at the floor -> labels."""
    sc = np.stack(res.item_scores).reshape(n, n, 2)          # [read j][original i][strand]
    best = sc.max(axis=2)
    j, i = np.nonzero((best >= floor * lens[:, None]) & (np.arange(n)[None, :] < np.arange(n)[:, None]))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return [find(x) for x in range(n)]


med = statistics.median
spread = lambda xs: (max(xs) - min(xs)) / med(xs)


def case_a(da, calls, scale):
    n = max(40, int(4000 * scale))
    params = da.MutatorParams.fromFlags()
    reads, truth = make_pool(da, n)
    lens = np.array([len(r) for r in reads], np.float64)
    new = lambda: da.clusterReads(params, reads, band=BAND)
    old = lambda: union_of_assign(da.assignReads(params, reads, reads, band=BAND, strands="both", item_scores=True), n, lens)
    found, labels = new(), old()                             # warm-up: code objects, the allocator
    t_new, t_old = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        found = new()
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        labels = old()
        t_old.append(time.perf_counter() - t0)
    st = found.stats
    return dict(case="a", reads=n, calls=calls, cluster_call_s=med(t_new), cluster_call_spread=spread(t_new), cluster_call_max_s=max(t_new),
                assign_union_call_s=med(t_old), assign_union_call_spread=spread(t_old), assign_union_call_min_s=min(t_old),
                call_ratio=med(t_old) / med(t_new), faster_beyond_spread=bool(max(t_new) < min(t_old)),
                sketch_ms=st["sketch_ms"], filter_ms=st["filter_ms"], score_ms=st["score_ms"], fold_ms=st["fold_ms"],
                candidates=st["candidates"], pairs=st["pairs"], edges=st["edges"], clusters=st["clusters"],
                planted=len(set(truth)), planted_found=partition(found.cluster) == partition(truth),
                arms_agree=partition(found.cluster) == partition(labels))


def case_b(da, calls, scale):
    n = max(40, int(1000 * scale))
    params = da.MutatorParams.fromFlags()
    reads, truth = make_pool(da, n)
    new = lambda: da.clusterReads(params, reads, band=BAND, min_shared=0)
    below = [list(range(j)) for j in range(n)]
    old = lambda: da.assignReads(params, reads, reads, band=BAND, strands="both", candidates=below)
    new(), old()
    c_rate, a_rate = [], []
    for _ in range(calls):
        st = new().stats
        c_rate.append(st["cells"] / (st["score_ms"] / 1e3))
        found = st
        st = old().stats
        a_rate.append(st["cells"] / (st["score_ms"] / 1e3))
    allowed = max(spread(c_rate), spread(a_rate))
    return dict(case="b", reads=n, calls=calls, cluster_items=found["items"], cluster_cells=found["cells"], assign_items=st["items"],
                assign_cells=st["cells"], cluster_score_cells_per_s=med(c_rate), cluster_score_spread=spread(c_rate),
                assign_score_cells_per_s=med(a_rate), assign_score_spread=spread(a_rate), score_ratio=med(c_rate) / med(a_rate),
                level_within_spread=bool(med(c_rate) >= med(a_rate) * (1 - allowed)))


def case_large(da, n, calls):
    params = da.MutatorParams.fromFlags()
    t0 = time.perf_counter()
    reads, truth = make_pool(da, n)
    made = time.perf_counter() - t0
    da.clusterReads(params, reads[:2000], band=BAND)           # warm-up
    runs, walls = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        found = da.clusterReads(params, reads, band=BAND)
        walls.append(time.perf_counter() - t0)
        runs.append(found.stats)
    pick = lambda key: med([r[key] for r in runs])
    st = runs[-1]
    return dict(case="c", reads=n, calls=calls, pool_made_s=made, call_s=med(walls), call_spread=spread(walls) if calls > 1 else None,
                sketch_ms=pick("sketch_ms"), filter_ms=pick("filter_ms"), score_ms=pick("score_ms"), fold_ms=pick("fold_ms"),
                pairs=st["pairs"], candidates=st["candidates"], candidates_per_read=st["candidates"] / n, edges=st["edges"],
                chunks=st["chunks"], clusters=st["clusters"], planted=len(set(truth)), strand_conflicts=st["strand_conflicts"],
                planted_found=partition(found.cluster) == partition(truth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ab")
    ap.add_argument("--large", default="", help="comma-separated pool sizes of (c), e.g. 20000,100000")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--large-calls", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the reads of (a) and (b) (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    lines = []
    for case in args.cases:
        lines.append({"a": case_a, "b": case_b}[case](da, args.calls, args.scale))
        print(json.dumps(lines[-1]), flush=True)
    for n in [int(x) for x in args.large.split(",") if x]:
        print(json.dumps(case_large(da, n, args.large_calls)), flush=True)
    by = {x["case"]: x for x in lines}
    verdict = dict(condition="(a) every timed clusterReads call faster than every timed assignReads + union call; (b) cluster_score_kernel's "
                             "cells/s not below assign_score_kernel's by more than the larger spread",
                   met=bool(by["a"]["faster_beyond_spread"] and by["b"]["level_within_spread"]) if len(by) == 2 else None,
                   call_ratio=by.get("a", {}).get("call_ratio"), score_ratio=by.get("b", {}).get("score_ratio"))
    print(json.dumps(verdict), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
