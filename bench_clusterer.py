"""Measures the persistent clusterer (dnas_clusterer_*, csrc/clusterer_kernels.hip): what it costs to add a batch of reads to a
pool that is already clustered, against clustering the grown pool again from nothing.

The pools of bench_cluster.py (make_pool: ten reads per cluster, 205 - 235 nt, shuffled), the CLI's default error model, the default
sketch, band 32, the edit-distance gate at 300 thousandths.  One warm-up, then --calls timed calls per arm, the arms alternated in
one run, every call ending with its results (the partition and the edge list) in host memory.

  row 1  (A) a handle already holds 20 000 reads (made before the clock starts): the add of 2 000 more, plus result.
         (B) the only route there was before: clusterReads on all 22 000.
         Condition: both arms return the same partition and edges, and the slowest A is faster than the fastest B.
  row 2  the handle fed the 22 000 reads in 11 adds of 2 000, plus result, against one one-shot call: what batching costs.
         Reported only.

    python bench_clusterer.py [--calls 5] [--scale 1.0]

prints one JSON line per row and a last line with the verdict."""
import argparse
import json
import sys
import time

import numpy as np

from bench_cluster import BAND, make_pool, med, spread

HELD, BATCH = 20000, 2000
PERMILLE = 300
KERNEL_MS = ("sketch_ms", "filter_ms", "score_ms", "fold_ms")


def same(a, b):
    """Two ReadClusters with edges: the partition, the strands and the edge list with its score bits."""
    return bool(all(np.array_equal(getattr(a, key), getattr(b, key)) for key in ("root", "cluster", "strand", "status"))
                and all(x.shape == y.shape and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                              y.view(np.uint64) if y.dtype == np.float64 else y)
                        for x, y in zip(a.edges, b.edges))
                and all(a.stats[key] == b.stats[key] for key in ("pairs", "candidates", "items", "cells", "edges", "clusters", "strand_conflicts"))
                and all(a.gate[key] == b.gate[key] for key in ("tested", "passed", "long_pairs", "word_steps")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the reads (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    held, batch = max(40, int(HELD * args.scale)), max(4, int(BATCH * args.scale))
    n = held + batch
    params = da.MutatorParams.fromFlags()
    reads, _ = make_pool(da, n)
    opts = dict(band=BAND, max_edit_permille=PERMILLE)

    def arm_a():
        h = da.Clusterer(params, **opts)
        h.add(reads[:held])
        t0 = time.perf_counter()
        add = h.add(reads[held:])
        found = h.result(edges=True)
        t = time.perf_counter() - t0
        h.close()
        return t, found, add

    def arm_b():
        t0 = time.perf_counter()
        found = da.clusterReads(params, reads, edges=True, **opts)
        return time.perf_counter() - t0, found

    def arm_batches():
        t0 = time.perf_counter()
        with da.Clusterer(params, **opts) as h:
            for at in range(0, n, batch):
                h.add(reads[at:at + batch])
            found = h.result(edges=True)
        return time.perf_counter() - t0, found

    arm_a(), arm_b(), arm_batches()                          # warm-up: code objects, the allocator
    t_a, t_b, t_c, t_d, adds, agree = [], [], [], [], [], True
    for _ in range(args.calls):
        t, found_a, add = arm_a()
        t_a.append(t)
        adds.append(add)
        t, found_b = arm_b()
        t_b.append(t)
        agree = agree and same(found_a, found_b)
    for _ in range(args.calls):
        t, found_c = arm_batches()
        t_c.append(t)
        t, found_d = arm_b()
        t_d.append(t)
        agree = agree and same(found_c, found_d)
    pick = lambda rows, key: med([r[key] for r in rows])
    st = found_b.stats
    row1 = dict(row=1, held=held, added=batch, calls=args.calls, add_result_s=med(t_a), add_result_spread=spread(t_a), add_result_max_s=max(t_a),
                one_shot_s=med(t_b), one_shot_spread=spread(t_b), one_shot_min_s=min(t_b), call_ratio=med(t_b) / med(t_a),
                add_pairs=adds[-1]["pairs"], add_candidates=adds[-1]["candidates"], add_passed=adds[-1]["gate"]["passed"],
                add_edges=adds[-1]["edges"], add_gate_ms=pick([a["gate"] for a in adds], "gate_ms"),
                one_shot_pairs=st["pairs"], one_shot_candidates=st["candidates"], one_shot_gate_ms=found_b.gate["gate_ms"],
                clusters=st["clusters"], arms_agree=agree, faster_beyond_spread=bool(max(t_a) < min(t_b)))
    row1.update({"add_" + key: pick(adds, key) for key in KERNEL_MS})
    row1.update({"one_shot_" + key: st[key] for key in KERNEL_MS})
    print(json.dumps(row1), flush=True)
    row2 = dict(row=2, reads=n, adds=-(-n // batch), calls=args.calls, batched_s=med(t_c), batched_spread=spread(t_c), one_shot_s=med(t_d),
                one_shot_spread=spread(t_d), batched_over_one_shot=med(t_c) / med(t_d), batched_gate_ms=found_c.gate["gate_ms"])
    row2.update({"batched_" + key: found_c.stats[key] for key in KERNEL_MS})
    print(json.dumps(row2), flush=True)
    print(json.dumps(dict(condition="both arms return the same partition and edges, and every timed add + result on a handle that holds "
                                    "%d reads is faster than every timed clusterReads call on all %d" % (held, n),
                          met=bool(row1["arms_agree"] and row1["faster_beyond_spread"]), call_ratio=row1["call_ratio"])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
