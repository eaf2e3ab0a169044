"""Measures the edit-distance gate of dnas_cluster_reads_gated (csrc/cluster_gate_kernels.hip) with the method of
bench_cluster.py: its make_pool (ten reads of 205 - 235 nt per cluster), the CLI's default error model, band 32, the default
sketch; after a warm-up call the median of --calls timed calls, the arms of a case alternated in one run, every call returning
with its results in host memory, the spread as (max - min) / median.

  (a) N = 4 000 and (b) N = 20 000.  clusterReads(max_edit_permille=300) against clusterReads() in the same run.  Condition of
      record: both arms return the planted partition with equal edges, and the slowest gated call is faster than the fastest
      ungated call.  Reported: gate_ms, score_ms, filter_ms, passed per read, word_steps / gate_ms.  No target ratio.
  (c) N = 100 000 (--large), gated only, reported.  The ungated arm was never run at this size (an estimated minute of score
      kernel) and is not run here.
  (r) The register route against the long route at these read lengths (4 words): editDistances over the candidates of the
      N = 4 000 pool as shipped and with DNAS_CLUSTER_GATE_WORDS=0, alternated.  Reported: a baseline for the long route.

    python bench_cluster_gate.py [--cases abr] [--large 100000] [--calls 5] [--scale 1.0]

prints one JSON line per case and a last line with the verdict."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_cluster import BAND, make_pool, med, partition, spread  # noqa: E402

PERMILLE = 300


def case_gate(da, name, n, calls):
    params = da.MutatorParams.fromFlags()
    reads, truth = make_pool(da, n)
    gated = lambda: da.clusterReads(params, reads, band=BAND, edges=True, max_edit_permille=PERMILLE)
    plain = lambda: da.clusterReads(params, reads, band=BAND, edges=True)
    g, u = gated(), plain()                                  # warm-up: code objects, the allocator
    t_g, t_u, gs, us = [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        g = gated()
        t_g.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        u = plain()
        t_u.append(time.perf_counter() - t0)
        gs.append(dict(g.stats, **g.gate))
        us.append(u.stats)
    pick = lambda runs, key: med([r[key] for r in runs])
    same_edges = all(a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                           b.view(np.uint64) if b.dtype == np.float64 else b)
                     for a, b in zip(g.edges, u.edges))
    planted = partition(g.cluster) == partition(truth) and partition(u.cluster) == partition(truth)
    return dict(case=name, reads=n, calls=calls, permille=PERMILLE, gated_call_s=med(t_g), gated_call_spread=spread(t_g), gated_call_max_s=max(t_g),
                ungated_call_s=med(t_u), ungated_call_spread=spread(t_u), ungated_call_min_s=min(t_u), call_ratio=med(t_u) / med(t_g),
                faster_beyond_spread=bool(max(t_g) < min(t_u)), planted_found_both=bool(planted), equal_edges=bool(same_edges),
                gate_ms=pick(gs, "gate_ms"), gated_score_ms=pick(gs, "score_ms"), gated_filter_ms=pick(gs, "filter_ms"),
                ungated_score_ms=pick(us, "score_ms"), ungated_filter_ms=pick(us, "filter_ms"), candidates=g.stats["candidates"],
                tested=g.gate["tested"], passed=g.gate["passed"], passed_per_read=g.gate["passed"] / n, edges=g.stats["edges"],
                long_pairs=g.gate["long_pairs"], word_steps=g.gate["word_steps"],
                word_steps_per_s=g.gate["word_steps"] / (pick(gs, "gate_ms") / 1e3), gated_chunks=g.stats["chunks"])


def case_large(da, n, calls):
    params = da.MutatorParams.fromFlags()
    t0 = time.perf_counter()
    reads, truth = make_pool(da, n)
    made = time.perf_counter() - t0
    da.clusterReads(params, reads[:2000], band=BAND, max_edit_permille=PERMILLE)   # warm-up
    runs, walls = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        found = da.clusterReads(params, reads, band=BAND, max_edit_permille=PERMILLE)
        walls.append(time.perf_counter() - t0)
        runs.append(dict(found.stats, **found.gate))
    pick = lambda key: med([r[key] for r in runs])
    st = runs[-1]
    return dict(case="c", reads=n, calls=calls, permille=PERMILLE, ungated="not run", pool_made_s=made, call_s=med(walls),
                call_spread=spread(walls) if calls > 1 else None, sketch_ms=pick("sketch_ms"), filter_ms=pick("filter_ms"),
                gate_ms=pick("gate_ms"), score_ms=pick("score_ms"), fold_ms=pick("fold_ms"), candidates=st["candidates"],
                passed=st["passed"], passed_per_read=st["passed"] / n, edges=st["edges"], chunks=st["chunks"], word_steps=st["word_steps"],
                word_steps_per_s=st["word_steps"] / (pick("gate_ms") / 1e3), clusters=st["clusters"], planted=len(set(truth)),
                planted_found=partition(found.cluster) == partition(truth))


def case_routes(da, calls, scale):
    """Wall time of editDistances (upload, kernels, download) over the candidates of the pool of (a), per route."""
    n = max(40, int(4000 * scale))
    params = da.MutatorParams.fromFlags()
    reads, _ = make_pool(da, n)
    pairs = da.clusterReads(params, reads, band=BAND, edges=True, min_score_per_nt=float("-inf")).edges[0]   # every candidate
    steps = sum(2 * ((min(len(reads[i]), len(reads[j])) + 63) // 64) * max(len(reads[i]), len(reads[j])) for i, j in pairs)

    def run(words):
        if words is None:
            os.environ.pop("DNAS_CLUSTER_GATE_WORDS", None)
        else:
            os.environ["DNAS_CLUSTER_GATE_WORDS"] = str(words)
        t0 = time.perf_counter()
        out = da.editDistances(reads, pairs)
        return time.perf_counter() - t0, out
    (_, regs), (_, long) = run(None), run(0)
    t_r, t_l = [], []
    for _ in range(calls):
        t_r.append(run(None)[0])
        t_l.append(run(0)[0])
    os.environ.pop("DNAS_CLUSTER_GATE_WORDS", None)
    return dict(case="r", reads=n, pairs=len(pairs), calls=calls, word_steps=steps, routes_agree=bool(np.array_equal(regs, long)),
                register_call_s=med(t_r), register_call_spread=spread(t_r), long_call_s=med(t_l), long_call_spread=spread(t_l),
                long_over_register=med(t_l) / med(t_r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abr")
    ap.add_argument("--large", default="", help="comma-separated pool sizes of (c), e.g. 100000")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--large-calls", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the reads of (a), (b) and (r) (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    lines = []
    for case in args.cases:
        if case == "r":
            lines.append(case_routes(da, args.calls, args.scale))
        else:
            lines.append(case_gate(da, case, max(40, int({"a": 4000, "b": 20000}[case] * args.scale)), args.calls))
        print(json.dumps(lines[-1]), flush=True)
    for n in [int(x) for x in args.large.split(",") if x]:
        print(json.dumps(case_large(da, n, args.large_calls)), flush=True)
    ab = [x for x in lines if x["case"] in "ab"]
    verdict = dict(condition="(a), (b): both arms return the planted partition with equal edges, and every timed gated call is faster than "
                             "every timed ungated call",
                   met=bool(all(x["faster_beyond_spread"] and x["planted_found_both"] and x["equal_edges"] for x in ab)) if ab else None,
                   call_ratios={x["case"]: x["call_ratio"] for x in ab})
    print(json.dumps(verdict), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
