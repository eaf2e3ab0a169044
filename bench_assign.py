"""Measures dnas_assign_reads (read assignment, csrc/assign_kernels.hip) against what the library offered for the same job
before it: dnas_align_pairs on the (read, original, strand) list expanded on the host, plus a numpy fold.

Seeded pools, the CLI's default error model with the rates below (P = 6); every read is an original after substitutions,
deletions and tandem copies at those rates, in case (a) every other one reverse-complemented:
  (a) 20 000 reads x 256 originals of 150 nt, band 16, both strands      (b) 2 000 reads x 64 originals of 1 000 nt, band 32, forward
A few distinct reads per original are tiled to those numbers (making them all in Python would take longer than the measurement).

Per case, after a warm-up call, the median of --calls timed calls, each returning with the results in host memory:
  assign_call_*    items/s and band cells/s over the host clock around dnas_assign_reads -- handle, copies in, kernels, copies out;
  assign_kernel_*  the same over score_ms + fold_ms of dnas_assign_stats (HIP events around the kernels only);
  score_cells_per_s  band cells over score_ms alone: the score kernel against ...
  fill_cells_per_s   ... pair_align_fill_kernel, band cells over fill_ms of the other arm, in the same run;
  expand_call_*    the other arm: dnas_align_pairs over the expanded list of the first reads/--expand-share reads (the whole list
                   of (a) is 10 M pairs, 3 GB of op slots on the host and a 6 GB arena per 100 000 pairs in HBM) plus the fold in
                   numpy, per item; the expansion itself (expand_s) is outside the clock.
The two arms are timed alternately.  Their results are compared bit for bit on the reads both saw.  The condition of record:
assign_call_items_per_s > expand_call_items_per_s by more than the spread of the timed calls on (a) and (b), and
score_cells_per_s >= fill_cells_per_s.

    python bench_assign.py [--cases ab] [--calls 5] [--scale 1.0] [--expand-share 8]

prints one JSON line per case and a last line with the verdict."""
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

CASES = {"a": dict(reads=20000, originals=256, nt=150, band=16, strands="both", variants=8, share=8),
         "b": dict(reads=2000, originals=64, nt=1000, band=32, strands="forward", variants=4, share=1)}
RATES = dict(sub=.03, dup=.02, del_open=.02, del_ext=.2)


def mutate(rng, src):
    out = []
    for i, c in enumerate(src):
        r = rng.random()
        if r < .02:
            continue
        out.append(int(rng.choice([b for b in range(4) if b != c])) if rng.random() < .03 else int(c))
        if r < .04 and i >= 3:
            out.extend(int(b) for b in src[i + 1 - rng.randint(1, 3):i + 1])
    return np.array(out, np.int8)


def make_pool(case, n):
    cfg = CASES[case]
    rng = random.Random("bench-assign/" + case)
    originals = [np.array([rng.randrange(4) for _ in range(cfg["nt"])], np.int8) for _ in range(cfg["originals"])]
    uniq = []
    for v in range(cfg["variants"]):
        for k, a in enumerate(originals):
            b = mutate(rng, a)
            if cfg["strands"] == "both" and (k + v) % 2:
                b = (3 - b[::-1]).astype(np.int8)
            uniq.append(b)
    order = list(range(len(uniq)))
    rng.shuffle(order)
    return originals, [uniq[order[i % len(order)]] for i in range(n)]


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.ascontiguousarray(np.concatenate(seqs)), off


class AssignArm:
    def __init__(self, params, originals, reads, band, strands):
        from dnastore_amd import lib as _l
        self.L, self.params, self.band, self.mode = _l.lib(), params, band, _l.strand_mode(strands)
        self.K, self.n = len(originals), len(reads)
        self.orig, self.orig_off = concat(originals)
        self.reads, self.read_off = concat(reads)
        self.original = np.zeros(self.n, np.int64)
        self.strand, self.status = np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        self.score, self.second = np.zeros(self.n), np.zeros(self.n)
        self.stats = _l.AssignStatsC()

    def call(self):
        from dnastore_amd import lib as _l
        _l.check(self.L.dnas_assign_reads(ctypes.byref(self.params.c), self.band, self.K, self.orig.ctypes.data, self.orig_off.ctypes.data,
                                          self.n, self.reads.ctypes.data, self.read_off.ctypes.data, self.mode, None, None, 0,
                                          self.original.ctypes.data, self.strand.ctypes.data, self.score.ctypes.data,
                                          self.second.ctypes.data, self.status.ctypes.data, None, ctypes.byref(self.stats)))


class ExpandArm:
    """dnas_align_pairs over every (read, original, strand) of the reads given, then the fold in numpy."""

    def __init__(self, params, originals, reads, band, strands):
        from dnastore_amd import lib as _l
        t0 = time.perf_counter()
        self.L, self.params, self.band = _l.lib(), params, band
        self.K, self.n, self.s = len(originals), len(reads), 2 if strands == "both" else 1
        self.n_pairs = self.n * self.K * self.s
        block = np.concatenate([a for a in originals for _ in range(self.s)])
        self.ins = np.ascontiguousarray(np.tile(block, self.n))
        in_len = np.tile(np.repeat([len(a) for a in originals], self.s), self.n)
        per = [np.concatenate([b, (3 - b[::-1]).astype(np.int8)]) if self.s == 2 else b for b in reads]
        self.outs = np.ascontiguousarray(np.concatenate([np.tile(p, self.K) for p in per]))
        out_len = np.repeat([len(b) for b in reads], self.K * self.s)
        self.in_off, self.out_off = np.zeros(self.n_pairs + 1, np.int64), np.zeros(self.n_pairs + 1, np.int64)
        self.in_off[1:], self.out_off[1:] = np.cumsum(in_len), np.cumsum(out_len)
        self.ops_off = (self.in_off + self.out_off).astype(np.uint64)
        self.ops = np.zeros(int(self.ops_off[-1]) + 1, np.uint8)
        self.n_ops, self.pair_score = np.zeros(self.n_pairs, np.uint32), np.zeros(self.n_pairs)
        self.pair_status = np.zeros(self.n_pairs, np.uint8)
        self.stats = _l.AlignStatsC()
        self.expand_s = time.perf_counter() - t0

    def call(self):
        from dnastore_amd import lib as _l
        _l.check(self.L.dnas_align_pairs(ctypes.byref(self.params.c), self.band, self.n_pairs, self.ins.ctypes.data, self.in_off.ctypes.data,
                                         self.outs.ctypes.data, self.out_off.ctypes.data, 0, 0, self.ops.ctypes.data,
                                         self.ops_off.ctypes.data, self.n_ops.ctypes.data, self.pair_score.ctypes.data,
                                         self.pair_status.ctypes.data, ctypes.byref(self.stats)))
        sc = self.pair_score.reshape(self.n, self.K * self.s)
        first = np.argmax(sc, axis=1)                                   # the first of equal maxima: the first strictly greater
        self.score = sc[np.arange(self.n), first]
        self.original, self.strand = first // self.s, first % self.s
        others = sc.reshape(self.n, self.K, self.s).max(axis=2)
        others[np.arange(self.n), self.original] = -np.inf
        self.second = others.max(axis=1) if self.K > 1 else np.full(self.n, -np.inf)


def run_case(case, calls, scale, share):
    import dnastore_amd as da
    cfg = CASES[case]
    n = max(16, int(cfg["reads"] * scale))
    share = share or cfg["share"]
    params = da.MutatorParams.fromFlags(**RATES)
    originals, reads = make_pool(case, n)
    new = AssignArm(params, originals, reads, cfg["band"], cfg["strands"])
    old = ExpandArm(params, originals, reads[:max(1, n // share)], cfg["band"], cfg["strands"])
    new.call()                                                          # warm-up: code objects, the allocator
    old.call()
    t_new, t_old, score_ms, fold_ms, fill_ms, tb_ms = [], [], [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        new.call()
        t_new.append(time.perf_counter() - t0)
        score_ms.append(new.stats.score_ms)
        fold_ms.append(new.stats.fold_ms)
        t0 = time.perf_counter()
        old.call()
        t_old.append(time.perf_counter() - t0)
        fill_ms.append(old.stats.fill_ms)
        tb_ms.append(old.stats.traceback_ms)
    m = old.n
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    same = bool(np.array_equal(new.original[:m], old.original) and np.array_equal(new.strand[:m], old.strand) and
                np.array_equal(bits(new.score[:m]), bits(old.score)) and np.array_equal(bits(new.second[:m]), bits(old.second)))
    items, cells = int(new.stats.items), int(new.stats.cells)
    old_items, old_cells = old.n_pairs, int(old.stats.cells)
    med = statistics.median
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)
    out = dict(case=case, reads=n, originals=cfg["originals"], nt=cfg["nt"], band=cfg["band"], strands=cfg["strands"], calls=calls,
               items=items, band_cells=cells, chunks=int(new.stats.chunks),
               assign_call_s=med(t_new), assign_call_items_per_s=items / med(t_new), assign_call_cells_per_s=cells / med(t_new),
               assign_call_reads_per_s=n / med(t_new), assign_call_spread=spread(t_new),
               assign_kernel_items_per_s=items / (med([a + b for a, b in zip(score_ms, fold_ms)]) / 1e3),
               score_ms=med(score_ms), fold_ms=med(fold_ms), score_cells_per_s=cells / (med(score_ms) / 1e3),
               expand_reads=m, expand_share=share, expand_items=old_items, expand_s=old.expand_s, expand_batches=int(old.stats.batches),
               expand_call_s=med(t_old), expand_call_items_per_s=old_items / med(t_old), expand_call_spread=spread(t_old),
               fill_ms=med(fill_ms), traceback_ms=med(tb_ms), fill_cells_per_s=old_cells / (med(fill_ms) / 1e3),
               results_equal=same)
    out["call_ratio"] = out["assign_call_items_per_s"] / out["expand_call_items_per_s"]
    out["kernel_cells_ratio"] = out["score_cells_per_s"] / out["fill_cells_per_s"]
    out["faster_beyond_spread"] = bool(min(t_old) / old_items > max(t_new) / items)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ab")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every case's reads (a rehearsal)")
    ap.add_argument("--expand-share", type=int, default=0, help="the expanded arm takes reads / this (default: 8 for (a), 1 for (b))")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    lines = []
    for case in args.cases:
        lines.append(run_case(case, args.calls, args.scale, args.expand_share))
        print(json.dumps(lines[-1]), flush=True)
    verdict = dict(condition="per item, every timed assign call faster than every timed expanded call, and score_cells_per_s >= "
                             "fill_cells_per_s, on (a) and (b)",
                   met=all(x["faster_beyond_spread"] and x["kernel_cells_ratio"] >= 1 for x in lines) if len(lines) == 2 else None,
                   call_ratios={x["case"]: x["call_ratio"] for x in lines},
                   kernel_cells_ratios={x["case"]: x["kernel_cells_ratio"] for x in lines},
                   results_equal=all(x["results_equal"] for x in lines))
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["results_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
