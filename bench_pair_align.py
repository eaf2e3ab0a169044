"""Measures dnas_align_pairs (the pair-HMM Viterbi aligner, csrc/pair_align_kernels.hip) against its host statement.

Seeded pairs from tests/synth.py::synthetic_alignment (sub=.03, dele=.02, dup=.02), the CLI's default error model with those
rates (P = 6):
  (a) 100 000 pairs of 150 nt, band 16      (b) 4 000 pairs of 1 000 nt, band 32      (c) 2 000 pairs of 300 nt, full matrix
A few thousand distinct pairs are tiled to those numbers (making them all in Python would take longer than the measurement).

Per case, after a warm-up call, the median of --calls timed calls of dnas_align_pairs (each returns after the device has been
synchronised and the results are back in host memory):
  gpu_call_*    pairs/s and band cells/s over the host clock around the whole call -- allocation, copies in, kernels, copies out;
  gpu_kernel_*  the same over fill_ms + traceback_ms of dnas_align_stats (HIP events around the kernels only);
  traceback_share  traceback_ms / (fill_ms + traceback_ms).
In the same run dnas_align_pairs_host is timed over a subset: on one thread, and on 16 threads (the subset split over a pool of
16, each thread calling the library on its share: ctypes releases the GIL).  The GPU's results are compared with the host's on
the one-thread subset, bit for bit.  The condition of record: gpu_call_pairs_per_s > host16_pairs_per_s on (a) and (b).

    python bench_pair_align.py [--cases abc] [--calls 5] [--scale 1.0]

prints one JSON line per case and a last line with the verdict."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"a": dict(pairs=100000, nt=150, band=16, unique=8000, host1=4000, host16=32000),
         "b": dict(pairs=4000, nt=1000, band=32, unique=1000, host1=250, host16=2000),
         "c": dict(pairs=2000, nt=300, band=-1, unique=1000, host1=250, host16=2000)}
RATES = dict(sub=.03, dup=.02, del_open=.02, del_ext=.2)
THREADS = 16


def make_pairs(case, n, unique):
    from synth import synthetic_alignment
    import dnastore_amd as da
    uniq = []
    for u in range(min(unique, n)):
        r = synthetic_alignment(random.Random("bench-pair-align/%s/%d" % (case, u)), CASES[case]["nt"], sub=.03, dele=.02, dup=.02)
        uniq.append((da.tokenize(r[0][1].replace("-", "")).astype(np.int8), da.tokenize(r[1][1].replace("-", "")).astype(np.int8)))
    return [uniq[i % len(uniq)] for i in range(n)]


class Packed:
    """The arrays of one dnas_align_pairs call, made once."""

    def __init__(self, pairs):
        self.n = len(pairs)
        self.in_off = np.zeros(self.n + 1, np.int64)
        self.out_off = np.zeros(self.n + 1, np.int64)
        self.in_off[1:] = np.cumsum([len(a) for a, _ in pairs])
        self.out_off[1:] = np.cumsum([len(b) for _, b in pairs])
        self.ins = np.ascontiguousarray(np.concatenate([a for a, _ in pairs]))
        self.outs = np.ascontiguousarray(np.concatenate([b for _, b in pairs]))
        self.ops_off = (self.in_off + self.out_off).astype(np.uint64)
        self.ops = np.zeros(int(self.ops_off[-1]) + 1, np.uint8)
        self.n_ops = np.zeros(self.n, np.uint32)
        self.score = np.zeros(self.n)
        self.status = np.zeros(self.n, np.uint8)

    def slice(self, lo, hi):
        p = Packed.__new__(Packed)
        p.n = hi - lo
        p.in_off = self.in_off[lo:hi + 1] - self.in_off[lo]
        p.out_off = self.out_off[lo:hi + 1] - self.out_off[lo]
        p.ins = np.ascontiguousarray(self.ins[self.in_off[lo]:self.in_off[hi]])
        p.outs = np.ascontiguousarray(self.outs[self.out_off[lo]:self.out_off[hi]])
        p.ops_off = (p.in_off + p.out_off).astype(np.uint64)
        p.ops = np.zeros(int(p.ops_off[-1]) + 1, np.uint8)
        p.n_ops, p.score, p.status = np.zeros(p.n, np.uint32), np.zeros(p.n), np.zeros(p.n, np.uint8)
        return p

    def gpu(self, L, params, band, stats):
        from dnastore_amd import lib as _l
        _l.check(L.dnas_align_pairs(ctypes.byref(params.c), band, self.n, self.ins.ctypes.data, self.in_off.ctypes.data,
                                    self.outs.ctypes.data, self.out_off.ctypes.data, 0, 0, self.ops.ctypes.data, self.ops_off.ctypes.data,
                                    self.n_ops.ctypes.data, self.score.ctypes.data, self.status.ctypes.data, ctypes.byref(stats)))

    def host(self, L, params, band):
        from dnastore_amd import lib as _l
        _l.check(L.dnas_align_pairs_host(ctypes.byref(params.c), band, self.n, self.ins.ctypes.data, self.in_off.ctypes.data,
                                         self.outs.ctypes.data, self.out_off.ctypes.data, self.ops.ctypes.data, self.ops_off.ctypes.data,
                                         self.n_ops.ctypes.data, self.score.ctypes.data, self.status.ctypes.data))


def run_case(case, calls, scale):
    import dnastore_amd as da
    from dnastore_amd import lib as _l
    L = _l.lib()
    cfg = CASES[case]
    n = max(THREADS, int(cfg["pairs"] * scale))
    band = cfg["band"]
    params = da.MutatorParams.fromFlags(**RATES)
    pk = Packed(make_pairs(case, n, cfg["unique"]))
    stats = _l.AlignStatsC()
    pk.gpu(L, params, band, stats)                                   # warm-up: code objects, the allocator
    wall, fill, tb = [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        pk.gpu(L, params, band, stats)
        wall.append(time.perf_counter() - t0)
        fill.append(stats.fill_ms)
        tb.append(stats.traceback_ms)
    cells = int(stats.cells)
    call_s = statistics.median(wall)
    kern_s = statistics.median([f + t for f, t in zip(fill, tb)]) / 1e3

    # the host, one thread
    n1 = min(n, max(1, int(cfg["host1"] * scale)))
    h1 = pk.slice(0, n1)
    h1.host(L, params, band)                                         # (warm-up: page faults of the result arrays)
    t0 = time.perf_counter()
    h1.host(L, params, band)
    host1_s = time.perf_counter() - t0
    same = bool(np.array_equal(h1.status, pk.status[:n1]) and np.array_equal(h1.score.view(np.uint64), pk.score[:n1].view(np.uint64))
                and np.array_equal(h1.n_ops, pk.n_ops[:n1])
                and all(np.array_equal(h1.ops[int(h1.ops_off[i]):int(h1.ops_off[i]) + int(h1.n_ops[i])],
                                       pk.ops[int(pk.ops_off[i]):int(pk.ops_off[i]) + int(pk.n_ops[i])]) for i in range(n1)))
    # ... and 16
    n16 = min(n, max(THREADS, int(cfg["host16"] * scale)))
    cut = [n16 * k // THREADS for k in range(THREADS + 1)]
    parts = [pk.slice(cut[k], cut[k + 1]) for k in range(THREADS)]
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(lambda p: p.host(L, params, band), parts))
        t0 = time.perf_counter()
        list(pool.map(lambda p: p.host(L, params, band), parts))
        host16_s = time.perf_counter() - t0
    per_pair = cells / n
    out = dict(case=case, pairs=n, nt=cfg["nt"], band=band, band_cells=cells, calls=calls, batches=int(stats.batches),
               pairs_too_large=int(stats.pairs_too_large),
               gpu_call_s=call_s, gpu_call_pairs_per_s=n / call_s, gpu_call_cells_per_s=cells / call_s,
               gpu_kernel_s=kern_s, gpu_kernel_pairs_per_s=n / kern_s, gpu_kernel_cells_per_s=cells / kern_s,
               fill_ms=statistics.median(fill), traceback_ms=statistics.median(tb),
               traceback_share=statistics.median(tb) / max(statistics.median(fill) + statistics.median(tb), 1e-12),
               gpu_call_spread=(max(wall) - min(wall)) / call_s,
               host1_pairs=n1, host1_pairs_per_s=n1 / host1_s, host1_cells_per_s=n1 * per_pair / host1_s,
               host16_pairs=n16, host16_pairs_per_s=n16 / host16_s, host16_cells_per_s=n16 * per_pair / host16_s,
               gpu_equals_host=same)
    out["gpu_call_over_host16"] = out["gpu_call_pairs_per_s"] / out["host16_pairs_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every case's pairs (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    lines = []
    for case in args.cases:
        lines.append(run_case(case, args.calls, args.scale))
        print(json.dumps(lines[-1]), flush=True)
    need = [x for x in lines if x["case"] in "ab"]
    verdict = dict(condition="gpu_call_pairs_per_s > host16_pairs_per_s on (a) and (b)",
                   met=bool(need) and all(x["gpu_call_over_host16"] > 1 for x in need) if len(need) == 2 else None,
                   ratios={x["case"]: x["gpu_call_over_host16"] for x in lines},
                   results_equal=all(x["gpu_equals_host"] for x in lines))
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["results_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
