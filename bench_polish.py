"""Measures dnas_cluster_consensus (consensus reads, csrc/polish_kernels.hip) against the only route the library offered for the
same job before it.

20 000 clusters x 10 reads of 150 nt, band 16, rounds = 1, the error model with the rates of bench_consensus.py (P = 6): the
sizes of bench_consensus.py.  A cluster's reads are its strand after substitutions, deletions and tandem copies at those rates,
its template one more such read.  A few hundred distinct clusters are tiled to that number.
  new_*   dnas_cluster_consensus: the host clock around the call -- copies in, fill, vote and emit kernels, copies out;
  old_*   dnas_align_pairs with the template repeated once per read, which copies one op byte per alignment column to the host,
          then the vote and the emit of include/dnastore_amd.h in numpy over those bytes.
The arms are timed alternately, --calls times after a warm-up call; medians, and (max - min) / median as the spread.  The
consensus reads of the two arms are compared.  The condition of record: the new call's slowest run is faster than the old
route's fastest.  Also reported: the share of vote_ms (HIP events around the vote and emit kernels) in the new call, and
vote_ms with every table in LDS (as shipped at 150 nt) against every table in HBM (DNAS_POLISH_LDS_POSITIONS=0), the two routes
alternated in the same run.

    python bench_polish.py [--calls 5] [--scale 1.0]

prints one JSON line and a line with the verdict."""
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

from bench_consensus import RATES, concat, mutate  # noqa: E402

POLISH = dict(clusters=20000, reads=10, nt=150, band=16, distinct=250)
MAX_INSERT = 4


def make_clusters(n):
    """-> (templates, reads): per cluster one template and POLISH['reads'] reads, as int8 arrays."""
    cfg = POLISH
    rng = random.Random("bench-polish")
    uniq = []
    for _ in range(min(n, cfg["distinct"])):
        a = np.array([rng.randrange(4) for _ in range(cfg["nt"])], np.int8)
        uniq.append((mutate(rng, a), [mutate(rng, a) for _ in range(cfg["reads"])]))
    return [uniq[i % len(uniq)][0] for i in range(n)], [uniq[i % len(uniq)][1] for i in range(n)]


class NewArm:
    def __init__(self, params, templates, reads, band):
        from dnastore_amd import lib as _l
        self.L, self.params, self.band = _l.lib(), params, band
        self.nc = len(templates)
        self.cl_read = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        self.tmpl, self.tmpl_off = concat(templates)
        self.reads, self.read_off = concat([x for r in reads for x in r])
        self.n_reads = len(self.read_off) - 1
        self.out_off = np.zeros(self.nc + 1, np.int64)
        self.rounds, self.voters = np.zeros(self.nc, np.int32), np.zeros(self.nc, np.int32)
        self.converged, self.status = np.zeros(self.nc, np.uint8), np.zeros(self.nc, np.uint8)
        self.stats = _l.PolishStatsC()
        self.seqs = None

    def call(self):
        from dnastore_amd import lib as _l
        out = ctypes.c_void_p()
        _l.check(self.L.dnas_cluster_consensus(ctypes.byref(self.params.c), self.band, self.nc, self.tmpl.ctypes.data,
                                               self.tmpl_off.ctypes.data, self.n_reads, self.reads.ctypes.data, self.read_off.ctypes.data,
                                               None, self.cl_read.ctypes.data, 1, 0, 0, ctypes.byref(out), self.out_off.ctypes.data,
                                               self.rounds.ctypes.data, self.converged.ctypes.data, self.voters.ctypes.data,
                                               self.status.ctypes.data, ctypes.byref(self.stats)))
        total = int(self.out_off[-1])
        self.seqs = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int8)), shape=(max(total, 1),))[:total].copy()
        self.L.dnas_free(out)


class OldArm:
    """The route before dnas_cluster_consensus: dnas_align_pairs over (template, read) pairs with the template copied once per
    read, the op bytes copied out, and one round's vote and emit in numpy."""

    def __init__(self, new, R):
        from dnastore_amd import lib as _l
        self.L, self.new, self.R = _l.lib(), new, R
        n = new.n_reads
        t_len = np.diff(new.tmpl_off)
        self.ins, self.in_off = concat([new.tmpl[new.tmpl_off[c]:new.tmpl_off[c + 1]] for c in range(new.nc) for _ in range(R)])
        self.ops_off = np.zeros(n + 1, np.uint64)
        self.ops_off[1:] = np.cumsum(np.repeat(t_len, R) + np.diff(new.read_off))
        self.ops = np.zeros(int(self.ops_off[-1]), np.uint8)
        self.n_ops, self.score, self.status = np.zeros(n, np.uint32), np.zeros(n), np.zeros(n, np.uint8)
        self.stats = _l.AlignStatsC()
        self.seqs = None

    def call(self):
        from dnastore_amd import lib as _l
        new, R = self.new, self.R
        _l.check(self.L.dnas_align_pairs(ctypes.byref(new.params.c), new.band, new.n_reads, self.ins.ctypes.data, self.in_off.ctypes.data,
                                         new.reads.ctypes.data, new.read_off.ctypes.data, 0, 0, self.ops.ctypes.data,
                                         self.ops_off.ctypes.data, self.n_ops.ctypes.data, self.score.ctypes.data, self.status.ctypes.data,
                                         ctypes.byref(self.stats)))
        nc, n = new.nc, new.n_reads
        t_len = np.diff(new.tmpl_off)
        P = int(t_len.max()) + 1                                        # positions per cluster, padded
        n_ops = self.n_ops.astype(np.int64)                             # 0 for a pair without an alignment: it does not vote
        pair = np.repeat(np.arange(n, dtype=np.int64), n_ops)           # the pair of every column
        first = np.concatenate([[0], np.cumsum(n_ops)])[:-1]            # a pair's first column in the packed list
        within = np.arange(len(pair), dtype=np.int64) - first[pair]
        col = self.ops[self.ops_off[:-1].astype(np.int64)[pair] + within]
        kind = col & 3
        ip_inc, op_inc = (kind != 2).astype(np.int64), (kind != 1).astype(np.int64)
        ip_all, op_all = np.cumsum(ip_inc) - ip_inc, np.cumsum(op_inc) - op_inc
        ip, op = ip_all - ip_all[first][pair], op_all - op_all[first][pair]     # before the column
        cluster = pair // R
        V = np.bincount(np.arange(n)[self.status == _l.ALIGN_OK] // R, minlength=nc)
        pos = cluster * P + ip
        m = kind == 0
        base = new.reads[new.read_off[:-1][pair] + op].astype(np.int64)
        M = np.bincount(pos[m] * 4 + base[m], minlength=nc * P * 4).reshape(nc, P, 4)
        D = np.bincount(pos[kind == 1], minlength=nc * P).reshape(nc, P)
        d = kind == 2                                                   # runs of duplication columns: k counts from the run's first
        idx = np.arange(len(pair), dtype=np.int64)
        starts = d & ~(np.concatenate([[False], d[:-1]]) & (within > 0))
        k = idx - np.maximum.accumulate(np.where(starts, idx, 0))
        take = d & (k < MAX_INSERT)
        N = np.bincount(pos[take] * MAX_INSERT + k[take], minlength=nc * P * MAX_INSERT).reshape(nc, P, MAX_INSERT)
        B = np.bincount((pos[take] * MAX_INSERT + k[take]) * 4 + base[take], minlength=nc * P * MAX_INSERT * 4).reshape(nc, P, MAX_INSERT, 4)
        # emit: per gap up to four insertion bases while a majority has them, then the position's base unless a majority deleted it
        ins_on = np.logical_and.accumulate(2 * N > V[:, None, None], axis=2)
        ins_base = np.argmax(B, axis=3)                                 # the first of equal maxima: the smallest code
        tmpl = np.zeros((nc, P), np.int64)
        gaps = np.arange(P)[None, :]
        has = gaps < t_len[:, None]
        tmpl[has] = new.tmpl[:int(new.tmpl_off[-1])]
        top = M.max(axis=2)
        own = np.take_along_axis(M, tmpl[:, :, None], axis=2)[:, :, 0]
        keep_base = np.where(own == top, tmpl, np.argmax(M, axis=2))
        keep_on = has & ~(2 * D > V[:, None])
        bases = np.concatenate([ins_base, keep_base[:, :, None]], axis=2)
        on = np.concatenate([ins_on & (gaps <= t_len[:, None])[:, :, None], keep_on[:, :, None]], axis=2)
        self.seqs = bases[on].astype(np.int8)
        self.lengths = on.reshape(nc, -1).sum(axis=1)


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    import dnastore_amd as da
    cfg = POLISH
    n = max(8, int(cfg["clusters"] * args.scale))
    params = da.MutatorParams.fromFlags(**RATES)
    templates, reads = make_clusters(n)
    new = NewArm(params, templates, reads, cfg["band"])
    old = OldArm(new, cfg["reads"])
    new.call()                                                          # warm-up: code objects, the allocator
    old.call()
    same = bool(np.array_equal(new.seqs, old.seqs) and np.array_equal(np.diff(new.out_off), old.lengths))
    t_new, t_old, t_align, fill, vote = [], [], [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        new.call()
        t_new.append(time.perf_counter() - t0)
        fill.append(new.stats.fill_ms)
        vote.append(new.stats.vote_ms)
        t0 = time.perf_counter()
        old.call()
        t_old.append(time.perf_counter() - t0)
        t_align.append(old.stats.fill_ms + old.stats.traceback_ms)
    lds_clusters = int(new.stats.lds_clusters)
    vote_lds, vote_hbm, hbm_same = [], [], True                         # the two routes of the table, alternated
    for _ in range(args.calls):
        new.call()
        vote_lds.append(new.stats.vote_ms)
        os.environ["DNAS_POLISH_LDS_POSITIONS"] = "0"
        new.call()
        os.environ.pop("DNAS_POLISH_LDS_POSITIONS")
        vote_hbm.append(new.stats.vote_ms)
        hbm_same = hbm_same and int(new.stats.hbm_clusters) == n and bool(np.array_equal(new.seqs, old.seqs))
    med = statistics.median
    out = dict(part="polish", clusters=n, reads=cfg["reads"], nt=cfg["nt"], band=cfg["band"], rounds=1, calls=args.calls,
               pairs=int(new.stats.pairs), cells=int(new.stats.cells), batches=int(new.stats.batches), lds_clusters=lds_clusters,
               new_ms=med(t_new) * 1e3, new_min_ms=min(t_new) * 1e3, new_max_ms=max(t_new) * 1e3, new_spread=spread(t_new),
               old_ms=med(t_old) * 1e3, old_min_ms=min(t_old) * 1e3, old_max_ms=max(t_old) * 1e3, old_spread=spread(t_old),
               old_kernels_ms=med(t_align), ratio_old_over_new=med(t_old) / med(t_new),
               fill_ms=med(fill), vote_ms=med(vote), vote_share_of_call=med(vote) / (med(t_new) * 1e3),
               vote_lds_ms=med(vote_lds), vote_lds_spread=spread(vote_lds), vote_hbm_ms=med(vote_hbm), vote_hbm_spread=spread(vote_hbm),
               arms_equal=same, hbm_route_equal=hbm_same)
    print(json.dumps(out))
    ok = same and hbm_same and max(t_new) < min(t_old)
    print("polish: %s -- new call %.1f ms (slowest %.1f), old route %.1f ms (fastest %.1f), %.1fx; vote %.1f%% of the call; vote_ms LDS %.2f / HBM %.2f"
          % ("PASS" if ok else "FAIL", out["new_ms"], out["new_max_ms"], out["old_ms"], out["old_min_ms"], out["ratio_old_over_new"],
             100 * out["vote_share_of_call"], out["vote_lds_ms"], out["vote_hbm_ms"]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
