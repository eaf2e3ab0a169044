"""Measures dnas_trim_reads (csrc/trim_kernels.hip) against its host statement, at the C ABI: the pool is built once as packed
arrays (what a caller with a FASTQ parser of its own holds), a call is dnas_trim_reads on them and returns with every output in
host memory.  After a warm-up call the median of --calls timed calls, the spread as (max - min) / median; the kernel time is the
call's own (HIP events, dnas_trim_stats.kernel_ms).

  (a) 1 000 000 reads of 150 nt + primers, K = 16 pairs,   max_offset = 8
  (b)   100 000 reads of 150 nt + primers, K = 1 024 pairs, max_offset = 8
  (c)   200 000 reads of 1 000 nt,         K = 16 pairs,   max_offset = -1

A read is junk(0..5) . F_k . payload . R_k . junk(0..5) with substitutions at 5 % of the primers' bases, every other read
reverse-complemented, k uniform.  The host statement is timed in the same run on 1 thread and on a pool of 16 threads, each on a
sample of the reads (a contiguous block: --host-share of them for one thread, 16 times as many for the pool), and its time for
the whole pool is the sample's scaled by reads / sample -- the statement treats every read alone, so its time is linear in them;
the full pools would take minutes per call on one thread.  The GPU's outputs are compared with the statement's on the pool's
sample, and the pairs and strands it names with the planted ones.

Condition of record (the one of alignPairs): on (a) and (b) the slowest timed GPU call is faster than the host statement on 16
threads.  No ratio is fixed in advance.

    python bench_trim.py [--cases abc] [--calls 5] [--scale 1.0] [--host-share 256]

prints one JSON line per case and a last line with the verdict."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CASES = {"a": (1000000, 150, 16, 8), "b": (100000, 150, 1024, 8), "c": (200000, 960, 16, -1)}
PRIMER, JUNK, PERMILLE = 20, 5, 250


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


def make_pool(seed, n, payload, pairs):
    """-> (primer_seqs int8, primer_off, read_seqs int8, read_off, pair int64[n], strand int64[n])."""
    rng = np.random.default_rng(seed)
    primers = rng.integers(0, 4, size=(pairs, 2, PRIMER), dtype=np.int8)
    k = rng.integers(0, pairs, size=n)
    width = 2 * JUNK + 2 * PRIMER + payload
    mol = rng.integers(0, 4, size=(n, width), dtype=np.int8)
    mol[:, JUNK:JUNK + PRIMER] = primers[k, 0]
    mol[:, width - JUNK - PRIMER:width - JUNK] = primers[k, 1]
    for at in (JUNK, width - JUNK - PRIMER):                # substitutions, in the primers only
        hit = rng.random((n, PRIMER), dtype=np.float32) < .05
        mol[:, at:at + PRIMER] = np.where(hit, (mol[:, at:at + PRIMER] + rng.integers(1, 4, size=(n, PRIMER), dtype=np.int8)) & 3,
                                          mol[:, at:at + PRIMER])
    col = np.arange(width)[None, :]
    keep = (col >= JUNK - rng.integers(0, JUNK + 1, size=(n, 1))) & (col < width - JUNK + rng.integers(0, JUNK + 1, size=(n, 1)))
    strand = np.arange(n) % 2
    flip = strand.astype(bool)
    mol[flip] = 3 - mol[flip, ::-1]
    keep[flip] = keep[flip, ::-1]
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(keep.sum(axis=1))
    poff = np.arange(2 * pairs + 1, dtype=np.int64) * PRIMER
    return np.ascontiguousarray(primers.reshape(-1)), poff, np.ascontiguousarray(mol[keep]), off, k, strand


class Outputs:
    def __init__(self, n):
        n = max(n, 1)
        self.pair, self.begin, self.end, self.second = (np.zeros(n, np.int32) for _ in range(4))
        self.edits, self.strand, self.status = np.zeros(2 * n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)

    def pointers(self):
        return [x.ctypes.data for x in (self.pair, self.strand, self.begin, self.end, self.edits, self.second, self.status)]

    def equal(self, other, n):
        return all(np.array_equal(getattr(self, f)[:m], getattr(other, f)[:m])
                   for f, m in (("pair", n), ("strand", n), ("begin", n), ("end", n), ("edits", 2 * n), ("second", n), ("status", n)))


def host_call(L, pseqs, poff, seqs, off, first, last, max_offset, threads):
    """dnas_trim_reads_host over reads [first, last), cut into `threads` blocks, one thread each -> (seconds, Outputs)."""
    pairs = (len(poff) - 1) // 2
    cuts = np.linspace(first, last, threads + 1).astype(np.int64)
    parts = []
    for t in range(threads):
        lo, hi = int(cuts[t]), int(cuts[t + 1])
        sub_off = np.ascontiguousarray(off[lo:hi + 1] - off[lo])
        sub = np.ascontiguousarray(seqs[off[lo]:off[hi]]) if off[hi] > off[lo] else np.zeros(1, np.int8)
        parts.append((sub, sub_off, Outputs(hi - lo), hi - lo))

    def work(part):
        sub, sub_off, out, n = part
        rc = L.dnas_trim_reads_host(pairs, pseqs.ctypes.data, poff.ctypes.data, n, sub.ctypes.data, sub_off.ctypes.data, max_offset, PERMILLE,
                                    0, 0, *out.pointers())
        if rc:
            raise RuntimeError(L.dnas_last_error().decode())
    t0 = time.perf_counter()
    if threads == 1:
        work(parts[0])
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, parts))
    took = time.perf_counter() - t0
    whole = Outputs(last - first)
    at = 0
    for _, _, out, n in parts:
        for f, w in (("pair", 1), ("strand", 1), ("begin", 1), ("end", 1), ("edits", 2), ("second", 1), ("status", 1)):
            getattr(whole, f)[w * at:w * (at + n)] = getattr(out, f)[:w * n]
        at += n
    return took, whole


def run_case(da, name, calls, scale, host_share):
    n, payload, pairs, max_offset = CASES[name]
    n = max(1024, int(n * scale))
    L = da.lib.lib()
    pseqs, poff, seqs, off, k, strand = make_pool(20260000 + ord(name), n, payload, pairs)
    out, st = Outputs(n), da.lib.TrimStatsC()

    def gpu():
        t0 = time.perf_counter()
        da.lib.check(L.dnas_trim_reads(pairs, pseqs.ctypes.data, poff.ctypes.data, n, seqs.ctypes.data, off.ctypes.data, max_offset, PERMILLE,
                                       0, 0, 0, *out.pointers(), ctypes.byref(st)))
        return time.perf_counter() - t0
    gpu()                                                    # warm-up: code objects, the allocator
    walls, kernel = [], []
    for _ in range(calls):
        walls.append(gpu())
        kernel.append(st.kernel_ms / 1e3)
    n1 = max(64, n // host_share)
    n16 = min(n, 16 * n1)
    t1, _ = host_call(L, pseqs, poff, seqs, off, 0, n1, max_offset, 1)
    t16, ref = host_call(L, pseqs, poff, seqs, off, 0, n16, max_offset, 16)
    host1, host16 = t1 * n / n1, t16 * n / n16
    ok = out.status[:n] == 0
    return dict(case=name, reads=n, bases=int(off[n]), pairs=pairs, max_offset=max_offset, calls=calls, gpu_call_s=med(walls),
                gpu_call_spread=spread(walls), gpu_call_max_s=max(walls), kernel_s=med(kernel), kernel_spread=spread(kernel),
                kernel_share_of_call=med(kernel) / med(walls), items=st.items, chunks=st.chunks, columns=st.columns,
                columns_per_kernel_s=st.columns / med(kernel), trimmed=int(st.trimmed),
                named_as_planted=int((ok & (out.pair[:n] == k) & (out.strand[:n] == strand)).sum()),
                host_sample_reads_1_thread=n1, host_sample_s_1_thread=t1, host_1_thread_s_scaled=host1,
                host_sample_reads_16_threads=n16, host_sample_s_16_threads=t16, host_16_threads_s_scaled=host16,
                gpu_equals_host_on_sample=bool(out.equal(ref, n16)), host_16_over_gpu=host16 / med(walls), host_1_over_gpu=host1 / med(walls),
                faster_than_16_threads=bool(max(walls) < host16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every case's reads (a rehearsal)")
    ap.add_argument("--host-share", type=int, default=256, help="the one-thread host sample is reads / this; the 16-thread one 16 x that")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    if da.lib.lib().dnas_device_count() <= 0:
        raise SystemExit("bench_trim.py measures the GPU: no device is visible")
    lines = []
    for case in args.cases:
        lines.append(run_case(da, case, args.calls, args.scale, args.host_share))
        print(json.dumps(lines[-1]), flush=True)
    ab = [x for x in lines if x["case"] in "ab"]
    print(json.dumps(dict(condition="(a), (b): every timed GPU call is faster than the host statement on 16 threads, and equal to it on the sample",
                          met=bool(all(x["faster_than_16_threads"] and x["gpu_equals_host_on_sample"] for x in ab)) if ab else None,
                          host_16_over_gpu={x["case"]: x["host_16_over_gpu"] for x in ab})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
