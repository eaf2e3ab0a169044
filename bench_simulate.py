"""Measures dnas_simulate_reads (csrc/simulate_kernels.hip) against its host statement, at the C ABI: a call is dnas_simulate_reads
on packed strands and returns with every output in host memory, allocated by the library; the benchmark frees it.  After a warm-up
call the median of --calls timed calls, the spread as (max - min) / median; the kernels' times are the call's own (HIP events,
dnas_simulate_stats.count_ms and write_ms).

  pool   1 000 000 reads of 150 nt strands (10 000 strands, 100 reads each) at the default flags, with ops and without:
         the call, the two kernels, the bytes the second pass stores per second of its time against the HBM peak, and the host
         statement on 1 thread and on a pool of 16 (dnas_simulate_reads_host over blocks of the list, first_index moved; each on a
         sample -- reads / --host-share for one thread, 16 times as many for the pool -- scaled by reads / sample: the statement
         treats every read alone).  The GPU's reads are compared with the statement's on the pool's sample.
  thread the same pool with ops through the thread-per-read kernels (DNAS_SIMULATE_THREAD_PER_READ=1): the layout the shipped one,
         a wave per read, was chosen over; calls of the two routes alternate, the kernels' times side by side.
  loop   20 000 simulated pairs of 150 nt at sub=.04, dup=.01, del_open=.02, del_ext=.2, length=4: the generating
         parameters, the ones the true paths' counts give (dnas_alignment_expand summed, positions P <= ip < I for what the edges
         bend), and the ones baumWelchPairs fits from the unaligned pairs, side by side.

    python bench_simulate.py [--calls 5] [--scale 1.0] [--host-share 64] [--no-loop]

prints one JSON line."""
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

HBM_PEAK = 8.0e12                                            # bytes per second, MI355X
READS, STRANDS, NT = 1000000, 10000, 150
LOOP = dict(sub=.04, dup=.01, del_open=.02, del_ext=.2, global_=True, length=4)


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


class Call:
    """One call's library-allocated outputs."""

    def __init__(self, L, n):
        self.L, self.n = L, n
        self.seqs, self.off, self.rev, self.ops, self.ops_off = (ctypes.c_void_p() for _ in range(5))
        self.status = np.zeros(max(n, 1), np.uint8)

    def pointers(self):
        return [ctypes.byref(x) for x in (self.seqs, self.off, self.rev, self.ops, self.ops_off)] + [self.status.ctypes.data]

    def arrays(self, want_ops):
        view = lambda p, t, m: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), shape=(max(m, 1),))[:m].copy()
        off = view(self.off, ctypes.c_int64, self.n + 1)
        out = dict(off=off, seqs=view(self.seqs, ctypes.c_int8, int(off[-1])), rev=view(self.rev, ctypes.c_uint8, self.n))
        if want_ops:
            out["ops_off"] = view(self.ops_off, ctypes.c_int64, self.n + 1)
            out["ops"] = view(self.ops, ctypes.c_uint8, int(out["ops_off"][-1]))
        return out

    def free(self):
        for p in (self.seqs, self.off, self.rev, self.ops, self.ops_off):
            if p.value:
                self.L.dnas_free(p)
                p.value = None


def host_call(L, params, seqs, off, read_strand, seed, first, last, want_ops, threads):
    """dnas_simulate_reads_host over reads [first, last) in `threads` blocks, one thread each -> (seconds, [arrays per block])."""
    cuts = np.linspace(first, last, threads + 1).astype(np.int64)
    calls = [Call(L, int(cuts[t + 1] - cuts[t])) for t in range(threads)]

    def work(t):
        lo, c = int(cuts[t]), calls[t]
        rc = L.dnas_simulate_reads_host(ctypes.byref(params.c), len(off) - 1, seqs.ctypes.data, off.ctypes.data, c.n,
                                        read_strand[lo:].ctypes.data, seed, lo, 0., want_ops, *c.pointers())
        if rc:
            raise RuntimeError(L.dnas_last_error().decode())
    t0 = time.perf_counter()
    if threads == 1:
        work(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, range(threads)))
    took = time.perf_counter() - t0
    parts = [c.arrays(want_ops) for c in calls]
    for c in calls:
        c.free()
    return took, parts


def run_pool(da, want_ops, calls, scale, host_share):
    L = da.lib.lib()
    n, ns = max(1024, int(READS * scale)), max(16, int(STRANDS * scale))
    rng = np.random.default_rng(20261020)
    seqs = rng.integers(0, 4, size=ns * NT, dtype=np.int8)
    off = np.arange(ns + 1, dtype=np.int64) * NT
    read_strand = np.ascontiguousarray(np.arange(n, dtype=np.int64) % ns)
    params = da.MutatorParams.fromFlags(global_=True)
    seed, st = 20261020, da.lib.SimulateStatsC()
    kept = {}

    def gpu(keep=False):
        c = Call(L, n)
        t0 = time.perf_counter()
        da.lib.check(L.dnas_simulate_reads(ctypes.byref(params.c), ns, seqs.ctypes.data, off.ctypes.data, n, read_strand.ctypes.data, seed, 0, 0.,
                                           want_ops, 0, 0, *c.pointers(), ctypes.byref(st)))
        took = time.perf_counter() - t0
        if keep:
            kept.update(c.arrays(want_ops))
        c.free()
        return took
    gpu(keep=True)                                           # warm-up: code objects, the allocator
    walls, count, write = [], [], []
    for _ in range(calls):
        walls.append(gpu())
        count.append(st.count_ms / 1e3)
        write.append(st.write_ms / 1e3)
    n1 = max(64, n // host_share)
    n16 = min(n, 16 * n1)
    t1, _ = host_call(L, params, seqs, off, read_strand, seed, 0, n1, want_ops, 1)
    t16, parts = host_call(L, params, seqs, off, read_strand, seed, 0, n16, want_ops, 16)
    same = np.array_equal(np.concatenate([p["seqs"] for p in parts]), kept["seqs"][:kept["off"][n16]])
    same &= np.array_equal(np.concatenate([p["rev"] for p in parts]), kept["rev"][:n16])
    same &= np.array_equal(np.concatenate([np.diff(p["off"]) for p in parts]), np.diff(kept["off"][:n16 + 1]))
    if want_ops:
        same &= np.array_equal(np.concatenate([p["ops"] for p in parts]), kept["ops"][:kept["ops_off"][n16]])
    host1, host16 = t1 * n / n1, t16 * n / n16
    stored = st.bases_out + st.ops
    return dict(reads=n, strands=ns, nt=NT, ops=bool(want_ops), calls=calls, gpu_call_s=med(walls), gpu_call_spread=spread(walls),
                gpu_call_max_s=max(walls), count_kernel_s=med(count), count_kernel_spread=spread(count), write_kernel_s=med(write),
                write_kernel_spread=spread(write), kernels_share_of_call=(med(count) + med(write)) / med(walls), batches=st.batches,
                bases_in=st.bases_in, bases_out=st.bases_out, op_bytes=st.ops, stored_bytes_per_write_kernel_s=stored / med(write),
                share_of_hbm_peak=stored / med(write) / HBM_PEAK, positions_per_kernel_s=(st.bases_in + n) / (med(count) + med(write)),
                host_sample_reads_1_thread=n1, host_sample_s_1_thread=t1, host_1_thread_s_scaled=host1, host_sample_reads_16_threads=n16,
                host_sample_s_16_threads=t16, host_16_threads_s_scaled=host16, gpu_equals_host_on_sample=bool(same),
                host_16_over_gpu=host16 / med(walls), host_1_over_gpu=host1 / med(walls))


def run_routes(da, calls, scale):
    """The wave-per-read kernels and the thread-per-read ones on the pool with ops, calls alternating."""
    L = da.lib.lib()
    n, ns = max(1024, int(READS * scale)), max(16, int(STRANDS * scale))
    rng = np.random.default_rng(20261020)
    seqs = rng.integers(0, 4, size=ns * NT, dtype=np.int8)
    off = np.arange(ns + 1, dtype=np.int64) * NT
    read_strand = np.ascontiguousarray(np.arange(n, dtype=np.int64) % ns)
    params = da.MutatorParams.fromFlags(global_=True)
    st = da.lib.SimulateStatsC()
    times = {"wave_per_read": ([], []), "thread_per_read": ([], [])}
    for k in range(2 * (calls + 1)):
        route = "thread_per_read" if k % 2 else "wave_per_read"
        if k % 2:
            os.environ["DNAS_SIMULATE_THREAD_PER_READ"] = "1"
        else:
            os.environ.pop("DNAS_SIMULATE_THREAD_PER_READ", None)
        c = Call(L, n)
        da.lib.check(L.dnas_simulate_reads(ctypes.byref(params.c), ns, seqs.ctypes.data, off.ctypes.data, n, read_strand.ctypes.data, 20261020, 0,
                                           0., 1, 0, 0, *c.pointers(), ctypes.byref(st)))
        c.free()
        if k >= 2:                                           # the first call of each route warms it up
            times[route][0].append(st.count_ms / 1e3)
            times[route][1].append(st.write_ms / 1e3)
    os.environ.pop("DNAS_SIMULATE_THREAD_PER_READ", None)
    out = {route: dict(count_kernel_s=med(c), count_kernel_spread=spread(c), write_kernel_s=med(w), write_kernel_spread=spread(w))
           for route, (c, w) in times.items()}
    out["thread_over_wave"] = dict(count=out["thread_per_read"]["count_kernel_s"] / out["wave_per_read"]["count_kernel_s"],
                                   write=out["thread_per_read"]["write_kernel_s"] / out["wave_per_read"]["write_kernel_s"])
    return out


def rates_of_truth(da, sim, I):
    """The parameters the true paths' counts give, over the positions P <= ip < I."""
    P = sim.params.c.n_len
    total = np.zeros(21 + P)
    for i in range(len(sim)):
        total += sim.alignment(i)[2]
    ops = np.concatenate(sim.ops)
    lens = np.array([len(o) for o in sim.ops])
    kind, n = ops & 3, ops >> 2
    consumes = (kind != 2).astype(np.int64)
    before = np.cumsum(consumes) - consumes
    ip = before - np.repeat(before[np.cumsum(lens) - lens], lens)
    last = np.zeros(len(ops), bool)
    last[np.cumsum(lens) - 1] = True
    inside = (ip >= P) & (ip < I)
    opened, extended, dup_open, match = (kind == 1) & (n == 1), (kind == 1) & (n == 0), (kind == 2) & (n > 0), kind == 0
    visits = (inside & (opened | dup_open | match)).sum()
    entered = (kind == 1) & (ip + 1 >= P) & (ip + 1 < I)
    n_ext = (entered & np.append(extended[1:], False) & ~last).sum()
    sub = total[5:21].reshape(4, 4)
    n_ti = sum(sub[x][x ^ 2] for x in range(4))
    n_dup = (inside & dup_open).sum()
    return dict(pDelOpen=float((inside & opened).sum() / visits), pTanDup=float(n_dup / visits), pDelExtend=float(n_ext / entered.sum()),
                pTransition=float(n_ti / sub.sum()), pTransversion=float((sub.sum() - n_ti - np.trace(sub)) / sub.sum()),
                pLen=[float((inside & dup_open & (n == k + 1)).sum() / n_dup) for k in range(P)])


def as_dict(mp):
    c = mp.c
    return dict(pDelOpen=c.p_del_open, pTanDup=c.p_tan_dup, pDelExtend=c.p_del_extend, pTransition=c.p_transition,
                pTransversion=c.p_transversion, pLen=list(mp.pLen))


def run_loop(da, scale):
    pairs, I = max(256, int(20000 * scale)), 150
    gen = da.MutatorParams.fromFlags(**LOOP)
    rng = np.random.default_rng(20261021)
    strands = [rng.integers(0, 4, size=I, dtype=np.int8) for _ in range(pairs)]
    t0 = time.perf_counter()
    sim = da.simulateReads(gen, strands, seed=20261021)
    t_sim = time.perf_counter() - t0
    t0 = time.perf_counter()
    fit, iterations, trace = da.baumWelchPairs(da.MutatorParams.fromFlags(global_=True, length=LOOP["length"]), strands, sim.reads, band=32)
    t_fit = time.perf_counter() - t0
    return dict(pairs=pairs, nt=I, simulate_s=t_sim, generating=as_dict(gen), from_true_paths=rates_of_truth(da, sim, I),
                baum_welch_pairs=as_dict(fit), baum_welch_iterations=iterations, baum_welch_s=t_fit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the reads and pairs (a rehearsal)")
    ap.add_argument("--host-share", type=int, default=64, help="the one-thread host sample is reads / this; the 16-thread one 16 x that")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    if da.lib.lib().dnas_device_count() <= 0:
        raise SystemExit("bench_simulate.py measures the GPU: no device is visible")
    result = dict(bench="simulate", with_ops=run_pool(da, 1, args.calls, args.scale, args.host_share),
                  without_ops=run_pool(da, 0, args.calls, args.scale, args.host_share), routes=run_routes(da, args.calls, args.scale))
    if not args.no_loop:
        result["loop"] = run_loop(da, args.scale)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
