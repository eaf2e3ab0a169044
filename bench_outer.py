"""Measures the outer code (csrc/rs_kernels.hip) against its host statement, at the C ABI, and reports whether a file comes back
from a simulated pool.  A call is dnas_rs_decode / dnas_rs_encode on host arrays and returns with every output in host memory.
After a warm-up call the median of --calls timed calls, the spread as (max - min) / median; the kernel time is the call's own
(HIP events, dnas_rs_stats.kernel_ms).

  (a) decode, RS(255, 223), L = 32, 65 536 blocks (535 MB, beyond the caches): 5 % of the strands erased, 1 % corrupted in
      every byte -- nearly every column goes through the solver.  columns_decoded_to_another_codeword: columns beyond capacity
      (many erasures and an error or two) that lie within reach of a codeword that was not sent; the rule returns that codeword
  (b) the same pool with erasures only -- no column goes through the solver -- and dnas_rs_encode of its data
  (c) end to end: a file -> OuterCode(40, 30, 16) -> the inner code (l4c4) -> simulateReads at the default error model, coverage
      3, 5 % of the strands without reads, half of the reads reverse-complemented -> decode_pool -> decode_messages.  Reported,
      not asserted: whether the file came back byte for byte, and the strands erased, corrected and the columns failed.

The host statement is timed in the same run on 1 thread and on a pool of 16 threads, each on a sample of the blocks (a
contiguous range: blocks / --host-share for one thread, 16 times as many for the pool); its time for the whole pool is the
sample's scaled by blocks / sample -- the statement treats every block alone.  The GPU's outputs are compared with the
statement's on the pool's sample.

    python bench_outer.py [--cases abc] [--calls 5] [--scale 1.0] [--host-share 256]

prints one JSON line per arm."""
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

N, K, L, BLOCKS = 255, 223, 32, 65536
ERASED, CORRUPTED = .05, .01


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


class Outputs:
    def __init__(self, B):
        self.blocks = np.zeros((max(B, 1), N, L), np.uint8)
        self.status, self.errors = np.zeros((max(B, 1), L), np.uint8), np.zeros((max(B, 1), L), np.uint8)
        self.fixed = np.zeros((max(B, 1), N), np.int32)

    def pointers(self):
        return [x.ctypes.data for x in (self.blocks, self.status, self.errors, self.fixed)]

    def equal(self, other, B):
        return all(np.array_equal(getattr(self, f)[:B], getattr(other, f)[:B]) for f in ("blocks", "status", "errors", "fixed"))


def host_decode(lib, received, present, first, last, threads):
    """dnas_rs_decode_host over blocks [first, last), cut into `threads` ranges, one thread each -> (seconds, Outputs)."""
    out = Outputs(last - first)
    cuts = np.linspace(first, last, threads + 1).astype(np.int64)

    def work(t):
        lo, hi = int(cuts[t]), int(cuts[t + 1])
        at = lo - first
        rc = lib.dnas_rs_decode_host(N, K, L, hi - lo, received[lo:].ctypes.data, present[lo:].ctypes.data, out.blocks[at:].ctypes.data,
                                     out.status[at:].ctypes.data, out.errors[at:].ctypes.data, out.fixed[at:].ctypes.data)
        if rc:
            raise RuntimeError(lib.dnas_last_error().decode())
    t0 = time.perf_counter()
    if threads == 1:
        work(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, range(threads)))
    return time.perf_counter() - t0, out


def host_encode(lib, data, first, last, threads):
    out = np.zeros((last - first, N, L), np.uint8)
    cuts = np.linspace(first, last, threads + 1).astype(np.int64)

    def work(t):
        lo, hi = int(cuts[t]), int(cuts[t + 1])
        rc = lib.dnas_rs_encode_host(N, K, L, hi - lo, data[lo:].ctypes.data, out[lo - first:].ctypes.data)
        if rc:
            raise RuntimeError(lib.dnas_last_error().decode())
    t0 = time.perf_counter()
    if threads == 1:
        work(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, range(threads)))
    return time.perf_counter() - t0, out


def timed(fn, calls):
    fn()                                                     # warm-up: code objects, the allocator
    walls, kernel = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        st = fn()
        walls.append(time.perf_counter() - t0)
        kernel.append(st.kernel_ms / 1e3)
    return walls, kernel, st


def decode_arm(da, name, clean, received, present, calls, host_share):
    lib = da.lib.lib()
    B = len(received)
    out = Outputs(B)

    def gpu():
        st = da.lib.RsStatsC()
        da.lib.check(lib.dnas_rs_decode(N, K, L, B, received.ctypes.data, present.ctypes.data, *out.pointers(), ctypes.byref(st), 0))
        return st
    walls, kernel, st = timed(gpu, calls)
    b1 = max(1, B // host_share)
    b16 = min(B, 16 * b1)
    t1, _ = host_decode(lib, received, present, 0, b1, 1)
    t16, ref = host_decode(lib, received, present, 0, b16, 16)
    host1, host16 = t1 * B / b1, t16 * B / b16
    ok = out.status[:B] != da.lib.RS_FAILED
    return dict(case=name, code=[N, K], strand_bytes=L, blocks=B, bytes=int(received.nbytes), calls=calls,
                strands_erased=int((present == 0).sum()), columns=int(st.columns), columns_solved=int(st.columns_solved),
                columns_ok=int((out.status[:B] == da.lib.RS_OK).sum()), columns_corrected=int((out.status[:B] == da.lib.RS_CORRECTED).sum()),
                columns_failed=int((~ok).sum()), columns_decoded_to_another_codeword=int((~(out.blocks[:B] == clean).all(axis=1))[ok].sum()),
                gpu_call_s=med(walls), gpu_call_spread=spread(walls), gpu_call_max_s=max(walls), kernel_s=med(kernel),
                kernel_spread=spread(kernel), kernel_bytes_per_s=received.nbytes / med(kernel), call_bytes_per_s=received.nbytes / med(walls),
                host_sample_blocks_1_thread=b1, host_sample_s_1_thread=t1, host_1_thread_s_scaled=host1,
                host_sample_blocks_16_threads=b16, host_sample_s_16_threads=t16, host_16_threads_s_scaled=host16,
                gpu_equals_host_on_sample=bool(out.equal(ref, b16)), host_16_over_gpu_call=host16 / med(walls),
                host_16_over_kernel=host16 / med(kernel), host_1_over_gpu_call=host1 / med(walls))


def encode_arm(da, clean, calls, host_share):
    lib = da.lib.lib()
    B = len(clean)
    data = np.ascontiguousarray(clean[:, :K])
    out = np.zeros((B, N, L), np.uint8)

    def gpu():
        st = da.lib.RsStatsC()
        da.lib.check(lib.dnas_rs_encode(N, K, L, B, data.ctypes.data, out.ctypes.data, ctypes.byref(st), 0))
        return st
    walls, kernel, st = timed(gpu, calls)
    b1 = max(1, B // host_share)
    b16 = min(B, 16 * b1)
    t1, _ = host_encode(lib, data, 0, b1, 1)
    t16, ref = host_encode(lib, data, 0, b16, 16)
    host1, host16 = t1 * B / b1, t16 * B / b16
    return dict(case="b-encode", code=[N, K], strand_bytes=L, blocks=B, bytes=int(out.nbytes), calls=calls, gpu_call_s=med(walls),
                gpu_call_spread=spread(walls), gpu_call_max_s=max(walls), kernel_s=med(kernel), kernel_spread=spread(kernel),
                kernel_bytes_per_s=out.nbytes / med(kernel), host_sample_blocks_1_thread=b1, host_1_thread_s_scaled=host1,
                host_sample_blocks_16_threads=b16, host_16_threads_s_scaled=host16, gpu_equals_host_on_sample=bool(np.array_equal(out[:b16], ref)),
                gpu_equals_the_pool=bool(np.array_equal(out, clean)), host_16_over_gpu_call=host16 / med(walls),
                host_16_over_kernel=host16 / med(kernel))


def make_pool(da, B, seed):
    """-> clean uint8[B, N, L] (encoded on the host statement's side of the comparison: by dnas_rs_encode_host in 16 threads),
    corrupted, erasures-only, present."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(B, K, L), dtype=np.uint8)
    _, clean = host_encode(da.lib.lib(), data, 0, B, 16)
    draw = rng.random((B, N))
    present = (draw >= ERASED).astype(np.uint8)
    wrong = (draw >= ERASED) & (draw < ERASED + CORRUPTED)
    erased_only = clean.copy()
    erased_only[present == 0] = 0xA5                          # what is stored at an erased strand is never read
    corrupted = erased_only.copy()
    corrupted[wrong] ^= rng.integers(1, 256, size=(int(wrong.sum()), L), dtype=np.uint8)
    return clean, corrupted, erased_only, present


def end_to_end(da, scale):
    n, k, body, length, coverage, lost = 40, 30, 16, max(100, int(10000 * scale)), 3, .05
    rng = np.random.default_rng(20261021)
    data = rng.integers(0, 256, size=length, dtype=np.uint8).tobytes()
    machine = da.Machine.fromFile(os.path.join(ROOT, "tests", "golden", "ref_data", "l4c4.json"))
    params = da.MutatorParams.fromFlags(global_=True)
    code = da.OuterCode(n, k, body)
    t0 = time.perf_counter()
    records, B = code.encode(data)
    strands = [machine.encodeBytes(r) for r in records]
    kept = [s for s in range(len(strands)) if rng.random() >= lost]
    sim = da.simulateReads(params, strands, read_strand=[s for s in kept for _ in range(coverage)], seed=7, reverse_prob=.5, shuffle=True,
                           ops=False)
    reads = ["".join("ACGT"[b] for b in r) for r in sim.reads]
    t1 = time.perf_counter()
    dec = da.ViterbiDecoder(machine, params, device=0)
    pool = dec.decode_pool(reads, strands="both")
    dec.close()
    t2 = time.perf_counter()
    out = code.decode_messages(pool, B)
    t3 = time.perf_counter()
    exact = sum(1 for m in pool.symbols if len(m) and da.symbolsToBytes(m) in set(records))
    return dict(case="c", code=[n, k], body_bytes=body, file_bytes=length, blocks=B, strands=len(strands), strands_without_reads=len(strands) - len(kept),
                reads=len(reads), read_bases=int(sum(len(r) for r in reads)), clusters=len(pool.symbols), messages_that_are_records=exact,
                file_came_back=bool(out.data == data and out.status == da.lib.OUTER_OK), outer_status=int(out.status),
                failed_ranges=out.failed_ranges[:8], records_dropped=out.stats["dropped"], slots_in_conflict=out.stats["conflicts"],
                strands_erased=out.stats["erased"], strands_corrected=out.stats["strands_fixed"], columns_corrected=out.stats["columns_corrected"],
                columns_failed=out.stats["columns_failed"], encode_and_simulate_s=t1 - t0, decode_pool_s=t2 - t1, outer_decode_s=t3 - t2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the blocks and of the file (a rehearsal)")
    ap.add_argument("--host-share", type=int, default=256, help="the one-thread host sample is blocks / this; the 16-thread one 16 x that")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    import dnastore_amd as da
    if da.lib.lib().dnas_device_count() <= 0:
        raise SystemExit("bench_outer.py measures the GPU: no device is visible")
    if set(args.cases) & set("ab"):
        clean, corrupted, erased_only, present = make_pool(da, max(64, int(BLOCKS * args.scale)), 20261021)
        if "a" in args.cases:
            print(json.dumps(decode_arm(da, "a", clean, corrupted, present, args.calls, args.host_share)), flush=True)
        if "b" in args.cases:
            print(json.dumps(decode_arm(da, "b-decode", clean, erased_only, present, args.calls, args.host_share)), flush=True)
            print(json.dumps(encode_arm(da, clean, args.calls, args.host_share)), flush=True)
    if "c" in args.cases:
        print(json.dumps(end_to_end(da, args.scale)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
