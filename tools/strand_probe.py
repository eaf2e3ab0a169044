"""What does decoding both strands cost?  The headline workload (bench.py: s16h74l4c4, reads by index, 1 % substitutions,
--error-global, P = 6), 2 880 reads of which a seeded half are reverse-complemented, inputs resident in HBM, a warm-up call,
then the median of 5 timed calls each (wall clock around the call + dnas_model_sync):

  A  forward call on the 2 880 reads (dnas_viterbi_batch_device)
  B  forward call on the 5 760 reads {reads + their reverse complements}: what gives the same answer without the strand
     mode, a host-side pick on top
  C  "both" call on the 2 880 reads (dnas_viterbi_batch_strands_device)
  F  forward call through the strand entry point (the same code path as A)

and C's decoded symbols against the pick from B's.  A library without the strand entry points gives A and B alone.
    python tools/strand_probe.py [reads] [calls]        (--once: one call of C only, for a kernel trace)"""
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import dnastore_amd as da  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 2880
calls = int(args[1]) if len(args) > 1 else 5
once = "--once" in sys.argv
have_strands = hasattr(da.lib.lib(), "dnas_viterbi_batch_strands_device")
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s[::-1].translate(COMP)


m = da.Machine.fromFile(bench.MACHINE)
written = bench.make_reads(m, 0, n)
rng = random.Random(2880)
flipped = [rng.random() < 0.5 for _ in range(n)]
reads = [revcomp(r) if f else r for r, f in zip(written, flipped)]
torch.cuda.init()               # (PyTorch's HIP runtime comes up before the library's: tests/conftest.py)
dev = torch.device("cuda", 0)
dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True), device=0)


class Resident:
    """A read set with its inputs and outputs on the device."""

    def __init__(self, rs):
        self.k = len(rs)
        self.off, bases = da.pack_reads(rs)
        self.cap = int(np.diff(self.off).max()) + 64
        self.out_off = np.arange(self.k + 1, dtype=np.uint64) * np.uint64(self.cap)
        self.bases = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
        self.sym = torch.zeros(self.k * self.cap, dtype=torch.uint8, device=dev)
        self.len = torch.zeros(self.k, dtype=torch.int32, device=dev)
        self.ll = torch.zeros(self.k, dtype=torch.float64, device=dev)
        self.st = torch.zeros(self.k, dtype=torch.uint8, device=dev)
        self.strand = torch.zeros(self.k, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def call(self, mode=None):
        t0 = time.perf_counter()
        if mode is None:
            dec.decode_device(self.off, self.bases.data_ptr(), self.sym.data_ptr(), self.out_off, self.len.data_ptr(), self.ll.data_ptr(),
                              self.st.data_ptr())
        else:
            dec.decode_device(self.off, self.bases.data_ptr(), self.sym.data_ptr(), self.out_off, self.len.data_ptr(), self.ll.data_ptr(),
                              self.st.data_ptr(), strands=mode, d_strand_ptr=self.strand.data_ptr())
        dec.sync()
        return (time.perf_counter() - t0) * 1e3

    def strings(self):
        sym, olen = self.sym.cpu().numpy(), self.len.cpu().numpy()
        return [sym[i * self.cap:i * self.cap + int(olen[i])].tobytes() for i in range(self.k)]


def timed(res, mode=None):
    res.call(mode)                                              # warm-up
    ms = [res.call(mode) for _ in range(calls)]
    s = dec.stats()
    return statistics.median(ms), ms, s


one = Resident(reads)
if once:
    one.call("both")
    one.call("both")
    print("one warm-up and one traced call of C done:", dec.strand_stats(), flush=True)
    sys.exit(0)
two = Resident(reads + [revcomp(r) for r in reads])
print("%d reads (%d reverse-complemented), %d nt; %s" % (n, sum(flipped), int(one.off[-1]), dec.tier[:70]), flush=True)
a, a_all, sa = timed(one)
print("A  forward, %d reads:            median %.2f ms  %s  fill %.1f ms traceback %.1f ms, %d launches" % (
    n, a, ["%.2f" % x for x in a_all], sa["fill_ms"], sa["traceback_ms"], sa["fill_launches"]), flush=True)
b, b_all, sb = timed(two)
print("B  forward, %d reads:            median %.2f ms  %s  fill %.1f ms traceback %.1f ms, %d launches" % (
    2 * n, b, ["%.2f" % x for x in b_all], sb["fill_ms"], sb["traceback_ms"], sb["fill_launches"]), flush=True)
ll_b, str_b = two.ll.cpu().numpy(), two.strings()
pick = [1 if ll_b[n + i] > ll_b[i] else 0 for i in range(n)]
if have_strands:
    c, c_all, sc = timed(one, "both")
    print("C  both strands, %d reads:       median %.2f ms  %s  fill %.1f ms traceback %.1f ms, %d launches" % (
        n, c, ["%.2f" % x for x in c_all], sc["fill_ms"], sc["traceback_ms"], sc["fill_launches"]), flush=True)
    print("   strand stats:", dec.strand_stats(), flush=True)
    str_c, ll_c, strand_c = one.strings(), one.ll.cpu().numpy(), one.strand.cpu().numpy()
    bad = sum(1 for i in range(n) if str_c[i] != str_b[i + n * pick[i]] or ll_c[i] != ll_b[i + n * pick[i]] or int(strand_c[i]) != pick[i])
    f, f_all, _ = timed(one, "forward")
    print("F  forward through the strand entry point: median %.2f ms  %s" % (f, ["%.2f" % x for x in f_all]), flush=True)
    print("C / B = %.3f   C / A = %.3f   B / A = %.3f   F / A = %.3f" % (c / b, c / a, b / a, f / a))
    print("mismatches of C against the pick from B (symbols, log-likelihood bits, strand): %d of %d" % (bad, n))
    print("strand equals the coin that flipped the read: %d of %d" % (sum(1 for i in range(n) if int(strand_c[i]) == int(flipped[i])), n))
    ok = bad == 0 and c <= 1.05 * b
    print("DONE" if ok else "NOT DONE (C <= 1.05 B and 0 mismatches)", flush=True)
else:
    ok = True
    print("B / A = %.3f   (this library has no strand entry points: A and B only)" % (b / a))
dec.close()
sys.exit(0 if ok else 1)
