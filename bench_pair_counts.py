"""Measures the marginal E-step (dnas_pair_counts) and the fit on top of it (dnas_baum_welch_pairs) on one MI355X.

a         100 000 pairs of 150 nt, band 16, P = 6, one E-step: the whole call (host clock, results in host memory), the kernel
          (HIP events), band cells/s, the scratch, the grid the arena allowed; beside it pair_forward_score_kernel<6> on the same
          pairs (dnas_pair_likelihoods), the arms alternated, --calls times after a warm-up call; medians.  The ratio of the two
          kernels says what the backward pass and the 16 exp per cell cost; no condition on it.
b         4 000 pairs of 1 000 nt, band 32, the same.
          Condition of record on a and b: the slowest of the whole calls beats the fastest of dnas_pair_counts_host on 16 host
          threads over the same pairs in the same run (--host-calls calls, the pairs cut in 16 consecutive shares).
route     for orientation, no condition: one E-step of the existing route on the pairs of a (alignPairs, ForwardBackward.load,
          expectedCounts) and a whole fit each way.  The two routes compute different quantities.
planted   20 000 pairs of 150 nt drawn with tests/synth.py::mutate at the two noise levels of bench_forward.py: the parameters
          each route fits beside the planted rates, with the final sum of pairLikelihoods.  No accuracy threshold.

    python bench_pair_counts.py [--parts abrp] [--calls 5] [--host-calls 1] [--scale 1.0]

prints one JSON line per part."""
import argparse
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

import synth  # noqa: E402

RATES = dict(sub=.04, dup=.01, del_open=.02, del_ext=.2)
NOISE = (("as tests", dict(sub=.04, dele=.02, dup=.01)), ("twice", dict(sub=.08, dele=.04, dup=.02)))
HOST_THREADS = 16
med = statistics.median


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


def make_pairs(n, nt, seed, noise=NOISE[0][1]):
    rng = random.Random(seed)
    ins, outs = [], []
    for _ in range(n):
        a = "".join(rng.choice("ACGT") for _ in range(nt))
        ins.append(a)
        outs.append(synth.mutate(a, rng, **noise) or a[:1])
    return ins, outs


def tokens(da, seqs):
    return [da.tokenize(s).astype(np.int8) for s in seqs]


def host_call(da, params, ins, outs, band):
    """dnas_pair_counts_host on HOST_THREADS threads: consecutive shares, the totals added in share order -> wall seconds."""
    n = len(ins)
    cuts = [n * k // HOST_THREADS for k in range(HOST_THREADS + 1)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        parts = list(pool.map(lambda k: da.pairCounts(params, ins[cuts[k]:cuts[k + 1]], outs[cuts[k]:cuts[k + 1]], band=band, host=True),
                              range(HOST_THREADS)))
    return time.perf_counter() - t0, sum(p.counts for p in parts)


def run_estep(part, n, nt, band, calls, host_calls):
    import dnastore_amd as da
    params = da.MutatorParams.fromFlags(length=12, **RATES)
    assert params.c.n_len == 6
    ins, outs = make_pairs(n, nt, "bench-pair-counts/%s" % part)
    ins, outs = tokens(da, ins), tokens(da, outs)
    da.pairCounts(params, ins, outs, band=band)                           # warm-up
    da.pairLikelihoods(params, ins, outs, band=band)
    wall, kernel, fwall, fkernel = [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = da.pairCounts(params, ins, outs, band=band)
        wall.append(time.perf_counter() - t0)
        kernel.append(res.stats["kernel_ms"])
        t0 = time.perf_counter()
        ll = da.pairLikelihoods(params, ins, outs, band=band)
        fwall.append(time.perf_counter() - t0)
        fkernel.append(da.pairLikelihoods.last_stats["score_ms"])
    assert np.array_equal(ll.view(np.uint64), res.pair_ll.view(np.uint64))
    host = [host_call(da, params, ins, outs, band) for _ in range(host_calls)]
    np.testing.assert_allclose(res.counts, host[0][1], rtol=1e-9)
    st = res.stats
    out = dict(part=part, pairs=n, nt=nt, band=band, P=6, calls=calls, host_calls=host_calls, host_threads=HOST_THREADS,
               call_s=med(wall), call_slowest_s=max(wall), call_spread=spread(wall), kernel_ms=med(kernel), kernel_spread=spread(kernel),
               band_cells=int(st["cells"]), cells_per_s=st["cells"] / (med(kernel) / 1e3), scratch_bytes=int(st["scratch_bytes"]),
               waves=int(st["waves"]), chunks=int(st["chunks"]), pairs_too_large=int(st["pairs_too_large"]),
               forward_call_s=med(fwall), forward_kernel_ms=med(fkernel),
               counts_over_forward_kernel_time=med(kernel) / med(fkernel), counts_over_forward_call_time=med(wall) / med(fwall),
               host_fastest_s=min(h[0] for h in host))
    out["host_over_gpu"] = out["host_fastest_s"] / out["call_slowest_s"]
    out["condition_of_record_holds"] = bool(out["call_slowest_s"] < out["host_fastest_s"])
    return out


def params_row(p):
    return dict(pDelOpen=p.c.p_del_open, pDelExtend=p.c.p_del_extend, pTanDup=p.c.p_tan_dup, pTransition=p.c.p_transition,
                pTransversion=p.c.p_transversion)


def guided_fit(da, start, ins, outs, band):
    """The existing route: one Viterbi alignment under the start, then the guided EM inside its envelope."""
    al = da.alignPairs(start, ins, outs, band=band)
    return da.baumWelchParams(start, al.packed())


def run_route(n, calls):
    import dnastore_amd as da
    params = da.MutatorParams.fromFlags(length=12, **RATES)
    ins, outs = make_pairs(n, 150, "bench-pair-counts/a")
    ins, outs = tokens(da, ins), tokens(da, outs)
    guided, marginal = [], []
    for k in range(calls + 1):                                            # the first round is the warm-up
        t0 = time.perf_counter()
        al = da.alignPairs(params, ins, outs, band=16)
        fb = da.ForwardBackward(None, device=0)
        fb.load(al.packed())
        fb.expectedCounts(params)
        fb.close()
        guided.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        da.pairCounts(params, ins, outs, band=16)
        marginal.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    _, it_g = guided_fit(da, params, ins, outs, 16)
    fit_g = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, it_m, _ = da.baumWelchPairs(params, ins, outs, band=16)
    fit_m = time.perf_counter() - t0
    return dict(part="route", pairs=n, calls=calls, guided_estep_s=med(guided[1:]), marginal_estep_s=med(marginal[1:]),
                guided_fit_s=fit_g, guided_fit_iterations=it_g, marginal_fit_s=fit_m, marginal_fit_iterations=it_m)


def run_planted(n):
    import dnastore_amd as da
    start = da.MutatorParams.fromFlags(length=8, sub=.01, dup=.001, del_open=.001, del_ext=.01)
    out = dict(part="planted", pairs=n, nt=150, band=16, start=params_row(start), levels=[])
    for name, noise in NOISE:
        ins, outs = make_pairs(n, 150, "bench-pair-counts/planted/%s" % name, noise)
        ins, outs = tokens(da, ins), tokens(da, outs)
        t0 = time.perf_counter()
        marginal, it_m, _ = da.baumWelchPairs(start, ins, outs, band=16)
        t_m = time.perf_counter() - t0
        t0 = time.perf_counter()
        guided, it_g = guided_fit(da, start, ins, outs, 16)
        t_g = time.perf_counter() - t0
        ll = {k: float(da.pairLikelihoods(p, ins, outs, band=16).sum()) for k, p in (("start", start), ("guided", guided), ("marginal", marginal))}
        out["levels"].append(dict(noise=name, planted=noise, marginal=params_row(marginal), marginal_iterations=it_m, marginal_fit_s=t_m,
                                  guided=params_row(guided), guided_iterations=it_g, guided_fit_s=t_g, sum_pair_likelihoods=ll))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abrp", help="a, b = the two E-step cases, r = the existing route, p = planted parameters")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every part's pairs (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    size = lambda n: max(16, int(n * args.scale))  # noqa: E731
    if "a" in args.parts:
        print(json.dumps(run_estep("a", size(100000), 150, 16, args.calls, args.host_calls)), flush=True)
    if "b" in args.parts:
        print(json.dumps(run_estep("b", size(4000), 1000, 32, args.calls, args.host_calls)), flush=True)
    if "r" in args.parts:
        print(json.dumps(run_route(size(100000), args.calls)), flush=True)
    if "p" in args.parts:
        print(json.dumps(run_planted(size(20000))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
