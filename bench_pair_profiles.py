"""Measures the pair-HMM row profiles (dnas_pair_profiles) on one MI355X beside the kernel they were cut from.

a         100 000 pairs of 150 nt, band 16, P = 6 (case a of bench_pair_counts.py, the same pairs).  Four arms, alternated in one
          run, --calls times after a warm-up call each; medians and the slowest:
            counts          pairCounts: pair_counts_kernel, unchanged -- the yardstick
            profiles        pairProfiles(per_pair=False): pair_profile_kernel, the aggregate formed chunk by chunk
            profiles+pairs  pairProfiles(per_pair=True): the same with every pair's block copied out to the caller
            host            pairProfiles(host=True, per_pair=False) on 16 host threads (--host-calls calls, the pairs cut in 16
                            consecutive shares)
          Whole calls by the host clock (results in host memory), kernels by HIP events.  The one condition: the slowest whole GPU
          call of either profile arm beats the fastest host call.  The ratio of the two kernels is reported, with no condition on
          it: the profile kernel forms 1 + KP fewer exp per cell and adds one store per plane and stripe.
b         4 000 pairs of 1 000 nt, band 32, the same.

    python bench_pair_profiles.py [--parts ab] [--calls 5] [--host-calls 1] [--scale 1.0]

prints one JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_pair_counts import HOST_THREADS, RATES, make_pairs, spread, tokens  # noqa: E402

med = statistics.median


def host_call(da, params, ins, outs, band):
    """dnas_pair_profiles_host on HOST_THREADS threads over consecutive shares -> (wall seconds, the shares' aggregates added)."""
    n = len(ins)
    cuts = [n * k // HOST_THREADS for k in range(HOST_THREADS + 1)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        parts = list(pool.map(lambda k: da.pairProfiles(params, ins[cuts[k]:cuts[k + 1]], outs[cuts[k]:cuts[k + 1]], band=band, host=True,
                                                        per_pair=False), range(HOST_THREADS)))
    return time.perf_counter() - t0, sum(p.profile for p in parts), sum(p.coverage for p in parts)


def run(part, n, nt, band, calls, host_calls):
    import dnastore_amd as da
    params = da.MutatorParams.fromFlags(length=12, **RATES)
    assert params.c.n_len == 6
    ins, outs = make_pairs(n, nt, "bench-pair-counts/%s" % part)
    ins, outs = tokens(da, ins), tokens(da, outs)
    arms = (("counts", lambda: da.pairCounts(params, ins, outs, band=band)),
            ("profiles", lambda: da.pairProfiles(params, ins, outs, band=band, per_pair=False)),
            ("profiles+pairs", lambda: da.pairProfiles(params, ins, outs, band=band, per_pair=True)))
    last = {}
    for name, call in arms:                                               # warm-up
        call()
    wall, kernel = {name: [] for name, _ in arms}, {name: [] for name, _ in arms}
    for _ in range(calls):
        for name, call in arms:
            t0 = time.perf_counter()
            last[name] = call()
            wall[name].append(time.perf_counter() - t0)
            kernel[name].append(last[name].stats["kernel_ms"])
    host = [host_call(da, params, ins, outs, band) for _ in range(host_calls)]
    agg, per = last["profiles"], last["profiles+pairs"]
    assert np.array_equal(agg.profile.view(np.uint64), per.profile.view(np.uint64)) and np.array_equal(agg.coverage, per.coverage)
    assert np.array_equal(agg.coverage, host[0][2])
    np.testing.assert_allclose(agg.profile, host[0][1], rtol=1e-9, atol=np.finfo(np.float64).tiny)
    c = last["counts"].counts
    rows = agg.profile.sum(axis=1)
    np.testing.assert_allclose([rows[:3].sum(), rows[3], rows[4]] + list(rows[5:]), [c[2], c[0], c[3]] + list(c[21:]), rtol=1e-9)
    st = agg.stats
    out = dict(part=part, pairs=n, nt=nt, band=band, P=6, calls=calls, host_calls=host_calls, host_threads=HOST_THREADS,
               band_cells=int(st["cells"]), scratch_bytes=int(st["scratch_bytes"]), waves=int(st["waves"]),
               counts_waves=int(last["counts"].stats["waves"]), chunks=int(st["chunks"]), pairs_too_large=int(st["pairs_too_large"]),
               profile_bytes=int(8 * 12 * sum(len(a) + 1 for a in ins)))
    for name, _ in arms:
        key = name.replace("+", "_")
        out.update({key + "_call_s": med(wall[name]), key + "_call_slowest_s": max(wall[name]), key + "_call_spread": spread(wall[name]),
                    key + "_kernel_ms": med(kernel[name]), key + "_kernel_spread": spread(kernel[name])})
    out["profile_over_counts_kernel_time"] = out["profiles_kernel_ms"] / out["counts_kernel_ms"]
    out["per_pair_copy_s"] = out["profiles_pairs_call_s"] - out["profiles_call_s"]
    out["cells_per_s"] = st["cells"] / (out["profiles_kernel_ms"] / 1e3)
    out["host_fastest_s"] = min(h[0] for h in host)
    slowest = max(out["profiles_call_slowest_s"], out["profiles_pairs_call_slowest_s"])
    out["host_over_gpu"] = out["host_fastest_s"] / slowest
    out["condition_of_record_holds"] = bool(slowest < out["host_fastest_s"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab", help="a, b = the two cases")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every part's pairs (a rehearsal)")
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    size = lambda n: max(16, int(n * args.scale))  # noqa: E731
    if "a" in args.parts:
        print(json.dumps(run("a", size(100000), 150, 16, args.calls, args.host_calls)), flush=True)
    if "b" in args.parts:
        print(json.dumps(run("b", size(4000), 1000, 32, args.calls, args.host_calls)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
