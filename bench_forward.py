"""Measures the forward (sum-product) mode of the pair-HMM score kernel beside the Viterbi mode, and what the posterior it
yields says about planted clusters.

score     the rescore items of bench_consensus.py (20 000 clusters x 10 reads x 4 candidates of 150 nt, band 16, P = 6) through
          dnas_consensus_score_ex in both modes, the arms alternated, --calls times after a warm-up call; medians.  Band cells/s
          over score_ms (HIP events around the score kernel) and items/s over the host clock around the call, results in host
          memory.  Then the forward mode alone at P = 2 and P = 13 (the other two instances of the kernel).  No condition: the
          forward cell carries three dependent table look-ups where the Viterbi cell has compares.
decode    ViterbiDecoder.decode_clusters(score="forward") against the default on the decode part of bench_consensus.py (400
          clusters of 5 reads on s16h74l4c4.json), the arms alternated: wall time per call and rescore_wall_ms.  No condition.
planted   the 40 planted clusters of 3 reads on h74l4c4.json of tests/test_gpu_consensus.py (same generator, seed and draw order)
          at its noise and at twice that noise: how many planted messages each mode names, and a calibration table -- the
          clusters binned by confidence, with the share named correctly per bin.  No threshold: forty clusters cannot carry one.

    python bench_forward.py [--parts sdp] [--calls 5] [--scale 1.0] [--decode-clusters 400]

prints one JSON line per part."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_consensus as BC  # noqa: E402

PLANTED = dict(sub=.04, dup=.01, del_open=.02, del_ext=.2, length=4)
NOISE = (("as tests", dict(sub=.04, dele=.02, dup=.01)), ("twice", dict(sub=.08, dele=.04, dup=.02)))
BINS = (0., .5, .9, .99, .999, 1.)
med = statistics.median


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


class ScoreArm(BC.ConsensusArm):
    """dnas_consensus_score_ex in one mode on the arrays of bench_consensus.ConsensusArm."""

    def __init__(self, params, cands, reads, band, mode):
        super().__init__(params, cands, reads, band)
        self.mode = mode
        self.post = np.zeros(self.n_cand) if mode else None

    def call(self):
        from dnastore_amd import lib as _l
        _l.check(self.L.dnas_consensus_score_ex(ctypes.byref(self.params.c), self.band, self.nc, self.n_cand, self.cand.ctypes.data,
                                                self.cand_off.ctypes.data, self.cl_cand.ctypes.data, self.n_reads, self.reads.ctypes.data,
                                                self.read_off.ctypes.data, None, self.cl_read.ctypes.data, 0, self.mode,
                                                self.winner.ctypes.data, self.total.ctypes.data, self.second.ctypes.data,
                                                self.status.ctypes.data, None, self.post.ctypes.data if self.mode else None,
                                                ctypes.byref(self.stats)))


def timed(arms, calls):
    """Every arm once as a warm-up, then `calls` rounds with the arms alternated -> per arm (wall seconds, score_ms)."""
    for a in arms:
        a.call()
    wall, ms = [[] for _ in arms], [[] for _ in arms]
    for _ in range(calls):
        for k, a in enumerate(arms):
            t0 = time.perf_counter()
            a.call()
            wall[k].append(time.perf_counter() - t0)
            ms[k].append(a.stats.score_ms)
    return wall, ms


def params_with(da, P):
    """The rates of bench_consensus.RATES with P duplication lengths, uniform."""
    p = da.MutatorParams.fromFlags(length=2 * P, **BC.RATES)            # --length L gives L / 2 duplication lengths
    assert p.c.n_len == P
    return p


def run_score(calls, scale):
    import dnastore_amd as da
    cfg = BC.RESCORE
    n = max(8, int(cfg["clusters"] * scale))
    cands, reads = BC.make_clusters(n)
    out = dict(part="score", clusters=n, reads_per_cluster=cfg["reads"], candidates_per_cluster=cfg["candidates"], nt=cfg["nt"],
               band=cfg["band"], calls=calls)
    p6 = da.MutatorParams.fromFlags(**BC.RATES)
    assert p6.c.n_len == 6
    vit, fwd = ScoreArm(p6, cands, reads, cfg["band"], 0), ScoreArm(p6, cands, reads, cfg["band"], 1)
    wall, ms = timed([vit, fwd], calls)
    items, cells = int(fwd.stats.items), int(fwd.stats.cells)
    out.update(items=items, band_cells=cells, chunks=int(fwd.stats.chunks))
    for name, k in (("viterbi", 0), ("forward", 1)):
        out["%s_p6_score_ms" % name] = med(ms[k])
        out["%s_p6_cells_per_s" % name] = cells / (med(ms[k]) / 1e3)
        out["%s_p6_score_spread" % name] = spread(ms[k])
        out["%s_p6_call_s" % name] = med(wall[k])
        out["%s_p6_items_per_s" % name] = items / med(wall[k])
        out["%s_p6_call_spread" % name] = spread(wall[k])
    out["forward_over_viterbi_kernel_time"] = out["forward_p6_score_ms"] / out["viterbi_p6_score_ms"]
    out["forward_over_viterbi_call_time"] = out["forward_p6_call_s"] / out["viterbi_p6_call_s"]
    out["winners_differ"] = int((vit.winner != fwd.winner).sum())
    for P in (2, 13):
        arm = ScoreArm(params_with(da, P), cands, reads, cfg["band"], 1)
        wall, ms = timed([arm], calls)
        out["forward_p%d_score_ms" % P] = med(ms[0])
        out["forward_p%d_cells_per_s" % P] = int(arm.stats.cells) / (med(ms[0]) / 1e3)
        out["forward_p%d_score_spread" % P] = spread(ms[0])
        out["forward_p%d_call_s" % P] = med(wall[0])
    return out


def run_decode(n_clusters, calls):
    import dnastore_amd as da
    machine = da.Machine.fromFile(os.path.join(ROOT, "tests", "golden", "ref_data", "s16h74l4c4.json"))
    params = da.MutatorParams.fromFlags(global_=True)
    rng = random.Random("bench-consensus/decode")                        # the pool of bench_consensus.run_decode
    nrng = np.random.default_rng(20261017)
    reads, labels, strands = [], [], []
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    for k in range(n_clusters):
        dna = np.frombuffer(machine.encodeBytes(bytes(rng.randrange(256) for _ in range(29))).encode(), dtype=np.uint8)
        strands.append(dna.tobytes().decode())
        for i in range(5):
            b = dna.copy()
            hit = nrng.random(len(b)) < .01
            cur = np.array([code[int(c)] for c in b[hit]], dtype=np.int64)
            b[hit] = letters[(cur + nrng.integers(1, 4, size=cur.size)) % 4]
            r = b.tobytes().decode()
            reads.append(da.reverse_complement(r) if i % 2 else r)
            labels.append(k)
    dec = da.ViterbiDecoder(machine, params, device=0)
    modes = ("viterbi", "forward")
    for m in modes:
        dec.decode_clusters(reads, labels, strands="both", band=32, score=m)             # warm-up
    wall, rescore, score_ms, res = {m: [] for m in modes}, {m: [] for m in modes}, {m: [] for m in modes}, {}
    for _ in range(calls):
        for m in modes:
            t0 = time.perf_counter()
            res[m] = dec.decode_clusters(reads, labels, strands="both", band=32, score=m)
            wall[m].append(time.perf_counter() - t0)
            rescore[m].append(res[m].stats["rescore_wall_ms"])
            score_ms[m].append(res[m].stats["score_ms"])
    dec.close()
    out = dict(part="decode", machine="s16h74l4c4.json", clusters=n_clusters, reads=len(reads), calls=calls,
               candidates=int(res["forward"].stats["candidates"]), items=int(res["forward"].stats["items"]))
    for m in modes:
        right = sum(machine.encodeSymbols(s) == strands[k] if s else False for k, s in enumerate(res[m].symbols))
        out.update({"%s_call_s" % m: med(wall[m]), "%s_call_spread" % m: spread(wall[m]), "%s_rescore_wall_ms" % m: med(rescore[m]),
                    "%s_score_ms" % m: med(score_ms[m]), "%s_clusters_right" % m: int(right)})
    out["forward_over_viterbi_call_time"] = out["forward_call_s"] / out["viterbi_call_s"]
    out["min_confidence"] = float(res["forward"].confidence.min())
    return out


def planted_pool(da, machine, noise, n_clusters=40, n_reads=3):
    """tests/test_gpu_consensus.py::planted_pool with the noise as an argument: the same seed and draw order."""
    import synth
    rng = random.Random("consensus/planted")
    messages, reads, labels = [], [], []
    for k in range(n_clusters):
        payload = bytes(rng.randrange(256) for _ in range(6))
        message = synth.bytes_to_symbols(payload)
        strand = machine.encodeSymbols(message)
        mine = [synth.mutate(strand, rng, **noise) for _ in range(n_reads)]
        flip = [rng.random() < .5 for _ in range(n_reads)]
        messages.append(message)
        reads += [da.reverse_complement(r) if f else r for r, f in zip(mine, flip)]
        labels += ["cluster%d" % k] * n_reads
    return messages, reads, labels


def run_planted():
    import dnastore_amd as da
    machine = da.Machine.fromFile(os.path.join(ROOT, "tests", "golden", "ref_data", "h74l4c4.json"))
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    dec = da.ViterbiDecoder(machine, params, device=0)
    out = dict(part="planted", machine="h74l4c4.json", clusters=40, reads_per_cluster=3, band=16, bins=list(BINS), levels=[])
    for name, noise in NOISE:
        messages, reads, labels = planted_pool(da, machine, noise)
        for polish in (0, 3):
            vit = dec.decode_clusters(reads, labels, strands="both", band=16, polish=polish)
            fwd = dec.decode_clusters(reads, labels, strands="both", band=16, polish=polish, score="forward")
            ok_v = np.array([s == m for s, m in zip(vit.symbols, messages)])
            ok_f = np.array([s == m for s, m in zip(fwd.symbols, messages)])
            conf = fwd.confidence
            table = []
            for lo, hi in zip(BINS, BINS[1:]):
                inside = (conf >= lo) & ((conf < hi) if hi < 1. else (conf <= hi))
                table.append(dict(lo=lo, hi=hi, clusters=int(inside.sum()), right=int(ok_f[inside].sum())))
            out["levels"].append(dict(noise=name, rates=noise, polish=polish, viterbi_right=int(ok_v.sum()), forward_right=int(ok_f.sum()),
                                      winners_differ=int(sum(a != b for a, b in zip(vit.symbols, fwd.symbols))),
                                      no_winner=int((conf == 0).sum()), calibration=table,
                                      confidence_of_wrong=[float(c) for c in conf[~ok_f]],
                                      min_confidence_of_right=float(conf[ok_f].min()) if ok_f.any() else None))
    dec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="sdp", help="s = score, d = decode, p = planted")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the score part's clusters (a rehearsal)")
    ap.add_argument("--decode-clusters", type=int, default=400)
    args = ap.parse_args()
    if args.calls < 5 and args.scale == 1.0:
        ap.error("the median needs at least 5 timed calls")
    if "s" in args.parts:
        print(json.dumps(run_score(args.calls, args.scale)), flush=True)
    if "d" in args.parts:
        print(json.dumps(run_decode(args.decode_clusters, args.calls)), flush=True)
    if "p" in args.parts:
        print(json.dumps(run_planted()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
