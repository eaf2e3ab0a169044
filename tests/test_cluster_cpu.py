"""Clustering a pool of reads on the host (dnas_cluster_reads_host, csrc/host/cluster.cpp) -- no GPU, but for the command line,
which has no host arm.

The expectation is built here, independently of the library: sketch_py transcribes the signature of include/dnastore_amd.h,
dnas_align_pairs_host on the expanded (candidate, strand) list gives the item scores, and cluster_py restates the filter, the pick
and the components over them (by relabelling, not by the library's union-find)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")
DATA = os.path.join(_HERE, "golden", "ref_data")

import synth  # noqa: E402
from test_assign_cpu import NOISY, NOISY_FLAGS, _bits, _fasta, _rand  # noqa: E402

NEG = float("-inf")
MASK = (1 << 64) - 1
NOSIG = 0xFFFFFFFF
K = 8                                                        # the k of the shape pool


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


# ------------------------------------------------------------------------------------------------ the definition, restated
def mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK
    return x ^ x >> 31


def kmer_codes(read, k):
    base = ["ACGT".index(c) for c in read.upper()]
    out = []
    for p in range(len(base) - k + 1):
        f = sum(base[p + q] << 2 * (k - 1 - q) for q in range(k))
        r = sum((3 - base[p + k - 1 - q]) << 2 * (k - 1 - q) for q in range(k))
        out.append(min(f, r))
    return out


def sketch_py(read, k, m):
    """sig[t] in plain Python integers."""
    codes = kmer_codes(read, k)
    return [min([mix64((c + (t + 1) * 0x9E3779B97F4A7C15) & MASK) >> 32 for c in codes] + [NOSIG]) for t in range(m)]


def sketch_np(read, k, m):
    """The same with numpy's wrapping uint64 arithmetic, for whole pools (test_signatures holds it to sketch_py)."""
    codes = np.array(kmer_codes(read, k), dtype=np.uint64)
    sig = np.full(m, NOSIG, dtype=np.uint64)
    if len(codes):
        with np.errstate(over="ignore"):
            for t in range(m):
                x = codes + np.uint64((t + 1) * 0x9E3779B97F4A7C15 & MASK)
                x ^= x >> np.uint64(30)
                x *= np.uint64(0xBF58476D1CE4E5B9)
                x ^= x >> np.uint64(27)
                x *= np.uint64(0x94D049BB133111EB)
                x ^= x >> np.uint64(31)
                sig[t] = (x >> np.uint64(32)).min()
    return sig.astype(np.uint32)


def candidates_py(reads, k, m, min_shared):
    sig = [sketch_np(r, k, m) for r in reads]
    out = []
    for i in range(len(reads)):
        for j in range(i + 1, len(reads)):
            if min_shared >= 1:
                ok = int(((sig[i] == sig[j]) & (sig[i] != NOSIG)).sum()) >= min_shared
            else:
                ok = len(reads[i]) > 0 and len(reads[j]) > 0
            if ok:
                out.append((i, j))
    return out


def cluster_py(da, params, reads, band=32, k=12, m=32, min_shared=2, floor=0.0):
    """Everything dnas_cluster_reads returns, from the definition."""
    n = len(reads)
    cands = candidates_py(reads, k, m, min_shared)
    ins = [reads[i] for i, _ in cands for _ in (0, 1)]
    outs = [r for _, j in cands for r in (reads[j], da.reverse_complement(reads[j]))]
    scores = da.alignPairs(params, ins, outs, band=band, host=True).score.reshape(len(cands), 2) if cands else np.zeros((0, 2))
    edges = []
    for (i, j), (s0, s1) in zip(cands, scores):
        strand = 1 if s1 > s0 else 0
        best = s1 if strand else s0
        if best >= floor * float(len(reads[j])):
            edges.append((i, j, best, strand))
    comp, flip, conflicts = list(range(n)), [0] * n, 0        # the component's smallest index, and the orientation relative to it
    for i, j, _, s in edges:
        if comp[i] == comp[j]:
            conflicts += flip[i] ^ flip[j] ^ s
            continue
        keep, go = min(comp[i], comp[j]), max(comp[i], comp[j])
        turn = flip[i] ^ flip[j] ^ s                          # the two roots relative to each other
        for x in range(n):
            if comp[x] == go:
                comp[x], flip[x] = keep, flip[x] ^ turn
    ids = {}
    for r in comp:
        ids.setdefault(r, len(ids))
    status = [2 if not len(r) else (1 if min_shared >= 1 and len(r) < k else 0) for r in reads]
    cells = 2 * sum(band_cells(len(reads[i]), len(reads[j]), band) for i, j in cands)
    counts = dict(pairs=n * (n - 1) // 2, candidates=len(cands), items=2 * len(cands), cells=cells, edges=len(edges),
                  clusters=len(ids), strand_conflicts=conflicts)
    return dict(cands=cands, scores=scores, edges=edges, root=comp, cluster=[ids[r] for r in comp], strand=flip, status=status,
                counts=counts)


def band_cells(I, O, band):
    b = I + O + 1 if band < 0 or band > I + O + 1 else band
    lo, hi = min(0, O - I) - b, max(0, O - I) + b
    return sum(min(ip + hi, O) - max(ip + lo, 0) + 1 for ip in range(I + 1))


def same_as_expected(got, want):
    assert [int(x) for x in got.root] == want["root"]
    assert [int(x) for x in got.cluster] == want["cluster"]
    assert [int(x) for x in got.strand] == want["strand"]
    assert [int(x) for x in got.status] == want["status"]
    ij, score, strand = got.edges
    assert [tuple(int(x) for x in e) for e in ij] == [(i, j) for i, j, _, _ in want["edges"]]
    assert np.array_equal(_bits(score), _bits([e[2] for e in want["edges"]]))
    assert [int(x) for x in strand] == [e[3] for e in want["edges"]]
    assert {key: got.stats[key] for key in want["counts"]} == want["counts"]
    assert got.n_clusters == want["counts"]["clusters"] and int(got.sizes.sum()) == len(want["root"])


def same_results(got, want, counts=("pairs", "candidates", "items", "cells", "edges", "clusters", "strand_conflicts")):
    """Two ReadClusters with edges, bit for bit."""
    for key in ("root", "cluster", "strand", "status"):
        assert np.array_equal(getattr(got, key), getattr(want, key)), key
    for a, b in zip(got.edges, want.edges):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                     b.view(np.uint64) if b.dtype == np.float64 else b)
    assert {key: got.stats[key] for key in counts} == {key: want.stats[key] for key in counts}


# ---------------------------------------------------------------------------------------------------------------- cases
def cluster_models(da):
    """P = 2, 6 and 13 duplication lengths: the three instances of the score kernel."""
    from test_pair_align_cpu import make_params
    zero = [1. / 12] * 13
    zero[4] = 0.
    return (("P2", make_params(da, [.7, .3])), ("P6", da.MutatorParams.fromFlags(**NOISY)),
            ("P13-zero", make_params(da, zero, pDelOpen=.05, pTanDup=.1)))


def shape_pool(da):
    """67 reads (a full filter tile and a ragged one): founders of 63, 64, 65, 129 and 200 nt (either side of the score kernel's
    64-row stripe), each with edited copies, reverse complements and an exact duplicate; two reads of about 1100 nt (the boundary
    row leaves LDS); reads of 0, 5, K and K + 1 nt; unrelated reads."""
    from test_gpu_pair_align import _related
    from test_pair_align_cpu import edited
    rng = random.Random("cluster/shapes")
    reads = []
    for n in (63, 64, 65, 129, 200):
        a = _rand(rng, n)
        reads += [a, edited(rng, a, 3), da.reverse_complement(edited(rng, a, 3)), a, da.reverse_complement(a)]
        reads += [edited(rng, a, 4), da.reverse_complement(edited(rng, a, 2)), edited(rng, a, 6)]
    long = _rand(rng, 1100)
    reads += [long, da.reverse_complement(_related(rng, long, 1096))]
    reads += ["", _rand(rng, 5), _rand(rng, K), _rand(rng, K + 1)]
    reads += [_rand(rng, rng.randrange(20, 140)) for _ in range(21)]
    order = list(range(len(reads)))
    rng.shuffle(order)
    reads = [reads[i] for i in order]
    assert len(reads) == 67
    return reads


def planted_pool(da, nbytes=16, sub=.01, dele=.005, dup=.005, clusters=40, per=3, seed="cluster/planted"):
    """clusters x per reads on h74l4c4.json: per cluster a random payload, encoded, and per read synth.mutate of the strand,
    reverse-complemented with probability 1/2.  -> (reads, [(cluster, turned)])."""
    from oracle import oracle as O
    machine = O.Machine.from_file(os.path.join(DATA, "h74l4c4.json"))
    rng = random.Random(seed)
    reads, truth = [], []
    for c in range(clusters):
        payload = bytes(rng.randrange(256) for _ in range(nbytes))
        strand = synth.encode(machine, synth.bytes_to_symbols(payload))
        for _ in range(per):
            read = synth.mutate(strand, rng, sub=sub, dele=dele, dup=dup)
            turned = rng.random() < .5
            reads.append(da.reverse_complement(read) if turned else read)
            truth.append((c, int(turned)))
    return reads, truth


def pool_a(da):
    return planted_pool(da)


def pool_b(da):
    return planted_pool(da, nbytes=6, sub=.04, dele=.02, dup=.01)


def source_constant(filename, name):
    """The value of `constexpr int <name> = <integer>;` in dnastore_amd/csrc/<filename>.  The shapes of the tests that stand on a
    kernel's tile or LDS budget are built from the source's own number, so that they move with it; not finding it is an error."""
    import re
    with open(os.path.join(ROOT, "dnastore_amd", "csrc", filename)) as f:
        found = re.findall(r"^\s*constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), f.read(), re.M)
    if len(found) != 1:
        raise RuntimeError("%s: expected one 'constexpr int %s = <integer>;', found %d" % (filename, name, len(found)))
    return int(found[0])


def one_edit(rng, a):
    """a after one substitution, one deleted base or one base copied in tandem."""
    at, kind = rng.randrange(len(a)), rng.choice("sdt")
    if kind == "s":
        return a[:at] + rng.choice([b for b in "ACGT" if b != a[at]]) + a[at + 1:]
    return a[:at] + a[at + 1:] if kind == "d" else a[:at + 1] + a[at] + a[at + 1:]


def pool_t(da, tile=None):
    """4 tile + 1 reads (tile: the filter's kClTile; 257 reads) of 37 - 43 nt in families: a founder of 38 - 42 nt and copies of it
    with one edit each, every other copy turned round.  One family of 71, the others of 1, 2, 3 or 6; shuffled.  Under a filter
    (k = 8) the rows of the big family's first members have more candidates than a tile has columns, spread over every column
    tile; the last member of every family has none."""
    tile = tile or source_constant("cluster_kernels.hip", "kClTile")
    n = 4 * tile + 1
    rng = random.Random("cluster/pool-t")
    sizes = [tile + 7]
    while sum(sizes) < n:
        sizes.append(min(rng.choice((1, 2, 3, 6)), n - sum(sizes)))
    reads = []
    for size in sizes:
        founder = _rand(rng, rng.randint(38, 42))
        copies = [one_edit(rng, founder) for _ in range(size - 1)]
        reads += [founder] + [da.reverse_complement(c) if i % 2 else c for i, c in enumerate(copies)]
    rng.shuffle(reads)
    assert len(reads) == n and 37 <= min(map(len, reads)) and max(map(len, reads)) <= 43
    return reads


def partition(labels):
    groups = {}
    for i, lab in enumerate(labels):
        groups.setdefault(int(lab), []).append(i)
    return sorted(groups.values())


def is_planted(found, truth):
    """The planted partition, and every read's orientation relative to its root."""
    return (partition(found.cluster) == partition(c for c, _ in truth)
            and all(int(found.strand[i]) == truth[i][1] ^ truth[int(found.root[i])][1] for i in range(len(truth))))


# ---------------------------------------------------------------------------------------------------------------- tests
def test_signatures(da):
    rng = random.Random("cluster/signatures")
    for k, m in ((1, 16), (8, 32), (12, 32), (12, 64), (31, 16), (31, 64)):
        reads = ["", _rand(rng, k - 1), _rand(rng, k), _rand(rng, k + 1), _rand(rng, 70), _rand(rng, 200)]
        reads += [da.reverse_complement(r) for r in reads]
        sig = da.clusterSketch(reads, k=k, sketch=m)
        assert sig.shape == (len(reads), m) and sig.dtype == np.uint32
        for r, s in zip(reads, sig):
            want = sketch_py(r, k, m)
            assert [int(x) for x in s] == want and [int(x) for x in sketch_np(r, k, m)] == want
            assert (len(r) < k) == all(x == NOSIG for x in want)
        half = len(reads) // 2
        assert np.array_equal(sig[:half], sig[half:])                     # a read and its reverse complement: one signature
        if k >= 8:                                                        # ... and different reads have different ones
            assert len({tuple(s) for s in sig[2:half]}) == half - 2
    assert da.clusterSketch([], k=12, sketch=32).shape == (0, 32)


CPU_CONFIGS = (("P2", 4, 0), ("P6", 16, 2), ("P13-zero", -1, 2), ("P6", 0, 0))


@pytest.mark.parametrize("name,band,min_shared", CPU_CONFIGS)
def test_shape_pool_matches_the_definition(da, name, band, min_shared):
    reads = shape_pool(da)
    params = dict(cluster_models(da))[name]
    want = cluster_py(da, params, reads, band=band, k=K, m=32, min_shared=min_shared)
    got = da.clusterReads(params, reads, band=band, k=K, sketch=32, min_shared=min_shared, host=True, edges=True)
    same_as_expected(got, want)
    ij, scores = da.clusterCandidates(params, reads, band=band, k=K, sketch=32, min_shared=min_shared)
    assert [tuple(int(x) for x in c) for c in ij] == want["cands"]
    assert np.array_equal(_bits(scores), _bits(want["scores"]))          # both items of every candidate, as bits
    assert set(want["status"]) == ({0, 1, 2} if min_shared else {0, 2})
    assert got.stats["sketch_ms"] == 0 and got.stats["chunks"] == 0
    if min_shared == 0:
        empty = sum(1 for r in reads if not r)
        assert want["counts"]["candidates"] == (67 - empty) * (66 - empty) // 2
    else:
        assert 0 < want["counts"]["candidates"] < want["counts"]["pairs"] // 4
    # every founder's family is one cluster under the models that allow its edits
    if name == "P6":
        assert want["counts"]["clusters"] < 40 and max(got.sizes) >= 8
    # without the edge list nothing else changes
    bare = da.clusterReads(params, reads, band=band, k=K, sketch=32, min_shared=min_shared, host=True)
    assert bare.edges is None and np.array_equal(bare.cluster, got.cluster) and bare.stats == got.stats


def test_other_sketch_sizes(da):
    reads = shape_pool(da)[:40]
    params = da.MutatorParams.fromFlags(**NOISY)
    for k, m, min_shared in ((5, 16, 3), (12, 64, 1)):
        want = cluster_py(da, params, reads, band=8, k=k, m=m, min_shared=min_shared)
        same_as_expected(da.clusterReads(params, reads, band=8, k=k, sketch=m, min_shared=min_shared, host=True, edges=True), want)
        assert want["counts"]["candidates"] > 0


def test_pool_t_matches_the_definition(da):
    """Pool T (257 reads, more than four filter tiles) at min_shared = 2, sketch = 16, band = 4: the host statement, to which the
    GPU tests of test_gpu_pair_hmm_edges.py hold the tiled filter at this size, against the restated definition.  Measured with
    this host statement: 2802 candidates of 32 896 pairs, 72 in the fullest row, 61 rows without one, 2782 edges, 62 clusters."""
    reads = pool_t(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    want = cluster_py(da, params, reads, band=4, k=K, m=16, min_shared=2)
    got = da.clusterReads(params, reads, band=4, k=K, sketch=16, min_shared=2, host=True, edges=True)
    same_as_expected(got, want)
    ij, scores = da.clusterCandidates(params, reads, band=4, k=K, sketch=16, min_shared=2)
    assert [tuple(int(x) for x in c) for c in ij] == want["cands"] and np.array_equal(_bits(scores), _bits(want["scores"]))
    per_row = np.bincount(ij[:, 0], minlength=len(reads))
    print("pool T: %d candidates, fullest row %d, rows without one %d, %d edges, %d clusters"
          % (len(ij), per_row.max(), int((per_row == 0).sum()), want["counts"]["edges"], want["counts"]["clusters"]))
    tile = source_constant("cluster_kernels.hip", "kClTile")
    assert len(reads) == 4 * tile + 1 and per_row.max() > tile and 1 < want["counts"]["clusters"] < len(reads)


def test_ties_floor_and_conflicts(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("cluster/ties")
    run = lambda reads, **kw: da.clusterReads(params, reads, band=8, host=True, edges=True, **kw)
    # exact duplicates, one of them turned round: one cluster, the turned copy's strand is 1
    a = _rand(rng, 64)
    got = run([a, _rand(rng, 64), a, da.reverse_complement(a)])
    assert list(got.cluster) == [0, 1, 0, 0] and list(got.root) == [0, 1, 0, 0] and list(got.strand) == [0, 0, 0, 1]
    assert [tuple(e) for e in got.edges[0]] == [(0, 2), (0, 3), (2, 3)] and list(got.edges[2]) == [0, 1, 1]
    assert got.stats["strand_conflicts"] == 0 and list(got.sizes) == [3, 1]
    # a read that is its own reverse complement: both items score the same, strand 0
    half = _rand(rng, 32)
    pal = half + da.reverse_complement(half)
    assert da.reverse_complement(pal) == pal
    got = run([pal, pal])
    ij, scores = da.clusterCandidates(params, [pal, pal], band=8)
    assert _bits(scores)[0, 0] == _bits(scores)[0, 1] and list(got.strand) == [0, 0] and list(got.edges[2]) == [0]
    # exactly at the floor: len_j = 64, so (best / 64) * 64 is best again, exactly; one ulp above it the edge is gone
    b = synth.mutate(a, rng, sub=.1)
    assert len(b) == 64 and b != a
    best = float(run([a, b], min_shared=0, min_score_per_nt=NEG).edges[1][0])
    floor = best / 64
    assert floor * 64.0 == best and np.isfinite(best)
    at = run([a, b], min_shared=0, min_score_per_nt=floor)
    above = run([a, b], min_shared=0, min_score_per_nt=float(np.nextafter(floor, np.inf)))
    assert list(at.cluster) == [0, 0] and at.stats["edges"] == 1 and list(above.cluster) == [0, 1] and above.stats["edges"] == 0
    assert above.stats["candidates"] == 1 and above.edges[0].shape == (0, 2)
    # a planted strand conflict: x and y share their first half, y and z their second, and x's second half is z's first, turned
    # round -- (x, y) and (y, z) are forward, (x, z) is reverse: the last edge in (i, j) order contradicts the first two
    X, Y, Z = (_rand(rng, 60) for _ in range(3))
    trio = [X + Y, X + Z, da.reverse_complement(Y) + Z]
    want = cluster_py(da, params, trio, band=-1, min_shared=0, floor=NEG)
    got = da.clusterReads(params, trio, band=-1, min_shared=0, min_score_per_nt=NEG, host=True, edges=True)
    same_as_expected(got, want)
    assert list(got.edges[2]) == [0, 1, 0] and got.stats["strand_conflicts"] == 1 and list(got.strand) == [0, 0, 1]
    # random short reads with every pair an edge: conflicts as the restatement counts them
    noise = [_rand(rng, 30) for _ in range(8)]
    want = cluster_py(da, params, noise, band=-1, min_shared=0, floor=NEG)
    same_as_expected(da.clusterReads(params, noise, band=-1, min_shared=0, min_score_per_nt=NEG, host=True, edges=True), want)
    assert want["counts"]["strand_conflicts"] > 0 and want["counts"]["edges"] == 28 and want["counts"]["clusters"] == 1
    # no reads; one read; only empty reads
    got = run([])
    assert len(got) == 0 and got.n_clusters == 0 and got.edges[0].shape == (0, 2) and got.labels() == []
    assert all(v == 0 for v in got.stats.values())
    got = run([a])
    assert list(got.cluster) == [0] and got.stats["pairs"] == 0 and got.stats["clusters"] == 1
    got = run(["", "", "ACGT"], min_shared=0)
    assert list(got.cluster) == [0, 1, 2] and list(got.status) == [2, 2, 0] and got.stats["candidates"] == 0
    got = run(["", "ACGT", "ACGT"])
    assert list(got.status) == [2, 1, 1] and list(got.cluster) == [0, 1, 2]          # shorter than k: never a candidate


def test_pool_a_is_recovered(da):
    """Pool A (reads of 205 - 235 nt, three per strand) with the defaults gives exactly the planted partition and every relative
    orientation.  Measured with this host statement: k = 12, m = 32, min_shared = 2 leaves 439 of the 7 140 pairs."""
    reads, truth = pool_a(da)
    assert len(reads) == 120 and (min(map(len, reads)), max(map(len, reads))) == (205, 235)
    for params, band in ((da.MutatorParams.fromFlags(), 32), (da.MutatorParams.fromFlags(**NOISY), 16)):
        got = da.clusterReads(params, reads, band=band, host=True, edges=True)
        assert is_planted(got, truth)
        assert got.stats["candidates"] == 439 and got.stats["edges"] == 120 and got.stats["clusters"] == 40
        assert got.stats["strand_conflicts"] == 0 and list(got.sizes) == [3] * 40 and (got.status == 0).all()
        print("pool A: smallest edge score per base", float((got.edges[1] / [len(reads[j]) for _, j in got.edges[0]]).min()))


def test_pool_b_exact_mode_and_filter_limit(da):
    """Pool B (reads of 80 - 95 nt, sub .04, del .02, dup .01): with min_shared = 0 the planted partition; with the defaults the
    sketch loses some pairs (52 components for 40 strands, measured with this host statement), but every cluster found lies
    inside one planted cluster: the verification is the same in both modes."""
    reads, truth = pool_b(da)
    assert (min(map(len, reads)), max(map(len, reads))) == (80, 95)
    params = da.MutatorParams.fromFlags(**NOISY)
    exact = da.clusterReads(params, reads, band=16, min_shared=0, host=True)
    assert is_planted(exact, truth) and exact.stats["candidates"] == 7140
    found = da.clusterReads(params, reads, band=16, host=True)
    assert found.n_clusters >= 40
    for c in range(found.n_clusters):
        assert len({truth[i][0] for i in np.flatnonzero(found.cluster == c)}) == 1
    print("pool B: components with the default filter", found.n_clusters)


def test_argument_errors(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    reads = ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"]
    for bad in (dict(k=0), dict(k=32), dict(sketch=0), dict(sketch=48), dict(sketch=128), dict(min_shared=-1), dict(band=-2)):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.clusterReads(params, reads, host=True, **bad)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.clusterSketch(reads, k=40)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.clusterReads(params, [np.array([0, 4], np.int8)], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        from test_pair_align_cpu import make_params
        da.clusterReads(make_params(da, [1. / 14] * 14), reads, host=True)
    L = da.lib.lib()
    seqs, off = np.zeros(4, np.int8), np.array([0, 4], np.int64)
    assert L.dnas_cluster_reads_host(None, 8, 12, 32, 2, 0.0, 1, seqs.ctypes.data, off.ctypes.data, *([None] * 9)) == -1
    assert L.dnas_cluster_reads_host(params.c, 8, 12, 32, 2, 0.0, 1, seqs.ctypes.data, off.ctypes.data, *([None] * 9)) == -1
    assert L.dnas_cluster_reads_host(params.c, 8, 12, 32, 2, 0.0, 0, *([None] * 11)) == 0          # no reads: a valid call
    bad_off = np.array([1, 4], np.int64)
    out = [np.zeros(1, np.int64).ctypes.data] * 2 + [np.zeros(1, np.uint8).ctypes.data] * 2
    assert L.dnas_cluster_reads_host(params.c, 8, 12, 32, 2, 0.0, 1, seqs.ctypes.data, bad_off.ctypes.data, *out, *([None] * 5)) == -1
    assert L.dnas_cluster_reads_host(params.c, 8, 12, 32, 2, 0.0, 1, seqs.ctypes.data, off.ctypes.data, *out, *([None] * 5)) == 0


def test_cli_usage(tmp_path):
    pool = str(tmp_path / "pool.fa")
    _fasta(pool, ["a", "b"], ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"])
    run = lambda args: subprocess.run([BIN, "-v0"] + args, capture_output=True, timeout=60)
    for args in (["--cluster-reads", pool, "--cluster-kmer", "32"], ["--cluster-reads", pool, "--cluster-sketch", "48"],
                 ["--cluster-reads", pool, "--cluster-min-shared", "-1"], ["--cluster-reads", pool, "--align-band", "-2"],
                 ["--cluster-reads"], ["--cluster-auto"], ["--cluster-auto", "--cluster-reads", pool],
                 ["-V", pool, "--cluster-auto", "--cluster-file", pool], ["--cluster-table", "--cluster-reads", pool]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b"" and bad.stderr, args
    missing = run(["--cluster-reads", str(tmp_path / "none.fa")])
    assert missing.returncode == 1 and missing.stdout == b""
    assert b"--cluster-reads" in run(["--help"]).stdout and b"--cluster-auto" in run(["--help"]).stdout


@pytest.mark.gpu
def test_cli(da, tmp_path):
    """--cluster-reads prints what clusterReads finds, in the format --cluster-file reads: piped into -V it gives the records
    of --cluster-auto, which are those of the planted labels."""
    reads, truth = pool_a(da)
    reads, truth = reads[:36], truth[:36]
    pool, labels, planted = str(tmp_path / "pool.fa"), str(tmp_path / "labels.txt"), str(tmp_path / "planted.txt")
    _fasta(pool, ["read%d" % i for i in range(len(reads))], reads)
    machine = ["-L", os.path.join(DATA, "h74l4c4.json")]
    run = lambda args: subprocess.run([BIN, "-v0"] + NOISY_FLAGS + args, capture_output=True, timeout=300)
    r = run(["--cluster-reads", pool, "--align-band", "16"])
    assert r.returncode == 0, r.stderr.decode()
    found = da.clusterReads(da.MutatorParams.fromFlags(**NOISY), reads, band=16)
    assert r.stdout.decode().split() == ["cluster%d" % c for c in found.cluster] and is_planted(found, truth)
    exact = run(["--cluster-reads", pool, "--align-band", "16", "--cluster-min-shared", "0", "--cluster-kmer", "10", "--cluster-sketch",
                 "16", "--cluster-min-score", "0.25", "--device", "-1"])
    assert exact.returncode == 0 and exact.stdout == r.stdout
    with open(labels, "wb") as f:
        f.write(r.stdout)
    with open(planted, "w") as f:
        f.write("".join("cluster%d\n" % c for c, _ in truth))
    decode = machine + ["-V", pool, "--both-strands", "--align-band", "16"]
    piped, auto, want = run(decode + ["--cluster-file", labels]), run(decode + ["--cluster-auto"]), run(decode + ["--cluster-file", planted])
    assert piped.returncode == 0 and piped.stdout.count(b">") == 12
    assert auto.returncode == 0 and auto.stdout == piped.stdout == want.stdout
    table = run(decode + ["--cluster-auto", "--cluster-table"])
    assert table.returncode == 0 and [l.split("\t")[:2] for l in table.stdout.decode().splitlines()] == [["cluster%d" % c, "3"] for c in range(12)]
