"""The edit-distance gate of dnas_cluster_reads_gated on the host (csrc/host/cluster.cpp) and dnas_edit_distances_host -- no GPU.

The expectation is built here, independently of the library: lev_np is a numpy Levenshtein (row by row, the insertions by
minimum.accumulate), the limit and the pass test are restated in Python integers, and a gated call is held to the ungated call's
edges kept where the restated distances pass, and to cluster_py's union over the candidates that pass."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import test_cluster_cpu as tc  # noqa: E402
from test_assign_cpu import NOISY, _bits, _fasta, _rand  # noqa: E402
from test_cluster_cpu import BIN, K, cluster_py, is_planted, partition, pool_a, pool_b, shape_pool  # noqa: E402

PERMILLES = (0, 100, 230, 300, 1000)
LENGTHS = ((0, 0), (0, 5), (1, 1), (63, 64), (64, 64), (65, 64), (128, 129), (200, 129))
MORE_LENGTHS = ((256, 257), (300, 257), (512, 600), (513, 515))          # either side of 4 and of 8 words, the register route's last


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


# ------------------------------------------------------------------------------------------------ the definition, restated
def codes(read):
    return np.array(["ACGT".index(c) for c in read.upper()], dtype=np.int64)


def lev_np(a, b):
    """The Levenshtein distance of two code arrays."""
    at = np.arange(len(b) + 1)
    row = at.copy()
    for i, x in enumerate(a, 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[:-1] + (b != x), row[1:] + 1)          # substitution or match, deletion
        row = np.minimum.accumulate(new - at) + at                       # insertions: new[j] = min over j' <= j of new[j'] + j - j'
    return int(row[-1])


def edits_np(read_i, read_j):
    """e[0], e[1] of a candidate."""
    a, b = codes(read_i), codes(read_j)
    return lev_np(a, b), lev_np(a, 3 - b[::-1])


def passes(e, permille, len_i, len_j):
    return min(e) <= permille * max(len_i, len_j) // 1000


def distance_cases(da):
    """(reads, pairs, named) of test_distances, which the GPU tests run through every route of the kernels; named: the index in
    pairs of the cases with a known answer."""
    from test_pair_align_cpu import edited
    rng = random.Random("gate/distances")
    reads, pairs, named = [], [], {}

    def pair(a, b):
        reads.extend([a, b])
        pairs.append((len(reads) - 2, len(reads) - 1))

    for la, lb in LENGTHS + MORE_LENGTHS:
        pair(_rand(rng, la), _rand(rng, lb))                             # unrelated
        a = _rand(rng, la)
        b = edited(rng, a, 4)
        pair(a, (b + _rand(rng, lb))[:lb])                               # related: an edited copy, cut or filled to its length
        pair((b + _rand(rng, lb))[:lb], da.reverse_complement(a))
    long = [r for r in shape_pool(da) if len(r) > 1000]
    assert len(long) == 2
    pair(*long)
    a = _rand(rng, 150)
    named["equal"] = len(pairs)
    pair(a, a)                                                           # e[0] = 0
    named["turned"] = len(pairs)
    pair(a, da.reverse_complement(a))                                    # e[1] = 0
    half = _rand(rng, 45)
    named["palindrome"] = len(pairs)
    pair(half + da.reverse_complement(half), edited(rng, _rand(rng, 80), 3))   # a reverse palindrome against anything: e[0] = e[1]
    named["mono"] = len(pairs)
    pair("A" * 70, "C" * 131)
    named["same"] = len(pairs)
    pairs.append((pairs[named["palindrome"]][1],) * 2)                   # i = j
    pairs.append((pairs[3][1], pairs[3][0]))                             # j < i
    return reads, pairs, named


@pytest.fixture(scope="module")
def shape_edits(da):
    """The restated e[0], e[1] of every pair of non-empty reads of the shape pool: {(i, j): (e0, e1)}, computed once."""
    reads = shape_pool(da)
    code = [codes(r) for r in reads]
    turned = [3 - c[::-1] for c in code]
    return {(i, j): (lev_np(code[i], code[j]), lev_np(code[i], turned[j]))
            for i in range(len(reads)) for j in range(i + 1, len(reads)) if len(reads[i]) and len(reads[j])}


def gate_counts(reads, cands, edits, permille):
    """dnas_cluster_gate_stats without the time, from the definition."""
    words = lambda i, j: (min(len(reads[i]), len(reads[j])) + 63) // 64
    return dict(gate_ms=0.0, tested=len(cands), passed=sum(passes(edits[c], permille, len(reads[c[0]]), len(reads[c[1]])) for c in cands),
                long_pairs=sum(words(i, j) > 8 for i, j in cands),
                word_steps=sum(2 * words(i, j) * max(len(reads[i]), len(reads[j])) for i, j in cands))


# ---------------------------------------------------------------------------------------------------------------- tests
def test_distances(da):
    reads, pairs, named = distance_cases(da)
    got = da.editDistances(reads, pairs, host=True)
    assert got.shape == (len(pairs), 2) and got.dtype == np.int32
    want = [edits_np(reads[i], reads[j]) for i, j in pairs]
    assert [tuple(int(x) for x in e) for e in got] == want
    assert want[0] == (0, 0) and want[3] == (5, 5) and want[-1] == (5, 5)            # d("", b) = len(b), either way round
    assert want[named["equal"]][0] == 0 < want[named["equal"]][1] and want[named["turned"]][1] == 0 < want[named["turned"]][0]
    assert want[named["palindrome"]][0] == want[named["palindrome"]][1] > 0
    assert want[named["mono"]] == (131, 131) and want[named["same"]][0] == 0
    assert max(max(e) for e in want) > 512 and {len(reads[i]) for i, _ in pairs} >= {0, 1, 63, 64, 65, 128, 200}
    assert da.editDistances(reads, [], host=True).shape == (0, 2)
    assert da.editDistances(reads, pairs[:1], host=True).tolist() == [list(want[0])]


@pytest.mark.parametrize("min_shared", (0, 2))
def test_gated_equals_filtered_ungated(da, shape_edits, monkeypatch, min_shared):
    reads = shape_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    opts = dict(band=16, k=K, sketch=32, min_shared=min_shared, host=True, edges=True)
    cands = tc.candidates_py(reads, K, 32, min_shared)
    ungated = da.clusterReads(params, reads, **opts)
    assert ungated.gate is None and ungated.stats["candidates"] == len(cands)
    edge_at = {tuple(int(x) for x in ij): e for e, ij in enumerate(ungated.edges[0])}
    passed_at = {}
    for permille in PERMILLES:
        keep = [c for c in cands if passes(shape_edits[c], permille, len(reads[c[0]]), len(reads[c[1]]))]
        got = da.clusterReads(params, reads, max_edit_permille=permille, **opts)
        passed_at[permille] = len(keep)
        # the ungated call's edges, kept where the restated distances pass the restated limit
        rows = [edge_at[c] for c in keep if c in edge_at]
        assert [tuple(int(x) for x in ij) for ij in got.edges[0]] == [c for c in keep if c in edge_at]
        assert np.array_equal(_bits(got.edges[1]), _bits(ungated.edges[1][rows])) and np.array_equal(got.edges[2], ungated.edges[2][rows])
        # ... and the union over them as cluster_py makes it from the candidates that pass
        monkeypatch.setattr(tc, "candidates_py", lambda *_, keep=keep: keep)
        want = cluster_py(da, params, reads, band=16, k=K, m=32, min_shared=min_shared)
        monkeypatch.undo()
        assert [int(x) for x in got.root] == want["root"] and [int(x) for x in got.cluster] == want["cluster"]
        assert [int(x) for x in got.strand] == want["strand"] and [int(x) for x in got.status] == want["status"]
        assert [tuple(int(x) for x in ij) for ij in got.edges[0]] == [(i, j) for i, j, _, _ in want["edges"]]
        assert np.array_equal(_bits(got.edges[1]), _bits([e[2] for e in want["edges"]]))
        # the counts
        assert got.gate == gate_counts(reads, cands, shape_edits, permille)
        assert got.gate["tested"] == got.stats["candidates"] == len(cands) and got.gate["passed"] == len(keep)
        assert got.stats["items"] == 2 * len(keep) and got.stats["cells"] == want["counts"]["cells"]
        assert {key: got.stats[key] for key in ("pairs", "edges", "clusters", "strand_conflicts")} == \
               {key: want["counts"][key] for key in ("pairs", "edges", "clusters", "strand_conflicts")}
        assert got.stats["chunks"] == 0 and got.stats["score_ms"] == 0
    assert passed_at[1000] == len(cands) and 0 < passed_at[0] < passed_at[100] <= passed_at[230] <= passed_at[300] < len(cands)
    assert got.stats == ungated.stats and all(np.array_equal(a, b) for a, b in zip(got.edges, ungated.edges))   # at 1000
    # at 0 only pairs that are identical in some orientation pass
    zero = [c for c in cands if 0 in shape_edits[c]]
    assert passed_at[0] == len(zero) and all(reads[i] in (reads[j], da.reverse_complement(reads[j])) for i, j in zero)
    if min_shared == 0:                                                  # the two reads of 1100 nt are the one pair with a pattern beyond 512 rows
        assert got.gate["long_pairs"] == 1


def test_permille_minus_one_is_the_old_entry_point(da):
    """dnas_cluster_reads_host, called as before, against clusterReads, which goes through dnas_cluster_reads_gated_host."""
    import ctypes
    reads = shape_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    new = da.clusterReads(params, reads, band=16, k=K, sketch=32, min_shared=2, host=True, edges=True, max_edit_permille=-1)
    assert new.gate is None
    n = len(reads)
    seqs = np.concatenate([tc_codes.astype(np.int8) for tc_codes in map(codes, reads)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    root, cluster = np.zeros(n, np.int64), np.zeros(n, np.int64)
    strand, status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    e_ij, e_score, e_strand, n_edges = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    st = da.lib.ClusterStatsC()
    L = da.lib.lib()
    assert L.dnas_cluster_reads_host(params.c, 16, K, 32, 2, 0.0, n, seqs.ctypes.data, off.ctypes.data, root.ctypes.data, cluster.ctypes.data,
                                     strand.ctypes.data, status.ctypes.data, ctypes.byref(e_ij), ctypes.byref(e_score),
                                     ctypes.byref(e_strand), ctypes.byref(n_edges), ctypes.byref(st)) == 0
    ne = n_edges.value
    take = lambda p, ctype, count: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)).copy()
    old_edges = (take(e_ij, ctypes.c_int64, 2 * ne).reshape(ne, 2), take(e_score, ctypes.c_uint64, ne), take(e_strand, ctypes.c_uint8, ne))
    for p in (e_ij, e_score, e_strand):
        L.dnas_free(p)
    assert np.array_equal(root, new.root) and np.array_equal(cluster, new.cluster) and np.array_equal(strand, new.strand)
    assert np.array_equal(status, new.status) and ne == len(new.edges[0]) > 0
    assert np.array_equal(old_edges[0], new.edges[0]) and np.array_equal(old_edges[1], _bits(new.edges[1]))
    assert np.array_equal(old_edges[2], new.edges[2])
    assert {k: getattr(st, k) for k, _ in st._fields_} == new.stats


def test_the_limits_edge(da, shape_edits):
    reads = shape_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    (i, j), e = next((c, e) for c, e in sorted(shape_edits.items()) if 0 < min(e) < 12 and max(len(reads[c[0]]), len(reads[c[1]])) > 100)
    D, L = min(e), max(len(reads[i]), len(reads[j]))
    p = next(p for p in range(1001) if p * L // 1000 == D)               # the smallest permille whose limit is D
    q = max(q for q in range(1001) if q * L // 1000 == D - 1)            # the largest whose limit is D - 1
    assert q == p - 1 and L < 1000
    run = lambda permille: da.clusterReads(params, [reads[i], reads[j]], band=16, min_shared=0, host=True, edges=True,
                                           max_edit_permille=permille)
    at, below = run(p), run(q)
    assert at.gate["tested"] == below.gate["tested"] == 1 and at.gate["passed"] == 1 and below.gate["passed"] == 0
    assert at.stats["items"] == 2 and at.stats["edges"] == 1 and list(at.cluster) == [0, 0]
    assert below.stats["items"] == 0 and below.stats["cells"] == 0 and below.stats["edges"] == 0 and list(below.cluster) == [0, 1]
    assert below.stats["candidates"] == 1 and below.edges[0].shape == (0, 2)


def test_pools_a_and_b(da):
    """Pool A at 300 thousandths: all 120 edges are among the 120 of 439 candidates that pass.  Pool B (NOISY, band 16, default
    filter): 90 of 144 pass and the partition is the ungated one.  Counted with the host statement and a numpy Levenshtein."""
    reads, truth = pool_a(da)
    got = da.clusterReads(da.MutatorParams.fromFlags(), reads, host=True, edges=True, max_edit_permille=300)
    assert is_planted(got, truth)
    assert got.stats["candidates"] == 439 and got.gate["passed"] == 120 and got.stats["edges"] == 120 and got.gate["tested"] == 439
    reads, truth = pool_b(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    ungated = da.clusterReads(params, reads, band=16, host=True, edges=True)
    got = da.clusterReads(params, reads, band=16, host=True, edges=True, max_edit_permille=300)
    assert partition(got.cluster) == partition(ungated.cluster) and np.array_equal(got.strand, ungated.strand)
    assert got.stats["candidates"] == 144 and got.gate["passed"] == 90 and got.stats["edges"] == ungated.stats["edges"] == 90


def test_argument_errors(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    reads = ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"]
    for bad in (-2, 1001):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.clusterReads(params, reads, host=True, max_edit_permille=bad)
    for pairs in ([(0, 2)], [(-1, 0)], [(0, 1), (2, 0)]):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.editDistances(reads, pairs, host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.editDistances([], [(0, 0)], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.editDistances([np.array([0, 4], np.int8)], [(0, 0)], host=True)
    assert da.editDistances([], [], host=True).shape == (0, 2)
    assert da.clusterReads(params, reads, host=True, max_edit_permille=0).gate["tested"] == 1


def test_cli_usage(tmp_path):
    pool = str(tmp_path / "pool.fa")
    _fasta(pool, ["a", "b"], ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"])
    run = lambda args: subprocess.run([BIN, "-v0"] + args, capture_output=True, timeout=60)
    for args in (["--cluster-reads", pool, "--cluster-max-edit", "-2"], ["--cluster-reads", pool, "--cluster-max-edit", "1001"],
                 ["--cluster-reads", pool, "--cluster-max-edit"], ["--cluster-max-edit", "300"],
                 ["-V", pool, "--cluster-file", pool, "--cluster-max-edit", "300"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b"" and bad.stderr, args
    assert b"--cluster-max-edit" in run(["--help"]).stdout
