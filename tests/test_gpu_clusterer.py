"""The persistent clusterer on the GPU (csrc/clusterer_kernels.hip): a pool built up in batches through dnas_clusterer_add
against the one-thread statement dnas_cluster_reads_gated_host on the concatenation, to which test_cluster_cpu.py and
test_cluster_gate_cpu.py hold a restatement of the definition.  Every comparison is an equality: roots, ids, strands, statuses,
the sorted edges with their scores as bit patterns, the counts, and the gate's counts -- whatever the batch boundaries, the row
segments and the band size."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY, NOISY_FLAGS, _fasta, _rand  # noqa: E402
from test_cluster_cpu import BIN, K, cluster_models, is_planted, pool_a, pool_t, same_results, shape_pool, source_constant  # noqa: E402

# the three CONFIGS of test_gpu_cluster_gate.py: every model, every band, the filter off once
CONFIGS = (("P2", 4, 0), ("P6", 16, 2), ("P13-zero", -1, 2))
COUNTS = ("pairs", "candidates", "items", "cells", "edges", "chunks")
GATE_COUNTS = ("tested", "passed", "long_pairs", "word_steps")
NEG = float("-inf")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def shapes(da):
    return shape_pool(da)


@pytest.fixture(scope="module")
def tpool(da):
    """(pool T, its host answer gated at 100 thousandths, the tile)."""
    reads = pool_t(da)
    want = da.clusterReads(da.MutatorParams.fromFlags(**NOISY), reads, host=True, **T_OPTS)
    return reads, want, source_constant("cluster_kernels.hip", "kClTile")


T_OPTS = dict(band=4, k=K, sketch=16, min_shared=2, edges=True, max_edit_permille=100)


def handle_options(opts):
    """clusterReads' options -> Clusterer's."""
    return {key: value for key, value in opts.items() if key != "edges"}


def same_pool(got, want):
    """same_results, and the gate's counts."""
    same_results(got, want)
    if want.gate is None:
        assert got.gate is None
    else:
        assert {key: got.gate[key] for key in GATE_COUNTS} == {key: want.gate[key] for key in GATE_COUNTS}


def cut(reads, sizes):
    """reads in batches of the given sizes, the rest as a last batch."""
    out, at = [], 0
    for size in sizes:
        out.append(reads[at:at + size])
        at += size
    if at < len(reads):
        out.append(reads[at:])
    assert sum(map(len, out)) == len(reads)
    return out


def feed(da, params, batches, **opts):
    """The batches through a fresh handle -> (the result, the adds' stats)."""
    with da.Clusterer(params, **handle_options(opts)) as h:
        adds = [h.add(batch) for batch in batches]
        assert h.n_reads == sum(map(len, batches))
        return h.result(edges=True), adds


def summed(adds, result):
    """The adds' own counts add up to the result's, and every add counts its own pairs."""
    n0 = 0
    for add, size in adds:
        assert add["pairs"] == size * n0 + size * (size - 1) // 2 and add["clusters"] == 0 and add["strand_conflicts"] == 0
        n0 += size
    for key in COUNTS:
        assert sum(add[key] for add, _ in adds) == result.stats[key], key
    if result.gate is not None:
        for key in GATE_COUNTS:
            assert sum(add["gate"][key] for add, _ in adds) == result.gate[key], key


@pytest.mark.parametrize("permille", (-1, 300))
@pytest.mark.parametrize("name,band,min_shared", CONFIGS)
def test_shape_pool_after_every_add(da, shapes, monkeypatch, name, band, min_shared, permille):
    """67 reads in batches of 1, 63, 1 and 2: a batch of one read, a batch that ends on the 64-column tile edge, a batch that is one
    tile's first column, the rest.  Bands of 37 pairs end inside columns, and there are several per add."""
    params = dict(cluster_models(da))[name]
    opts = dict(band=band, k=K, sketch=32, min_shared=min_shared, edges=True, max_edit_permille=permille)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    monkeypatch.setenv("DNAS_CLUSTER_CHUNK", "37")
    batches = cut(shapes, (1, 63, 1))
    assert [len(b) for b in batches] == [1, 63, 1, 2]
    adds, n = [], 0
    with da.Clusterer(params, **handle_options(opts)) as h:
        for batch in batches:
            adds.append((h.add(batch), len(batch)))
            n += len(batch)
            assert h.n_reads == n
            got = h.result(edges=True)
            same_pool(got, da.clusterReads(params, shapes[:n], host=True, **opts))
            assert np.array_equal(h.result().cluster, got.cluster) and h.result().edges is None      # asking changes nothing
        summed(adds, got)
    assert adds[1][0]["candidates"] > 2 * 37 and adds[1][0]["chunks"] > 1 and got.stats["edges"] > 0      # several bands in one add
    if permille >= 0:
        assert 0 < got.gate["passed"] < got.gate["tested"] == got.stats["candidates"]


def test_pool_t_in_tiles_and_in_one_add(da, tpool):
    """4 tiles + 1 reads with a family larger than a tile, in batches of tile - 1, 1, tile, tile + 1 and the rest: columns with
    more candidates than a row tile has rows, over every row tile and segment.  And as a single add: the triangle, N0 = 0."""
    reads, want, tile = tpool
    params = da.MutatorParams.fromFlags(**NOISY)
    batches = cut(reads, (tile - 1, 1, tile, tile + 1))
    got, adds = feed(da, params, batches, **T_OPTS)
    same_pool(got, want)
    summed(list(zip(adds, map(len, batches))), got)
    per_column = np.bincount(got.edges[0][:, 1], minlength=len(reads))
    assert len(batches) == 5 and per_column.max() > tile and want.stats["candidates"] > 2000
    one, adds = feed(da, params, [reads], **T_OPTS)
    same_pool(one, want)
    assert adds[0]["pairs"] == want.stats["pairs"] and adds[0]["candidates"] == want.stats["candidates"]


@pytest.mark.parametrize("segments", ("1", "3", "tiles+1"))
def test_row_segments(da, tpool, monkeypatch, segments):
    """The same split with the number of row segments forced: one, three, and one more than the pool has row tiles, so that
    segments are empty."""
    reads, want, tile = tpool
    row_tiles = -(-len(reads) // tile)
    monkeypatch.setenv("DNAS_CLUSTERER_SEGMENTS", str(row_tiles + 1) if segments == "tiles+1" else segments)
    monkeypatch.setenv("DNAS_CLUSTER_CHUNK", "101")
    got, _ = feed(da, da.MutatorParams.fromFlags(**NOISY), cut(reads, (tile - 1, 1, tile, tile + 1)), **T_OPTS)
    same_pool(got, want)


def test_growth(da):
    """Pool A (120 reads) in adds of 1, 2, .., 15 reads: the buffers grow several times and fit several times."""
    reads, truth = pool_a(da)
    params = da.MutatorParams.fromFlags()
    opts = dict(edges=True, max_edit_permille=300)
    batches = cut(reads, range(1, 16))
    assert [len(b) for b in batches] == list(range(1, 16)) and len(reads) == 120
    got, adds = feed(da, params, batches, **opts)
    same_pool(got, da.clusterReads(params, reads, host=True, **opts))
    same_pool(got, da.clusterReads(params, reads, **opts))
    summed(list(zip(adds, map(len, batches))), got)
    assert is_planted(got, truth) and got.stats["candidates"] == 439 and got.gate["passed"] == 120 and got.stats["edges"] == 120
    ungated, _ = feed(da, params, batches, edges=True)
    same_pool(ungated, da.clusterReads(params, reads, host=True, edges=True))


def test_gate_reopens_for_longer_patterns(da):
    """A gated handle whose later adds bring longer reads: eight 40-base reads, then eight with one of 200 bases among them, after
    every add the one-shot host answer on the concatenation, edges included.  A pair's pattern is its shorter read, so the gate's
    buffers are opened again for more words only once a second long read is there: two more adds bring a near copy of the 200-base
    read (4 words, still in registers) and two near copies of a 600-base read (10 words: the long route and its scratch)."""
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("clusterer/reopen")
    opts = dict(band=16, k=K, min_shared=0, edges=True, max_edit_permille=200)

    def near(read, subs):
        codes = list(read)
        for at in rng.sample(range(len(codes)), subs):
            codes[at] = {"A": "C", "C": "G", "G": "T", "T": "A"}[codes[at]]
        return "".join(codes)

    base = [_rand(rng, 40) for _ in range(6)]
    r200, r600 = _rand(rng, 200), _rand(rng, 600)
    batches = [base[:4] + [near(r, 2) for r in base[:4]],
               base[4:] + [near(r, 1) for r in base[:5]] + [r200],
               [near(r200, 9), near(base[5], 3)],
               [r600, near(r600, 30)]]
    assert [len(b) for b in batches] == [8, 8, 2, 2] and [max(map(len, b)) for b in batches] == [40, 200, 200, 600]
    pool = []
    with da.Clusterer(params, **handle_options(opts)) as h:
        for batch in batches:
            h.add(batch)
            pool += batch
            want = da.clusterReads(params, pool, host=True, **opts)
            same_pool(h.result(edges=True), want)
    assert want.gate["long_pairs"] == 1 and want.gate["tested"] == 20 * 19 // 2 and 8 < want.gate["passed"] < want.gate["tested"]
    assert want.stats["edges"] >= 10


def test_ties_and_conflicts(da):
    """A contradictory strand cycle (test_ties_floor_and_conflicts' trio) and exact duplicates, cut so that the edge that
    contradicts arrives in a later batch than the edges it contradicts, and so that later batches bring edges that sort in front
    of earlier ones; then random short reads with every pair an edge."""
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("clusterer/ties")
    opts = dict(band=-1, min_shared=0, min_score_per_nt=NEG, edges=True)
    X, Y, Z, a = (_rand(rng, 60) for _ in range(4))
    trio = [X + Y, X + Z, da.reverse_complement(Y) + Z]
    pool = [trio[0], a, trio[1], a, trio[2], da.reverse_complement(a)]
    want = da.clusterReads(params, pool, host=True, **opts)
    assert want.stats["strand_conflicts"] > 0 and want.stats["edges"] == 15
    for sizes in ((3, 1), (4, 1), (1, 1, 1, 1, 1), (5,)):
        got, _ = feed(da, params, cut(pool, sizes), **opts)
        same_pool(got, want)
    # the trio alone, its last read in a batch of its own: (0, 1) forward, then (0, 2) reverse and (1, 2) forward
    want = da.clusterReads(params, trio, host=True, **opts)
    got, _ = feed(da, params, cut(trio, (2,)), **opts)
    same_pool(got, want)
    assert list(want.edges[2]) == [0, 1, 0] and want.stats["strand_conflicts"] == 1 and list(got.strand) == [0, 0, 1]
    noise = [_rand(rng, 30) for _ in range(8)]
    opts = dict(band=-1, min_shared=0, min_score_per_nt=NEG, edges=True)
    want = da.clusterReads(params, noise, host=True, **opts)
    assert want.stats["strand_conflicts"] > 0 and want.stats["edges"] == 28
    got, _ = feed(da, params, cut(noise, (3, 3)), **opts)
    same_pool(got, want)


def test_refused_adds(da, shapes):
    params = da.MutatorParams.fromFlags(**NOISY)
    opts = dict(band=16, k=K, min_shared=2, edges=True, max_edit_permille=300)
    codes = [da.tokenize(r).astype(np.int8) for r in shapes]
    with da.Clusterer(params, **handle_options(opts)) as h:
        fresh = h.result(edges=True)                             # the N = 0 answer of the one-shot call
        same_pool(fresh, da.clusterReads(params, [], host=True, **opts))
        assert h.n_reads == 0 and len(fresh) == 0 and fresh.edges[0].shape == (0, 2) and all(v == 0 for v in fresh.stats.values())
        h.add(codes[:40])
        before = h.result(edges=True)
        bad = [c.copy() for c in codes[40:50]]
        bad[-1][-1] = 4
        with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
            h.add(bad)
        L = da.lib.lib()
        seqs, off = np.zeros(4, np.int8), np.array([1, 4], np.int64)
        assert L.dnas_clusterer_add(h.h, 1, seqs.ctypes.data, off.ctypes.data, None, None) == -1      # offsets that do not start at 0
        assert L.dnas_clusterer_add(h.h, 1, None, None, None, None) == -1 and L.dnas_clusterer_add(h.h, -1, None, None, None, None) == -1
        assert L.dnas_clusterer_add(h.h, 2 ** 31 - 40, seqs.ctypes.data, off.ctypes.data, None, None) == -9
        assert h.n_reads == 40
        same_pool(h.result(edges=True), before)
        assert h.result(edges=True).stats == {**before.stats}    # the times too: nothing ran
        nothing = h.add([])
        assert h.n_reads == 40 and all(nothing[key] == 0 for key in COUNTS)
        same_pool(h.result(edges=True), before)
        h.add(codes[40:])
        same_pool(h.result(edges=True), da.clusterReads(params, shapes, host=True, **opts))
    with pytest.raises(ValueError):
        h.add(codes[:1])
    with pytest.raises(ValueError):
        h.result()
    with pytest.raises(ValueError):
        h.n_reads
    h.close()                                                    # closing twice is allowed


def test_two_handles(da, shapes):
    """Two handles with different k and gate on one device, their adds interleaved."""
    params = da.MutatorParams.fromFlags(**NOISY)
    first = dict(band=16, k=K, sketch=32, min_shared=2, edges=True, max_edit_permille=230)
    second = dict(band=8, k=5, sketch=16, min_shared=3, edges=True)
    other = shapes[::-1]
    with da.Clusterer(params, **handle_options(first)) as a, da.Clusterer(params, **handle_options(second)) as b:
        a.add(shapes[:30])
        b.add(other[:10])
        a.add(shapes[30:31])
        b.add(other[10:66])
        b.add(other[66:])
        a.add(shapes[31:])
        same_pool(b.result(edges=True), da.clusterReads(params, other, host=True, **second))
        same_pool(a.result(edges=True), da.clusterReads(params, shapes, host=True, **first))


def test_cli(da, tmp_path):
    """--cluster-reads a.fa --cluster-add b.fa --cluster-add c.fa prints what --cluster-reads abc.fa prints."""
    reads, _ = pool_a(da)
    reads = reads[:36]
    names = ["read%d" % i for i in range(len(reads))]
    path = lambda name: str(tmp_path / name)
    _fasta(path("abc.fa"), names, reads)
    for name, part in (("a.fa", slice(0, 20)), ("b.fa", slice(20, 21)), ("c.fa", slice(21, 36))):
        _fasta(path(name), names[part], reads[part])
    run = lambda args: subprocess.run([BIN, "-v0"] + NOISY_FLAGS + ["--align-band", "16"] + args, capture_output=True, timeout=300)
    batched = ["--cluster-reads", path("a.fa"), "--cluster-add", path("b.fa"), "--cluster-add", path("c.fa")]
    for gate in ([], ["--cluster-max-edit", "300"]):
        whole, parts = run(["--cluster-reads", path("abc.fa")] + gate), run(batched + gate)
        assert whole.returncode == 0 and parts.returncode == 0, parts.stderr.decode()
        assert parts.stdout == whole.stdout and len(parts.stdout.split()) == 36 and len(set(parts.stdout.split())) == 12
    assert run(batched + ["--device", "-1"]).returncode == 1
