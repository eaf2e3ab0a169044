"""Clustering a pool of reads on the GPU (csrc/cluster_kernels.hip): dnas_cluster_reads against its host statement
dnas_cluster_reads_host, which test_cluster_cpu.py holds to a Python restatement of the definition.  Every comparison is an
equality: roots, ids, strands, statuses, the sorted edges with their scores as uint64 bit patterns, and the counts."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY  # noqa: E402
from test_cluster_cpu import DATA, K, cluster_models, is_planted, partition, pool_a, same_results, shape_pool  # noqa: E402

# every model with every band; min_shared = 0 (every pair is scored) once per model and once per band
CONFIGS = (("P2", 4, 0), ("P2", 16, 2), ("P2", -1, 2), ("P6", 4, 2), ("P6", 16, 0), ("P6", -1, 2),
           ("P13-zero", 4, 2), ("P13-zero", 16, 2), ("P13-zero", -1, 0))


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def shapes(da):
    return shape_pool(da)


@pytest.mark.parametrize("name,band,min_shared", CONFIGS)
def test_every_shape_model_and_band(da, shapes, monkeypatch, name, band, min_shared):
    params = dict(cluster_models(da))[name]
    opts = dict(band=band, k=K, sketch=32, min_shared=min_shared, edges=True)
    want = da.clusterReads(params, shapes, host=True, **opts)
    assert want.stats["candidates"] > 37 and 0 < want.stats["edges"] and 1 < want.n_clusters < 67
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves over a band's 74 items: every wave walks several
    monkeypatch.setenv("DNAS_CLUSTER_CHUNK", "37")         # a prime: bands end inside rows
    got = da.clusterReads(params, shapes, **opts)
    same_results(got, want)
    assert got.stats["chunks"] == -(-want.stats["candidates"] // 37) > 1
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the band as shipped
    monkeypatch.delenv("DNAS_CLUSTER_CHUNK")
    got = da.clusterReads(params, shapes, **opts)
    same_results(got, want)
    assert got.stats["chunks"] == 1 and got.stats["score_ms"] > 0 and got.stats["sketch_ms"] > 0 and got.stats["filter_ms"] > 0


def test_sketch_sizes_and_floors(da, shapes):
    params = da.MutatorParams.fromFlags(**NOISY)
    for opts in (dict(k=5, sketch=16, min_shared=3), dict(k=12, sketch=64, min_shared=1), dict(k=31, sketch=32, min_shared=1),
                 dict(k=K, sketch=32, min_shared=2, min_score_per_nt=float("-inf")), dict(k=K, sketch=16, min_shared=1, min_score_per_nt=.5)):
        want = da.clusterReads(params, shapes, band=8, host=True, edges=True, **opts)
        same_results(da.clusterReads(params, shapes, band=8, edges=True, **opts), want)
        assert want.stats["candidates"] > 0
    floorless = da.clusterReads(params, shapes, band=8, k=K, min_score_per_nt=float("-inf"), edges=True)
    assert floorless.stats["edges"] == floorless.stats["candidates"]             # every candidate's best score, as the host has it
    # no reads, one read, reads without a candidate
    empty = da.clusterReads(params, [], edges=True)
    assert len(empty) == 0 and empty.edges[0].shape == (0, 2) and empty.stats["chunks"] == 0
    one = da.clusterReads(params, [shapes[0]])
    assert list(one.cluster) == [0] and one.stats["chunks"] == 0 and one.stats["candidates"] == 0
    apart = da.clusterReads(params, ["", "ACGT", "", "TTGCA"], edges=True)
    assert list(apart.cluster) == [0, 1, 2, 3] and list(apart.status) == [2, 1, 2, 1] and apart.stats["candidates"] == 0


def test_pool_a(da):
    reads, truth = pool_a(da)
    params = da.MutatorParams.fromFlags()
    want = da.clusterReads(params, reads, host=True, edges=True)
    got = da.clusterReads(params, reads, edges=True)
    same_results(got, want)
    assert is_planted(got, truth) and got.stats["candidates"] == 439 and got.stats["clusters"] == 40


def test_all_devices(da, shapes, monkeypatch):
    params = da.MutatorParams.fromFlags(**NOISY)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    for min_shared in (0, 2):
        opts = dict(band=16, k=K, min_shared=min_shared, edges=True)
        one = da.clusterReads(params, shapes, device=0, **opts)
        every = da.clusterReads(params, shapes, device=-1, **opts)
        same_results(every, one)
        assert every.stats["chunks"] > one.stats["chunks"] == 1                  # the bands were dealt
    same_results(da.clusterReads(params, shapes[:3], device=-1, edges=True), da.clusterReads(params, shapes[:3], host=True, edges=True))


def test_decode_pool(da):
    """Clusters found, then decoded: the partition and the messages of decode_clusters with the planted labels."""
    reads, truth = pool_a(da)
    reads, truth = reads[:36], truth[:36]
    machine = da.Machine.fromFile(os.path.join(DATA, "h74l4c4.json"))
    dec = da.ViterbiDecoder(machine, da.MutatorParams.fromFlags(**NOISY), device=0)
    got = dec.decode_pool(reads, band=16)
    want = dec.decode_clusters(reads, [c for c, _ in truth], band=16)
    dec.close()
    assert partition(got.clusters.cluster) == partition(c for c, _ in truth) and got.labels == list(range(12))
    assert got.symbols == want.symbols and np.array_equal(got.read, want.read)
    assert np.array_equal(got.total.view(np.uint64), want.total.view(np.uint64)) and np.array_equal(got.status, want.status)
