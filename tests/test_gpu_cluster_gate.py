"""The edit-distance gate on the GPU (csrc/cluster_gate_kernels.hip): dnas_edit_distances against dnas_edit_distances_host on every
route of the kernels, and dnas_cluster_reads_gated against dnas_cluster_reads_gated_host, which test_cluster_gate_cpu.py holds to
a restatement of the definition.  Every comparison is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY, NOISY_FLAGS, _fasta  # noqa: E402
from test_cluster_cpu import BIN, DATA, K, candidates_py, cluster_models, is_planted, pool_a, pool_t, same_results, shape_pool  # noqa: E402
from test_cluster_gate_cpu import distance_cases  # noqa: E402

# three of test_gpu_cluster.CONFIGS: every model, every band, the filter off once
CONFIGS = (("P2", 4, 0), ("P6", 16, 2), ("P13-zero", -1, 2))


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def shapes(da):
    return shape_pool(da)


@pytest.fixture(scope="module")
def distances(da, shapes):
    """(reads, pairs, the host's distances): the cases of test_cluster_gate_cpu.test_distances and every pair of non-empty reads of
    the shape pool (its candidates at min_shared = 0) -- lengths of 0 to 1100 nt mixed within a wave."""
    reads, pairs, _ = distance_cases(da)
    at = len(reads)
    full = [i for i, r in enumerate(shapes) if r]
    pairs = pairs + [(at + i, at + j) for i in full for j in full if i < j]
    reads = reads + shapes
    assert len(pairs) % 64 and len(pairs) > 2048
    return reads, pairs, da.editDistances(reads, pairs, host=True)


def counts_of(found):
    return {key: value for key, value in found.gate.items() if key != "gate_ms"}


@pytest.mark.parametrize("words", (None, 0, 1, 2, 4))
def test_every_route(da, distances, monkeypatch, words):
    """As shipped (the instance of 8 words and, for the pair of 1100-nt reads and the patterns of 513 nt, the long route), and with
    the register route capped at 4, 2, 1 and 0 words: every instance and the long route meet patterns on both sides of their limit."""
    reads, pairs, want = distances
    if words is not None:
        monkeypatch.setenv("DNAS_CLUSTER_GATE_WORDS", str(words))
    got = da.editDistances(reads, pairs)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    patterns = {(min(len(reads[i]), len(reads[j])) + 63) // 64 for i, j in pairs}
    assert {0, 1, 2, 3, 4, 5, 8, 9} <= patterns and max(patterns) > 16


def test_few_pairs_and_all_devices(da, distances, monkeypatch):
    reads, pairs, want = distances
    assert da.editDistances(reads, []).shape == (0, 2)
    assert np.array_equal(da.editDistances(reads, pairs[-1:]), want[-1:])
    short = [(i, j) for i, j in pairs if len(reads[i]) <= 64 and len(reads[j]) <= 64][:70]       # the instance of one word alone
    assert np.array_equal(da.editDistances(reads, short), da.editDistances(reads, short, host=True))
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    assert np.array_equal(da.editDistances(reads, pairs, device=-1), want)
    assert np.array_equal(da.editDistances(reads, pairs[:2], device=-1), want[:2])


@pytest.mark.parametrize("permille", (0, 230, 300))
@pytest.mark.parametrize("name,band,min_shared", CONFIGS)
def test_shape_pool_against_the_host(da, shapes, monkeypatch, name, band, min_shared, permille):
    params = dict(cluster_models(da))[name]
    opts = dict(band=band, k=K, sketch=32, min_shared=min_shared, edges=True, max_edit_permille=permille)
    want = da.clusterReads(params, shapes, host=True, **opts)
    assert 0 < want.gate["passed"] < want.gate["tested"] == want.stats["candidates"] and want.stats["items"] == 2 * want.gate["passed"]
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    monkeypatch.setenv("DNAS_CLUSTER_CHUNK", "37")         # a prime: bands end inside rows
    got = da.clusterReads(params, shapes, **opts)
    same_results(got, want)
    assert counts_of(got) == counts_of(want)
    # a band without a survivor launches no score kernel: at 0 thousandths that is most of them
    cands = candidates_py(shapes, K, 32, min_shared)
    edits = da.editDistances(shapes, cands, host=True).min(axis=1)
    live = {q // 37 for q, (i, j) in enumerate(cands) if edits[q] <= permille * max(len(shapes[i]), len(shapes[j])) // 1000}
    bands = -(-len(cands) // 37)
    assert len(cands) == want.stats["candidates"] and got.stats["chunks"] == len(live) > 1 and (permille > 0 or len(live) < bands)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the band as shipped
    monkeypatch.delenv("DNAS_CLUSTER_CHUNK")
    got = da.clusterReads(params, shapes, **opts)
    same_results(got, want)
    assert counts_of(got) == counts_of(want) and got.stats["chunks"] == 1 and got.gate["gate_ms"] > 0 and got.stats["score_ms"] > 0


def test_long_route_in_the_cluster_call(da, shapes, monkeypatch):
    """The gate's routes inside the call: as shipped the pair of 1100-nt reads takes the long route; capped at one word most do."""
    params = da.MutatorParams.fromFlags(**NOISY)
    opts = dict(band=16, k=K, sketch=32, min_shared=0, edges=True, max_edit_permille=230)
    want = da.clusterReads(params, shapes, host=True, **opts)
    assert want.gate["long_pairs"] == 1
    for words in ("1", "0"):
        monkeypatch.setenv("DNAS_CLUSTER_GATE_WORDS", words)
        got = da.clusterReads(params, shapes, **opts)
        same_results(got, want)
        assert got.gate["passed"] == want.gate["passed"] and got.gate["word_steps"] == want.gate["word_steps"]
        assert got.gate["long_pairs"] == (want.gate["tested"] if words == "0" else
                                          sum(min(len(shapes[i]), len(shapes[j])) > 64 for i, j in zip(*np.triu_indices(len(shapes), 1))
                                              if shapes[i] and shapes[j]))


def test_pool_t_and_pool_a(da):
    """Pool T (257 reads: more than four filter tiles, a row with more candidates than a tile) and pool A."""
    params = da.MutatorParams.fromFlags(**NOISY)
    opts = dict(band=4, k=K, sketch=16, min_shared=2, edges=True, max_edit_permille=100)
    reads = pool_t(da)
    want = da.clusterReads(params, reads, host=True, **opts)
    got = da.clusterReads(params, reads, **opts)
    same_results(got, want)
    assert counts_of(got) == counts_of(want) and 0 < want.gate["passed"] <= want.gate["tested"] == want.stats["candidates"] > 2000
    reads, truth = pool_a(da)
    params = da.MutatorParams.fromFlags()
    want = da.clusterReads(params, reads, host=True, edges=True, max_edit_permille=300)
    got = da.clusterReads(params, reads, edges=True, max_edit_permille=300)
    same_results(got, want)
    assert counts_of(got) == counts_of(want) and is_planted(got, truth)
    assert got.stats["candidates"] == 439 and got.gate["passed"] == 120 and got.stats["edges"] == 120


def test_all_devices(da, shapes, monkeypatch):
    params = da.MutatorParams.fromFlags(**NOISY)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    for min_shared in (0, 2):
        opts = dict(band=16, k=K, min_shared=min_shared, edges=True, max_edit_permille=230)
        one = da.clusterReads(params, shapes, device=0, **opts)
        every = da.clusterReads(params, shapes, device=-1, **opts)
        same_results(every, one)
        assert counts_of(every) == counts_of(one) and every.stats["chunks"] > one.stats["chunks"] == 1


def test_decode_pool(da):
    reads, _ = pool_a(da)
    reads = reads[:36]
    machine = da.Machine.fromFile(os.path.join(DATA, "h74l4c4.json"))
    dec = da.ViterbiDecoder(machine, da.MutatorParams.fromFlags(**NOISY), device=0)
    want = dec.decode_pool(reads, band=16)
    got = dec.decode_pool(reads, band=16, max_edit_permille=300)
    dec.close()
    assert want.clusters.gate is None and got.clusters.gate["passed"] < got.clusters.gate["tested"] == got.clusters.stats["candidates"]
    assert got.symbols == want.symbols and np.array_equal(got.read, want.read) and got.labels == want.labels
    assert np.array_equal(got.total.view(np.uint64), want.total.view(np.uint64)) and np.array_equal(got.status, want.status)


def test_cli(da, tmp_path):
    reads, _ = pool_a(da)
    reads = reads[:36]
    pool = str(tmp_path / "pool.fa")
    _fasta(pool, ["read%d" % i for i in range(len(reads))], reads)
    run = lambda args: subprocess.run([BIN] + NOISY_FLAGS + args, capture_output=True, timeout=300)
    labels = ["--cluster-reads", pool, "--align-band", "16"]
    ungated, gated = run(["-v0"] + labels), run(["-v3"] + labels + ["--cluster-max-edit", "300"])
    assert ungated.returncode == 0 and gated.returncode == 0, gated.stderr.decode()
    assert gated.stdout == ungated.stdout and len(gated.stdout.split()) == 36
    assert b"Edit-distance gate: " in gated.stderr and b"Edit-distance gate" not in run(["-v3"] + labels).stderr
    decode = ["-v0", "-L", os.path.join(DATA, "h74l4c4.json"), "-V", pool, "--both-strands", "--align-band", "16", "--cluster-auto"]
    ungated, gated = run(decode), run(decode + ["--cluster-max-edit", "300"])
    assert ungated.returncode == 0 and gated.returncode == 0, gated.stderr.decode()
    assert gated.stdout == ungated.stdout and gated.stdout.count(b">") == 12
