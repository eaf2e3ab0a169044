"""The structured pools of bitvector_cases.py through the kernels that run Myers' bit-vector recurrence (csrc/cluster_gate.hpp):
dnas_edit_distances on every route, dnas_cluster_reads_gated with the limit met exactly, dnas_trim_reads with every primer length
as F and as R.  test_bitvector_cpu.py holds the host statements to closed forms and independent restatements on the same pools, so
here every result is held to the host statement (and to the closed forms): equalities."""
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import bitvector_cases as B  # noqa: E402
import trim_cases as T  # noqa: E402
from test_cluster_cpu import cluster_models, same_results  # noqa: E402
from test_cluster_gate_cpu import codes, lev_np  # noqa: E402


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def ladder(da):
    """(reads, pairs, closed forms, the host's distances), the host after it met the closed forms."""
    reads, pairs, closed, _ = B.gate_ladder()
    want = da.editDistances(reads, pairs, host=True)
    assert B.check_closed(want, closed) >= 2 * 175 + 35
    return reads, pairs, closed, want


def held(got, want, closed):
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    B.check_closed(got, closed)


@pytest.mark.parametrize("words", (None, 0, 1, 2, 4))
def test_gate_ladder_every_route(da, ladder, monkeypatch, words):
    """1050 pairs, patterns of 1 to 11 words mixed within every wave: as shipped (the instance of 8 words and the long route), and
    with the register route capped at 4, 2, 1 and 0 words."""
    reads, pairs, closed, want = ladder
    if words is not None:
        monkeypatch.setenv("DNAS_CLUSTER_GATE_WORDS", str(words))
    held(da.editDistances(reads, pairs), want, closed)


def test_gate_ladder_every_instance(da, ladder):
    """The pairs whose pattern has at most 1, 2, 4 and 8 words, as shipped: the call's own bound picks the instance of that many
    words for all of them, and no long-route scratch is opened."""
    reads, pairs, closed, want = ladder
    for bound in (1, 2, 4, 8):
        keep = [q for q, p in enumerate(pairs) if B.pattern_words(reads, p) <= bound]
        assert max(B.pattern_words(reads, pairs[q]) for q in keep) == bound and len(keep) > 64
        held(da.editDistances(reads, [pairs[q] for q in keep]), want[keep], [closed[q] for q in keep])


def test_gate_ladder_all_devices(da, ladder, monkeypatch):
    reads, pairs, closed, want = ladder
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    held(da.editDistances(reads, pairs, device=-1), want, closed)


LIMIT_OPTIONS = dict(band=16, min_shared=0, edges=True, max_edit_permille=B.LIMIT_PERMILLE)


@pytest.fixture(scope="module")
def limit(da):
    """(reads, the closed-form counts, the host's result) of the pool at the gate's limit."""
    reads = B.limit_pool()
    edits = B.limit_edits(reads, lambda a, b: lev_np(codes(a), codes(b)))
    counts = B.limit_counts(reads, edits, B.LIMIT_PERMILLE)
    assert counts["at"] >= 40 and counts["above"] >= 40
    return reads, counts, da.clusterReads(dict(cluster_models(da))["P6"], reads, host=True, **LIMIT_OPTIONS)


@pytest.mark.parametrize("words", (None, 0))
def test_gate_at_its_limit(da, limit, monkeypatch, words):
    """Homopolymers of 90 to 110 bases and their reverse complements: 68 pairs with e == limit and 44 with e == limit + 1,
    through the register route's pass test and (capped at 0 words) through the ballot compaction of the long kernel."""
    reads, counts, want = limit
    if words is not None:
        monkeypatch.setenv("DNAS_CLUSTER_GATE_WORDS", str(words))
    got = da.clusterReads(dict(cluster_models(da))["P6"], reads, **LIMIT_OPTIONS)
    for found in (got, want):
        assert {k: found.gate[k] for k in ("tested", "passed", "word_steps")} == {k: counts[k] for k in ("tested", "passed", "word_steps")}
    assert got.gate["long_pairs"] == (counts["tested"] if words == 0 else 0)
    same_results(got, want)


@pytest.fixture(scope="module")
def trim_pool():
    return B.trim_ladder()


@pytest.mark.parametrize("max_offset", (0, 8, -1))
def test_trim_ladder(da, trim_pool, monkeypatch, max_offset):
    """64 pairs with F of 1 .. 64 and R of 64 .. 1 bases, homopolymers and repeats among them, 130 reads: the whole grid, then
    chunks of 5 pairs against the default and three workers."""
    primers, reads = trim_pool
    host = {}
    for permille, anchors in itertools.product((0, 250, 1000), ("both", "either")):
        options = dict(max_offset=max_offset, max_edit_permille=permille, anchors=anchors)
        host[permille, anchors] = T.arrays(da.trimReads(primers, reads, host=True, **options))
        got = da.trimReads(primers, reads, **options)
        T.assert_same(T.arrays(got), host[permille, anchors], options)
        assert got.stats["columns"] == B.trim_columns(primers, reads, max_offset) and got.stats["trimmed"] == int((got.status == 0).sum())
    options = dict(max_offset=max_offset, max_edit_permille=250, anchors="both")
    whole = da.trimReads(primers, reads, **options)
    monkeypatch.setenv("DNAS_TRIM_PAIR_CHUNK", "5")
    cut = da.trimReads(primers, reads, **options)
    monkeypatch.delenv("DNAS_TRIM_PAIR_CHUNK")
    T.assert_same(T.arrays(cut), T.arrays(whole), "chunks of 5")
    T.assert_same(T.arrays(cut), host[250, "both"], "chunks of 5 against the host")
    assert cut.stats["chunks"] == 13 and cut.stats["columns"] == whole.stats["columns"]
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    every = da.trimReads(primers, reads, device=-1, **options)
    T.assert_same(T.arrays(every), host[250, "both"], "three workers")
    assert every.stats["devices"] == 3 and every.stats["columns"] == whole.stats["columns"]
