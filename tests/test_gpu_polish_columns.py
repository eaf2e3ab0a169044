"""dnas_cluster_consensus on the GPU on the pools of tests/polish_columns.py: templates that grow, the cap of the LDS route as
shipped, every round.  Every comparison is an equality: with the host statement, on the planted pool with the Python
restatement too, and of the call's counters with what the census of the restatement's rounds predicts.

What test_polish_columns_cpu.py guarantees of the inputs is what makes these equalities bite: under P1, P6 and P13-zero the
planted pool emits insertions with even V, with V > 64, as the fourth base of a gap, at gap I, in the first and the last lane
of a chunk of the emit, with a tie in B and out of truncated runs; deletions likewise, and of trailing bases alone (the one
case in which the new length alone tells plEmit that the template changed); every tie; clusters that change in a
second and a third round; templates that cross 64 bases in both directions."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import polish_columns as pc  # noqa: E402
from test_assign_cpu import BANDS, NOISY, models  # noqa: E402
from test_polish_cpu import NO_READS, NO_VOTERS, OK, T, same, same_result, two_round_cluster  # noqa: E402

ROUNDS = 4
CAPS = (None, pc.SMALL_CAP, 0)                                  # DNAS_POLISH_LDS_POSITIONS: as shipped, mixed routes, every table in HBM
COUNTERS = ("rounds", "pairs", "lds_clusters", "hbm_clusters")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("DNAS_POLISH_LDS_POSITIONS", raising=False)
        return pc.LDS_POSITIONS
    monkeypatch.setenv("DNAS_POLISH_LDS_POSITIONS", str(cap))
    return cap


def model(da, name):
    return [m for m in models(da) if m[0] == name][0][1]


# ------------------------------------------------------------------------------------------------------------ the planted pool
@pytest.mark.parametrize("batched", (False, True), ids=("one-batch", "small-arena"))
@pytest.mark.parametrize("cap", CAPS, ids=("shipped", "cap64", "cap0"))
def test_planted_pool(da, monkeypatch, cap, batched):
    """Every model and band.  As shipped every table is in LDS; with the cap at 64 the routes are mixed and clusters change
    route between rounds in both directions; with the cap at 0 every non-empty template has its table in HBM, the clusters of
    65 to 70 reads included (more pairs than one work-group of the vote kernel has threads).  small-arena: two work-groups of
    the fill and an arena of 1 MiB, so that a round takes several batches, some with clusters of one route only."""
    limit = set_cap(monkeypatch, cap)
    monkeypatch.delenv("DNAS_FAKE_DEVICES", raising=False)
    if batched:
        monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    else:
        monkeypatch.delenv("DNAS_ALIGN_BLOCKS", raising=False)
    for name, params in models(da):
        for band in BANDS:
            (templates, reads, strands), (want, kinds, trace), host = pc.cached(da, pc.planted_pool, name, params, band, ROUNDS, pc.SMALL_CAP)
            got = da.consensusReads(params, templates, reads, band=band, read_strand=strands, rounds=ROUNDS, device=0,
                                    arena_bytes=1 << 20 if batched else 0)
            print(name, band, got.stats)
            same_result(got, host)
            same(got, want)
            predicted = pc.predicted_stats(trace, limit)
            assert {k: got.stats[k] for k in COUNTERS} == {k: predicted[k] for k in COUNTERS}, (name, band)
            if batched:
                assert got.stats["batches"] > got.stats["rounds"]
            else:
                assert got.stats["batches"] == predicted["batches"] == got.stats["rounds"]
            if cap == pc.SMALL_CAP and name in ("P1", "P6", "P13-zero"):
                assert kinds["cross_up"] > 0 and kinds["cross_down"] > 0 and predicted["lds_clusters"] > 0 and predicted["hbm_clusters"] > 0
            if cap == 0:
                assert predicted["lds_clusters"] == sum(1 for r in trace for _, I, _ in r if I == 0) <= 1
            if cap is None:
                assert predicted["hbm_clusters"] == 0


# -------------------------------------------------------------------------------------------------------------- the limit pool
@pytest.mark.parametrize("band", (8, -1))
@pytest.mark.parametrize("name", ("P6", "P13-zero"))
def test_limit_pool_as_shipped(da, monkeypatch, name, band):
    """Templates of L - 1, L and L + 1 bases, L = kPolishLdsPositions: a work-group asks for the whole table of L + 1 rows in
    LDS (65 104 bytes) and the votes in its last row decide the output; the cluster of L bases goes on in HBM, the one of
    L + 1 in LDS."""
    monkeypatch.delenv("DNAS_POLISH_LDS_POSITIONS", raising=False)
    monkeypatch.delenv("DNAS_FAKE_DEVICES", raising=False)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS", raising=False)
    L = pc.LDS_POSITIONS
    params = model(da, name)
    (templates, reads, strands), (want, kinds, trace), host = pc.cached(da, pc.limit_pool, name, params, band, ROUNDS)
    got = da.consensusReads(params, templates, reads, band=band, read_strand=strands, rounds=ROUNDS, device=0)
    print(name, band, got.stats)
    same_result(got, host)
    same(got, want)
    predicted = pc.predicted_stats(trace, L)
    assert {k: got.stats[k] for k in COUNTERS + ("batches",)} == predicted
    assert kinds["cross_up"] == 1 and kinds["cross_down"] == 1 and kinds["ins_gap_I"] == 1
    assert predicted == dict(rounds=2, batches=2, pairs=20, lds_clusters=4, hbm_clusters=2)
    assert [len(s) for s in got.strings()] == [L, L + 1, L] and got.strings()[1][L - 1] != templates[1][L - 1]


# --------------------------------------------------------------------------------------------------------------------- rounds
def shrinking_call():
    """Five clusters of which one fewer is active in every round: the two-round cluster, one that changes once, one that is
    converged, an empty template, which no read but the empty one aligns to, one without reads."""
    t, rs = two_round_cluster()
    more = T[:5] + T[4] + T[5:]
    return [t, T, T, "", T], [rs, [more, more, T], [T, T, T], ["ACGT"], []]


@pytest.mark.parametrize("cap", (None, 0), ids=("lds", "hbm"))
def test_rounds_on_the_device(da, monkeypatch, cap):
    limit = set_cap(monkeypatch, cap)
    monkeypatch.delenv("DNAS_FAKE_DEVICES", raising=False)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS", raising=False)
    p = da.MutatorParams.fromFlags(**NOISY)
    t, rs = two_round_cluster()
    route = lambda n: dict(lds_clusters=n if len(t) <= limit else 0, hbm_clusters=0 if len(t) <= limit else n)
    counters = lambda got: {k: got.stats[k] for k in COUNTERS + ("batches",)}
    results = {}
    for rounds, ran in ((6, 3), (2, 2), (1, 1)):
        host = da.consensusReads(p, [t], [rs], band=8, rounds=rounds, host=True)
        got = results[rounds] = da.consensusReads(p, [t], [rs], band=8, rounds=rounds, device=0)
        same_result(got, host)
        assert counters(got) == dict(rounds=ran, batches=ran, pairs=ran * len(rs), **route(ran))
    full, cut, first = results[6], results[2], results[1]
    assert full.rounds[0] == 2 and full.converged[0] == 1
    assert cut.strings() == full.strings() and cut.rounds[0] == 2 and cut.converged[0] == 0
    assert first.strings() != full.strings() and first.rounds[0] == 1 and first.converged[0] == 0
    again = da.consensusReads(p, first.strings(), [rs], band=8, rounds=1, device=0)      # rounds compose
    assert again.strings() == full.strings() and again.rounds[0] == 1 and again.converged[0] == 0
    # ... among clusters that drop out one by one
    templates, reads = shrinking_call()
    want, kinds, trace = pc.census(da, p, templates, reads, 8, None, 6, limit)
    assert [[c for c, _, _ in r] for r in trace] == [[0, 1, 2, 3], [0, 1], [0]]
    assert want[1] == [2, 1, 0, 0, 0] and want[2] == [1, 1, 1, 0, 0] and want[4] == [OK, OK, OK, NO_VOTERS, NO_READS]
    host = da.consensusReads(p, templates, reads, band=8, rounds=6, host=True)
    same(host, want)
    got = da.consensusReads(p, templates, reads, band=8, rounds=6, device=0)
    same_result(got, host)
    assert got.strings()[0] == full.strings()[0]
    assert counters(got) == pc.predicted_stats(trace, limit)
    for rounds in (1, 2):                                  # the cut falls while two clusters, then one, are still changing
        got = da.consensusReads(p, templates, reads, band=8, rounds=rounds, device=0)
        same_result(got, da.consensusReads(p, templates, reads, band=8, rounds=rounds, host=True))
        assert counters(got) == pc.predicted_stats(trace[:rounds], limit)


# -------------------------------------------------------------------------------------------------------------------- devices
@pytest.mark.parametrize("pool", (pc.planted_pool, pc.limit_pool), ids=("planted", "limit"))
def test_all_devices(da, monkeypatch, pool):
    monkeypatch.delenv("DNAS_POLISH_LDS_POSITIONS", raising=False)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS", raising=False)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    params = model(da, "P6")
    for cap in ((None, pc.SMALL_CAP) if pool is pc.planted_pool else (None,)):
        set_cap(monkeypatch, cap)
        (templates, reads, strands), _, host = pc.cached(da, pool, "P6", params, 8, ROUNDS, pc.SMALL_CAP if pool is pc.planted_pool else pc.LDS_POSITIONS)
        one = da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=ROUNDS, device=0)
        many = da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=ROUNDS, device=-1)
        same_result(one, host)
        same_result(many, one)
        for k in ("pairs", "cells", "lds_clusters", "hbm_clusters"):
            assert many.stats[k] == one.stats[k], k
        assert many.stats["rounds"] == one.stats["rounds"] and many.stats["batches"] > one.stats["batches"]
