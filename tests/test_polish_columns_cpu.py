"""The pools of tests/polish_columns.py hold what they are built to hold, by the host statement alone; and
dnas_cluster_consensus_host equals the Python restatement on them.  No GPU."""
import os
import sys

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import polish_columns as pc  # noqa: E402
from test_assign_cpu import BANDS, models  # noqa: E402
from test_polish_cpu import NO_READS, NO_VOTERS, OK, revcomp, same  # noqa: E402

ROUNDS = 4
CENSUS_MODELS = ("P1", "P6", "P13-zero")
CENSUS_BANDS = (-1, 8)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_the_source_constants():
    assert pc.LDS_POSITIONS == 650 and pc.ROW_WORDS == 25 and pc.LDS_TABLE_BYTES == 65104     # (a change of the source shows up here)


def test_planted_pool_holds_every_kind(da):
    """Every kind of the census occurs under P1, P6 and P13-zero at bands -1 and 8, with crossings of SMALL_CAP = 64 bases.
    A condition on the input, not a measurement.  Found when the pool was fixed (46 clusters, 477 reads), model/band:

      kind                  P1/-1        P1/8       P6/-1        P6/8 P13-zero/-1  P13-zero/8
      ins                     195         195         206         206         210         210
      ins_even_V               92          92          99          99          97          97
      ins_V_gt_64               8           8           8           8           8           8
      ins_k3                   24          24          32          32          33          33
      ins_gap_I                22          22          44          44          48          48
      ins_chunk_edge           35          35          38          38          22          22
      ins_B_tie                 2           2           4           4           3           3
      ins_four_gaps             3           3           1           1           1           1
      long_runs                75          75          81          81          98          98
      del                      51          51          61          61          67          67
      del_V_gt_64               4           4           4           4           4           4
      del_chunk_edge            9           9           9           9          11          11
      del_tail_only             4           4           4           4           4           4
      tie_2N_eq_V              44          44          36          36          32          32
      tie_2D_eq_V              43          43          59          59          53          53
      M_tie_excl                4           4           2           2           3           3
      changed_round2           10          10          14          14          14          14
      changed_round3            3           3           2           2           7           7
      cross_up                  2           2           2           2           2           2
      cross_down                2           2           2           2           2           2
      clusters active  45,41,10,3  45,41,10,3  45,41,14,2  45,41,14,2  45,40,14,7  45,40,14,7   (rounds 1 .. 4)"""
    seen = 0
    for name, params in models(da):
        if name not in CENSUS_MODELS:
            continue
        for band in CENSUS_BANDS:
            (templates, reads, strands), (want, kinds, trace), host = pc.cached(da, pc.planted_pool, name, params, band, ROUNDS, pc.SMALL_CAP)
            print(name, band, dict(kinds), [len(r) for r in trace])
            assert [k for k in pc.KINDS if kinds[k] < 1] == [], (name, band)
            assert len(trace) == ROUNDS and len(trace[0]) > len(trace[1]) > len(trace[2]) > len(trace[3]) > 0
            seen += 1
    assert seen == len(CENSUS_MODELS) * len(CENSUS_BANDS)


def test_planted_pool_shapes(da):
    """What the pool is described by: its sizes, and under P6 the clusters built for one shape of output."""
    templates, reads, strands = pc.planted_pool(da)
    assert pc.planted_pool(da) == (templates, reads, strands)                      # deterministic
    assert max(len(t) for t in templates) == 130 and min(len(t) for t in templates) == 0
    assert {len(r) for r in reads} >= {0, 2, 3, 4, 5, 65, 70}
    assert all(s == [i % 2 for i in range(len(s))] for s in strands)
    name, params = [m for m in models(da) if m[0] == "P6"][0]
    for band in CENSUS_BANDS:
        _, (want, kinds, trace), _ = pc.cached(da, pc.planted_pool, name, params, band, ROUNDS, pc.SMALL_CAP)
        seqs = want[0]
        c = templates.index("AC")                          # 2 -> 6 bases: a run of 4 at gap I
        assert seqs[c] == "ACACAC" and want[1][c] == 1 and want[2][c] == 1
        # copies of two bases at each of the gaps 62 .. 65
        four = [c for c, t in enumerate(templates) if len(t) == 70 and seqs[c] == pc.plant(t, [("h", g, 2) for g in (62, 63, 64, 65)])]
        assert len(four) == 1
        # twelve copies of one base, at most four a round and gap: 60 -> 72 bases over several rounds
        grown = [c for c, t in enumerate(templates) if len(t) == 60 and seqs[c] == pc.plant(t, [("h", 30, 12)])]
        assert len(grown) == 1 and want[1][grown[0]] >= 2
        lengths = [I for r in trace for c, I, n in r if c == grown[0]]
        assert lengths[0] == 60 and lengths[-1] == 72 and sorted(lengths) == lengths


def test_planted_pool_without_insertions_and_without_errors(da):
    """P0 has no duplication columns; P6-global-exact aligns a read only where it is the template."""
    for name, params in models(da):
        if name not in ("P0", "P6-global-exact"):
            continue
        for band in BANDS:
            (templates, reads, strands), (want, kinds, trace), host = pc.cached(da, pc.planted_pool, name, params, band, ROUNDS, pc.SMALL_CAP)
            same(host, want)
            assert kinds["ins"] == 0 and kinds["tie_2N_eq_V"] == 0 and kinds["long_runs"] == 0
            if name == "P0":
                assert kinds["del"] > 0 and kinds["cross_down"] > 0 and kinds["cross_up"] == 0
                continue
            seqs, n_rounds, converged, voters, status = want
            assert seqs == templates and not any(n_rounds) and len(trace) == 1
            for c, t in enumerate(templates):
                equal = sum((revcomp(r) if s else r) == t for r, s in zip(reads[c], strands[c]))
                assert voters[c] == equal and converged[c] == (equal > 0)
                assert status[c] == (NO_READS if not reads[c] else OK if equal else NO_VOTERS)
            assert sum(s == NO_VOTERS for s in status) >= 30


def test_limit_pool_crosses_the_cap_both_ways(da):
    """Under P6 and P13-zero, the models of the GPU test, bands -1 and 8 (found under both: ins 2, ins_even_V 1, ins_gap_I 1, ins_chunk_edge 1, del 1, cross_up 1, cross_down 1;
    lengths 649, 650, 651 -> 650, 651, 650; every cluster changes in its first round and returns its template in the second)."""
    L = pc.LDS_POSITIONS
    for name, params, band in [(n, p, b) for n, p in models(da) if n in ("P6", "P13-zero") for b in CENSUS_BANDS]:
        (templates, reads, strands), (want, kinds, trace), host = pc.cached(da, pc.limit_pool, name, params, band, ROUNDS)
        seqs, n_rounds, converged, voters, status = want
        assert [len(t) for t in templates] == [L - 1, L, L + 1] and [len(r) for r in reads] == [3, 4, 3]
        assert kinds["cross_up"] == 1 and kinds["cross_down"] == 1
        assert [len(s) for s in seqs] == [L, L + 1, L]
        assert seqs[1][L - 1] != templates[1][L - 1] and seqs[1][:L - 1] == templates[1][:L - 1] and len(seqs[1]) > L
        assert kinds["ins_gap_I"] == 1 and kinds["ins_chunk_edge"] == 1 and kinds["ins_even_V"] == 1 and kinds["del"] == 1
        assert trace == [[(0, L - 1, 3), (1, L, 4), (2, L + 1, 3)], [(0, L, 3), (1, L + 1, 4), (2, L, 3)]]
        assert n_rounds == [1, 1, 1] and converged == [1, 1, 1] and voters == [3, 4, 3]
        assert pc.predicted_stats(trace, L) == dict(rounds=2, batches=2, pairs=20, lds_clusters=4, hbm_clusters=2)


def test_host_statement_against_the_restatement(da):
    for pool, limit in ((pc.planted_pool, pc.SMALL_CAP), (pc.limit_pool, pc.LDS_POSITIONS)):
        for name, params in models(da):
            for band in BANDS:
                _, (want, kinds, trace), host = pc.cached(da, pool, name, params, band, ROUNDS, limit)
                same(host, want)
                assert host.stats is None
