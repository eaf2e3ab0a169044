"""The forward pair-HMM score on the host (dnas_pair_likelihoods_host, csrc/host/pairforward.cpp), the forward mode of the
consensus scorer's host statement and their argument checks -- no GPU.

Exact mode (the log-sum-exp of the host libm) is held to the exact references of pair_forward_cases.py: the sum over every
enumerated path on the tiny pairs, the mpmath forward pass on the medium ones.  Table mode (the reference's table, what the
kernels reproduce bit for bit) is held to exact mode under the derived, sign-aware bound stated in pair_forward_cases.py.

Measured with these tests (largest gap of table mode to exact mode, in nats): tiny 3.82e-05, medium 7.17e-04, boundary
4.25e-05; the largest share of the lower bound used was 2.6 %."""
import ctypes
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

import pair_forward_cases as C  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402

OK, NO_PATH, NO_CANDIDATES, NO_READS = 0, 1, 2, 3
E_INVALID, E_BAD_BASE, E_UNSUPPORTED = -1, -6, -9
PLANTED = dict(sub=.04, dup=.01, del_open=.02, del_ext=.2, length=4)
PLANTED_BAND = 16
# planted_cluster(66): the Viterbi totals name the planted strand, the forward totals another candidate.  Found by walking the
# seeds 0, 1, 2 ... of planted_cluster: the first of them on which the two modes disagree.
DIFFERENT_WINNER_SEED = 66


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def host(da, params, pairs, band=-1, exact=False, read_strand=None):
    a, b = C.seqs(pairs)
    return da.pairLikelihoods(params, a, b, band=band, host=True, exact=exact, read_strand=read_strand)


@pytest.fixture(scope="module")
def tiny(da):
    """[(name, params, pairs, every-path sum, paths walked, exact mode, table mode)] at band -1, computed once."""
    out = []
    for name, plain, pairs, want, walked in C.tiny_exact():
        p = C.lib_params(da, plain)
        out.append((name, p, pairs, want, walked, host(da, p, pairs, exact=True), host(da, p, pairs)))
    return out


@pytest.fixture(scope="module")
def medium(da):
    """[(name, params, pairs, {band: mpmath forward pass}, {band: exact mode}, {band: table mode})], computed once."""
    out = []
    for name, plain, pairs, want in C.medium_exact():
        p = C.lib_params(da, plain)
        out.append((name, p, pairs, want, {b: host(da, p, pairs, band=b, exact=True) for b in C.MEDIUM_BANDS},
                    {b: host(da, p, pairs, band=b) for b in C.MEDIUM_BANDS}))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1, 2
def test_exact_mode_against_every_path(tiny):
    compared, no_path = 0, 0
    for name, p, pairs, want, walked, got, _ in tiny:
        assert max(walked) <= C.X.MAX_PATHS                      # none skipped: enumerate_pair raises beyond MAX_PATHS
        for i in range(len(pairs)):
            # the mpmath forward pass (the reference of the longer pairs, and of the GPU test) is the same sum: one fp64 rounding
            passed = C.exact_forward(p.plain, *pairs[i])
            assert passed == want[i] or abs(passed - want[i]) <= 2.3e-16 * abs(want[i]), (name, i, passed, want[i])
            if want[i] == NEG:
                assert got[i] == NEG, (name, i, got[i])
                no_path += 1
            else:
                assert abs(got[i] - want[i]) <= 1e-12 * max(1., abs(want[i])), (name, i, got[i], want[i])
                compared += 1
    assert compared >= 150 and compared + no_path == 160 and no_path == 10


def test_exact_mode_against_the_mpmath_forward_pass(medium):
    n, worst = 0, 0.
    for name, p, pairs, want, got, _ in medium:
        for band in C.MEDIUM_BANDS:
            for i in range(len(pairs)):
                w, g = want[band][i], got[band][i]
                assert (g == NEG) if w == NEG else abs(g - w) <= 1e-12 * max(1., abs(w)), (name, band, i, g, w)
                if w != NEG:
                    worst = max(worst, abs(g - w) / max(1., abs(w)))
                n += 1
    print("exact mode against the mpmath forward pass: largest relative gap %.3g over %d pairs" % (worst, n))
    assert n == 3 * sum(len(m[2]) for m in medium) and n >= 60


# ---------------------------------------------------------------------------------------------------------------- 3
def _table_gap(label, rows):
    """rows: (name, pairs, exact-mode values, table-mode values) -> the largest gap, every pair inside the derived bound."""
    worst, share = 0., 0.
    for name, pairs, exact, table in rows:
        for i, (a, b) in enumerate(pairs):
            if exact[i] == NEG:
                assert table[i] == NEG, (name, i, table[i])
                continue
            lo, hi = C.table_bounds(exact[i], len(a), len(b))
            assert lo <= table[i] <= hi, (name, i, table[i], exact[i], lo, hi)
            worst = max(worst, abs(table[i] - exact[i]))
            share = max(share, (exact[i] - table[i]) / (exact[i] - lo))
    print("%s: largest |table - exact| = %.3g nats, largest share of the lower bound used %.3g" % (label, worst, share))
    return worst


def test_table_mode_within_the_derived_bound(tiny, medium):
    assert _table_gap("tiny", [(name, pairs, exact, table) for name, _, pairs, _, _, exact, table in tiny]) > 0
    rows = [("%s/band%d" % (name, b), pairs, exact[b], table[b]) for name, _, pairs, _, exact, table in medium for b in C.MEDIUM_BANDS]
    assert _table_gap("medium", rows) > 0


# ---------------------------------------------------------------------------------------------------------------- 4
def test_forward_is_never_below_viterbi(da, tiny, medium):
    above = 0
    for name, p, pairs, want, _, exact, _ in tiny:
        a, b = C.seqs(pairs)
        vit = da.alignPairs(p, a, b, band=-1, host=True).score
        for i in range(len(pairs)):
            assert exact[i] >= vit[i] - 1e-9, (name, i, exact[i], vit[i])
            assert (exact[i] == NEG) == (vit[i] == NEG)
            above += exact[i] != NEG and exact[i] - vit[i] > 1e-6
    assert above >= 120, above
    print("forward exceeds Viterbi by more than 1e-6 on %d of the 150 tiny pairs" % above)
    lo, hi = np.inf, 0.
    for name, p, pairs, _, exact, _ in medium:
        a, b = C.seqs(pairs)
        for band in C.MEDIUM_BANDS:
            vit = da.alignPairs(p, a, b, band=band, host=True).score
            for i in range(len(pairs)):
                assert exact[band][i] >= vit[i] - 1e-9, (name, band, i, exact[band][i], vit[i])
                if vit[i] != NEG:
                    lo, hi = min(lo, exact[band][i] - vit[i]), max(hi, exact[band][i] - vit[i])
    print("medium pairs: the forward score exceeds the Viterbi score by %.3g to %.3g nats" % (lo, hi))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_reverse_complement_in_place(da, tiny, medium):
    for name, p, pairs in [(t[0], t[1], t[2]) for t in tiny] + [(m[0], m[1], m[2]) for m in medium]:
        flipped = [(a, [3 - x for x in reversed(b)]) for a, b in pairs]
        for band in (-1, 2):
            for exact in (False, True):
                want = host(da, p, pairs, band=band, exact=exact)
                got = host(da, p, flipped, band=band, exact=exact, read_strand=[1] * len(pairs))
                assert np.array_equal(bits(got), bits(want)), (name, band, exact)
        mixed = [i % 2 for i in range(len(pairs))]
        got = host(da, p, [f if s else q for f, q, s in zip(flipped, pairs, mixed)], read_strand=mixed)
        assert np.array_equal(bits(got), bits(host(da, p, pairs))), name


# ---------------------------------------------------------------------------------------------------------------- 6
def _boundary_ids():
    return ["%s/%s" % (b, v) for b in C.X.BOUNDARY_ESTEP_BASES for v in C.X.BOUNDARY_NAMES]


@pytest.fixture(scope="module")
def boundary():
    return C.boundary_exact()


@pytest.mark.parametrize("index", range(4 * 14), ids=_boundary_ids())
def test_error_model_edges(da, boundary, index):
    """Probabilities of exactly 0 and 1, of 1e-300 and of 1 - 2^-53: never NaN, -inf exactly where no path has positive
    probability, exact mode on the mpmath pass, table mode inside its bound."""
    name, plain, pairs, want = boundary[index]
    assert name == _boundary_ids()[index]
    p = C.lib_params(da, plain)
    exact, table = host(da, p, pairs, exact=True), host(da, p, pairs)
    assert not np.isnan(exact).any() and not np.isnan(table).any()
    for i in range(len(pairs)):
        assert (exact[i] == NEG) == (want[i] == NEG) == (table[i] == NEG), (name, i, exact[i], table[i], want[i])
        if want[i] != NEG:
            assert np.isfinite(exact[i]) and np.isfinite(table[i])
            assert abs(exact[i] - want[i]) <= 1e-12 * max(1., abs(want[i])), (name, i, exact[i], want[i])
    _table_gap(name, [(name, pairs, exact, table)])


# ---------------------------------------------------------------------------------------------------------------- 7
def planted_cluster(seed):
    """A strand of 30 to 50 bases, four candidates (the strand and three copies of it with one or two edits, shuffled) and three
    reads of the strand under the noise of the planted pools (synth.mutate) -> (strand, candidates, reads)."""
    import synth
    from test_pair_align_cpu import edited
    rng = random.Random("pair-forward/planted/%d" % seed)
    strand = "".join(rng.choice(C.BASES) for _ in range(rng.randint(30, 50)))
    cands = [strand] + [edited(rng, strand, rng.randint(1, 2)) for _ in range(3)]
    rng.shuffle(cands)
    reads = [synth.mutate(strand, rng, sub=.04, dele=.02, dup=.01) for _ in range(3)]
    return strand, cands, reads


def _consensus_expected(da, params, cands, reads, strands, band):
    """Totals and picks restated over pairLikelihoods(host=True) with the rules of test_consensus_cpu.py."""
    from test_consensus_cpu import item_list, pick_py, totals_py
    items = item_list(cands, reads)
    ins = [cands[c][j] for c, j, _ in items]
    outs = [da.reverse_complement(reads[c][i]) if strands is not None and strands[c][i] else reads[c][i] for c, _, i in items]
    scores = da.pairLikelihoods(params, ins, outs, band=band, host=True) if items else np.zeros(0)
    totals = totals_py(cands, reads, items, scores)
    return totals, pick_py(totals, [len(r) for r in reads])


def test_consensus_forward_mode_on_the_host(da):
    from test_assign_cpu import BANDS, NOISY, models
    from test_consensus_cpu import same_as_expected, shape_pool
    cands, reads, strands = shape_pool(da)
    statuses = set()
    for name, params in models(da):
        for band in BANDS:
            res = da.consensusScore(params, cands, reads, band=band, read_strand=strands, host=True, score="forward")
            totals, rows = _consensus_expected(da, params, cands, reads, strands, band)
            same_as_expected(res, totals, rows)
            statuses |= set(int(x) for x in res.status)
            for c, row in enumerate(rows):
                post = res.posterior[c]
                assert len(post) == len(cands[c]) and not np.isnan(post).any()
                if row[3] == OK:
                    assert abs(post.sum() - 1.) <= 1e-12 and (post >= 0).all(), (name, band, c, post)
                    assert all(q == 0. for t, q in zip(totals[c], post) if t == NEG) and post[row[0]] > 0
                    assert bits(res.confidence[c]) == bits(post[row[0]])
                    # the formula, in candidate order
                    m = max(totals[c])
                    z = m + np.log(sum(np.exp(np.float64(t) - m) for t in totals[c]))
                    assert np.allclose(post, [np.exp(np.float64(t) - z) for t in totals[c]], rtol=1e-13, atol=1e-300)
                else:
                    assert (post == 0).all() and res.confidence[c] == 0
    assert statuses == {OK, NO_PATH, NO_CANDIDATES, NO_READS}
    # a candidate listed twice: equal totals, equal shares, the lower index wins with a margin of 0
    params = da.MutatorParams.fromFlags(**NOISY)
    res = da.consensusScore(params, [cands[0]], [reads[0]], band=8, read_strand=[strands[0]], host=True, score="forward")
    assert cands[0][0] == cands[0][2] and res.winner[0] == 0 and res.margin[0] == 0
    assert bits(res.posterior[0][0]) == bits(res.posterior[0][2]) and abs(res.posterior[0][0] - .5) < 1e-9
    # the default mode has neither attribute and is the call it was
    plain = da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True)
    assert not hasattr(plain, "posterior") and not hasattr(plain, "confidence")
    again = da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True, score="viterbi")
    assert np.array_equal(bits(plain.total), bits(again.total)) and np.array_equal(plain.winner, again.winner)
    with pytest.raises(ValueError):
        da.consensusScore(params, cands, reads, host=True, score="posterior")


def test_consensus_posterior_needs_the_forward_mode(da):
    from test_assign_cpu import NOISY
    L = da.lib.lib()
    params = da.MutatorParams.fromFlags(**NOISY)
    i64 = lambda x: np.array(x, dtype=np.int64)
    cand_off, cl_cand, read_off, cl_read = i64([0, 4, 8]), i64([0, 2]), i64([0, 3, 6]), i64([0, 2])
    seqs = np.zeros(16, np.int8)
    winner, status, total, second, post = np.zeros(2, np.int64), np.zeros(2, np.uint8), np.zeros(2), np.zeros(2), np.full(4, 7.)

    def call(mode, posterior):
        return L.dnas_consensus_score_host_ex(ctypes.byref(params.c), 8, 1, 2, seqs.ctypes.data, cand_off.ctypes.data, cl_cand.ctypes.data, 2,
                                              seqs.ctypes.data, read_off.ctypes.data, None, cl_read.ctypes.data, mode, winner.ctypes.data,
                                              total.ctypes.data, second.ctypes.data, status.ctypes.data, None,
                                              posterior.ctypes.data if posterior is not None else None)
    assert call(da.lib.SCORE_VITERBI, post) == E_INVALID and "posterior" in L.dnas_last_error().decode()
    assert call(2, None) == E_INVALID and call(-1, None) == E_INVALID
    assert call(da.lib.SCORE_VITERBI, None) == 0
    viterbi_total = total[0]
    assert call(da.lib.SCORE_FORWARD, None) == 0 and total[0] > viterbi_total
    assert call(da.lib.SCORE_FORWARD, post) == 0 and bits(post[0]) == bits(post[1]) and abs(post[0] - .5) <= 1e-12 and status[0] == OK
    assert post[2] == post[3] == 7.                                      # nothing is written beyond the call's candidates
    assert {"dnas_consensus_score_ex", "dnas_consensus_score_host_ex", "dnas_viterbi_clusters_scored", "dnas_pair_likelihoods",
            "dnas_pair_likelihoods_host"} <= set(da.lib.declared_symbols())
    assert all(hasattr(L, s) for s in ("dnas_consensus_score_ex", "dnas_viterbi_clusters_scored", "dnas_pair_likelihoods"))


def test_the_two_modes_can_name_different_winners(da):
    """The committed seed: under the Viterbi totals the planted strand wins, under the forward totals another candidate does --
    the margin in Viterbi nats and the posterior are different statements about a cluster."""
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    strand, cands, reads = planted_cluster(DIFFERENT_WINNER_SEED)
    vit = da.consensusScore(params, [cands], [reads], band=PLANTED_BAND, host=True)
    fwd = da.consensusScore(params, [cands], [reads], band=PLANTED_BAND, host=True, score="forward")
    assert vit.status[0] == OK and fwd.status[0] == OK
    assert cands[int(vit.winner[0])] == strand and cands[int(fwd.winner[0])] != strand
    assert 0 < fwd.posterior[0][int(vit.winner[0])] < fwd.confidence[0] < 1
    print("seed %d: Viterbi margin %.3f nats for the planted strand, forward posterior %.3f for another candidate (planted: %.3f)"
          % (DIFFERENT_WINNER_SEED, vit.margin[0], fwd.confidence[0], fwd.posterior[0][int(vit.winner[0])]))


# ---------------------------------------------------------------------------------------------------------------- 8
def test_argument_checks(da):
    from test_pair_align_cpu import make_params
    L = da.lib.lib()
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.pairLikelihoods(make_params(da, [1. / 14] * 14), ["ACGT"], ["ACT"], host=True)
    params = make_params(da, [.5, .5])
    ins, outs = np.array([0, 1, 2, 3], np.int8), np.array([0, 1, 3], np.int8)
    ll = np.zeros(1)

    def call(bases=ins, in_off=(0, 4), out_off=(0, 3), band=-1, n=1, out=ll, exact=0):
        io, oo = np.array(in_off, np.int64), np.array(out_off, np.int64)
        return L.dnas_pair_likelihoods_host(ctypes.byref(params.c), band, n, bases.ctypes.data if bases is not None else None, io.ctypes.data,
                                            outs.ctypes.data, oo.ctypes.data, None, exact, out.ctypes.data if out is not None else None)
    assert call() == 0 and np.isfinite(ll[0])
    table = ll[0]
    assert call(exact=1) == 0 and 0 < abs(ll[0] - table) < 1e-3
    assert call(np.array([0, 1, 2, 4], np.int8)) == E_BAD_BASE
    assert call(band=-2) == E_INVALID and "band" in L.dnas_last_error().decode()
    assert call(in_off=(1, 4)) == E_INVALID and call(out_off=(2, 3)) == E_INVALID
    assert call(in_off=(0, -1)) == E_INVALID and call(out_off=(0, -3)) == E_INVALID
    assert call(in_off=(0, (1 << 20) + 1)) == E_UNSUPPORTED
    assert call(n=-1) == E_INVALID and call(out=None) == E_INVALID and call(bases=None) == E_INVALID
    assert L.dnas_pair_likelihoods_host(None, -1, 0, None, None, None, None, None, 0, None) == E_INVALID
    assert call(n=0, bases=None, out=None) == 0                           # an empty call needs no arrays
    empty = da.pairLikelihoods(params, [], [], host=True)
    assert empty.shape == (0,) and empty.dtype == np.float64
    with pytest.raises(ValueError):
        da.pairLikelihoods(params, ["ACGT", "AC"], ["ACT"], host=True)
    with pytest.raises(ValueError):
        da.pairLikelihoods(params, ["ACGT"], ["ACT"], exact=True)          # exact is a mode of the host statement
    with pytest.raises(ValueError):
        da.pairLikelihoods(params, ["ACGT"], ["ACT", "AC"], read_strand=[0], host=True)
    one = da.pairLikelihoods(params, ["ACGT"], ["ACT", "ACGT", ""], host=True)       # one original pairs with every read
    assert one.shape == (3,) and np.array_equal(bits(one[:1]), bits(da.pairLikelihoods(params, ["ACGT"], ["ACT"], host=True)))


# ---------------------------------------------------------------------------------------------------------------- 9
def test_host_statement_under_sanitizers(tmp_path):
    """forwardPairHost over lengths 0 to 70 squared, bands 0, 1, 5 and -1, P of 0, 2, 6 and 13, on heap blocks of exactly the
    sequences' lengths, in a stand-alone host program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "pair_forward_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "pair_forward_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=600)
    assert r.returncode == 0 and b"pair forward host check: ok (80656 pairs)" in r.stdout, r.stderr.decode()
