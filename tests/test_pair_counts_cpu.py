"""Posterior move counts over the whole band on the host (dnas_pair_counts_host, csrc/host/paircounts.cpp), the EM on top of it
(dnas_baum_welch_pairs_host) and their argument checks -- no GPU.

Exact mode (the log-sum-exp of the host libm) is held to the exact references of pair_counts_cases.py: every enumerated path on
the tiny pairs, the mpmath forward and backward pass on the medium and boundary ones.  Table mode (the reference's table, what
the kernel reproduces) is held to those references under the derived bound stated in pair_counts_cases.py.

Measured with these tests: exact mode, largest relative gap of B_S(0,0) to Z 6.5e-16 (tiny), 7.8e-15 (medium) and 1.4e-15
(boundary), largest relative gap of a count 4.9e-15, 3.8e-13 and 9.1e-13; table mode, largest |count - exact| 1.32e-4 (tiny),
4.41e-3 (medium) and 1.28e-4 (boundary), using at most 0.67 %, 0.20 % and 1.0 % of the derived log bound."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)

import pair_counts_cases as K  # noqa: E402
import pair_forward_cases as C  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402

E_INVALID, E_BAD_BASE, E_UNSUPPORTED = -1, -6, -9


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def host(da, params, pairs, band=-1, exact=False, read_strand=None):
    a, b = C.seqs(pairs)
    return da.pairCounts(params, a, b, band=band, host=True, exact=exact, read_strand=read_strand)


@pytest.fixture(scope="module")
def tiny(da):
    """[(label, params, pairs, band, [(ll, counts)], exact mode, table mode)] at band -1, computed once."""
    out = []
    for name, plain, pairs, rows in K.tiny_exact():
        p = C.lib_params(da, plain)
        out.append((name, p, pairs, -1, rows, host(da, p, pairs, exact=True), host(da, p, pairs)))
    return out


@pytest.fixture(scope="module")
def medium(da):
    out = []
    for name, plain, pairs, by_band in K.medium_exact():
        p = C.lib_params(da, plain)
        for band in C.MEDIUM_BANDS:
            out.append(("%s/band%d" % (name, band), p, pairs, band, by_band[band], host(da, p, pairs, band=band, exact=True),
                        host(da, p, pairs, band=band)))
    return out


@pytest.fixture(scope="module")
def boundary(da):
    out = []
    for name, plain, pairs, rows in K.boundary_exact():
        p = C.lib_params(da, plain)
        out.append((name, p, pairs, -1, rows, host(da, p, pairs, exact=True), host(da, p, pairs)))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
def test_ll_is_the_forward_score_bit_for_bit(da, tiny, medium, boundary):
    n = 0
    for label, p, pairs, band, rows, exact, table in tiny + medium + boundary:
        a, b = C.seqs(pairs)
        for mode, got in ((True, exact), (False, table)):
            want = da.pairLikelihoods(p, a, b, band=band, host=True, exact=mode)
            assert np.array_equal(bits(got.pair_ll), bits(want)), (label, mode)
            assert np.array_equal(got.status == K.COUNTS_NO_PATH, want == NEG), (label, mode)
        n += len(pairs)
    assert n >= 160 + 60 + 56 * 20
    # ... and with reads given as their reverse complement, read in place
    label, p, pairs, band, rows, exact, table = medium[0]
    a, b = C.seqs(pairs)
    strand = [i % 2 for i in range(len(b))]
    flipped = [da.reverse_complement(y).astype(np.int8) if s else y for y, s in zip(b, strand)]
    got = da.pairCounts(p, a, flipped, band=band, read_strand=strand, host=True)
    assert np.array_equal(bits(got.pair_ll), bits(da.pairLikelihoods(p, a, flipped, band=band, read_strand=strand, host=True)))
    assert np.array_equal(bits(got.pair_ll), bits(table.pair_ll)) and np.array_equal(bits(got.pair_counts), bits(table.pair_counts))
    assert np.array_equal(bits(got.pair_ll_backward), bits(table.pair_ll_backward))


# ---------------------------------------------------------------------------------------------------------------- 2
def _exact_gaps(label, cases):
    back, count, n = 0., 0., 0
    for name, p, pairs, band, rows, exact, _ in cases:
        for i, ((a, b), (ll, want)) in enumerate(zip(pairs, rows)):
            if want is None:
                assert exact.status[i] == K.COUNTS_NO_PATH and (exact.pair_counts[i] == 0).all() and exact.pair_ll_backward[i] == NEG
                continue
            assert exact.status[i] == K.COUNTS_OK
            z, bk = exact.pair_ll[i], exact.pair_ll_backward[i]
            assert abs(z - ll) <= 1e-12 * max(1., abs(ll)), (name, i)
            assert abs(bk - z) <= 1e-12 * max(1., abs(z)), (name, i, bk, z)
            back = max(back, abs(bk - z) / max(1., abs(z)))
            rel = K.exact_rel_bound(p.plain, len(a), len(b))
            got = exact.pair_counts[i]
            assert (np.abs(got - want) <= rel * want + 1e-300).all(), (name, i, got, want, rel)
            nz = want > 0
            count = max(count, float((np.abs(got - want)[nz] / want[nz]).max(initial=0.)))
            n += 1
    print("%s, exact mode: largest relative gap of B_S(0,0) to Z %.3g, of a count %.3g, over %d pairs" % (label, back, count, n))
    return n


def test_exact_mode_against_the_exact_references(tiny, medium):
    assert _exact_gaps("tiny", tiny) >= 150
    # the mpmath pass (the reference of the longer pairs, and of the GPU test on these) gives what the enumeration gives
    for (name, _, pairs, walked), (_, _, _, passed) in zip(K.tiny_exact(), K.tiny_passed()):
        for (ll, counts), (ll2, counts2) in zip(walked, passed):
            assert (counts is None) == (counts2 is None) and (ll == ll2 or abs(ll - ll2) <= 2.3e-16 * abs(ll)), name
            assert counts is None or (np.abs(counts - counts2) <= 4.5e-16 * counts).all(), name
    assert _exact_gaps("medium", medium) >= 60


# ---------------------------------------------------------------------------------------------------------------- 3
def _table_gaps(label, cases):
    worst, share, n = 0., 0., 0
    for name, p, pairs, band, rows, _, table in cases:
        P = p.c.n_len
        for i, ((a, b), (ll, want)) in enumerate(zip(pairs, rows)):
            if want is None:
                assert table.status[i] == K.COUNTS_NO_PATH and (table.pair_counts[i] == 0).all(), (name, i)
                continue
            lo, hi = K.backward_table_bounds(ll, len(a), len(b), P)
            assert lo <= table.pair_ll_backward[i] <= hi, (name, i)
            e = K.table_log_bound(len(a), len(b), P)
            got = table.pair_counts[i]
            assert (got >= want * math.exp(-e) - 1e-300).all() and (got <= want * math.exp(e) + 1e-300).all(), (name, i, got, want)
            nz = (want > 1e-290) & (got > 0)
            worst = max(worst, float(np.abs(got - want).max()))
            share = max(share, float(np.abs(np.log(got[nz] / want[nz])).max(initial=0.)) / e)
            n += 1
    print("%s, table mode: largest |count - exact| = %.3g, largest share of the log bound used %.3g, over %d pairs" % (label, worst, share, n))
    return n


def test_table_mode_within_the_derived_bound(tiny, medium):
    assert _table_gaps("tiny", tiny) >= 150
    assert _table_gaps("medium", medium) >= 60


# ---------------------------------------------------------------------------------------------------------------- 4
def test_invariants(tiny, medium, boundary):
    """Every path emits O bases, consumes I, closes every deletion it opens and draws one length per duplication."""
    n = 0
    for name, p, pairs, band, rows, exact, table in tiny + medium + boundary:
        P = p.c.n_len
        for res, is_exact in ((exact, True), (table, False)):
            for i, (a, b) in enumerate(pairs):
                if res.status[i] != K.COUNTS_OK:
                    continue
                c = res.pair_counts[i]
                I, O = len(a), len(b)
                tol = 1e-9 if is_exact else math.expm1(K.table_log_bound(I, O, P))
                assert abs(c[5:21].sum() - O) <= tol * max(O, 1), (name, i, is_exact)
                assert abs(c[2] + c[0] + c[3] - I) <= tol * max(I, 1), (name, i, is_exact)
                assert abs(c[0] - c[4]) <= tol * max(c[0], 1), (name, i, is_exact)
                assert abs(c[1] - c[21:].sum()) <= tol * max(c[1], 1), (name, i, is_exact)
                n += 1
    assert n >= 2 * (150 + 60)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_cross_check_with_the_guided_estep(da, oracle_mod):
    """Where max(I, O) <= P the loose envelope of any guide is the whole matrix, so the guided E-step of the oracle and the
    counts at band -1 are the same quantity: they agree within twice the table bound."""
    X = C.X
    n = 0
    for name, plain, strict, rows in X.tiny_models():
        if strict:
            continue
        P = len(plain.pLen)
        p = C.lib_params(da, plain)
        for r in rows:
            ins, outs, cm_in, cm_out = X.guide_columns(*r)
            if max(len(ins), len(outs)) > P:
                continue
            got = host(da, p, [([int(x) for x in ins], [int(x) for x in outs])])
            oc, oll, oper = oracle_mod.expected_counts(plain, [(ins, outs, cm_in, cm_out)], strict=False)
            if got.status[0] == K.COUNTS_NO_PATH:
                assert oper[0] == NEG
                continue
            e = 2 * K.table_log_bound(len(ins), len(outs), P)
            assert abs(oper[0] - got.pair_ll[0]) <= e, (name, r)
            c = got.pair_counts[0]
            assert (oc >= c * math.exp(-e) - 1e-300).all() and (oc <= c * math.exp(e) + 1e-300).all(), (name, r, oc, c)
            n += 1
    print("guided E-step against the counts at band -1: %d pairs with max(I, O) <= P" % n)
    assert n >= 10


# ---------------------------------------------------------------------------------------------------------------- 6
def test_the_boundary_models(boundary):
    """Probabilities of 0, 1, 1e-300 and 1 - 2^-53: no NaN anywhere, NO_PATH exactly where the mpmath pass finds no path, the
    counts of zero-probability moves exactly 0, and the table bound holds."""
    assert len(boundary) == 56
    paths = no_path = 0
    for name, p, pairs, band, rows, exact, table in boundary:
        zero = K.zero_moves(p.plain)
        for res in (exact, table):
            assert not np.isnan(res.pair_counts).any() and not np.isnan(res.counts).any() and not math.isnan(res.ll), name
            assert not np.isnan(res.pair_ll).any() and not np.isnan(res.pair_ll_backward).any(), name
            want_none = np.array([c is None for _, c in rows])
            assert np.array_equal(res.status == K.COUNTS_NO_PATH, want_none), name
            assert (res.pair_counts[:, zero] == 0).all(), (name, zero)
        paths += int((table.status == K.COUNTS_OK).sum())
        no_path += int((table.status == K.COUNTS_NO_PATH).sum())
    assert paths > 0 and no_path > 0
    assert _table_gaps("boundary", boundary) == paths
    _exact_gaps("boundary", boundary)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_em(da):
    ins, outs = K.em_pairs()
    assert len(ins) == 60 and all(20 <= len(a) <= 40 for a in ins)
    start = K.em_start(da)
    fitted, iters, trace = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, host=True, exact=True)
    assert 1 <= iters < 100 and len(trace) == iters + 1            # stopped by the 1e-3 rule: the last E-step saw the small gain
    lls = [ll for _, ll in trace]
    for before, after in zip(lls, lls[1:]):
        assert after >= before - 1e-9 * abs(before), lls
    assert (lls[-1] - lls[-2]) / abs(lls[-2]) < 1e-3 and all((b - a) / abs(a) >= 1e-3 for a, b in zip(lls[:-2], lls[1:-1]))
    assert K.params_dict(trace[0][0]) == K.params_dict(start)
    for step in range(iters):
        p, ll = trace[step]
        assert p.pLen == [.25] * 4 and p.local == start.local
        res = da.pairCounts(p, ins, outs, band=K.EM_BAND, host=True, exact=True)
        assert ll == pytest.approx(res.ll + K.log_prior(p, 4), rel=1e-12)
        assert K.params_dict(trace[step + 1][0]) == pytest.approx(K.m_step(res.counts), rel=1e-12), step
    assert K.params_dict(fitted) == K.params_dict(trace[-1][0])
    capped, n, short = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, host=True, exact=True, max_iterations=2)
    assert n == 2 and len(short) == 2 and K.params_dict(capped) == K.params_dict(trace[2][0])
    assert [ll for _, ll in short] == lls[:2]
    table, n_table, _ = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, host=True)
    assert n_table == iters and K.params_dict(table) == pytest.approx(K.params_dict(fitted), rel=1e-2)


# ---------------------------------------------------------------------------------------------------------------- 8
def test_argument_checks(da):
    from test_pair_align_cpu import make_params
    L = da.lib.lib()
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.pairCounts(make_params(da, [1. / 14] * 14), ["ACGT"], ["ACT"], host=True)
    params = make_params(da, [.5, .5])
    ins, outs = np.array([0, 1, 2, 3], np.int8), np.array([0, 1, 3], np.int8)
    counts, ll, per, pll, back, status = np.zeros(23), np.zeros(1), np.zeros(23), np.zeros(1), np.zeros(1), np.zeros(1, np.uint8)

    def ptr(x):
        return x.ctypes.data if x is not None else None

    def call(bases=ins, in_off=(0, 4), out_off=(0, 3), band=-1, n=1, exact=0, counts=counts, ll=ll, per=per, pll=pll, back=back,
             status=status):
        io, oo = np.array(in_off, np.int64), np.array(out_off, np.int64)
        return L.dnas_pair_counts_host(ctypes.byref(params.c), band, n, ptr(bases), io.ctypes.data, outs.ctypes.data, oo.ctypes.data,
                                       None, exact, ptr(counts), ptr(ll), ptr(per), ptr(pll), ptr(back), ptr(status))
    assert call() == 0 and np.isfinite(pll[0]) and status[0] == K.COUNTS_OK and ll[0] == pll[0] and np.array_equal(counts, per)
    assert call(per=None, back=None) == 0                                  # the two optional outputs
    assert call(np.array([0, 1, 2, 4], np.int8)) == E_BAD_BASE
    assert call(band=-2) == E_INVALID and "band" in L.dnas_last_error().decode()
    assert call(in_off=(1, 4)) == E_INVALID and call(out_off=(2, 3)) == E_INVALID
    assert call(in_off=(0, -1)) == E_INVALID and call(out_off=(0, -3)) == E_INVALID
    assert call(in_off=(0, (1 << 20) + 1)) == E_UNSUPPORTED
    assert call(n=-1) == E_INVALID and call(bases=None) == E_INVALID
    assert call(counts=None) == E_INVALID and call(ll=None) == E_INVALID and call(pll=None) == E_INVALID and call(status=None) == E_INVALID
    assert call(n=0, bases=None, pll=None, status=None, per=None, back=None) == 0 and (counts == 0).all() and ll[0] == 0
    empty = da.pairCounts(params, [], [], host=True)
    assert empty.pair_ll.shape == (0,) and empty.pair_counts.shape == (0, 23) and empty.stats is None
    with pytest.raises(ValueError):
        da.pairCounts(params, ["ACGT", "AC"], ["ACT"], host=True)
    with pytest.raises(ValueError):
        da.pairCounts(params, ["ACGT"], ["ACT"], exact=True)               # exact is a mode of the host statement
    with pytest.raises(ValueError):
        da.baumWelchPairs(params, ["ACGT"], ["ACT"], exact=True)
    with pytest.raises(ValueError):
        da.pairCounts(params, ["ACGT"], ["ACT", "AC"], read_strand=[0], host=True)
    one = da.pairCounts(params, ["ACGT"], ["ACT", "ACGT", ""], host=True)  # one original pairs with every read
    assert one.pair_ll.shape == (3,) and (one.status == K.COUNTS_OK).all()
    out, it = da.lib.MutatorParamsC(), ctypes.c_int32()
    io, oo = np.array((0, 4), np.int64), np.array((0, 3), np.int64)
    fit = lambda band, max_it, dst: L.dnas_baum_welch_pairs_host(  # noqa: E731
        ctypes.byref(params.c), band, 1, ins.ctypes.data, io.ctypes.data, outs.ctypes.data, oo.ctypes.data, None, 0, max_it,
        ctypes.byref(dst) if dst is not None else None, ctypes.addressof(it), None, None, None)
    assert fit(-1, 1, out) == 0 and it.value == 1 and fit(-1, -1, out) == E_INVALID and fit(-2, 1, out) == E_INVALID
    assert fit(-1, 1, None) == E_INVALID


# ---------------------------------------------------------------------------------------------------------------- 9
def test_host_statement_under_sanitizers(tmp_path):
    """pairCountsHost over lengths 0 to 40 squared, bands 0, 1, 5 and -1, P of 0, 2, 6 and 13, on heap blocks of exactly the
    sequences' lengths, in a stand-alone host program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "pair_counts_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "pair_counts_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=600)
    assert r.returncode == 0 and b"pair counts host check: ok (26896 pairs)" in r.stdout, r.stderr.decode()
