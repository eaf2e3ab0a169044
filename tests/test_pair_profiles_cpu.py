"""Pair-HMM row profiles on the host (dnas_pair_profiles_host, pairProfileHost of csrc/host/paircounts.cpp): the posteriors of
dnas_pair_counts_host kept per row of the original, their aggregate per position, and the argument checks -- no GPU.

Exact mode is held to pair_profile_cases.exact_profile, the mpmath forward and backward pass with every move filed by the row it
leaves (itself held to pair_counts_cases.exact_counts by summing rows), within pair_counts_cases.exact_rel_bound; table mode
within a factor exp(+-table_log_bound) of it: a profile value sums some of the terms a count sums, so a count's bound is its."""
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
import pair_profile_cases as R  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402

E_INVALID, E_BAD_BASE, E_UNSUPPORTED = -1, -6, -9


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def host(da, params, pairs, band=-1, exact=False, **kw):
    a, b = C.seqs(pairs)
    return da.pairProfiles(params, a, b, band=band, host=True, exact=exact, **kw)


@pytest.fixture(scope="module")
def cases(da):
    """[(label, params, pairs, band, [(ll, profile or None)], exact mode, table mode)]: the tiny pairs over the whole matrix, the
    medium pairs at bands -1, 8 and 0, the boundary models; everything computed once."""
    out = {"tiny": [], "medium": [], "boundary": []}
    for name, plain, pairs, rows in R.tiny_exact():
        p = C.lib_params(da, plain)
        out["tiny"].append((name, p, pairs, -1, rows, host(da, p, pairs, exact=True), host(da, p, pairs)))
    for name, plain, pairs, by_band in R.medium_exact():
        p = C.lib_params(da, plain)
        for band in C.MEDIUM_BANDS:
            out["medium"].append(("%s/band%d" % (name, band), p, pairs, band, by_band[band], host(da, p, pairs, band=band, exact=True),
                                  host(da, p, pairs, band=band)))
    for name, plain, pairs, rows in R.boundary_exact():
        p = C.lib_params(da, plain)
        out["boundary"].append((name, p, pairs, -1, rows, host(da, p, pairs, exact=True), host(da, p, pairs)))
    return out


def everything(cases):
    return cases["tiny"] + cases["medium"] + cases["boundary"]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_exact_profile_rows_sum_to_the_exact_counts():
    n = 0
    for (name, plain, pairs, rows), (_, _, _, counted) in zip(R.tiny_exact(), K.tiny_passed()):
        for (ll, prof), (ll2, counts) in zip(rows, counted):
            assert (prof is None) == (counts is None) and ll == ll2, name
            if prof is not None:
                R.hold_to_exact_counts(prof, counts, len(plain.pLen))
                n += 1
    for (name, plain, pairs, by_band), (_, _, _, counted) in zip(R.medium_exact(), K.medium_exact()):
        for band in C.MEDIUM_BANDS:
            for (a, b), (ll, prof), (ll2, counts) in zip(pairs, by_band[band], counted[band]):
                assert (prof is None) == (counts is None) and ll == ll2, (name, band)
                if prof is not None:
                    assert prof.shape == (6 + len(plain.pLen), len(a) + 1)
                    R.hold_to_exact_counts(prof, counts, len(plain.pLen))
                    n += 1
    assert n >= 150 + 60


# ---------------------------------------------------------------------------------------------------------------- 2
def _against_exact(cases):
    """Every plane and row of both modes against the reference -> (pairs with a path, largest relative gap in exact mode, largest
    share of the table's log bound used)."""
    n, gap, share = 0, 0., 0.
    for name, p, pairs, band, rows, exact, table in cases:
        P = p.c.n_len
        zero = R.zero_planes(p.plain)
        for i, ((a, b), (ll, want)) in enumerate(zip(pairs, rows)):
            for res in (exact, table):
                assert res.status[i] == (K.COUNTS_NO_PATH if want is None else K.COUNTS_OK), (name, i)
                blk = res.pair_profiles[i]
                assert blk.shape == (6 + P, len(a) + 1) and not np.isnan(blk).any() and not np.isnan(res.pair_ll[i]), (name, i)
                assert (blk[zero] == 0).all(), (name, i, zero)
                if want is None:
                    assert (blk == 0).all() and res.pair_ll[i] == NEG, (name, i)
            if want is None:
                continue
            assert (exact.pair_profiles[i][:R.DUP, len(a)] == 0).all() and (table.pair_profiles[i][:R.DUP, len(a)] == 0).all()
            rel = K.exact_rel_bound(p.plain, len(a), len(b))
            got = exact.pair_profiles[i]
            assert (np.abs(got - want) <= rel * want + 1e-300).all(), (name, i, rel, np.abs(got - want).max())
            nz = want > 0
            gap = max(gap, float((np.abs(got - want)[nz] / want[nz]).max(initial=0.)))
            e = K.table_log_bound(len(a), len(b), P)
            got = table.pair_profiles[i]
            assert (got >= want * math.exp(-e) - 1e-300).all() and (got <= want * math.exp(e) + 1e-300).all(), (name, i)
            nz = (want > 1e-290) & (got > 0)
            share = max(share, float(np.abs(np.log(got[nz] / want[nz])).max(initial=0.)) / e)
            n += 1
    return n, gap, share


def test_host_statement_against_the_exact_reference(cases):
    for label, least in (("tiny", 150), ("medium", 60), ("boundary", 1)):
        n, gap, share = _against_exact(cases[label])
        print("%s: %d pairs; exact mode, largest relative gap %.3g; table mode, largest share of the log bound used %.3g" % (label, n, gap, share))
        assert n >= least
    assert len(cases["boundary"]) == 56
    none = sum(int((table.status == K.COUNTS_NO_PATH).sum()) for *_, table in cases["boundary"])
    assert none > 0


# ---------------------------------------------------------------------------------------------------------------- 3
def test_invariants(da, cases):
    """Every path consumes each base of the original exactly once; the rows summed are the counts; Z is the forward score."""
    n = 0
    for name, p, pairs, band, rows, exact, table in everything(cases):
        P = p.c.n_len
        a, b = C.seqs(pairs)
        for res, is_exact in ((exact, True), (table, False)):
            counts = da.pairCounts(p, a, b, band=band, host=True, exact=is_exact)
            assert np.array_equal(res.status, counts.status), name
            assert np.array_equal(bits(res.pair_ll), bits(da.pairLikelihoods(p, a, b, band=band, host=True, exact=is_exact))), name
            for i, (x, y) in enumerate(pairs):
                if res.status[i] != K.COUNTS_OK:
                    continue
                blk = res.pair_profiles[i]
                I, O = len(x), len(y)
                tol = 1e-9 if is_exact else math.expm1(K.table_log_bound(I, O, P))
                assert (np.abs(blk[:R.DUP, :I].sum(axis=0) - 1) <= tol).all(), (name, i, is_exact)
                c = counts.pair_counts[i]
                want = np.concatenate(([c[2], c[0], c[3]], c[21:]))
                got = np.concatenate(([blk[:R.DEL_OPEN].sum()], blk[R.DEL_OPEN:].sum(axis=1)))
                assert np.allclose(got, want, rtol=1e-12, atol=1e-300), (name, i, is_exact, got, want)
                n += 1
    assert n >= 2 * (150 + 60)
    # reads given as their reverse complement, read in place
    name, p, pairs, band, rows, exact, table = cases["medium"][0]
    a, b = C.seqs(pairs)
    strand = [i % 2 for i in range(len(b))]
    flipped = [da.reverse_complement(y).astype(np.int8) if s else y for y, s in zip(b, strand)]
    got = da.pairProfiles(p, a, flipped, band=band, read_strand=strand, host=True)
    assert np.array_equal(bits(got.pair_ll), bits(table.pair_ll)) and np.array_equal(bits(got.profile), bits(table.profile))
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got.pair_profiles, table.pair_profiles))


# ---------------------------------------------------------------------------------------------------------------- 4
def test_aggregates(da):
    """Both anchors over originals of different lengths with a NO_PATH pair among them, n_positions shorter than the longest
    original, against the numpy restatement from the per-pair blocks."""
    from test_pair_align_cpu import make_params
    for x in range(4):
        for y in range(4):
            assert (y == (x ^ 2)) == K._is_transition(x, y)                    # the fold of the aggregate, in the ACGT coding
    params = make_params(da, [.5, .3, .2], pTanDup=.05)
    ins = ["ACGTACGTAC", "GGATC", "", "TTGACCAGTACGG", "A", "CAGT"]
    outs = ["ACGTTACGAC", "GATC", "", "TTGACAGTACCGG", "G", "CAGT"]
    none = make_params(da, [])                                               # no duplications: a longer read has no path
    for p, reads in ((params, outs), (none, ["ACGTACGTAC", "GATC", "", "TTGACCAGTAGG", "AC", "CAT"])):
        full = da.pairProfiles(p, ins, reads, band=-1, host=True)
        lost = full.status == K.COUNTS_NO_PATH
        assert lost.sum() == (1 if p is none else 0) and full.profile.shape == (5 + p.c.n_len, 14) and full.anchor == "start"
        for anchor in ("start", "end"):
            got = da.pairProfiles(p, ins, reads, band=-1, host=True, anchor=anchor)
            codes = [da.tokenize(a) for a in ins]
            want, cover = R.fold(got.pair_profiles, codes, got.status, anchor, 14)
            assert np.array_equal(got.coverage, cover) and cover[0] == 6 - lost.sum() and cover[13] == 1
            np.testing.assert_allclose(got.profile, want, rtol=1e-13, atol=0)
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got.pair_profiles, full.pair_profiles))
            rates = got.rates()
            assert sorted(rates) == ["deletion", "duplication", "substitution"] and all(v.shape == (14,) for v in rates.values())
            np.testing.assert_allclose(rates["deletion"], (want[R.SUM_DEL_OPEN] + want[R.SUM_DEL_EXTEND]) / cover, rtol=1e-13)
            # fewer positions than the longest original has rows: the same columns, the rest dropped
            short = _host_call(da, p, ins, reads, anchor, 7)
            assert np.array_equal(bits(short[0]), bits(got.profile[:, :7])) and np.array_equal(short[1], got.coverage[:7])
            # without the per-pair output the aggregate is the same
            alone = da.pairProfiles(p, ins, reads, band=-1, host=True, anchor=anchor, per_pair=False)
            assert alone.pair_profiles is None and np.array_equal(bits(alone.profile), bits(got.profile))
            assert np.array_equal(alone.coverage, got.coverage)


def _host_call(da, params, ins, outs, anchor, n_pos):
    """dnas_pair_profiles_host through ctypes with a caller-chosen n_positions -> (profile[5 + P, n_pos], coverage)."""
    a = [da.tokenize(x) for x in ins]
    b = [da.tokenize(x) for x in outs]
    io = np.concatenate(([0], np.cumsum([len(x) for x in a]))).astype(np.int64)
    oo = np.concatenate(([0], np.cumsum([len(x) for x in b]))).astype(np.int64)
    av, bv = np.concatenate(a + [np.zeros(1, np.int8)]).astype(np.int8), np.concatenate(b + [np.zeros(1, np.int8)]).astype(np.int8)
    n = len(a)
    profile, coverage = np.zeros((5 + params.c.n_len, n_pos)), np.zeros(n_pos, dtype=np.int64)
    pll, status = np.zeros(n), np.zeros(n, dtype=np.uint8)
    rc = da.lib.lib().dnas_pair_profiles_host(ctypes.byref(params.c), -1, n, av.ctypes.data, io.ctypes.data, bv.ctypes.data, oo.ctypes.data,
                                              None, 0, 1 if anchor == "end" else 0, n_pos, profile.ctypes.data, coverage.ctypes.data, None,
                                              pll.ctypes.data, status.ctypes.data)
    assert rc == 0
    return profile, coverage


# ---------------------------------------------------------------------------------------------------------------- 5
def test_argument_checks_and_edge_shapes(da):
    from test_pair_align_cpu import make_params
    L = da.lib.lib()
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.pairProfiles(make_params(da, [1. / 14] * 14), ["ACGT"], ["ACT"], host=True)
    params = make_params(da, [.5, .5])
    ins, outs = np.array([0, 1, 2, 3], np.int8), np.array([0, 1, 3], np.int8)
    profile, coverage, per = np.zeros((7, 5)), np.zeros(5, np.int64), np.zeros(8 * 5)
    pll, status = np.zeros(1), np.zeros(1, np.uint8)

    def ptr(x):
        return x.ctypes.data if x is not None else None

    def call(bases=ins, in_off=(0, 4), out_off=(0, 3), band=-1, n=1, exact=0, anchor=0, n_pos=5, profile=profile, coverage=coverage,
             per=per, pll=pll, status=status):
        io, oo = np.array(in_off, np.int64), np.array(out_off, np.int64)
        return L.dnas_pair_profiles_host(ctypes.byref(params.c), band, n, ptr(bases), io.ctypes.data, outs.ctypes.data, oo.ctypes.data,
                                         None, exact, anchor, n_pos, ptr(profile), ptr(coverage), ptr(per), ptr(pll), ptr(status))
    assert call() == 0 and np.isfinite(pll[0]) and status[0] == K.COUNTS_OK and (coverage == 1).all()
    assert abs(per.reshape(8, 5)[:6, :4].sum() - 4) < 1e-3
    assert call(per=None) == 0 and call(n_pos=0, profile=None, coverage=None) == 0          # the optional outputs
    assert call(anchor=2) == E_INVALID and "anchor" in L.dnas_last_error().decode()
    assert call(anchor=-1) == E_INVALID and call(n_pos=-1) == E_INVALID
    assert call(profile=None) == E_INVALID and call(coverage=None) == E_INVALID
    assert call(np.array([0, 1, 2, 4], np.int8)) == E_BAD_BASE
    assert call(band=-2) == E_INVALID and "band" in L.dnas_last_error().decode()
    assert call(in_off=(1, 4)) == E_INVALID and call(out_off=(2, 3)) == E_INVALID
    assert call(in_off=(0, -1)) == E_INVALID and call(in_off=(0, (1 << 20) + 1)) == E_UNSUPPORTED
    assert call(n=-1) == E_INVALID and call(bases=None) == E_INVALID
    assert call(pll=None) == E_INVALID and call(status=None) == E_INVALID
    profile[:] = 7
    assert call(n=0, bases=None, pll=None, status=None, per=None) == 0 and (profile == 0).all() and (coverage == 0).all()
    empty = da.pairProfiles(params, [], [], host=True)
    assert empty.pair_ll.shape == (0,) and empty.profile.shape == (7, 0) and empty.pair_profiles == [] and empty.stats is None
    with pytest.raises(ValueError):
        da.pairProfiles(params, ["ACGT", "AC"], ["ACT"], host=True)
    with pytest.raises(ValueError):
        da.pairProfiles(params, ["ACGT"], ["ACT"], exact=True)               # exact is a mode of the host statement
    with pytest.raises(ValueError):
        da.pairProfiles(params, ["ACGT"], ["ACT"], host=True, anchor="middle")
    # I = 0 and O = 0: one row that holds nothing; an original with an empty read is all deletions
    edge = da.pairProfiles(params, ["", "ACG", ""], ["", "", "A"], host=True)
    assert list(edge.status) == [K.COUNTS_OK, K.COUNTS_OK, K.COUNTS_NO_PATH]
    assert edge.pair_profiles[0].shape == (8, 1) and (edge.pair_profiles[0] == 0).all() and edge.pair_ll[0] == 0
    gone = edge.pair_profiles[1]
    assert gone.shape == (8, 4) and (gone[:4] == 0).all() and (gone[R.DUP:] == 0).all()
    tol = math.expm1(K.table_log_bound(3, 0, 2))
    np.testing.assert_allclose(gone[R.DEL_OPEN, :3] + gone[R.DEL_EXTEND, :3], 1, rtol=tol)
    assert gone[R.DEL_OPEN, 0] == pytest.approx(1, rel=tol) and gone[R.DEL_EXTEND, 0] == 0
    assert (edge.pair_profiles[2] == 0).all() and list(edge.coverage) == [2, 1, 1, 1]
    one = da.pairProfiles(params, ["ACGT"], ["ACT", "ACGT", ""], host=True)  # one original pairs with every read
    assert one.pair_ll.shape == (3,) and (one.status == K.COUNTS_OK).all() and (one.coverage == 3).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_host_statement_under_sanitizers(tmp_path):
    """pairProfileHost and the aggregate over lengths 0 to 24 squared, bands 0, 1, 5 and -1, P of 0, 2, 6 and 13, both anchors, on
    heap blocks of exactly the sequences' and the profiles' sizes, in a stand-alone host program built with
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "pair_profile_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "pair_profile_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=600)
    assert r.returncode == 0 and b"pair profile host check: ok (20000 pairs)" in r.stdout, r.stderr.decode()
