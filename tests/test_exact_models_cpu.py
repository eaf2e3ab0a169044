"""The CPU oracle against exact references of the two models (tests/exact_models.py): the third pin.

The GPU tests hold the HIP kernels to the C oracle bit for bit, and the oracle is pinned to the reference by a handful of golden
files.  Here the oracle is held to references written from the models' generative definitions -- every path of the mutator pair
HMM enumerated in mpmath, the same sums by an exact forward-backward pass for pairs too large to enumerate, and the Viterbi
lattice as an explicit graph solved by Bellman-Ford -- so that a reading of the reference shared by oracle and kernels (a count
credited to the wrong lane, ctx[k] off by one, a term lost at a band edge, deletions that miss null edges) does not pass unseen.
The bounds are exact_models' (measured as its docstring says, never taken from the code under test)."""
import numpy as np
import pytest

import exact_models as X


@pytest.fixture(scope="module")
def tiny():
    """[(model, per-pair exact ll, summed exact counts, paths walked)] of the 16 tiny models, enumerated once."""
    return [(m,) + X.exact_database(m, "enumerate") for m in X.tiny_models()]


def test_guide_columns_agree_with_the_oracles_reader(oracle_mod):
    """exact_models reads a guide alignment by its own definition; the oracle's reader sees the same envelope columns."""
    for model in X.tiny_models() + X.medium_models():
        for r in model[3]:
            mine, theirs = X.guide_columns(*r), oracle_mod.alignment_pair([("in", r[0]), ("out", r[1])])
            assert all(np.array_equal(a, b) for a, b in zip(mine, theirs)), r


def test_case_list_shares(tiny):
    """At least 300 tiny pairs; between 5% and 20% of them have no path; for at least a quarter the guide envelope removes
    paths (fewer are walked than with the envelope wide open); inLen = 0, outLen = 0 and all-gap guides are among them."""
    n = no_path = restricted = 0
    for model, per, total, walked in tiny:
        for r, ll, inside in zip(model[3], per, walked):
            ins, outs, ci, co = X.guide_columns(*r)
            wide = X.enumerate_pair(model[1], ins, outs, ci, co, model[2], open_envelope=True, count_only=True)[2]
            counted = X.enumerate_pair(model[1], ins, outs, ci, co, model[2], count_only=True)[2]
            assert counted <= wide
            n += 1
            no_path += ll == float("-inf")
            restricted += counted < wide
    assert n >= 300
    assert .05 * n <= no_path <= .20 * n, (no_path, n)
    assert restricted >= n / 4, (restricted, n)
    rows = [r for model, *_ in tiny for r in model[3]]
    assert any(not r[0].replace("-", "") for r in rows) and any(not r[1].replace("-", "") for r in rows)
    assert any(r[0] and all(a == "-" or b == "-" for a, b in zip(*r)) for r in rows)
    assert {len(m[1].pLen) for m, *_ in tiny} == {0, 1, 2, 3, 5, 6, 8, 9} and {m[2] for m, *_ in tiny} == {False, True}
    assert any(0. in m[1].pLen for m, *_ in tiny) and any(len(set(m[1].pLen)) > 1 for m, *_ in tiny)


def test_enumerator_against_oracle(oracle_mod, tiny):
    """Per-pair log-likelihoods and the database's 21 + P expected counts of every tiny model; the pairs without a path are a
    database of their own, -inf on both sides."""
    O = oracle_mod
    for model, per, total, walked in tiny:
        name, params, strict, rows = model
        with_path, without = X.split_database(model, per)
        oc, oll, oper = O.expected_counts(params, with_path, strict=strict)
        want = per[per != float("-inf")]
        assert np.isfinite(oper).all(), name
        gap = np.abs(oper - want) / np.maximum(1., np.abs(want))
        print("%s: ll gap %.3e, count gap %.3e" % (name, gap.max(initial=0.), np.abs(oc - total).max()))
        assert (gap <= X.ESTEP_LL_REL["tiny"]).all(), (name, gap.max())
        assert (np.abs(oc - total) <= X.ESTEP_COUNT_ABS["tiny"]).all(), (name, np.abs(oc - total).max())
        if without:
            assert (O.expected_counts(params, without, strict=strict)[2] == float("-inf")).all(), name


def test_exact_fwdback_equals_enumerator(tiny):
    """The forward-backward form of the exact model agrees with the path enumeration to 1e-12 on every enumerable pair."""
    for model, per, total, walked in tiny:
        name, params, strict, rows = model
        for r, ll in zip(rows, per):
            ins, outs, ci, co = X.guide_columns(*r)
            l2, c2 = X.exact_fwdback(params, ins, outs, ci, co, strict)
            if ll == float("-inf"):
                assert l2 == ll and np.isnan(c2).all(), (name, r)
                continue
            c1 = X.enumerate_pair(params, ins, outs, ci, co, strict)[1]
            assert abs(l2 - ll) <= 1e-12 and np.abs(c1 - c2).max() <= 1e-12, (name, r, ll, l2)


def test_exact_fwdback_against_oracle(oracle_mod):
    """Pairs of 20 to 80 bases (a 24-base deletion block and long runs of duplications among them), realistic parameters."""
    O = oracle_mod
    for model in X.medium_models():
        name, params, strict, rows = model
        per, total, _ = X.exact_database(model, "fwdback")
        assert np.isfinite(per).all(), name
        pairs = [X.guide_columns(*r) for r in rows]
        assert max(len(p[0]) for p in pairs) == 80 and min(len(p[0]) for p in pairs) == 20
        oc, oll, oper = O.expected_counts(params, pairs, strict=strict)
        gap = np.abs(oper - per) / np.maximum(1., np.abs(per))
        print("%s: ll gap %.3e, count gap %.3e" % (name, gap.max(), np.abs(oc - total).max()))
        assert (gap <= X.ESTEP_LL_REL["medium"]).all(), (name, gap.max())
        assert (np.abs(oc - total) <= X.ESTEP_COUNT_ABS["medium"]).all(), (name, np.abs(oc - total).max())


def test_exact_viterbi_against_oracle(oracle_mod):
    """Random machines of 3 to 40 states at every duplication width 0..8, local and global, and a global case without a path: the
    optimum, every lane of every lattice cell (-inf in the same places), and the oracle's string among those readable along
    tight paths.  A read with more than 64 such strings is exempt from the string assertion only; at most 10% may be."""
    O = oracle_mod
    n = ambiguous = no_path = 0
    widths, sizes = set(), set()
    for case in X.viterbi_cases() + [X.no_path_case()]:
        name, text, ptext, reads = case
        orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_json(ptext))
        widths.add(orc.D)
        sizes.add(orc.n)
        for r, (ll, lat, strings) in zip(reads, X.exact_viterbi_case(case)):
            s, oll, olat = orc.decode(r, want_lattice=True)
            assert X.ll_close(oll, ll), (name, r, oll, ll)
            assert X.lattice_close(olat, lat), (name, r)
            n += 1
            no_path += ll == float("-inf")
            if strings is None:
                ambiguous += 1
            else:
                assert s in strings, (name, r, s, sorted(strings))
    assert widths == set(range(9)) and min(sizes) == 3 and max(sizes) == 40
    assert no_path >= 1 and n >= 150
    assert ambiguous <= .10 * n, (ambiguous, n)


@pytest.mark.parametrize("case", X.GRADIENT_CASES)
def test_gradient_identity_on_the_oracle(oracle_mod, case):
    """Pairs of 256 and 1000 bases, out of reach of the exact models: for every free parameter the central difference of the
    summed log-likelihood equals the matching combination of expected counts (n / p - n' / (1 - ...)), to GRADIENT_REL of the
    terms' sum.  A coarse structural check: the table's cut-off is what limits it."""
    params, pairs = X.gradient_case(*case)
    dev = X.gradient_deviation(oracle_mod, params, pairs)
    print(case, {k: "%.2e" % v for k, v in dev.items()})
    assert set(dev) == {"pDelOpen", "pTanDup", "pDelExtend", "pTransition", "pTransversion"} | {"pLen[%d]" % k for k in range(case[1])}
    assert max(dev.values()) <= X.GRADIENT_REL, dev
