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


def _oracle_against_enumeration(O, model, per, total):
    """The assertions of one database: per-pair log-likelihoods and the 21 + P summed counts of the pairs with a path within the
    tiny bounds; the pairs without a path as a database of their own, -inf on both sides -> (pairs with a path, pairs without)."""
    name, params, strict, rows = model
    with_path, without = X.split_database(model, per)
    if with_path:
        oc, oll, oper = O.expected_counts(params, with_path, strict=strict)
        want = per[per != float("-inf")]
        assert np.isfinite(oper).all() and not np.isnan(oc).any(), name
        gap = np.abs(oper - want) / np.maximum(1., np.abs(want))
        print("%s: ll gap %.3e, count gap %.3e" % (name, gap.max(initial=0.), np.abs(oc - total).max()))
        assert (gap <= X.ESTEP_LL_REL["tiny"]).all(), (name, gap.max())
        assert (np.abs(oc - total) <= X.ESTEP_COUNT_ABS["tiny"]).all(), (name, np.abs(oc - total).max())
    if without:
        assert (O.expected_counts(params, without, strict=strict)[2] == float("-inf")).all(), name
    return len(with_path), len(without)


def test_enumerator_against_oracle(oracle_mod, tiny):
    """Per-pair log-likelihoods and the database's 21 + P expected counts of every tiny model; the pairs without a path are a
    database of their own, -inf on both sides."""
    for model, per, total, walked in tiny:
        n_with, _ = _oracle_against_enumeration(oracle_mod, model, per, total)
        assert n_with >= 1, model[0]


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


# ------------------------------------------------------------------ probabilities of exactly 0 and 1, of 1e-300 and of 1 - 2^-53
@pytest.fixture(scope="module")
def boundary():
    """{model name: (model, per-pair exact ll, summed exact counts, paths walked)} of exact_models.boundary_estep_models()."""
    return {m[0]: (m,) + X.exact_database(m, "enumerate") for m in X.boundary_estep_models()}


@pytest.mark.parametrize("base", X.BOUNDARY_ESTEP_BASES)
def test_enumerator_against_oracle_at_boundary_probabilities(oracle_mod, boundary, base):
    """The assertions and bounds of test_enumerator_against_oracle on one tiny base under the 14 boundary variants: a move of
    probability 0 is a score of -inf, one of 1e-300 a score near -690.  A variant under which no pair of the base has a path
    (tiny-P2-strict/gaps0) has no with-path database to compare."""
    empty = []
    for v in X.BOUNDARY_NAMES:
        model, per, total, walked = boundary["%s/%s" % (base, v)]
        n_with, n_without = _oracle_against_enumeration(oracle_mod, model, per, total)
        assert n_with + n_without == X.TINY_PER_MODEL
        if not n_with:
            empty.append(v)
    assert empty == (["gaps0"] if base == "tiny-P2-strict" else []), empty


def test_boundary_estep_population(boundary):
    """Over the four bases every variant has at least 6 pairs with a path and at least 6 without: both the finite arithmetic
    and the -inf bookkeeping are reached under each."""
    assert len(boundary) == len(X.BOUNDARY_ESTEP_BASES) * 14 and len(X.BOUNDARY_NAMES) == len(set(X.BOUNDARY_NAMES)) == 14
    for v in X.BOUNDARY_NAMES:
        pers = np.concatenate([boundary["%s/%s" % (base, v)][1] for base in X.BOUNDARY_ESTEP_BASES])
        without = int((pers == float("-inf")).sum())
        assert len(pers) - without >= 6 and without >= 6, (v, len(pers) - without, without)


BOUNDARY_VITERBI = X.boundary_viterbi_cases()
BOUNDARY_VITERBI_BASES = sorted({c[0].split("/")[0] for c in BOUNDARY_VITERBI})


@pytest.mark.parametrize("base", BOUNDARY_VITERBI_BASES)
def test_exact_viterbi_against_oracle_at_boundary_probabilities(oracle_mod, base):
    """One machine and alignment mode under the 14 variants: the optimum, every lane of every lattice cell (-inf in the same
    places) and the oracle's string among those readable along tight paths."""
    O = oracle_mod
    cases = [c for c in BOUNDARY_VITERBI if c[0].split("/")[0] == base]
    assert [c[0].split("/")[1] for c in cases] == list(X.BOUNDARY_NAMES)
    for case in cases:
        name, text, ptext, reads = case
        assert 1 <= len(reads) <= X.BOUNDARY_MAX_READS and max(map(len, reads)) <= 30
        orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_json(ptext))
        for r, (ll, lat, strings) in zip(reads, X.exact_viterbi_case(case)):
            s, oll, olat = orc.decode(r, want_lattice=True)
            assert X.ll_close(oll, ll), (name, r, oll, ll)
            assert X.lattice_close(olat, lat), (name, r)
            if strings is not None:
                assert s in strings, (name, r, s, sorted(strings))


def test_boundary_viterbi_population():
    """Over all boundary Viterbi cases at most 10% of the reads are exempt from the string check, and every variant has a read
    with a path on every machine."""
    n = ambiguous = 0
    with_path = {}
    for case in BOUNDARY_VITERBI:
        base, v = case[0].split("/")
        for ll, lat, strings in X.exact_viterbi_case(case):
            n += 1
            ambiguous += strings is None
            key = (base.rsplit("-", 1)[0], v)
            with_path[key] = with_path.get(key, 0) + (ll != float("-inf"))
    assert len(BOUNDARY_VITERBI) == 2 * len(X.BOUNDARY_VITERBI_MACHINES) * 14 and n >= 7 * len(BOUNDARY_VITERBI)
    assert ambiguous <= .10 * n, (ambiguous, n)
    assert len(with_path) == len(X.BOUNDARY_VITERBI_MACHINES) * 14 and min(with_path.values()) >= 1, with_path
