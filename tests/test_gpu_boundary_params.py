"""Every kernel family at error-model probabilities of exactly 0 and 1, of 1e-300 and of 1 - 2^-53 (exact_models.BOUNDARY_VARIANTS).

A probability of 0 is a score of -inf that reaches the kernels through a *score*, not through an unreachable cell: the E-step's
log-sum-exp (csrc/fwdback_onchip.hip, csrc/fwdback_kernels.hip), the decoder's folds, offers and tracebacks
(csrc/viterbi_tiera.hip, csrc/viterbi_kernels.hip) and the max-plus bands of the pair-HMM family (csrc/pair_align_device.h) each
carry their own handling of it.  A probability of 1e-300 is a score near -690: every log-sum-exp difference is beyond the table,
and anything that leaves log space underflows.  The references are those of the rest of the suite and so are the bounds: the path
enumeration and the Bellman-Ford graph of exact_models (the tiny bounds, VITERBI_REL), the C oracle bit for bit, and the host
statements of the pair-HMM family bit for bit.  No tolerance is introduced here.  test_exact_models_cpu.py and
test_pair_align_cpu.py hold the CPU side of every case list used here to the same references."""
import contextlib
import os
import random
import sys
import types

import numpy as np
import pytest

import exact_models as X

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY, _rand, shape_pool as assign_pool  # noqa: E402
from test_cluster_cpu import K, same_results, shape_pool as cluster_pool  # noqa: E402
from test_consensus_cpu import shape_pool as consensus_pool  # noqa: E402
from test_gpu_assign import _same as same_assignments  # noqa: E402
from test_gpu_column_handover import _check as check_against_oracle, _forty, _machines, _revcomp, _tier_a, _want, bits  # noqa: E402
from test_gpu_consensus import _same as same_consensus  # noqa: E402
from test_gpu_exact_models import ROUTINGS, _check_read, _decoder, _estep, _library_params, _pack  # noqa: E402
from test_gpu_fwdback import _close  # noqa: E402
from test_gpu_pair_align import _related, _same as same_alignments  # noqa: E402
from test_pair_align_cpu import BOUNDARY_MODELS, boundary_cases, exact_viterbi_pair, make_params, tok  # noqa: E402
from test_polish_cpu import same_result as same_polish, shape_pool as polish_pool  # noqa: E402

NEG = float("-inf")
VARIANTS = X.BOUNDARY_NAMES


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _file_name(name):
    return name.replace("/", "-")


def _same_five(dp, params):
    c = dp.c
    return [c.p_del_open, c.p_del_extend, c.p_tan_dup, c.p_transition, c.p_transversion] == \
        [params.pDelOpen, params.pDelExtend, params.pTanDup, params.pTransition, params.pTransversion]


# ------------------------------------------------------------------------------------------------------------- the E-step
ESTEP_MODELS = {m[0]: m for m in X.boundary_estep_models()}
_estep_oracle = {}                     # (model name, "with" / "without") -> the oracle's (counts, ll, per-pair ll), computed once


def _oracle_counts(O, model, which, pairs):
    key = (model[0], which)
    if key not in _estep_oracle:
        _estep_oracle[key] = O.expected_counts(model[1], pairs, strict=model[2])
    return _estep_oracle[key]


@pytest.mark.parametrize("routing", ROUTINGS, ids=[r or "default" for r in ROUTINGS])
@pytest.mark.parametrize("name", list(ESTEP_MODELS))
def test_estep_against_every_path_and_the_oracle(da, oracle_mod, monkeypatch, tmp_path, name, routing):
    """One tiny base under one variant and one routing.  The pairs with a path: per-pair log-likelihoods and the 21 + P counts
    within the tiny bounds of the sum over every path, the log-likelihoods bit-identical to the oracle's and the counts within
    1e-9 of its (as test_gpu_fwdback.py compares them); the census says which kernel ran.  The pairs without a path, a database
    of their own: -inf per pair, counts NaN exactly where the oracle's are."""
    model = ESTEP_MODELS[name]
    _, params, strict, rows = model
    P = len(params.pLen)
    per_x, total_x, _ = X.exact_database(model, "enumerate")
    with_path, without = X.split_database(model, per_x)
    dp = _library_params(da, tmp_path, _file_name(name), X.params_text(params))
    assert list(dp.pLen) == list(params.pLen) and _same_five(dp, params)
    if with_path:                          # (tiny-P2-strict/gaps0 has none)
        want = per_x[per_x != NEG]
        oc, oll, oper = _oracle_counts(oracle_mod, model, "with", with_path)
        counts, ll, per, st = _estep(da, monkeypatch, _pack(with_path), dp, strict, routing)
        n = len(with_path)
        gap = np.abs(per - want) / np.maximum(1., np.abs(want))
        print("%s %s: ll gap %.3e, count gap %.3e, %s" % (name, routing, gap.max(), np.abs(counts - total_x).max(),
                                                          {k: st[k] for k in ("pairs_onchip", "pairs_streaming", "pairs_narrow")}))
        assert len(counts) == 21 + P and np.isfinite(per).all() and np.isfinite(counts).all()
        assert (gap <= X.ESTEP_LL_REL["tiny"]).all(), gap.max()
        assert (np.abs(counts - total_x) <= X.ESTEP_COUNT_ABS["tiny"]).all(), np.abs(counts - total_x).max()
        assert abs(ll - want.sum()) <= X.ESTEP_LL_REL["tiny"] * np.maximum(1., np.abs(want)).sum()
        assert np.array_equal(per.view(np.uint64), oper.view(np.uint64)), (per, oper)
        assert _close(counts, oc), (counts, oc)
        assert ll == pytest.approx(oll, rel=1e-12)
        if routing != "devices":
            assert st["pairs_onchip"] + st["pairs_streaming"] == n
            assert st["pairs_onchip"] == (0 if routing == "DNAS_FB_STREAMING" or P > 8 else n), st
        if routing == "DNAS_FB_NO_NARROW":
            assert st["pairs_narrow"] == 0
    if without:
        oc, oll, oper = _oracle_counts(oracle_mod, model, "without", without)
        counts, ll, per, st = _estep(da, monkeypatch, _pack(without), dp, strict, routing)
        assert (oper == NEG).all() and (per == NEG).all(), (per, oper)
        assert np.array_equal(np.isnan(counts), np.isnan(oc)), (counts, oc)
    assert len(with_path) + len(without) == X.TINY_PER_MODEL


@pytest.mark.parametrize("variant", ("tanDup0", "sub0", "rare"))
def test_fit_started_at_a_boundary(da, oracle_mod, tmp_path, variant):
    """baumWelchParams from a start with a probability of 0 (or of 1e-300) on the pairs of tiny-P3-loose that have a path under
    that start: the oracle's fit from the same start, as test_gpu_fwdback.py compares fits; the first M-step's Laplace prior has
    made every parameter positive."""
    O = oracle_mod
    model = ESTEP_MODELS["tiny-P3-loose/" + variant]
    _, params, strict, rows = model
    with_path, _ = X.split_database(model, X.exact_database(model, "enumerate")[0])
    assert len(with_path) >= 6
    dp = _library_params(da, tmp_path, _file_name(model[0]), X.params_text(params))
    assert _same_five(dp, params)
    fit, iters = da.baumWelchParams(dp, _pack(with_path), strict=strict)
    ofit = O.baum_welch(params, with_path, strict=strict)
    got = [fit.c.p_del_open, fit.c.p_del_extend, fit.c.p_tan_dup, fit.c.p_transition, fit.c.p_transversion]
    want = [ofit.pDelOpen, ofit.pDelExtend, ofit.pTanDup, ofit.pTransition, ofit.pTransversion]
    assert np.allclose(got, want, rtol=1e-9), (got, want)
    assert fit.pLen == ofit.pLen and fit.local == ofit.local
    assert 1 <= iters <= 100
    assert all(0. < x < 1. for x in got) and all(x > 0. for x in fit.pLen), (got, fit.pLen)


# ------------------------------------------------------------------------------- the decoder on small machines: Bellman-Ford
VITERBI_CASES = {c[0]: c for c in X.boundary_viterbi_cases()}
VITERBI_OPTIONS = (None, "tier=B", "tier=C,cluster=2")
_base_cases = {}
_base_tier = {}                        # (base case, options) -> dec.tier under the base parameters, None where the tier is refused


def _program(tier):
    """The tier string without its last clause: where a tier-C model puts its sync words is measured when the model is made and
    differs from one model to the next; everything in front of it names the plan and the kernel."""
    return tier.split("; sync words at")[0]


def _tier_of_the_base(da, tmp_path, base, options):
    if not _base_cases:
        _base_cases.update({c[0]: c for c in X.viterbi_cases()})
    if (base, options) not in _base_tier:
        name, text, ptext, reads = _base_cases[base]
        dec = _decoder(da, da.Machine.fromJSON(text), _library_params(da, tmp_path, name, ptext), options)
        _base_tier[base, options] = None if dec is None else dec.tier
        if dec is not None:
            dec.close()
    return _base_tier[base, options]


@pytest.mark.parametrize("options", VITERBI_OPTIONS, ids=["default", "tierB", "tierC-cluster2"])
@pytest.mark.parametrize("name", list(VITERBI_CASES))
def test_viterbi_against_bellman_ford(da, tmp_path, name, options):
    """One random machine (3 to 40 states, D = 0, 2, 4, 8), global or local, under one variant and one tier: the batch and every
    read alone give the exact optimum, the status and a string readable along tight paths; read by read, every lane of every
    lattice cell.  The tier string is that of the base parameters: parameters do not change the program."""
    case = VITERBI_CASES[name]
    _, text, ptext, reads = case
    base = name.split("/")[0]
    base_tier = _tier_of_the_base(da, tmp_path, base, options)
    dec = _decoder(da, da.Machine.fromJSON(text), _library_params(da, tmp_path, _file_name(name), ptext), options)
    assert (dec is None) == (base_tier is None), (name, options, base_tier)
    if dec is None:                        # the machine does not admit this tier, whatever the parameters
        assert options is not None
        return
    try:
        assert _program(dec.tier) == _program(base_tier), (dec.tier, base_tier)
        if options:
            assert dec.tier.startswith("tier " + options[5]), dec.tier
        want = X.exact_viterbi_case(case)
        out, ll, st = dec.decode(reads)
        for i, r in enumerate(reads):
            _check_read((name, options, "batch"), r, (out[i], ll[i], st[i]), want[i])
        for i, r in enumerate(reads):
            out1, ll1, st1 = dec.decode([r])
            _check_read((name, options, "alone"), r, (out1[0], ll1[0], st1[0]), want[i])
            lat = np.ascontiguousarray(dec.lattice(0, len(r)).transpose(0, 2, 1))
            assert X.lattice_close(lat, want[i][1]), (name, options, r)
    finally:
        dec.close()                        # (a failing case must not leave its model on the card for the cases after it)


# ------------------------------------------------------------------------- the shipped tier-A programs: the oracle, bit for bit
SHIPPED = (("s16h74l4c4.json", False), ("h74l4c4.json", True))        # T1024 with 14 rows; at most 8 rows, two work-groups per CU
ROUTE_VARIANTS = ("tanDup0", "sub0", "delExt1", "rare")
ROUTES = ("thread-traceback", "csr-wave-traceback", "csr-thread-traceback", "segments", "both-strands")
_shipped_tier = {}


def _shipped(da, O, ref_data, tmp_path, mach, variant):
    """-> (library machine, oracle machine, library params, oracle params, the cache's name of the model, the three reads)."""
    m, om = _machines(da, O, ref_data, mach)
    q = X.boundary_params(O.MutatorParams.from_cli(global_=True), variant)
    dp = _library_params(da, tmp_path, variant, X.params_text(q))
    assert list(dp.pLen) == list(q.pLen) and _same_five(dp, q) and not dp.local
    long_ = _forty(m)
    return m, om, dp, q, "boundary/" + variant, [long_, long_[:9], ""]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mach,two_per_cu", SHIPPED)
def test_shipped_programs_against_the_oracle(da, oracle_mod, ref_data, tmp_path, mach, two_per_cu, variant):
    """The 12 361-state machine's 14-row program and the 1 013-state machine's two-per-CU program, global mode, under one
    variant: a read of about 40 nt, its 9-nt prefix and the empty read; string, log-likelihood bits, status and every lattice
    cell as uint64 equal the oracle's.  The program is the one the default parameters get."""
    O = oracle_mod
    m, om, dp, q, key, reads = _shipped(da, O, ref_data, tmp_path, mach, variant)
    if mach not in _shipped_tier:
        dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True))
        _shipped_tier[mach] = dec.tier
        dec.close()
    with contextlib.closing(da.ViterbiDecoder(m, dp)) as dec:
        _tier_a(dec, two_per_cu)
        assert dec.tier == _shipped_tier[mach], (dec.tier, _shipped_tier[mach])
        check_against_oracle(dec, O, om, mach, key, reads, dec.decode(reads), params=q)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("variant", ROUTE_VARIANTS)
def test_shipped_program_other_routes(da, oracle_mod, ref_data, tmp_path, monkeypatch, variant, route):
    """The 14-row program's other routes under four variants: the thread-per-read traceback, both tracebacks through the CSR
    arrays instead of the node records, lattice segments of the minimum width (string and log-likelihood only: no whole lattice
    exists), and both strands on the read and its reverse complement."""
    O = oracle_mod
    mach = "s16h74l4c4.json"
    m, om, dp, q, key, reads = _shipped(da, O, ref_data, tmp_path, mach, variant)
    monkeypatch.delenv("DNAS_NO_NODE_RECORDS", raising=False)
    if route.startswith("csr"):
        monkeypatch.setenv("DNAS_NO_NODE_RECORDS", "1")
    options = {"segments": "checkpoint=always,segment=6", "thread-traceback": "traceback=thread",
               "csr-thread-traceback": "traceback=thread"}.get(route)
    with contextlib.closing(da.ViterbiDecoder(m, dp, options=options)) as dec:
        _tier_a(dec, False)
        if route == "segments":
            assert dec.max_dup_len == 4
            got = dec.decode(reads[:1])
            assert dec.stats()["checkpointed_reads"] == 1
            check_against_oracle(dec, O, om, mach, key, reads[:1], got, lattice=False, params=q)
        elif route == "both-strands":
            for given in (reads[0], _revcomp(reads[0])):
                out, ll, st, strand = dec.decode([given], strands="both")
                f = _want(O, om, mach, key, given, lattice=False, params=q)
                b = _want(O, om, mach, key, _revcomp(given), lattice=False, params=q)
                rev = b[1] > f[1]
                s, oll = (b if rev else f)[:2]
                assert out[0] == s and bits(ll[0]) == bits(oll) and strand[0] == int(rev), (out[0], s, ll[0], oll, strand[0])
        else:
            check_against_oracle(dec, O, om, mach, key, reads, dec.decode(reads), params=q)


# ----------------------------------------------------------------------------------- the pair-HMM family: the host, bit for bit
ALIGN_IDS = ["%s/%s" % (m, v) for m in BOUNDARY_MODELS for v in VARIANTS]
SCORE_VARIANTS = ("gaps0", "match0", "tanDup0", "rare")
_align_cases = {}


def _variant_of(da, params, variant):
    """A library MutatorParams with the variant's overrides."""
    c = params.c
    base = types.SimpleNamespace(pDelOpen=c.p_del_open, pDelExtend=c.p_del_extend, pTanDup=c.p_tan_dup, pTransition=c.p_transition,
                                 pTransversion=c.p_transversion, pLen=[c.p_len[k] for k in range(c.n_len)], local=bool(c.local))
    q = X.boundary_params(base, variant)
    return make_params(da, q.pLen, q.pDelOpen, q.pDelExtend, q.pTanDup, q.pTransition, q.pTransversion, q.local)


@pytest.mark.parametrize("name", ALIGN_IDS)
def test_align_pairs(da, monkeypatch, name):
    """alignPairs on the 64 pairs of P2 or P4 under one variant, full matrix and band 4, with the grid as shipped and with two
    work-groups (8 waves, every wave walks several pairs): score bits, statuses and op strings of the host; the full-matrix
    scores and statuses also against the exact model, which is no code of the library's."""
    if not _align_cases:
        _align_cases.update({c[0]: c for c in boundary_cases(da)})
    _, params, pairs = _align_cases[name]
    ins, outs = [a for a, _ in pairs], [b for _, b in pairs]
    for band in (-1, 4):
        want = da.alignPairs(params, ins, outs, band=band, host=True)
        for blocks in (None, "2"):
            monkeypatch.delenv("DNAS_ALIGN_BLOCKS", raising=False)
            if blocks:
                monkeypatch.setenv("DNAS_ALIGN_BLOCKS", blocks)
            got = da.alignPairs(params, ins, outs, band=band)
            same_alignments(got, want)
            assert got.stats["pairs_too_large"] == 0
        if band == -1:
            assert {int(s) for s in got.status} == {da.lib.ALIGN_OK, da.lib.ALIGN_NO_PATH}
            for i, (a, b) in enumerate(pairs):
                exact = exact_viterbi_pair(params.plain, tok(a), tok(b))
                assert (exact == NEG) == (got.status[i] == da.lib.ALIGN_NO_PATH), (name, a, b, got.score[i], exact)
                assert X.ll_close(float(got.score[i]), exact), (name, a, b, got.score[i], exact)


@pytest.mark.parametrize("variant", ("gaps0", "match0", "rare"))
def test_align_pairs_boundary_row_beyond_lds(da, variant):
    """Reads of more than 1015 bases, whose stripes hand their last row on through HBM: that row then carries -inf (gaps0,
    match0) and scores of -690 a step (rare).  The list of test_gpu_pair_align.py and a copy with substitutions only, which
    keeps a path without gaps."""
    rng = random.Random("gpu-pair-align/long")
    params = _variant_of(da, da.MutatorParams.fromFlags(**NOISY), variant)
    a = _rand(rng, 1100)
    ins = [a, _rand(rng, 130), a[:200]]
    outs = [_related(rng, a, 1104), _rand(rng, 1100), _related(rng, a[:200], 198)]
    sub = list(a)
    for at in (0, 511, 1024, 1099):
        sub[at] = "ACGT"[("ACGT".index(sub[at]) + 2) % 4]          # a transition
    ins.append(a)
    outs.append("".join(sub))
    for band in (8, -1):
        want = da.alignPairs(params, ins, outs, band=band, host=True)
        same_alignments(da.alignPairs(params, ins, outs, band=band), want)
        if variant == "gaps0":
            assert list(want.status) == [da.lib.ALIGN_NO_PATH] * 3 + [da.lib.ALIGN_OK]
        if variant == "rare":
            assert (want.status == da.lib.ALIGN_OK).all() and (want.score < -690).all()


def _chunks_of_37(monkeypatch, env):
    monkeypatch.setenv(env, "37")                          # a prime: chunks end inside a read's (a candidate's, a row's) items


@pytest.mark.parametrize("variant", SCORE_VARIANTS)
def test_assign_reads(da, monkeypatch, variant):
    """assignReads on the shape pool of test_assign_cpu.py in chunks of 37 items: winners, runners-up, statuses (NO_PATH among
    them) and every item score, -inf included."""
    params = _variant_of(da, da.MutatorParams.fromFlags(**NOISY), variant)
    originals, reads = assign_pool(da)
    _chunks_of_37(monkeypatch, "DNAS_ASSIGN_CHUNK")
    want = da.assignReads(params, originals, reads, band=8, host=True, item_scores=True)
    assert any(np.isneginf(x).any() for x in want.item_scores) and any(np.isfinite(x).any() for x in want.item_scores)
    got = da.assignReads(params, originals, reads, band=8, item_scores=True)
    same_assignments(got, want)
    assert got.stats["chunks"] == -(-got.stats["items"] // 37) > 1


@pytest.mark.parametrize("variant", SCORE_VARIANTS)
def test_consensus_score(da, monkeypatch, variant):
    """consensusScore on the shape pool of test_consensus_cpu.py in chunks of 37 items."""
    params = _variant_of(da, da.MutatorParams.fromFlags(**NOISY), variant)
    cands, reads, strands = consensus_pool(da)
    _chunks_of_37(monkeypatch, "DNAS_CONSENSUS_CHUNK")
    want = da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True)
    assert np.isneginf(want.total).any() and np.isfinite(want.total).any()
    got = da.consensusScore(params, cands, reads, band=8, read_strand=strands)
    same_consensus(got, want)
    assert got.stats["chunks"] == -(-got.stats["items"] // 37) > 1


@pytest.mark.parametrize("variant", SCORE_VARIANTS)
def test_consensus_reads(da, variant):
    """consensusReads on the shape pool of test_polish_cpu.py, two rounds."""
    params = _variant_of(da, da.MutatorParams.fromFlags(**NOISY), variant)
    templates, reads, strands = polish_pool(da)
    want = da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=2, host=True)
    got = da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=2)
    same_polish(got, want)
    assert got.stats["rounds"] >= 1 and got.stats["pairs"] >= sum(len(r) for r in reads)


@pytest.mark.parametrize("variant", SCORE_VARIANTS)
def test_cluster_reads(da, monkeypatch, variant):
    """clusterReads on the shape pool of test_cluster_cpu.py with every pair scored on both strands and no floor, in bands of
    37 pairs: the edge list is the candidate list with every pair's better score, -inf included; and once through the
    edit-distance gate."""
    params = _variant_of(da, da.MutatorParams.fromFlags(**NOISY), variant)
    reads = cluster_pool(da)
    opts = dict(band=8, k=K, min_shared=0, min_score_per_nt=NEG, edges=True)
    want = da.clusterReads(params, reads, host=True, **opts)
    assert want.stats["edges"] == want.stats["candidates"] > 37
    if variant in ("gaps0", "tanDup0"):                    # (under the other two the host finds a path for every pair)
        assert np.isneginf(want.edges[1]).any() and np.isfinite(want.edges[1]).any()
    _chunks_of_37(monkeypatch, "DNAS_CLUSTER_CHUNK")
    got = da.clusterReads(params, reads, **opts)
    same_results(got, want)
    assert got.stats["chunks"] == -(-want.stats["candidates"] // 37)
    gated = da.clusterReads(params, reads, host=True, max_edit_permille=300, **opts)
    assert 0 < gated.stats["edges"] < want.stats["edges"]
    same_results(da.clusterReads(params, reads, max_edit_permille=300, **opts), gated)
