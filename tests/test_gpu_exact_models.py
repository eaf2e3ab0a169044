"""The HIP kernels against the exact references of the two models (tests/exact_models.py); the C oracle is not in the loop.

Every other GPU test asserts kernel == oracle bit for bit, so a reading of the reference that oracle and kernels share passes
them all.  Here the E-step (on-chip, half-width off, streaming, strict and loose guides, three handles on one card) is compared
with every path of the mutator pair HMM summed in mpmath, and the Viterbi decoder (default tier, tier B, a cluster of two; a batch
and one read at a time; both strands) with a Bellman-Ford solution of the explicit decoding graph: log-likelihoods, database
counts, status, every lattice cell, and the decoded string among those readable along tight paths.  The case lists and the
bounds are those of test_exact_models_cpu.py (exact_models' docstring says how the bounds were measured)."""
import numpy as np
import pytest

import exact_models as X

pytestmark = pytest.mark.gpu

NO_PATH = 1      # DNAS_READ_NO_PATH
ROUTINGS = (None, "DNAS_FB_NO_NARROW", "DNAS_FB_STREAMING", "devices")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _library_params(da, tmp_path, name, text):
    path = tmp_path / (name + ".params.json")
    path.write_text(text)
    return da.MutatorParams.fromFile(str(path))


def _pack(pairs):
    """The packed arrays dnas_fb_load_pairs takes: sequences and guide columns concatenated, with offsets."""
    def cat(idx, dt):
        off = np.zeros(len(pairs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p[idx]) for p in pairs])
        return (np.concatenate([p[idx] for p in pairs]).astype(dt) if off[-1] else np.zeros(1, dt)), off
    pk = dict(n=len(pairs))
    pk["ins"], pk["in_off"] = cat(0, np.int8)
    pk["outs"], pk["out_off"] = cat(1, np.int8)
    pk["cm_in"], pk["cm_in_off"] = cat(2, np.int32)
    pk["cm_out"], pk["cm_out_off"] = cat(3, np.int32)
    return pk


def _estep(da, monkeypatch, pk, params, strict, routing):
    for env in ("DNAS_FB_NO_NARROW", "DNAS_FB_STREAMING", "DNAS_FAKE_DEVICES"):
        monkeypatch.delenv(env, raising=False)
    if routing == "devices":
        monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    elif routing:
        monkeypatch.setenv(routing, "1")
    fb = da.ForwardBackward(pk, device=-1 if routing == "devices" else 0)
    if routing == "devices":
        assert fb.devices == 3
    counts, ll, per = fb.expectedCounts(params, strict=strict)
    st = fb.stats()
    fb.close()
    return counts, ll, per, st


def _check_estep(da, monkeypatch, tmp_path, model, method, kind):
    name, params, strict, rows = model
    per_x, total_x, _ = X.exact_database(model, method)
    with_path, without = X.split_database(model, per_x)
    want = per_x[per_x != float("-inf")]
    dp = _library_params(da, tmp_path, name, X.params_text(params))
    assert list(dp.pLen) == list(params.pLen)
    pk = _pack(with_path)
    census = {}
    for routing in ROUTINGS:
        counts, ll, per, st = _estep(da, monkeypatch, pk, dp, strict, routing)
        gap = np.abs(per - want) / np.maximum(1., np.abs(want))
        print("%s %s: ll gap %.3e, count gap %.3e, %s" % (name, routing, gap.max(), np.abs(counts - total_x).max(),
                                                          {k: st[k] for k in ("pairs_onchip", "pairs_streaming", "pairs_narrow")}))
        assert len(counts) == 21 + len(params.pLen) and np.isfinite(per).all() and np.isfinite(counts).all(), (name, routing)
        assert (gap <= X.ESTEP_LL_REL[kind]).all(), (name, routing, gap.max())
        assert (np.abs(counts - total_x) <= X.ESTEP_COUNT_ABS[kind]).all(), (name, routing, np.abs(counts - total_x).max())
        assert abs(ll - want.sum()) <= X.ESTEP_LL_REL[kind] * np.maximum(1., np.abs(want)).sum(), (name, routing)
        census[routing] = st
    if without:                       # a database of its own: the reference's counts are NaN where there is no path
        per = _estep(da, monkeypatch, _pack(without), dp, strict, None)[2]
        assert (per == float("-inf")).all(), (name, per)
    return census, len(with_path)


@pytest.mark.parametrize("index", range(len(X.TINY_P) * 2))
def test_estep_against_every_path(da, monkeypatch, tmp_path, index):
    """One tiny model (a duplication width P of 0..9, strict or loose guides, probabilities up to 0.5, 20 pairs of at most 5 x 6
    bases): per-pair log-likelihoods and the database's 21 + P counts equal the sum over every path, under every routing; the
    tiny database runs on-chip (P <= 8; wider models stream), and DNAS_FB_STREAMING streams it."""
    model = X.tiny_models()[index]
    census, n = _check_estep(da, monkeypatch, tmp_path, model, "enumerate", "tiny")
    P = len(model[1].pLen)
    for routing in (None, "DNAS_FB_NO_NARROW"):
        st = census[routing]
        assert st["pairs_onchip"] + st["pairs_streaming"] == n
        assert st["pairs_onchip"] == (n if P <= 8 else 0), (routing, st)
    assert census["DNAS_FB_NO_NARROW"]["pairs_narrow"] == 0
    assert census["DNAS_FB_STREAMING"]["pairs_onchip"] == 0 and census["DNAS_FB_STREAMING"]["pairs_streaming"] == n


@pytest.mark.parametrize("index", range(3))
def test_estep_against_exact_forward_backward(da, monkeypatch, tmp_path, index):
    """Pairs of 20 to 80 bases at realistic parameters (a 24-base deletion block, long runs of duplications) against the exact
    forward-backward pass, under every routing."""
    model = X.medium_models()[index]
    census, n = _check_estep(da, monkeypatch, tmp_path, model, "fwdback", "medium")
    assert census["DNAS_FB_STREAMING"]["pairs_onchip"] == 0 and census["DNAS_FB_STREAMING"]["pairs_streaming"] == n
    if len(model[1].pLen) <= 8:
        assert census[None]["pairs_onchip"] >= 1, census[None]


# ------------------------------------------------------------------------------------------------------------- Viterbi
def _decoder(da, m, dp, options):
    """The decoder under a forced tier, or None where the machine does not admit that tier (it says so by name)."""
    try:
        return da.ViterbiDecoder(m, dp, options=options)
    except da.DnasError as e:
        if options and "was asked for" in str(e):
            return None
        raise


def _check_read(case, r, got, want):
    s, ll, st = got
    ll_x, lat_x, strings = want
    assert X.ll_close(float(ll), ll_x), (case, r, ll, ll_x)
    assert st == (NO_PATH if ll_x == float("-inf") else 0), (case, r, st)
    if strings is not None:
        assert s in strings, (case, r, s, sorted(strings))


VITERBI_CASES = X.viterbi_cases() + [X.no_path_case()]


@pytest.mark.parametrize("options", [None, "tier=B", "tier=C,cluster=2"])
def test_viterbi_against_bellman_ford(da, tmp_path, options):
    """Random machines of 3 to 40 states at every duplication width 0..8, local and global, reads of 0 to 30 bases, and a global
    case without a path: under the default tier, tier B and a cluster of two (where the machine admits one), the batch and every
    read on its own give the exact optimum, the status, a string readable along tight paths, and -- read by read -- every lane
    of every lattice cell."""
    ran = []
    for case in VITERBI_CASES:
        name, text, ptext, reads = case
        m = da.Machine.fromJSON(text)
        dec = _decoder(da, m, _library_params(da, tmp_path, name, ptext), options)
        if dec is None:
            continue
        ran.append(name)
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
        dec.close()
    print(options, "ran on", len(ran), "of", len(VITERBI_CASES), "machines")
    if options == "tier=C,cluster=2":
        assert len(ran) >= len(VITERBI_CASES) // 4, ran       # (machines of a few states do not split over two work-groups)
    else:
        assert len(ran) == len(VITERBI_CASES), ran


def _revcomp(r):
    return r[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_both_strands_against_bellman_ford(da, tmp_path):
    """strands="both": the winner's log-likelihood is the larger of the two exact optima and its string is tight for that strand;
    the strand is the reverse one only where its optimum is strictly larger, and a read that is its own reverse complement (an
    exact tie) goes forward."""
    from oracle.oracle import Machine, MutatorParams
    name, text, ptext, reads = next(c for c in VITERBI_CASES if c[0] == "D4-N17-local")
    reads = [r for r in reads if r] + ["ACGT", "AATT", "GGATCC"]
    g = X.ViterbiGraph(Machine.from_json(text), MutatorParams.from_json(ptext))
    dec = da.ViterbiDecoder(da.Machine.fromJSON(text), _library_params(da, tmp_path, name, ptext))
    out, ll, st, strand = dec.decode(reads, strands="both")
    dec.close()
    decided = 0
    for i, r in enumerate(reads):
        fwd, rev = X.exact_viterbi(g, None, r), X.exact_viterbi(g, None, _revcomp(r))
        assert X.ll_close(float(ll[i]), max(fwd[0], rev[0])), (r, ll[i], fwd[0], rev[0])
        if r == _revcomp(r):
            assert strand[i] == 0, r
        if abs(fwd[0] - rev[0]) > X.TIGHT:
            decided += 1
            assert strand[i] == (1 if rev[0] > fwd[0] else 0), (r, strand[i], fwd[0], rev[0])
        strings = (rev if strand[i] else fwd)[2]
        if strings is not None:
            assert out[i] in strings, (r, out[i], strand[i])
    assert decided >= 3, (decided, list(strand))
