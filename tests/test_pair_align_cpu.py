"""The pair-HMM Viterbi aligner on the host (dnas_align_pairs_host, csrc/host/pairalign.cpp) and its helpers -- no GPU.

Three statements of one model are held against each other: the generative definition (exact_models._moves, the maximum over
its move graph in 160-bit mpmath), a Python fp64 transcription of the recurrence as include/dnastore_amd.h states it (written
here, scores from dnas_mutator_scores so that log is evaluated once), and the library's host code, which the kernels are held
to bit for bit in test_gpu_pair_align.py."""
import ctypes
import math
import os
import random
import sys
import types

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

NEG = float("-inf")
BASES = "ACGT"


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


# ---------------------------------------------------------------------------------------------------------------- cases
def make_params(da, pLen, pDelOpen=.02, pDelExtend=.2, pTanDup=.03, pTransition=.03, pTransversion=.02, local=True):
    c = da.lib.MutatorParamsC()
    c.p_del_open, c.p_del_extend, c.p_tan_dup, c.p_transition, c.p_transversion = pDelOpen, pDelExtend, pTanDup, pTransition, pTransversion
    c.n_len, c.local = len(pLen), int(local)
    for k, x in enumerate(pLen):
        c.p_len[k] = x
    p = da.MutatorParams(c)
    p.plain = types.SimpleNamespace(pDelOpen=pDelOpen, pDelExtend=pDelExtend, pTanDup=pTanDup, pTransition=pTransition,
                                    pTransversion=pTransversion, pLen=list(pLen), local=local)
    return p


def edited(rng, src, n_edits):
    """A read: the original after up to n_edits substitutions, deletions of 1-2 bases and tandem copies of 1-3 bases."""
    s = list(src)
    for _ in range(n_edits):
        kind = rng.choice("sdt")
        if kind == "s" and s:
            at = rng.randrange(len(s))
            s[at] = rng.choice([b for b in BASES if b != s[at]])
        elif kind == "d" and s:
            at = rng.randrange(len(s))
            del s[at:at + rng.randint(1, 2)]
        elif kind == "t" and s:
            at = rng.randrange(len(s))
            k = rng.randint(1, min(3, at + 1))
            s[at + 1:at + 1] = s[at + 1 - k:at + 1]
    return "".join(s)


SMALL_MODELS = (("P0", []), ("P1", [1.]), ("P2", [.7, .3]), ("P4", [.4, .3, .2, .1]), ("P4-zero", [.5, 0., .3, .2]))
SMALL_PER_MODEL = 64


def small_cases(da):
    """320 pairs, 64 per model: I, O in 0..9, P in {0, 1, 2, 4}, a pLen with a zero entry, probabilities up to 0.4 (and
    pTransversion = 0 in the last model: substitution scores of -inf); reads are the original after 0-3 edits, or unrelated."""
    out = []
    for name, pLen in SMALL_MODELS:
        rng = random.Random("pair-align/" + name)
        params = make_params(da, pLen, pDelOpen=rng.uniform(.01, .3), pDelExtend=rng.uniform(.05, .5), pTanDup=rng.uniform(.01, .3),
                             pTransition=rng.uniform(.01, .2), pTransversion=0. if name == "P4-zero" else rng.uniform(.01, .2))
        pairs = [("", ""), ("", "ACG"), ("ACG", ""), ("A", "A")]
        while len(pairs) < SMALL_PER_MODEL:
            a = "".join(rng.choice(BASES) for _ in range(rng.randint(0, 9)))
            if rng.random() < .2:
                b = "".join(rng.choice(BASES) for _ in range(rng.randint(0, 9)))
            else:
                b = edited(rng, a, rng.randint(0, 3))[:9]
            pairs.append((a, b))
        out.append((name, params, pairs))
    return out


def long_cases(da):
    """20 pairs of 40 to 120 bases from synth.synthetic_alignment, P = 6 (the CLI's default model with more noise)."""
    from synth import synthetic_alignment
    rng = random.Random("pair-align/long")
    params = da.MutatorParams.fromFlags(sub=.03, dup=.02, del_open=.02, del_ext=.2)
    pairs = []
    for _ in range(20):
        r = synthetic_alignment(rng, rng.randint(40, 120), sub=.03, dele=.02, dup=.02)
        pairs.append((r[0][1].replace("-", ""), r[1][1].replace("-", "")))
    return [("long-P6", params, pairs)]


# ------------------------------------------------------------------------------------------ the recurrence, transcribed
def viterbi_py(scores, P, a, b, band=-1):
    """The normative recurrence in Python floats -> (score, op bytes).  scores: dnas_mutator_scores."""
    delOpen, tanDup, noGap, delExtend, delEnd = (float(x) for x in scores[:5])
    sub = [[float(scores[5 + 4 * x + y]) for y in range(4)] for x in range(4)]
    ln = [float(x) for x in scores[21:21 + P]]
    I, O = len(a), len(b)
    lo, hi = (min(0, O - I) - band, max(0, O - I) + band) if band >= 0 else (-(I + O + 1), I + O + 1)
    inside = lambda ip, op: 0 <= ip <= I and 0 <= op <= O and lo <= op - ip <= hi
    S = [[NEG] * (O + 1) for _ in range(I + 1)]
    D = [[NEG] * (O + 1) for _ in range(I + 1)]
    T = [[None] * (O + 1) for _ in range(I + 1)]
    cS = [[None] * (O + 1) for _ in range(I + 1)]
    cD = [[None] * (O + 1) for _ in range(I + 1)]
    cT = [[None] * (O + 1) for _ in range(I + 1)]
    val = lambda M, ip, op: M[ip][op] if inside(ip, op) else NEG
    for ip in range(I + 1):
        lanes = min(ip, P)
        for op in range(O + 1):
            if not inside(ip, op):
                continue
            best, pick = NEG, None
            if ip > 0:
                for name, c in (("d0", val(S, ip - 1, op) + delOpen), ("d1", val(D, ip - 1, op) + delExtend)):
                    if c > best:
                        best, pick = c, name
            D[ip][op], cD[ip][op] = best, pick
            best, pick = NEG, None
            if ip == 0 and op == 0:
                best = 0.
            else:
                cands = []
                if ip > 0 and op > 0:
                    cands.append(("s0", val(S, ip - 1, op - 1) + noGap + sub[a[ip - 1]][b[op - 1]]))
                    if P > 0:
                        left = T[ip][op - 1][0] if inside(ip, op - 1) and lanes > 0 else NEG
                        cands.append(("s1", left + sub[a[ip - 1]][b[op - 1]]))
                cands.append(("s2", D[ip][op] + delEnd))
                for name, c in cands:
                    if c > best:
                        best, pick = c, name
            S[ip][op], cS[ip][op] = best, pick
            tk, ck = [NEG] * lanes, [None] * lanes
            for k in range(lanes):
                best, pick = NEG, None
                if op > 0 and k + 1 < lanes:
                    left = T[ip][op - 1][k + 1] if inside(ip, op - 1) else NEG
                    c = left + sub[a[ip - 2 - k]][b[op - 1]]
                    if c > best:
                        best, pick = c, "t0"
                c = S[ip][op] + tanDup + ln[k]
                if c > best:
                    best, pick = c, "t1"
                tk[k], ck[k] = best, pick
            T[ip][op], cT[ip][op] = tk, ck
    score = S[I][O]
    if score == NEG:
        return score, []
    ops, ip, op, lane = [], I, O, "S"
    while (ip, op, lane) != (0, 0, "S"):
        if lane == "S":
            c = cS[ip][op]
            if c == "s0":
                ops.append(0); ip -= 1; op -= 1
            elif c == "s1":
                ops.append(2); op -= 1; lane = 0
            else:
                lane = "D"
        elif lane == "D":
            if cD[ip][op] == "d0":
                ops.append(1 | 1 << 2); ip -= 1; lane = "S"
            else:
                ops.append(1); ip -= 1
        else:
            if cT[ip][op][lane] == "t0":
                ops.append(2); op -= 1; lane += 1
            else:
                ops[-1] |= (lane + 1) << 2      # the column written last is the event's first
                lane = "S"
    return score, ops[::-1]


def exact_viterbi_pair(params, a, b):
    """log of the maximum path weight over the move graph of exact_models._moves, in mpmath -> float (or -inf)."""
    import exact_models as X
    m = X.PairModel(params)
    order = [(ip, op, ln) for ip in range(len(a) + 1) for op in range(len(b) + 1) for ln in ["D", "S"] + list(range(min(ip, m.P)))]
    best = {n: X.mpf(0) for n in order}
    best[(0, 0, "S")] = X.mpf(1)
    for n in order:
        if best[n] != 0:
            for nxt, wt, _ in X._moves(m, n, a, b):
                if best[n] * wt > best[nxt]:
                    best[nxt] = best[n] * wt
    z = best[(len(a), len(b), "S")]
    return NEG if z == 0 else float(X.mp.log(z))


def tok(s):
    return [BASES.index(c) for c in s]


def excursion(ops, I, O):
    """How far the path leaves the diagonals min(0, O-I) .. max(0, O-I)."""
    lo, hi, ip, op, e = min(0, O - I), max(0, O - I), 0, 0, 0
    for o in ops:
        kind = int(o) & 3
        ip += kind != 2
        op += kind != 1
        e = max(e, lo - (op - ip), (op - ip) - hi)
    return e


@pytest.fixture(scope="module")
def cases(da):
    """Every model with its pairs and the host's full-matrix result, computed once: [(name, params, pairs, PairAlignments)]."""
    out = []
    for name, params, pairs in small_cases(da) + long_cases(da):
        res = da.alignPairs(params, [a for a, _ in pairs], [b for _, b in pairs], band=-1, host=True)
        out.append((name, params, pairs, res))
    return out


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_host_against_the_exact_model(da, cases):
    import exact_models as X
    n, worst = 0, 0.
    for name, params, pairs, res in cases:
        if name.startswith("long"):
            continue
        for i, (a, b) in enumerate(pairs):
            want = exact_viterbi_pair(params.plain, tok(a), tok(b))
            got = float(res.score[i])
            assert (want == NEG) == (res.status[i] == da.lib.ALIGN_NO_PATH) == (got == NEG), (name, a, b, got, want)
            assert X.ll_close(got, want), (name, a, b, got, want)
            if want != NEG:
                worst = max(worst, abs(got - want) / max(1., abs(want)))
            n += 1
    assert n >= 300
    print("largest relative gap to the exact model: %.3g over %d pairs" % (worst, n))


def test_host_against_the_transcribed_recurrence(da, cases):
    for name, params, pairs, res in cases:
        scores = da.mutatorScores(params)
        P = params.c.n_len
        for i, (a, b) in enumerate(pairs):
            score, ops = viterbi_py(scores, P, tok(a), tok(b))
            assert _bits(score) == _bits(res.score[i]), (name, a, b, score, res.score[i])
            assert ops == [int(o) for o in res.ops[i]], (name, a, b)


BOUNDARY_MODELS = ("P2", "P4")


def boundary_cases(da):
    """P2 and P4 of small_cases under the 14 boundary variants of exact_models (probabilities of exactly 0 and 1, of 1e-300 and
    of 1 - 2^-53): [("<model>/<variant>", params, pairs)], the 64 pairs of the base."""
    import exact_models as X
    out = []
    for name, params, pairs in small_cases(da):
        if name in BOUNDARY_MODELS:
            for v in X.BOUNDARY_NAMES:
                q = X.boundary_params(params.plain, v)
                out.append(("%s/%s" % (name, v), make_params(da, q.pLen, q.pDelOpen, q.pDelExtend, q.pTanDup, q.pTransition,
                                                             q.pTransversion, q.local), pairs))
    return out


def _boundary_ids():
    import exact_models as X
    return ["%s/%s" % (m, v) for m in BOUNDARY_MODELS for v in X.BOUNDARY_NAMES]


@pytest.mark.parametrize("index", range(2 * 14), ids=_boundary_ids())
def test_host_at_boundary_probabilities(da, index):
    """The host aligner under one boundary variant against the exact model (equal -inf, equal ALIGN_NO_PATH, ll_close
    otherwise) and against the transcribed recurrence bit for bit, ops included; between 2 and 48 of the 64 pairs have no path,
    so that both the -inf bookkeeping and the finite arithmetic are reached."""
    import exact_models as X
    name, params, pairs = boundary_cases(da)[index]
    assert name == _boundary_ids()[index] and len(pairs) == SMALL_PER_MODEL
    res = da.alignPairs(params, [a for a, _ in pairs], [b for _, b in pairs], band=-1, host=True)
    scores = da.mutatorScores(params)
    no_path = 0
    for i, (a, b) in enumerate(pairs):
        want = exact_viterbi_pair(params.plain, tok(a), tok(b))
        got = float(res.score[i])
        assert (want == NEG) == (res.status[i] == da.lib.ALIGN_NO_PATH) == (got == NEG), (name, a, b, got, want)
        assert X.ll_close(got, want), (name, a, b, got, want)
        score, ops = viterbi_py(scores, params.c.n_len, tok(a), tok(b))
        assert _bits(score) == _bits(res.score[i]), (name, a, b, score, res.score[i])
        assert ops == [int(o) for o in res.ops[i]], (name, a, b)
        no_path += want == NEG
    assert 2 <= no_path <= 48, (name, no_path)


def test_expand_rows_guides_and_counts(da, cases):
    import exact_models as X
    seen = set()
    for name, params, pairs, res in cases:
        scores = da.mutatorScores(params)
        for i, (a, b) in enumerate(pairs):
            if res.status[i] != da.lib.ALIGN_OK:
                continue
            r1, r2 = res.rows(i)
            assert r1.replace("-", "") == a and r2.replace("-", "") == b and len(r1) == len(r2) == len(res.ops[i])
            _, _, cm_in, cm_out, counts = res._expand(i, True)
            _, _, want_in, want_out = X.guide_columns(r1, r2)
            assert np.array_equal(cm_in, want_in) and np.array_equal(cm_out, want_out)
            used = counts > 0
            total = math.fsum(counts[used] * scores[used])
            assert abs(total - res.score[i]) <= 1e-12 * max(1., abs(res.score[i])), (name, a, b, total, res.score[i])
            assert counts[0] == counts[4] and counts[1] == counts[21:].sum() and counts[2] == sum(x != "-" and y != "-" for x, y in zip(r1, r2))
            seen.add((params.c.n_len == 0, len(b) == 0 and len(a) > 0, len(a) == 0 and len(b) == 0))
    assert {(True, False, False), (False, True, False), (False, False, True)} <= seen      # P = 0, all deleted, (0, 0)
    # ops that are no path of the model are refused
    a, b = np.array([0, 1], np.int8), np.array([0, 1, 1], np.int8)
    for bad in ([0, 0], [0, 0, 2], [0, 0, 2 | 3 << 2], [0, 1, 2 | 1 << 2, 2 | 1 << 2], [0, 0, 2 | 2 << 2]):
        ops = np.array(bad, np.uint8)
        rc = da.lib.lib().dnas_alignment_expand(2, a.ctypes.data, 2, b.ctypes.data, 3, ops.ctypes.data, len(ops), None, None, None, None, None)
        assert rc == -1, bad
    ops = np.array([0, 0, 2 | 1 << 2], np.uint8)
    assert da.lib.lib().dnas_alignment_expand(2, a.ctypes.data, 2, b.ctypes.data, 3, ops.ctypes.data, 3, None, None, None, None, None) == 0


def test_band(da, cases):
    narrowed = 0
    for name, params, pairs, res in cases:
        ins, outs = [a for a, _ in pairs], [b for _, b in pairs]
        e = [excursion(res.ops[i], len(a), len(b)) if res.status[i] == da.lib.ALIGN_OK else 0 for i, (a, b) in enumerate(pairs)]
        for width in sorted(set(e)):
            idx = [i for i in range(len(pairs)) if e[i] == width]
            got = da.alignPairs(params, [ins[i] for i in idx], [outs[i] for i in idx], band=width, host=True)
            for j, i in enumerate(idx):
                assert _bits(got.score[j]) == _bits(res.score[i]) and got.status[j] == res.status[i], (name, pairs[i], width)
                assert np.array_equal(got.ops[j], res.ops[i]), (name, pairs[i], width)
        idx = [i for i in range(len(pairs)) if e[i] > 0]
        if idx:
            got = da.alignPairs(params, [ins[i] for i in idx], [outs[i] for i in idx], band=0, host=True)
            for j, i in enumerate(idx):
                assert got.score[j] <= res.score[i]
                if got.status[j] == da.lib.ALIGN_OK:
                    r1, r2 = got.rows(j)
                    assert r1.replace("-", "") == ins[i] and r2.replace("-", "") == outs[i]
                    assert excursion(got.ops[j], len(ins[i]), len(outs[i])) == 0
                    narrowed += 1
        if name.startswith("long"):
            assert max(e) <= 3, e                 # what synthetic_alignment(sub=.03, dele=.02, dup=.02) was measured to need
            sc = da.mutatorScores(params)         # ... and the banded recurrence itself, transcribed
            for i in (0, 7):
                score, ops = viterbi_py(sc, params.c.n_len, tok(ins[i]), tok(outs[i]), band=2)
                got = da.alignPairs(params, [ins[i]], [outs[i]], band=2, host=True)
                assert _bits(score) == _bits(got.score[0]) and ops == [int(o) for o in got.ops[0]]
    assert narrowed >= 5


def test_stockholm_round_trip(da, cases, tmp_path):
    name, params, pairs, res = cases[3]
    text = res.stockholm()
    assert text.startswith("# STOCKHOLM 1.0\n") and text.count("//\n") == len(res.kept()) and len(res.skipped) >= 2
    path = tmp_path / "pairs.stk"
    path.write_text(text)
    back, want = da.StockholmDB(str(path)).arrays(), res.packed()
    assert back["n"] == want["n"] == len(res.kept())
    for k in ("ins", "in_off", "outs", "out_off", "cm_in", "cm_in_off", "cm_out", "cm_out_off"):
        assert np.array_equal(back[k], want[k]), k
    # equal names: the read's gets a suffix, and the database still reads back the same
    keep = res.kept()
    names = ["strand%d" % i for i in range(len(pairs))]
    same = res.stockholm(names_in=names, names_out=names)
    assert "strand%d/read " % keep[0] in same and same.count("/read ") == len(keep)
    path.write_text(same)
    again = da.StockholmDB(str(path)).arrays()
    assert all(np.array_equal(again[k], want[k]) for k in ("ins", "outs", "cm_in", "cm_out"))
    one = res.stockholm(names_in=["original"])
    assert sum(line.startswith("original ") for line in one.splitlines()) == len(keep)


def test_errors(da):
    L = da.lib.lib()
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.alignPairs(make_params(da, [1. / 14] * 14), ["ACGT"], ["ACT"], host=True)
    params = make_params(da, [.5, .5])
    ins, outs = np.array([0, 1, 2, 3], np.int8), np.array([0, 1, 3], np.int8)
    in_off, out_off = np.array([0, 4], np.int64), np.array([0, 3], np.int64)
    ops, n_ops, score, status = np.zeros(16, np.uint8), np.zeros(1, np.uint32), np.zeros(1), np.zeros(1, np.uint8)

    def call(slot, bases=ins):
        ops_off = np.array([0, slot], np.uint64)
        return L.dnas_align_pairs_host(ctypes.byref(params.c), -1, 1, bases.ctypes.data, in_off.ctypes.data, outs.ctypes.data,
                                       out_off.ctypes.data, ops.ctypes.data, ops_off.ctypes.data, n_ops.ctypes.data,
                                       score.ctypes.data, status.ctypes.data)
    assert call(6) == -1 and "slot" in L.dnas_last_error().decode()        # DNAS_E_INVALID
    assert call(7) == 0 and status[0] == 0 and n_ops[0] == 4
    assert call(7, np.array([0, 1, 2, 4], np.int8)) == -6                   # DNAS_E_BAD_BASE
    empty = da.alignPairs(params, [], [], host=True)
    assert len(empty) == 0 and empty.packed()["n"] == 0 and empty.stockholm() == ""
