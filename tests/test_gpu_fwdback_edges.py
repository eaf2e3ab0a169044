"""The forward-backward E-step at the thresholds of its routing: dnas_fb_estep sends every alignment pair to one of nine
kernels by the widest row of its envelope (<= 16, <= 32, wider), the half-width conditions hi(ip) - lo(ip + W) < W (W = 8, 16),
the input length against the LDS an on-chip launch may take, and the number of duplication lengths (<= 6, <= 8, more).  The pairs
of tests/fb_edge_pairs.py sit on both sides of each of these (tests/test_fb_census_cpu.py proves that on the CPU), fill the
waves of the on-chip kernels to one pair short of, exactly, and one pair past a wave, go round their persistent loop twice,
stream in more than one batch, and reduce over more than one block.

Every comparison is the contract of tests/test_gpu_fwdback.py: per-pair log-likelihoods equal to the oracle's as uint64 bits,
the 21 + P counts within 1e-9 relative, the total within 1e-12 relative.  Every database runs under the default routing, without
the half-width kernels (DNAS_FB_NO_NARROW) and with everything streamed (DNAS_FB_STREAMING), and in each the
(pairs_onchip, pairs_narrow, pairs_streaming) of the handle's statistics EQUAL what tests/fb_census.py predicts from the
definition of the envelope: that pins fwdback_census_kernel.  The statistics do not tell the 8-lane kernel from the 16-lane one
of the half-width pairs (nor the two full-width ones), so every database is of one kind, or a stated mixture."""
import numpy as np
import pytest

import fb_census as C
import fb_edge_pairs as E

pytestmark = pytest.mark.gpu

WIDTH_CASES = [(name, P, strict, width) for name, P, strict in E.WIDTH_SETTINGS for width in E.WIDTHS
               if any(E.width_k(P, strict, where, width) is not None for where in E.PLACES)]
HALF_CASES = E.half_cases()
ENV = ("DNAS_FB_NO_NARROW", "DNAS_FB_STREAMING")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _set_mode(monkeypatch, mode):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if mode:
        monkeypatch.setenv(mode, "1")


def _triple(st):
    return (st["pairs_onchip"], st["pairs_narrow"], st["pairs_streaming"])


def _against_oracle(got, want, what):
    (counts, ll, per), (oc, oll, oper) = got, want
    assert np.isfinite(oper).all() and np.isfinite(oc).all(), what             # (no path: the reference's counts are NaN)
    assert np.array_equal(_bits(per), _bits(oper)), what
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-300), what
    assert ll == pytest.approx(oll, rel=1e-12), what


def _describe(pairs, P, strict):
    """(kind, width, max(hi - lo(ip + 8)), max(hi - lo(ip + 16))) of the pairs, each once."""
    seen = []
    for pair in pairs[:64]:
        kind, chip, c = C.route(pair, P, strict)
        d = (kind if chip else "s%d" % kind, c["width"], c["margin8"], c["margin16"])
        if d not in seen:
            seen.append(d)
    return seen


def run_database(da, O, monkeypatch, pairs, P, what, strict=False, modes=C.MODES, device=0, predicted=None, want=None, twice=False):
    """One database through the E-step in each mode: the oracle's numbers, the predicted statistics; twice: a second E-step on
    the same handle gives the same bits."""
    want = want or O.expected_counts(O.MutatorParams.from_cli(length=2 * P), pairs, strict=strict)
    predicted = predicted or C.predict_modes(pairs, P, strict)
    params = da.MutatorParams.fromFlags(length=2 * P)
    assert params.c.n_len == P
    pk = O.pack_pairs(pairs)
    for mode in modes:
        _set_mode(monkeypatch, mode)
        fb = da.ForwardBackward(pk, device=device)
        got = fb.expectedCounts(params, strict=strict)
        st = fb.stats()
        print("%s | %d pairs P=%d%s %s | (kind, width, margin8, margin16) %s | stats %s" %
              (what, len(pairs), P, " strict" if strict else "", mode or "default", _describe(pairs, P, strict), _triple(st)))
        assert len(got[0]) == 21 + P
        assert _triple(st) == predicted[mode], (what, mode, st)
        _against_oracle(got, want, (what, mode))
        if twice:
            again = fb.expectedCounts(params, strict=strict)
            assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(_bits(again[2]), _bits(got[2])), (what, mode)
            assert np.array_equal(_bits(again[1]), _bits(got[1])) and _triple(fb.stats()) == _triple(st), (what, mode)
        fb.close()
    _set_mode(monkeypatch, None)


# ---- (a) the widest row at 16 | 17 and 32 | 33
@pytest.mark.parametrize("name,P,strict,width", WIDTH_CASES, ids=["%s-w%d" % (c[0], c[3]) for c in WIDTH_CASES])
def test_row_width_thresholds(da, oracle_mod, monkeypatch, name, P, strict, width):
    """k inserted bases after the first match, in the middle and after the last base make the widest row 16, 17, 32 or 33 cells:
    the 8-lane, the 16-lane (twice) and the streaming kernel; without the half-width kernels the 16-lane, the 32-lane (twice)
    and the streaming kernel.  Databases of 1, PPG - 1, PPG and PPG + 1 pairs for the pairs per wave of both: full waves, a wave
    with one dead slot, and a wave with one live slot whose dead slots look at pair 0."""
    kind = {16: 0, 17: 2, 32: 2, 33: 4}[width]
    sizes = {1, 2, 3}
    if kind < 4:
        for ppg in (C.PPG[kind], C.PPG[kind | 1]):
            sizes |= {ppg - 1, ppg, ppg + 1}
    for where in E.PLACES:
        k = E.width_k(P, strict, where, width)
        if k is None:
            continue
        db = E.width_database((name, where, width), P, where, k, max(sizes))
        assert all(C.route(p, P, strict)[0] == kind and C.census(p, 0 if strict else P)["width"] == width for p in db)
        for size in sorted(sizes - {0}):
            run_database(da, oracle_mod, monkeypatch, db[:size], P, "a/%s/%s/w%d/k%d" % (name, where, width, k), strict=strict)


# ---- (b) the half-width conditions at equality
@pytest.mark.parametrize("case", HALF_CASES, ids=[c["id"] for c in HALF_CASES])
def test_half_width_thresholds(da, oracle_mod, monkeypatch, case):
    """A block of d deleted input bases (behind `ins` inserted ones) one base short of where hi(ip) - lo(ip + W) reaches W, and
    at it: the half-width kernel and the full-width one."""
    P, strict, W = case["P"], case["strict"], case["W"]
    db = E.half_database(case)
    for pair in db:
        m = C.census(pair, 0 if strict else P)["margin%d" % W]
        assert (m >= W) == bool(case["side"]) and (not case["exact"] or m == W - 1 + case["side"]), (case, m)
    run_database(da, oracle_mod, monkeypatch, db, P, "b/" + case["id"], strict=strict)


# ---- (c) the LDS limit
@pytest.mark.parametrize("kind", range(4))
def test_lds_limit(da, oracle_mod, monkeypatch, kind):
    """inLen = longest[kind] - 63 and longest[kind] (the on-chip kernel, its dynamic LDS exactly at the limit, LO[] / HI[] used up
    to the last row) and longest[kind] + 1 (the streaming kernel, whatever the pair's kind)."""
    for n, db in E.lds_databases(kind):
        assert len(db[0][0]) == n and C.route(db[0], E.KIND_P)[:2] == (kind, n <= C.LONGEST[kind])
        assert C.lds_bytes(kind, C.LONGEST[kind]) <= C.LDS_LIMIT < C.lds_bytes(kind, C.LONGEST[kind] + 64)
        run_database(da, oracle_mod, monkeypatch, db, E.KIND_P, "c/kind%d/inLen%d" % (kind, n))


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    db = E.mixed_database()
    return db, oracle_mod.expected_counts(oracle_mod.MutatorParams.from_cli(length=2 * E.KIND_P), db), C.predict_modes(db, E.KIND_P)


def test_lds_limit_mixed_lists(da, oracle_mod, monkeypatch, mixed):
    """All four on-chip kernels at their LDS limit in one E-step, beside 8-base pairs; in every list the longest input and the
    most wavefront steps (the scratch of a wave) come from different pairs."""
    db, want, predicted = mixed
    lists = C.lists(db, E.KIND_P)
    for q in range(4):
        ins = [len(db[i][0]) for i in lists[q]]
        steps = [C.census(db[i], E.KIND_P)["steps"] for i in lists[q]]
        assert max(ins) == C.LONGEST[q] and ins.index(max(ins)) != steps.index(max(steps))
    run_database(da, oracle_mod, monkeypatch, db, E.KIND_P, "c/mixed", predicted=predicted, want=want)


# ---- (g) ... and dealt over three handles: every shard has its own lists and its own longest input
def test_lds_limit_mixed_lists_on_three_fake_devices(da, oracle_mod, monkeypatch, mixed):
    db, want, predicted = mixed
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    run_database(da, oracle_mod, monkeypatch, db, E.KIND_P, "g/mixed/3 devices", device=-1, predicted=predicted, want=want)


# ---- (d) the persistent loop of the on-chip kernels
@pytest.mark.parametrize("kind,P", [(0, 3), (1, 3), (2, 3), (3, 3), (3, 8)])
def test_persistent_loop_goes_round_twice(da, oracle_mod, monkeypatch, kind, P):
    """One pair more than compute units x waves per compute unit x pairs per wave (the count the handle launches for): wave 0
    goes round its loop a second time with one live slot.  The counts of a pair are fp64 atomic adds into LDS from all its
    lanes: the second E-step on the handle must give the same bits with every wave of the chip running."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count        # hipDeviceAttributeMultiprocessorCount, as dnas_fb_create reads it
    db = E.persistent_database(kind, cus, P)
    assert len(db) == cus * C.WAVES_PER_CU * C.PPG[kind] + 1
    predicted = C.predict_modes(db, P)
    assert predicted[None] == (len(db), len(db) if kind in (0, 2) else 0, 0)
    run_database(da, oracle_mod, monkeypatch, db, P, "d/kind%d" % kind, predicted=predicted, twice=True)


# ---- (e) streaming beyond one batch, the reduction beyond one block
@pytest.fixture(scope="module")
def tiny():
    db = E.tiny_pairs(65537)
    cs = [(C.census(p, 6), len(p[0])) for p in db]
    decisions = {mode: [C.decide(c, n, 6, mode == ENV[0], mode == ENV[1]) for c, n in cs] for mode in C.MODES}
    return db, decisions


@pytest.mark.parametrize("first,count,modes", [(1000, 256, C.MODES[:1]), (2000, 257, C.MODES), (256, 65281, C.MODES[:1]), (1, 65536, C.MODES[:1]),
                                               (0, 65537, C.MODES)], ids=["256", "257", "65281", "65536", "65537"])
def test_reduction_and_streaming_batches(da, oracle_mod, monkeypatch, tiny, first, count, modes):
    """Pairs of 1 .. 4 bases, neighbours never alike.  256 | 257 pairs: one | two blocks of fwdback_reduce_kernel; 65 281: the
    first size with 256 blocks; 65 536 | 65 537: its strided loop once | twice, and streamed one | two launches of
    fwdback_estep_kernel, the second from pair 65 536 on."""
    db, decisions = tiny
    predicted = {mode: C.triple(decisions[mode][first:first + count]) for mode in C.MODES}
    assert predicted[None] == (count, count, 0) and predicted[ENV[1]] == (0, 0, count)
    run_database(da, oracle_mod, monkeypatch, db[first:first + count], 6, "e/%d" % count, modes=modes, predicted=predicted)


# ---- (f) the length limit, and pairs without bases
def test_thirty_thousand_bases(da, oracle_mod, monkeypatch):
    db = [E.long_pair(30000, 30000)] + E.short_kind_pairs("long", 0, 3, 6)
    assert C.predict(db, 6) == (3, 3, 1)
    run_database(da, oracle_mod, monkeypatch, db, 6, "f/30000")


@pytest.mark.parametrize("n_in,n_out", [(30001, 30000), (30000, 30001)])
def test_thirty_thousand_and_one_bases_are_refused(da, oracle_mod, n_in, n_out):
    O = oracle_mod
    good = E.short_kind_pairs("long", 0, 3, 6)
    bad = good[:2] + [E.long_pair(n_in, n_out)] + good[2:]
    fb = da.ForwardBackward(None)
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED.*pair 2: sequences longer than 30000"):
        fb.load(O.pack_pairs(bad))
    fb.load(O.pack_pairs(good))                                   # the handle takes a good database afterwards
    got = fb.expectedCounts(da.MutatorParams.fromFlags())
    fb.close()
    _against_oracle(got, O.expected_counts(O.MutatorParams.from_cli(), good), "after a refused database")


@pytest.mark.parametrize("which", ["all deleted", "no bases"])
@pytest.mark.parametrize("P,strict", [(6, False), (6, True), (8, False)])
def test_pairs_without_output(da, oracle_mod, monkeypatch, which, P, strict):
    """A pair whose input is all deleted (outLen = 0) and one without any base (one cell), alone and as pair 0 of a list with dead
    slots, whose lanes look at pair 0's offsets.  The oracle gives both finite numbers (test_fb_census_cpu.py), so both are kept."""
    pair = E.all_deleted_pair() if which == "all deleted" else E.empty_pair()
    run_database(da, oracle_mod, monkeypatch, [pair], P, "f/%s alone" % which, strict=strict)
    db = [pair] + E.tiny_pairs(2, "degenerate")
    assert C.lists(db, P, strict)[0] == [0, 1, 2]
    run_database(da, oracle_mod, monkeypatch, db, P, "f/%s as pair 0 of three" % which, strict=strict)
