"""The constructions of tests/fb_edge_pairs.py hit the routing thresholds of the forward-backward E-step they claim to hit,
proven on the CPU with the restatement of the census in tests/fb_census.py before any GPU call; the oracle gives every pair
of them a finite log-likelihood and finite counts (the reference's counts are NaN where a pair has no path); and the
inequalities that tests/test_gpu_fwdback.py asserts of the routing statistics follow from the restatement."""
import random

import numpy as np
import pytest

import fb_census as C
import fb_edge_pairs as E


def _finite(O, pairs, P, strict=False):
    counts, ll, per = O.expected_counts(O.MutatorParams.from_cli(length=2 * P), pairs, strict=strict)
    return np.isfinite(per).all() and np.isfinite(counts).all() and np.isfinite(ll)


def test_constants_of_the_source():
    assert C.WAVE == 64 and C.LDS_LIMIT == 64 * 1024 and C.WAVES_PER_CU == 12
    assert C.LONGEST == (1920, 3968, 3968, 8064) and C.PPG == (8, 4, 4, 2)
    for q in range(4):
        L = C.LONGEST[q]
        assert L % 64 == 0 and C.lds_bytes(q, L) <= C.LDS_LIMIT < C.lds_bytes(q, L + 64)
        # LO[] and HI[] hold rows 0 .. maxInLen (+ one of padding each) as int16 behind the 56 doubles of counts and scores
        assert C.pair_doubles(L) * 8 >= 56 * 8 + 2 * 2 * (L + 2)
        assert C.lds_bytes(q, L - 63) > C.lds_bytes(q, L - 64)


def test_envelope_against_the_predicate():
    """envelope() (two searches in sorted arrays) against the predicate |cm_out[op] - cm_in[ip]| <= Dm cell by cell."""
    from synth import synthetic_alignment
    rng = random.Random(1)
    pairs = [E.O.alignment_pair(synthetic_alignment(rng, rng.choice([1, 5, 40, 97]), sub=.03, dele=.05, dup=.05)) for _ in range(40)]
    pairs += E.tiny_pairs(50, "env") + [E.all_deleted_pair(), E.empty_pair()]
    for kind in range(4):
        pairs += E.short_kind_pairs("env", kind, 3)
    for case in E.half_cases()[::7]:
        pairs += E.half_database(case, 1)
    for pair in pairs:
        for Dm in (0, 1, 3, 8):
            lo, hi = C.envelope(pair[2], pair[3], Dm)
            lo2, hi2 = C.envelope_by_definition(pair[2], pair[3], Dm)
            assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)
            c = C.census(pair, Dm)
            assert c["cells"] == sum(1 for a in pair[2] for b in pair[3] if abs(int(a) - int(b)) <= Dm)
            for W in (8, 16):
                bad = [ip for ip in range(len(lo) - W) if hi[ip] - lo[ip + W] >= W]
                assert c["fits%d" % W] == (not bad)


# ---- (a)
def test_row_widths_land_on_16_17_32_33(oracle_mod):
    reached = set()
    for name, P, strict in E.WIDTH_SETTINGS:
        for where in E.PLACES:
            for width, kind in zip(E.WIDTHS, (0, 2, 2, 4)):
                k = E.width_k(P, strict, where, width)
                if k is None:
                    continue
                reached.add((name, where, width))
                assert k == (width - 1 if strict else width - 2 * P - 1)
                db = E.width_database((name, where, width), P, where, k, 9)
                routes = [C.route(p, P, strict) for p in db]
                assert all(r[2]["width"] == width and r[0] == kind for r in routes), (name, where, width)
                assert all(r[1] == (kind < 4) for r in routes)
                assert C.predict(db, P, strict, no_narrow=True) == ((9, 0, 0) if kind < 4 else (0, 0, 9))
                assert all(112 < len(p[0]) < 128 for p in db) and len(set(p[0].tobytes() for p in db)) == 9
                assert _finite(oracle_mod, db, P, strict), (name, where, width)
    # with P = 8 and loose guides a row holds at least the cells of 17 match counts: width 16 does not exist there
    assert reached == set((n, w, x) for n, _, _ in E.WIDTH_SETTINGS for w in E.PLACES for x in E.WIDTHS) - set(("P8", w, 16) for w in E.PLACES)


# ---- (b)
def test_half_width_cases_sit_on_both_sides_of_equality(oracle_mod):
    cases = E.half_cases()
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    # every setting flips at the start and in the middle; a block that ends at ip = I leaves rows of at most P + 1 match counts
    # in front of it, which without inserted bases is less than W cells: no flip there
    for name, P, strict, ins, W in E.HALF_SETTINGS:
        places = [c["where"] for c in cases if c["id"].startswith(name + "-")]
        assert places.count("first") == 2 and places.count("middle") == 2, name
        assert (places.count("last") == 2) == (ins > 0), name
    for case in cases:
        W, P, strict = case["W"], case["P"], case["strict"]
        db = E.half_database(case)
        for pair in db:
            kind, chip, c = C.route(pair, P, strict)
            m = c["margin%d" % W]
            assert (m >= W) == bool(case["side"]) and c["fits%d" % W] == (not case["side"]), case
            # W - 1 on one side and W on the other where that can be had: without inserted bases (the difference grows by one per
            # deleted base) and in the strict=W cases (ins = W - 1 | W).  Behind inserted bases it cannot: they come into the
            # reach of row ip + W all at once, and the difference jumps from below W - 1 to beyond W (strict+10: -1 | 10); those
            # cases are held to < W | >= W, which is the condition the routing tests.
            if case["exact"]:
                assert m == W - 1 + case["side"], (case, m)
            assert chip and kind == (1 if c["width"] <= 16 else 3) - (c["fits8"] if c["width"] <= 16 else c["fits16"])
        assert _finite(oracle_mod, db, P, strict), case
    # the flips of the issue's table, in the middle of a pair
    flips = {name: E.half_flip(P, strict, ins, W, "middle") for name, P, strict, ins, W in E.HALF_SETTINGS}
    assert flips == {"P6": 4, "P7": 2, "P8": 16, "strict+10": 8, "strict+20/8": 8, "strict+20/16": 16, "P3+14/8": 2, "P3+14/16": 12}
    # ... and the kinds on their two sides
    sides = {c["id"]: C.route(E.half_database(c)[0], c["P"], c["strict"])[0] for c in cases if c["where"] == "middle"}
    assert (sides["P6-middle-d3"], sides["P6-middle-d4"]) == (0, 1) and (sides["P7-middle-d1"], sides["P7-middle-d2"]) == (0, 1)
    assert (sides["P8-middle-d15"], sides["P8-middle-d16"]) == (2, 3)
    assert (sides["strict+10-middle-d7"], sides["strict+10-middle-d8"]) == (0, 1)
    assert (sides["strict+20/8-middle-d7"], sides["strict+20/8-middle-d8"]) == (2, 2)
    assert (sides["strict+20/16-middle-d15"], sides["strict+20/16-middle-d16"]) == (2, 3)
    assert (sides["P3+14/8-middle-d1"], sides["P3+14/8-middle-d2"]) == (2, 2)
    assert (sides["P3+14/16-middle-d11"], sides["P3+14/16-middle-d12"]) == (2, 3)
    assert (sides["strict=8-middle-ins7"], sides["strict=8-middle-ins8"]) == (0, 1)
    assert (sides["strict=16-middle-ins15"], sides["strict=16-middle-ins16"]) == (1, 3)      # width 16 | 17 and the half-width at once


# ---- (c)
@pytest.mark.parametrize("kind", range(4))
def test_lds_limit_databases(oracle_mod, kind):
    L = C.LONGEST[kind]
    narrow = kind in (0, 2)
    dbs = E.lds_databases(kind)
    assert [n for n, _ in dbs] == [L - 63, L, L + 1]
    for n, db in dbs:
        assert len(db[0][0]) == n and all(C.route(p, E.KIND_P)[0] == kind for p in db)
        assert C.lists(db, E.KIND_P)[kind] == ([0, 1, 2] if n <= L else [1, 2])                 # past the limit: streams, whatever its kind
        chip = 3 if n <= L else 2
        wide = 3 if n <= C.LONGEST[kind | 1] else 2             # without the half-width kernels: the limit of the full-width one
        assert C.predict_modes(db, E.KIND_P) == {None: (chip, chip if narrow else 0, 3 - chip), "DNAS_FB_NO_NARROW": (wide, 0, 3 - wide),
                                                  "DNAS_FB_STREAMING": (0, 0, 3)}
        assert _finite(oracle_mod, db, E.KIND_P)


def test_mixed_database_takes_longest_input_and_most_steps_from_different_pairs(oracle_mod):
    db = E.mixed_database()
    lists = C.lists(db, E.KIND_P)
    assert not lists[4]
    for q in range(4):
        ins = [len(db[i][0]) for i in lists[q]]
        steps = [C.census(db[i], E.KIND_P)["steps"] for i in lists[q]]
        assert max(ins) == C.LONGEST[q] and min(ins) <= 29 and len(ins) >= 3
        assert ins.index(max(ins)) != steps.index(max(steps)) and steps.count(max(steps)) == 1
    assert [len(x) % C.PPG[q] for q, x in enumerate(lists[:4])] != [0, 0, 0, 0]                  # dead slots
    assert _finite(oracle_mod, db, E.KIND_P)


# ---- (d)
@pytest.mark.parametrize("kind,P", [(0, 3), (1, 3), (2, 3), (3, 3), (3, 8)])
def test_persistent_loop_databases(oracle_mod, kind, P):
    """(two compute units here; a GPU run takes the device's number)"""
    db = E.persistent_database(kind, 2, P)
    assert len(db) == 2 * C.WAVES_PER_CU * C.PPG[kind] + 1
    assert [256 * C.WAVES_PER_CU * ppg + 1 for ppg in C.PPG] == [24577, 12289, 12289, 6145]      # on 256 compute units
    assert all(C.route(p, P)[:2] == (kind, True) for p in db)
    assert all(16 <= len(p[0]) <= 29 for p in db)
    assert len(set((p[0].tobytes(), p[1].tobytes()) for p in db)) > .9 * len(db)
    assert all((db[i][0].tobytes(), db[i][1].tobytes()) != (db[i + 1][0].tobytes(), db[i + 1][1].tobytes()) for i in range(len(db) - 1))
    assert _finite(oracle_mod, db, P)


# ---- (e)
def test_tiny_pairs(oracle_mod):
    db = E.tiny_pairs(65537)
    assert len(db) == 65537 and all(1 <= len(p[0]) <= 4 and len(p[1]) >= 1 for p in db)
    key = lambda p: (p[0].tobytes(), p[1].tobytes(), p[2].tobytes(), p[3].tobytes())
    assert all(key(db[i]) != key(db[i + 1]) for i in range(len(db) - 1))
    assert C.predict_modes(db[:3000], 6)[None] == (3000, 3000, 0)
    per = oracle_mod.expected_counts(oracle_mod.MutatorParams.from_cli(), db)[2]
    assert np.isfinite(per).all()
    assert (per[:-1] != per[1:]).mean() > .9                  # a pair read at its neighbour's index shows in its log-likelihood
    assert _finite(oracle_mod, db, 6)


# ---- (f)
def test_longest_and_degenerate_pairs(oracle_mod):
    big = E.long_pair(30000, 30000)
    assert len(big[0]) == len(big[1]) == C.MAX_LEN
    assert C.route(big, 6)[:2] == (0, False)                  # a diagonal, but no on-chip kernel holds 30 001 rows of bounds
    assert _finite(oracle_mod, [big], 6)
    assert (len(E.long_pair(30001, 30000)[0]), len(E.long_pair(30001, 30000)[1])) == (30001, 30000)
    assert (len(E.long_pair(30000, 30001)[0]), len(E.long_pair(30000, 30001)[1])) == (30000, 30001)
    # the pairs without output bases: finite in the oracle, so both are worth a GPU run
    gone, empty = E.all_deleted_pair(), E.empty_pair()
    assert (len(gone[0]), len(gone[1]), len(empty[0]), len(empty[1])) == (5, 0, 0, 0)
    assert C.census(gone, 6)["width"] == 1 and C.census(empty, 6) == dict(width=1, cells=1, steps=1, fits8=True, fits16=True, margin8=None, margin16=None)
    for P, strict in ((6, False), (6, True), (3, False), (8, False)):
        assert _finite(oracle_mod, [gone], P, strict) and _finite(oracle_mod, [empty], P, strict)
        assert C.route(gone, P, strict)[:2] == (0, True) and C.route(empty, P, strict)[:2] == (0, True)
    counts, ll, per = oracle_mod.expected_counts(oracle_mod.MutatorParams.from_cli(), [empty])
    assert ll == 0 and not counts.any()                       # no base, no transition: probability one, nothing counted


# ---- the databases of test_gpu_fwdback.py: what it asserts of the statistics follows from the restatement
def test_inequalities_of_test_gpu_fwdback_follow(oracle_mod):
    """The databases below are COPIES of the recipes (seeds, lengths, rates) of the named tests of test_gpu_fwdback.py, which
    build them inline; only _estep_database can be imported.  Who changes a database there changes its copy here."""
    from synth import synthetic_alignment
    from test_gpu_fwdback import _estep_database
    O = oracle_mod
    # test_onchip_and_streaming_kernels_agree
    rng = random.Random(21)
    pairs = [O.alignment_pair(synthetic_alignment(rng, rng.choice([1, 7, 33, 100, 256]), sub=.03, dele=.02, dup=.02)) for _ in range(90)]
    pairs.append(O.alignment_pair(synthetic_alignment(random.Random(5), 60, sub=.02, dele=.0, dup=.35)))
    pairs.append(O.alignment_pair(synthetic_alignment(random.Random(6), 90, sub=.02, dele=.0, dup=.8)))
    for strict in (False, True):
        got = C.predict_modes(pairs, 6, strict)
        assert got[None][0] + got[None][2] == len(pairs) and got["DNAS_FB_STREAMING"] == (0, 0, len(pairs))
    got = C.predict(pairs, 6)
    assert got[0] >= 61 and got[2] >= 1
    # test_one_long_pair_does_not_fail_the_database
    rng = random.Random(8)
    pairs = [O.alignment_pair(synthetic_alignment(rng, n, sub=.02, dele=.01, dup=.01)) for n in (40, 256, 4000, 12000, 130)]
    got = C.predict(pairs, 6)
    assert got[2] >= 1 and got[0] >= 1
    # test_half_width_wavefront_is_chosen_per_pair
    rng = random.Random(77)
    rows = [synthetic_alignment(rng, 256) for _ in range(120)]
    for i in range(40):
        src = "".join(rng.choice("ACGT") for _ in range(200))
        cut = rng.randrange(40, 120)
        rows.append([("in", src), ("out", src[:cut] + "-" * 24 + src[cut + 24:])])
    got = C.predict_modes([O.alignment_pair(r) for r in rows], 6)
    assert got[None][1] >= 100 and got[None][1] <= got[None][0] - 30
    assert got["DNAS_FB_NO_NARROW"][1] == 0 and got["DNAS_FB_NO_NARROW"][0] == got[None][0]
    # test_one_handle_through_changing_databases_and_models
    a, b = _estep_database(O, 41, 40), _estep_database(O, 43, 124)
    got = C.predict(a, 8)
    assert got[0] >= len(a) // 2 and got[2] >= 1
    assert C.predict(a, 10)[0] == 0
    assert C.predict(a, 3)[0] >= len(a) // 2 and C.predict(a, 4, strict=True)[0] >= len(a) // 2
    assert C.predict(b, 4, strict=True)[0] >= len(b) // 2
    # test_every_dup_width_with_non_uniform_plen
    for P in (0, 1, 2, 5, 6, 7, 8, 9):
        rng = random.Random(90 + P)
        pairs = [O.alignment_pair(synthetic_alignment(rng, rng.choice([1, 7, 33, 100, 180]), sub=.03, dele=.02, dup=.04 if i % 2 and P else 0.))
                 for i in range(80)]
        got = C.predict_modes(pairs, P)
        assert got["DNAS_FB_STREAMING"][0] == 0 and got["DNAS_FB_NO_NARROW"][1] == 0
        for mode in (None, "DNAS_FB_NO_NARROW"):
            assert got[mode][0] == 0 if P > 8 else got[mode][0] >= 60, (P, mode, got)


# ---- the oracle's storage: a row's span of the envelope instead of the reference's (inLen + 1) x (outLen + 1) cells
def _dense_fwdback(O, p, strict, pair):
    """FwdBackMatrix and counts() (reference src/fwdback.cpp:43-128, 154-188) for one pair with the reference's dense storage --
    every cell exists and is -inf until written --, in Python: the operations of oracle/fwdback_oracle.c in their order, its
    log_sum_exp called from the library.  -> (counts, log-likelihood)."""
    import ctypes
    import math
    lse = O.lib().orc_log_sum_exp
    lse.restype, lse.argtypes = ctypes.c_double, (ctypes.c_double, ctypes.c_double)
    exp = lambda x: math.inf if x >= 700 else math.exp(x)           # (+inf where the log-likelihood is -inf; NaN stays NaN)
    ins, outs, cm_in, cm_out = ([int(x) for x in a] for a in pair)
    I, Oo, P = len(ins), len(outs), len(p.pLen)
    W, Dm, NEG = P + 2, 0 if strict else P, -math.inf
    del_open, tan_dup, no_gap = math.log(p.pDelOpen), math.log(p.pTanDup), math.log(1. - p.pDelOpen - p.pTanDup)
    del_ext, del_end = math.log(p.pDelExtend), math.log(1. - p.pDelExtend)
    null, match = math.log(1. / 4.), 1. - p.pTransition - p.pTransversion
    trans = lambda x, y: x != y and (x & 1) == (y & 1)
    sub = [[(math.log(match) if i == j else math.log(p.pTransition) if trans(i, j) else math.log(p.pTransversion / 2)) - null
            for j in range(4)] for i in range(4)]
    ln = [math.log(x) for x in p.pLen]
    inr = lambda i, o: abs(cm_in[i] - cm_out[o]) <= Dm
    mdl = lambda i: min(i, P)
    F = [[[NEG] * W for _ in range(Oo + 1)] for _ in range(I + 1)]
    B = [[[NEG] * W for _ in range(Oo + 1)] for _ in range(I + 1)]
    F[0][0][0] = 0.
    for ip in range(I + 1):
        for op in range(Oo + 1):
            if not inr(ip, op):
                continue
            c = F[ip][op]
            if ip > 0 and op > 0:
                if inr(ip - 1, op - 1):
                    c[0] = F[ip - 1][op - 1][0] + no_gap + sub[ins[ip - 1]][outs[op - 1]]
                if inr(ip, op - 1):
                    left = F[ip][op - 1]
                    for k in range(mdl(ip) - 1):
                        c[2 + k] = left[2 + k + 1] + sub[ins[ip - 1 - (k + 1)]][outs[op - 1]]
                    if P > 0:
                        c[0] = lse(c[0], left[2] + sub[ins[ip - 1]][outs[op - 1]])
            if ip > 0 and inr(ip - 1, op):
                up = F[ip - 1][op]
                c[1] = lse(up[0] + del_open, up[1] + del_ext)
            c[0] = lse(c[0], c[1] + del_end)
            for k in range(mdl(ip)):
                c[2 + k] = lse(c[2 + k], c[0] + tan_dup + ln[k])
    ll = F[I][Oo][0]
    B[I][Oo][0] = 0.
    for ip in range(I, -1, -1):
        for op in range(Oo, -1, -1):
            if not inr(ip, op):
                continue
            c = B[ip][op]
            if op < Oo:
                if ip < I and inr(ip + 1, op + 1):
                    c[0] = no_gap + sub[ins[ip]][outs[op]] + B[ip + 1][op + 1][0]
                if ip > 0 and inr(ip, op + 1):
                    right = B[ip][op + 1]
                    for k in range(1, mdl(ip)):
                        c[2 + k] = sub[ins[ip - 1 - k]][outs[op]] + right[2 + k - 1]
                    if P > 0:
                        c[2] = sub[ins[ip - 1]][outs[op]] + right[0]
            if ip < I and inr(ip + 1, op):
                down = B[ip + 1][op]
                c[0] = lse(c[0], del_open + down[1])
                c[1] = del_ext + down[1]
            for k in range(mdl(ip)):
                c[0] = lse(c[0], c[2 + k] + tan_dup + ln[k])
            c[1] = lse(c[1], c[0] + del_end)
    counts = [0.] * (21 + P)
    for ip in range(I + 1):
        for op in range(Oo + 1):
            if not inr(ip, op):
                continue
            b = B[ip][op]
            if ip > 0 and op > 0:
                cS = exp(F[ip - 1][op - 1][0] + no_gap + sub[ins[ip - 1]][outs[op - 1]] + b[0] - ll)
                counts[2] += cS
                counts[5 + ins[ip - 1] * 4 + outs[op - 1]] += cS
                for k in range(mdl(ip) - 1):
                    counts[5 + ins[ip - 1 - (k + 1)] * 4 + outs[op - 1]] += exp(F[ip][op - 1][2 + k + 1] + sub[ins[ip - 1 - (k + 1)]][outs[op - 1]] + b[2 + k] - ll)
                if P > 0:
                    counts[5 + ins[ip - 1] * 4 + outs[op - 1]] += exp(F[ip][op - 1][2] + sub[ins[ip - 1]][outs[op - 1]] + b[0] - ll)
            if ip > 0:
                counts[0] += exp(F[ip - 1][op][0] + del_open + b[1] - ll)
                counts[3] += exp(F[ip - 1][op][1] + del_ext + b[1] - ll)
            counts[4] += exp(F[ip][op][1] + del_end + b[0] - ll)
            for k in range(mdl(ip)):
                cT = exp(F[ip][op][0] + tan_dup + ln[k] + b[2 + k] - ll)
                counts[1] += cT
                counts[21 + k] += cT
    return np.array(counts), ll


def _same(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def test_oracle_span_storage_equals_dense_storage(oracle_mod):
    """The oracle keeps a row's span of the envelope; the reference keeps every cell.  Both give the same bits: on guides of
    alignments (rows found by the two-pointer scan), on pairs without a path (NaN counts), and on guides that go up and down,
    where rows are searched from both ends and hold cells out of range between cells in range."""
    from synth import synthetic_alignment
    O = oracle_mod
    rng = random.Random("dense")
    sorted_pairs = E.tiny_pairs(12, "dense") + [E.all_deleted_pair(), E.empty_pair()] + E.short_kind_pairs("dense", 1, 1)
    sorted_pairs += [O.alignment_pair(synthetic_alignment(rng, 14, sub=.1, dele=.15, dup=.15)) for _ in range(8)]
    sorted_pairs.append(O.alignment_pair([("in", "--ACGT"), ("out", "TTACG-")]))                 # output before any input: no path
    wild = []
    for _ in range(30):
        i, o = rng.randint(0, 6), rng.randint(0, 6)
        wild.append((np.array([rng.randrange(4) for _ in range(i)], np.int8), np.array([rng.randrange(4) for _ in range(o)], np.int8),
                     np.array([0] + [rng.randint(0, 4) for _ in range(i)], np.int32), np.array([0] + [rng.randint(0, 4) for _ in range(o)], np.int32)))
    gaps = 0
    for pair in wild:
        for a in pair[2]:
            hit = [abs(int(b) - int(a)) <= 0 for b in pair[3]]
            gaps += any(hit) and not all(hit[hit.index(True):len(hit) - hit[::-1].index(True)])
    assert gaps >= 5                                                   # rows with a cell out of range between two in range
    seen_nan = False
    for pairs in (sorted_pairs, wild):
        for length, strict in ((0, False), (2, False), (6, True), (6, False)):
            params = O.MutatorParams.from_cli(length=length, sub=.05, dup=.02, del_open=.02)
            for pair in pairs:
                counts, ll, per = O.expected_counts(params, [pair], strict=strict)
                want_counts, want_ll = _dense_fwdback(O, params, strict, pair)
                assert _same(per, want_ll) and _same(counts, want_counts), (pair, length, strict)
                seen_nan = seen_nan or np.isnan(counts).any()
    assert seen_nan
