"""dnas_simulate_reads_host (csrc/host/simulate.cpp), the statement of the read sampler, against its definition restated in pure
Python (simulate_model.py) -- no GPU: the generator's known answers, equality byte for byte, every sampled path a path of the
model, splitting, the distribution (chi-square against the enumerated outcomes), the sampler against the pair HMM the kernels
score (exact_models._moves, in mpmath), parameter recovery from the true paths, the arguments and the command line."""
import collections
import ctypes
import math
import os
import statistics
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import simulate_model as S  # noqa: E402

ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def values_of(da, name):
    if name != "default":
        return S.PARAM_SETS[name]
    c = da.MutatorParams.fromFlags(global_=True).c                     # the default flags
    return (c.p_del_open, c.p_del_extend, c.p_tan_dup, c.p_transition, c.p_transversion)


def test_library_declares_the_simulate_calls(da):
    names = ("dnas_simulate_reads", "dnas_simulate_reads_host", "dnas_simulate_draw_bits")
    assert set(names) <= set(da.lib.declared_symbols())
    assert all(hasattr(da.lib.lib(), s) for s in names)


# ---- the generator ----------------------------------------------------------------------------------------------------------------

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers(da):
    """Philox4x32-10 of the Random123 known-answer file, in the restatement and -- where a counter is one the library can be asked
    for (call numbers are j / 2 of a 32-bit j) -- in dnas_simulate_draw_bits."""
    bits = da.lib.lib().dnas_simulate_draw_bits
    for counter, key, want in KNOWN_ANSWERS:
        assert S.philox4x32(counter, key) == want
        c, position, lo, hi = counter
        if c < 1 << 31:
            seed, read = key[0] | key[1] << 32, lo | hi << 32
            assert bits(seed, read, position, 2 * c) == (want[0] | want[1] << 32) >> 11
            assert bits(seed, read, position, 2 * c + 1) == (want[2] | want[3] << 32) >> 11
    # the all-ones vector through the library as far as it reaches: key, read and position all ones, the last call number
    w = S.philox4x32((0x7fffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff))
    assert bits(2 ** 64 - 1, 2 ** 64 - 1, 0xffffffff, 0xfffffffe) == (w[0] | w[1] << 32) >> 11
    assert bits(2 ** 64 - 1, 2 ** 64 - 1, 0xffffffff, 0xffffffff) == (w[2] | w[3] << 32) >> 11


def test_draws_agree_with_the_restatement(da):
    bits = da.lib.lib().dnas_simulate_draw_bits
    rng = np.random.RandomState(5)
    points = [(0, 0, 0, 0), (1, 2 ** 32, 0, 1), (7, 2 ** 32 + 3, S.PER_READ, 0), (2 ** 63 + 11, 2 ** 64 - 1, S.PER_READ, 1), (3, 2 ** 40 + 9, 150, 35)]
    for _ in range(300):
        points.append((int(rng.randint(0, 2 ** 62)) * 4 + 1, int(rng.randint(0, 2 ** 62)) * 3, int(rng.randint(0, 2 ** 32)),
                       int(rng.randint(0, 1200))))
    for seed, read, position, j in points:
        got = bits(seed, read, position, j)
        assert got == S.draw_bits(seed, read, position, j) and got < 1 << 53, (seed, read, position, j)


# ---- the host statement against the restatement --------------------------------------------------------------------------------------

def python_pool(pp, strands, read_strand, seed, first_index, reverse_prob):
    return [S.simulate_read(pp, [int(b) for b in strands[s]], seed, first_index + i, reverse_prob) for i, s in enumerate(read_strand)]


def assert_is_python(sim, want, what):
    assert len(sim) == len(want)
    for i, (read, ops, rev) in enumerate(want):
        assert list(sim.reads[i]) == read and list(sim.ops[i]) == ops and bool(sim.reversed[i]) == rev, (what, i)
    assert not sim.status.any()


def assert_paths_are_model_paths(sim, what):
    """dnas_alignment_expand accepts every read's ops over (strand, unreversed read), and its rows spell the two."""
    text = lambda codes: "".join("ACGT"[b] for b in codes)
    for i in range(len(sim)):
        r1, r2, counts = sim.alignment(i)
        assert r1.replace("-", "") == text(sim.originals[int(sim.strand[i])]), (what, i)
        assert r2.replace("-", "") == text(sim.forward(i)), (what, i)
        assert len(r1) == len(r2) == len(sim.ops[i])


@pytest.mark.parametrize("name", list(S.PARAM_SETS))
def test_host_is_the_restatement(da, name):
    strands = S.random_strands(S.STRAND_LENGTHS, 11)
    seed, first = 0x1234567890abcdef, 2 ** 32 - 3                      # the reads' indices cross 2^32
    saw_cap = False
    for P in S.DUP_LENGTHS:
        for zeros in ((False, True) if P in (3, 13) else (False,)):
            mp, pp = S.make_params(da, values_of(da, name), S.p_len_of(P, zeros))
            for reverse_prob in S.REVERSE_PROBS:
                what = (name, P, zeros, reverse_prob)
                sim = da.simulateReads(mp, strands, coverage=2, seed=seed, first_index=first, reverse_prob=reverse_prob, host=True)
                assert list(sim.strand) == [s for s in range(len(strands)) for _ in range(2)] and sim.stats is None
                assert_is_python(sim, python_pool(pp, strands, sim.strand, seed, first, reverse_prob), what)
                assert_paths_are_model_paths(sim, what)
                if reverse_prob in (0., 1.):
                    assert all(bool(r) == (reverse_prob == 1.) for r in sim.reversed)
                else:
                    assert 0 < sim.reversed.sum() < len(sim)
                if name == "del-open-1":
                    assert all(len(r) == 0 for r in sim.reads)
                if name == "dup-0" or P == 0:
                    assert all(((o & 3) != S.OP_DUP).all() for o in sim.ops)
                if name == "del-extend-1":                             # a deletion, once open, runs to the strand's end
                    for o in sim.ops:
                        opened = np.flatnonzero(o == (S.OP_DELETE | 1 << 2))
                        assert len(opened) <= 1 and (len(opened) == 0 or (o[opened[0] + 1:] & 3 != S.OP_MATCH).all())
                if name == "dup-.9" and P:                             # the cap: some position made exactly 16 duplications
                    for i, o in enumerate(sim.ops):
                        ip = np.cumsum((o & 3) != S.OP_DUP) - ((o & 3) != S.OP_DUP)
                        opened = np.bincount(ip[((o & 3) == S.OP_DUP) & (o >> 2 > 0)], minlength=1)
                        assert opened.max() <= S.MAX_DUPS
                        saw_cap |= bool(opened.max() == S.MAX_DUPS)
    assert saw_cap == (name == "dup-.9")


def test_no_reads_and_empty_strands(da):
    mp, _ = S.make_params(da, S.NOISY_SET, S.p_len_of(3))
    sim = da.simulateReads(mp, ["ACGT"], coverage=0, host=True)
    assert len(sim) == 0 and sim.ops == [] and sim.reads == []
    sim = da.simulateReads(mp, [], host=True)
    assert len(sim) == 0
    sim = da.simulateReads(mp, ["", ""], coverage=3, seed=4, reverse_prob=.5, host=True)
    assert len(sim) == 6 and all(len(r) == 0 for r in sim.reads) and all(len(o) == 0 for o in sim.ops)
    sim = da.simulateReads(mp, ["ACGTACGT"], coverage=5, seed=4, ops=False, host=True)
    assert sim.ops is None
    with pytest.raises(ValueError):
        sim.alignment(0)
    assert [list(r) for r in sim.reads] == [list(r) for r in da.simulateReads(mp, ["ACGTACGT"], coverage=5, seed=4, host=True).reads]


def test_splitting_changes_nothing(da):
    mp, _ = S.make_params(da, S.NOISY_SET, S.p_len_of(3))
    strands = S.random_strands((40, 0, 65, 7, 130), 3)
    rng = np.random.RandomState(9)
    read_strand = [int(s) for s in rng.randint(0, len(strands), 101)]
    seed, first = 99, 2 ** 32 - 50
    whole = da.simulateReads(mp, strands, read_strand=read_strand, seed=seed, first_index=first, reverse_prob=.5, host=True)
    a = da.simulateReads(mp, strands, read_strand=read_strand[:50], seed=seed, first_index=first, reverse_prob=.5, host=True)
    b = da.simulateReads(mp, strands, read_strand=read_strand[50:], seed=seed, first_index=first + 50, reverse_prob=.5, host=True)
    for i in range(101):
        part, j = (a, i) if i < 50 else (b, i - 50)
        assert np.array_equal(whole.reads[i], part.reads[j]) and np.array_equal(whole.ops[i], part.ops[j])
        assert whole.reversed[i] == part.reversed[j]
    # the same list in another order, read by read, looked up by global index
    for i in rng.permutation(101)[:40]:
        one = da.simulateReads(mp, strands, read_strand=[read_strand[i]], seed=seed, first_index=first + int(i), reverse_prob=.5, host=True)
        assert np.array_equal(whole.reads[i], one.reads[0]) and np.array_equal(whole.ops[i], one.ops[0]) and whole.reversed[i] == one.reversed[0]
    # shuffle=True is random.Random(seed) on the host, before the call
    import random
    want = [s for s in range(len(strands)) for _ in range(4)]
    random.Random(seed).shuffle(want)
    shuffled = da.simulateReads(mp, strands, coverage=4, seed=seed, shuffle=True, host=True)
    assert list(shuffled.strand) == want
    S.assert_same_reads(shuffled, da.simulateReads(mp, strands, read_strand=want, seed=seed, host=True))


# ---- the distribution ---------------------------------------------------------------------------------------------------------------

def chi_square_quantile(cells, tail=1e-9):
    """The 1 - tail quantile of chi-square with cells - 1 degrees of freedom by Wilson and Hilferty: k (1 - 2/(9k) + z sqrt(2/(9k)))^3."""
    k = cells - 1
    z = statistics.NormalDist().inv_cdf(1 - tail)
    return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


def test_the_distribution_is_the_stated_one(da):
    """200 000 reads of ACG at the noisy set, P = 2, pLen = [.7, .3], against the enumerated outcomes (at most 2 duplications per
    position; the rest and every outcome of expected count below 5 in one cell): Pearson's statistic must not exceed the chi-square
    quantile at 1 - 1e-9.  The seed is fixed by its name; a failure is a defect, not a reason to choose another."""
    N = 200000
    mp, pp = S.make_params(da, S.NOISY_SET, [.7, .3])
    strand = [0, 1, 2]
    outcomes, _ = S.enumerate_outcomes(pp, strand, max_dups=2, floor=5. / N)
    cells = {k: p for k, p in outcomes.items() if p * N >= 5}
    rest = 1 - sum(cells.values())
    assert len(cells) > 100 and rest * N >= 5
    sim = da.simulateReads(mp, [np.array(strand, np.int8)], coverage=N, seed=S.seed_of("simulate/chi2"), host=True)
    seen = collections.Counter((tuple(int(x) for x in o), tuple(int(x) for x in r)) for o, r in zip(sim.ops, sim.reads))
    other = N - sum(seen[k] for k in cells)
    stat = sum((seen[k] - N * p) ** 2 / (N * p) for k, p in cells.items()) + (other - N * rest) ** 2 / (N * rest)
    cap = chi_square_quantile(len(cells) + 1)
    print("cells %d, Pearson %.1f, cap %.1f" % (len(cells) + 1, stat, cap))
    assert stat <= cap


def test_the_sampler_is_the_model_the_kernels_score(da):
    """P = 1 and a strand of 4 bases: every enumerated outcome is a walk along exact_models._moves, and the sampler's probability
    over the walk's weight (the move weights' product x 4^-O) is (1 - pTanDup) for a path that opens with a deletion and
    (1 - pTanDup)(noGap + pTanDup)/noGap for one that opens with a match, to 1e-12 relative in mpmath -- the two places the
    sampler normalises what the pair HMM leaves open, position 0 and position I.  A path that deletes the strand's last base has
    one more factor, 1/delEnd: the definition ends a deletion that reaches I without a draw, where the model charges delEnd; the
    test divides it out and holds those paths to the same two values."""
    import mpmath
    import exact_models as X
    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    pp = S.Params(*[mpf(str(x)) for x in S.NOISY_SET], [mpf(1)])
    strand = [2, 0, 3, 1]
    outcomes, _ = S.enumerate_outcomes(pp, strand, max_dups=2, floor=mpf("1e-6"), num=mpf)
    assert len(outcomes) > 1000
    m = X.PairModel(pp)
    with_deletion, with_match = 1 - m.tan_dup, (1 - m.tan_dup) * (m.no_gap + m.tan_dup) / m.no_gap
    seen = set()
    for (ops, read), prob in outcomes.items():
        node, weight, last_deleted = (0, 0, "S"), mpf(1), False
        for c, op in enumerate(ops):
            kind, n = op & 3, op >> 2
            ip, o, lane = node
            if lane == "D" and not (kind == S.OP_DELETE and n == 0):   # the deletion ends before this column
                nxt = [mv for mv in X._moves(m, node, strand, read) if mv[0] == (ip, o, "S")]
                assert len(nxt) == 1
                node, weight = nxt[0][0], weight * nxt[0][1]
                ip, o, lane = node
            if kind == S.OP_MATCH:
                want = (ip + 1, o + 1, "S")
            elif kind == S.OP_DELETE:
                assert (n == 1) == (lane == "S")
                want = (ip + 1, o, "D")
                last_deleted |= ip + 1 == len(strand)
            elif n:                                                    # a duplication opens: S -> T_{n-1}, which emits
                nxt = [mv for mv in X._moves(m, node, strand, read) if mv[0] == (ip, o, n - 1)]
                assert lane == "S" and len(nxt) == 1
                node, weight = nxt[0][0], weight * nxt[0][1]
                want = (ip, o + 1, n - 2 if n > 1 else "S")
            else:
                assert lane not in ("S", "D")
                want = (ip, o + 1, lane - 1 if lane else "S")
            nxt = [mv for mv in X._moves(m, node, strand, read) if mv[0] == want]
            assert len(nxt) == 1, (ops, read, c)
            node, weight = nxt[0][0], weight * nxt[0][1]
        if node[2] == "D":                                             # the last column deleted the last base
            weight *= m.del_end
            node = (node[0], node[1], "S")
        assert node == (len(strand), len(read), "S")
        ratio = prob / (weight * mpf(4) ** -len(read))
        if last_deleted:
            ratio *= m.del_end
        want = with_deletion if ops[0] & 3 == S.OP_DELETE else with_match
        assert abs(ratio / want - 1) < mpf("1e-12"), (ops, read, ratio, want)
        seen.add((ops[0] & 3, last_deleted))
    assert seen == {(S.OP_DELETE, False), (S.OP_DELETE, True), (S.OP_MATCH, False), (S.OP_MATCH, True)}


def test_parameter_recovery_from_the_truth(da):
    """20 000 reads of 150-base random strands at sub=.04, dele=.02, pDelExtend=.1, dup=.01, P=4: the counts of the true paths over
    the positions P <= ip < I recover every parameter within 5 binomial standard deviations."""
    N, I = 20000, 150
    mp = da.MutatorParams.fromFlags(sub=.04, dup=.01, del_open=.02, del_ext=.1, global_=True, length=8)
    P, p_len = mp.c.n_len, mp.pLen
    assert P == 4
    strands = S.random_strands([I] * 200, 21)
    sim = da.simulateReads(mp, strands, coverage=N // 200, seed=S.seed_of("simulate/recover"), host=True)
    total = np.zeros(21 + P)
    for i in range(N):
        total += sim.alignment(i)[2]
    # the columns of every read with the input position they belong to: a duplication column stands at the position it precedes
    ops = np.concatenate(sim.ops)
    lens = np.array([len(o) for o in sim.ops])
    kind, n = ops & 3, ops >> 2
    consumes = (kind != S.OP_DUP).astype(np.int64)
    before = np.cumsum(consumes) - consumes
    start = np.repeat(before[np.cumsum(lens) - lens], lens)
    ip = before - start
    last = np.zeros(len(ops), bool)
    last[np.cumsum(lens) - 1] = True
    inside = (ip >= P) & (ip < I)
    opened, extended = (kind == S.OP_DELETE) & (n == 1), (kind == S.OP_DELETE) & (n == 0)
    dup_open, match = (kind == S.OP_DUP) & (n > 0), kind == S.OP_MATCH
    # the whole walk agrees with the counts dnas_alignment_expand gives
    assert opened.sum() == total[0] and dup_open.sum() == total[1] and match.sum() == total[2] and extended.sum() == total[3]
    assert [int((dup_open & (n == k + 1)).sum()) for k in range(P)] == [int(x) for x in total[21:]]
    # a deletion column is followed by a position entered in D; it ends there unless the next column extends it (at I no draw is taken)
    is_del = kind == S.OP_DELETE
    next_extends = np.append(extended[1:], False) & ~last
    entered = is_del & (ip + 1 >= P) & (ip + 1 < I)
    n_ext, n_end = int((entered & next_extends).sum()), int((entered & ~next_extends).sum())
    visits = int((inside & (opened | dup_open | match)).sum())
    sub = total[5:21].reshape(4, 4)
    draws = sub.sum()
    n_ti = sum(sub[x][x ^ 2] for x in range(4))
    n_tv = draws - n_ti - np.trace(sub)
    n_dup = int((inside & dup_open).sum())
    checks = [("pDelOpen", int((inside & opened).sum()), visits, mp.c.p_del_open), ("pTanDup", n_dup, visits, mp.c.p_tan_dup),
              ("pDelExtend", n_ext, n_ext + n_end, mp.c.p_del_extend), ("pTransition", n_ti, draws, mp.c.p_transition),
              ("pTransversion", n_tv, draws, mp.c.p_transversion)]
    checks += [("pLen[%d]" % k, int((inside & dup_open & (n == k + 1)).sum()), n_dup, p_len[k]) for k in range(P)]
    for what, hits, trials, p in checks:
        sd = math.sqrt(p * (1 - p) / trials)
        print("%-14s %9d / %9d = %.6f, parameter %.6f, %+.2f sd" % (what, hits, trials, hits / trials, p, (hits / trials - p) / sd))
        assert abs(hits / trials - p) <= 5 * sd, what


def test_statement_under_sanitizers(tmp_path):
    """tools/simulate_host_check.cpp, a program of its own under ASan and UBSan: the statement over the list above with every strand
    in a heap block of exactly its length, the kernels' way of assembling a read from per-position outcomes and simEntryBits
    restated on the CPU and equal to the statement, simEntryBits against the bit-by-bit recurrence."""
    exe = str(tmp_path / "simulate_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "simulate_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"3528 reads" in r.stdout and b" 0 failures" in r.stdout, (r.stdout.decode(), r.stderr.decode()[-4000:])


# ---- arguments and the command line ------------------------------------------------------------------------------------------------

def test_arguments(da):
    L, lib = da.lib.lib(), da.lib
    strands = ["ACGTACGT", "GGA"]

    def code(values=S.NOISY_SET, p_len=(.5, .5), n_len=None, **kw):
        mp, _ = S.make_params(da, values, list(p_len))
        if n_len is not None:
            mp.c.n_len = n_len
        with pytest.raises(lib.DnasError) as e:
            da.simulateReads(mp, kw.pop("strands", strands), host=True, **kw)
        return e.value.code

    assert code(values=(-.1, .3, .1, .1, .1)) == -1
    assert code(values=(.1, 1.5, .1, .1, .1)) == -1
    assert code(values=(.1, .3, float("nan"), .1, .1)) == -1
    assert code(values=(.1, .3, .1, 1.1, 0)) == -1
    assert code(values=(.1, .3, .1, .1, -1e-9)) == -1
    assert code(values=(.6, .3, .5, .1, .1)) == -1                     # pDelOpen + pTanDup > 1
    assert code(values=(.1, .3, .1, .6, .5)) == -1                     # pTransition + pTransversion > 1
    assert code(p_len=(.5, 1.5)) == -1
    assert code(reverse_prob=1.5) == -1 and code(reverse_prob=-.1) == -1
    assert code(read_strand=[0, 2]) == -1 and code(read_strand=[-1]) == -1
    assert code(n_len=33) == -9 and code(n_len=-1) == -1
    assert code(strands=[np.array([0, 1, 4], np.int8)]) == -6
    # the same checks stand in front of the GPU call, device or not
    mp, _ = S.make_params(da, (.6, .3, .5, .1, .1), [1.])
    with pytest.raises(lib.DnasError) as e:
        da.simulateReads(mp, strands)
    assert e.value.code == -1
    # null outputs
    ok, _ = S.make_params(da, S.NOISY_SET, [1.])
    assert L.dnas_simulate_reads_host(ctypes.byref(ok.c), 0, None, None, 0, None, 0, 0, 0., 1, None, None, None, None, None, None) == -1


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))


def _records(text):
    recs, name = [], None
    for line in text.splitlines():
        if line.startswith(">"):
            name = line[1:]
            recs.append([name, ""])
        elif line:
            recs[-1][1] += line
    return recs


def test_cli(da, tmp_path):
    rng = np.random.RandomState(2)
    names = ["orig%d" % i for i in range(6)]
    strands = ["".join("ACGT"[b] for b in rng.randint(0, 4, n)) for n in (70, 1, 33, 64, 90, 12)]
    fa = str(tmp_path / "originals.fa")
    _fasta(fa, names, strands)
    flags = ["--error-sub-prob", ".05", "--error-del-open", ".03", "--error-dup-prob", ".04", "--error-global", "-l", "6"]
    mp = da.MutatorParams.fromFlags(sub=.05, dup=.04, del_open=.03, global_=True, length=6)
    run = lambda args: subprocess.run([BIN, "-v0", "--simulate-reads", fa] + flags + args, capture_output=True, timeout=120)

    def expected(sim):
        made, out = collections.Counter(), []
        for i, s in enumerate(sim.strand):
            made[int(s)] += 1
            out.append(["%s/%d%s" % (names[int(s)], made[int(s)], " strand=-" if sim.reversed[i] else ""), sim.strings()[i]])
        return out

    for shuffle in (False, True):
        done = run(["--simulate-coverage", "3", "--simulate-seed", "12345678901234567", "--simulate-reverse", ".5"] + (["--simulate-shuffle"] if shuffle else []))
        assert done.returncode == 0, done.stderr
        want = da.simulateReads(mp, strands, coverage=3, seed=12345678901234567, reverse_prob=.5, shuffle=shuffle, host=True)
        assert 0 < want.reversed.sum() < len(want)
        assert _records(done.stdout.decode()) == expected(want)
    done = run([])
    assert done.returncode == 0 and _records(done.stdout.decode()) == expected(da.simulateReads(mp, strands, host=True))

    # --simulate-stockholm: read back by dnas_stockholm_read, and --fit-error runs on it
    done = run(["--simulate-coverage", "4", "--simulate-seed", "5", "--simulate-reverse", ".5", "--simulate-stockholm"])
    assert done.returncode == 0, done.stderr
    sto = str(tmp_path / "truth.sto")
    with open(sto, "wb") as f:
        f.write(done.stdout)
    want = da.simulateReads(mp, strands, coverage=4, seed=5, reverse_prob=.5, host=True)
    assert done.stdout.decode() == want.stockholm([names[int(s)] for s in want.strand], [r[0].split()[0] for r in expected(want)])
    db = da.StockholmDB(sto).arrays()
    keep = [i for i in range(len(want)) if len(want.ops[i])]
    assert db["n"] == len(keep)
    for j, i in enumerate(keep):
        assert np.array_equal(db["ins"][db["in_off"][j]:db["in_off"][j + 1]], want.originals[int(want.strand[i])])
        assert np.array_equal(db["outs"][db["out_off"][j]:db["out_off"][j + 1]], want.forward(i))
    fit = subprocess.run([BIN, "-v0", "--fit-error", sto] + flags, capture_output=True, timeout=300)
    if da.lib.lib().dnas_device_count() > 0:
        assert fit.returncode == 0 and b"pDelOpen" in fit.stdout, fit.stderr
    else:                                                              # --fit-error is a GPU action: it read the database, then found no device
        assert b"No such" not in fit.stderr and b"parse" not in fit.stderr.lower(), fit.stderr

    # bad flags: exit 1, nothing on stdout
    for bad in (["--simulate-coverage", "0"], ["--simulate-reverse", "1.5"], ["--simulate-reverse", "-1"], ["--simulate-seed", "-3"],
                ["--simulate-seed", "x"]):
        done = run(bad)
        assert done.returncode == 1 and done.stdout == b"" and done.stderr, bad
    done = subprocess.run([BIN, "-v0", "--simulate-coverage", "3"], capture_output=True, timeout=60)
    assert done.returncode == 1 and done.stdout == b""
    done = subprocess.run([BIN, "-v0", "--simulate-reads", str(tmp_path / "missing.fa")], capture_output=True, timeout=60)
    assert done.returncode == 1 and done.stdout == b""
    assert b"--simulate-reads" in subprocess.run([BIN, "--help"], capture_output=True, timeout=60).stdout


def test_frame_primers(da):
    primers = [("ACGTAC", "TTGACA"), ("GGGTTT", "CACACA")]
    framed = da.framePrimers(["AAAA", "CCCC", ""], primers, [1, 0, 1])
    assert ["".join("ACGT"[b] for b in m) for m in framed] == ["GGGTTTAAAACACACA", "ACGTACCCCCTTGACA", "GGGTTTCACACA"]
    assert [len(m) for m in da.framePrimers(["AAAA", "CC"], primers, 0)] == [16, 14]
    mp, _ = S.make_params(da, (0., 0., 0., 0., 0.), [])
    sim = da.simulateReads(mp, framed, coverage=2, seed=3, reverse_prob=.5, host=True)               # a noiseless channel, either strand
    trimmed = da.trimReads(primers, sim.reads, host=True)
    assert list(trimmed.pair) == [1, 1, 0, 0, 1, 1] and list(trimmed.strand) == list(sim.reversed)
    assert ["".join("ACGT"[b] for b in p) for p in trimmed.payloads()] == ["AAAA", "AAAA", "CCCC", "CCCC", "", ""]
