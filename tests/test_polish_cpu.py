"""Consensus reads (dnas_cluster_consensus_host) against a Python restatement of the definition in include/dnastore_amd.h,
written from the header's words over alignPairs(host=True) op bytes.  No GPU."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")

from test_assign_cpu import BANDS, NOISY, _rand, models  # noqa: E402

BASES = "ACGT"
MAX_INSERT = 4
OK, NO_VOTERS, NO_READS = 0, 1, 2
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


# ------------------------------------------------------------------------------------------------ the definition, restated
def vote_and_emit(t, voters, kinds=None):
    """Steps 2 and 3 for one cluster: t the template, voters the (oriented read, op bytes) of the reads that aligned.  kinds: a
    Counter that receives what kinds of column the round held (tests/polish_columns.py names them), or None."""
    I, V = len(t), len(voters)
    M = [[0] * 4 for _ in range(I)]
    D = [0] * I
    N = [[0] * MAX_INSERT for _ in range(I + 1)]
    B = [[[0] * 4 for _ in range(MAX_INSERT)] for _ in range(I + 1)]
    long_runs = [0] * (I + 1)                                      # per gap, the voters whose run there was truncated
    for out, ops in voters:
        ip = op = 0
        c = 0
        while c < len(ops):
            kind = int(ops[c]) & 3
            if kind == 0:
                M[ip][BASES.index(out[op])] += 1
                ip, op, c = ip + 1, op + 1, c + 1
            elif kind == 1:
                D[ip] += 1
                ip, c = ip + 1, c + 1
            else:
                run = 0
                while c < len(ops) and int(ops[c]) & 3 == 2:
                    run, c = run + 1, c + 1
                for k in range(min(run, MAX_INSERT)):
                    N[ip][k] += 1
                    B[ip][k][BASES.index(out[op + k])] += 1
                long_runs[ip] += run > MAX_INSERT
                op += run
        assert ip == I and op == len(out)
    new = []
    edge = lambda g: g % 64 in (63, 0)                             # the first or the last lane of a chunk of the device's emit
    streak = 0                                                     # the gaps before g, without a break, that emitted insertions
    for g in range(I + 1):
        k = 0
        while k < MAX_INSERT and 2 * N[g][k] > V:
            new.append(BASES[B[g][k].index(max(B[g][k]))])         # index(): the smallest code on a tie
            if kinds is not None:
                kinds["ins"] += 1
                kinds["ins_even_V"] += V % 2 == 0
                kinds["ins_V_gt_64"] += V > 64
                kinds["ins_k3"] += k == 3
                kinds["ins_gap_I"] += g == I
                kinds["ins_chunk_edge"] += edge(g)
                kinds["ins_B_tie"] += B[g][k].count(max(B[g][k])) > 1
                if k == 0:
                    kinds["long_runs"] += long_runs[g]
            k += 1
        streak = streak + 1 if k else 0
        if kinds is not None and streak >= 4:
            kinds["ins_four_gaps"] += 1
        if kinds is not None and k < MAX_INSERT and N[g][k] and 2 * N[g][k] == V:
            kinds["tie_2N_eq_V"] += 1
        if g < I and kinds is not None:
            kinds["tie_2D_eq_V"] += D[g] > 0 and 2 * D[g] == V
            if 2 * D[g] > V:
                kinds["del"] += 1
                kinds["del_V_gt_64"] += V > 64
                kinds["del_chunk_edge"] += edge(g)
            else:
                kinds["M_tie_excl"] += M[g].count(max(M[g])) > 1 and M[g][BASES.index(t[g])] != max(M[g])
        if g < I and not 2 * D[g] > V:
            top = max(M[g])
            new.append(t[g] if M[g][BASES.index(t[g])] == top else BASES[M[g].index(top)])
    return "".join(new)


def consensus_py(da, params, templates, reads, band, read_strand=None, rounds=4, kinds=None, trace=None, limit=None):
    """-> (seqs, rounds, converged, voters, status) per cluster, by the words of the header.  kinds: a Counter for vote_and_emit,
    which also receives the rounds that only drop trailing bases, the clusters changing in a second and a third round and those whose template crosses `limit` bases
    upwards or downwards; trace: a list that receives, per round run, the (cluster, template length, reads) still active."""
    nc = len(templates)
    seqs = list(templates)
    oriented = [[revcomp(r) if read_strand is not None and read_strand[c][i] else r for i, r in enumerate(reads[c])] for c in range(nc)]
    n_rounds, converged, voters = [0] * nc, [0] * nc, [0] * nc
    status = [OK if reads[c] else NO_READS for c in range(nc)]
    active = [c for c in range(nc) if reads[c]]
    for run in range(1, rounds + 1):
        if not active:
            break
        if trace is not None:
            trace.append([(c, len(seqs[c]), len(reads[c])) for c in active])
        ins = [seqs[c] for c in active for _r in oriented[c]]
        outs = [r for c in active for r in oriented[c]]
        al = da.alignPairs(params, ins, outs, band=band, host=True)
        at, still = 0, []
        for c in active:
            mine = [(oriented[c][i], al.ops[at + i]) for i in range(len(oriented[c])) if al.status[at + i] == da.lib.ALIGN_OK]
            at += len(oriented[c])
            voters[c] = len(mine)
            if not mine:
                status[c] = NO_VOTERS
                continue
            status[c] = OK
            new = vote_and_emit(seqs[c], mine, kinds)
            if new == seqs[c]:
                converged[c] = 1
                continue
            if kinds is not None:
                kinds["del_tail_only"] += seqs[c].startswith(new)
                kinds["changed_round2"] += run == 2
                kinds["changed_round3"] += run == 3
                if limit is not None:
                    kinds["cross_up"] += len(seqs[c]) <= limit < len(new)
                    kinds["cross_down"] += len(new) <= limit < len(seqs[c])
            seqs[c] = new
            n_rounds[c] += 1
            still.append(c)
        active = still
    return seqs, n_rounds, converged, voters, status


def same(got, want):
    seqs, n_rounds, converged, voters, status = want
    assert got.strings() == seqs
    assert [int(x) for x in got.rounds] == n_rounds and [int(x) for x in got.converged] == converged
    assert [int(x) for x in got.voters] == voters and [int(x) for x in got.status] == status


def same_result(got, want):
    assert got.strings() == want.strings()
    for f in ("rounds", "converged", "voters", "status"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


# ---------------------------------------------------------------------------------------------------------------- cases
def shape_pool(da):
    """Templates of 0, 1, 63, 64, 65 and 130 nt (and of 20, 64 and 33), clusters of 0, 1, 2, 7 and 70 reads -- the 70 are reads of
    about 20 nt, more voters than a wave has lanes --, every other read given reverse-complemented with read_strand 1, and a
    cluster of two unequal reads, none of which the global exact model aligns.  -> (templates, reads, read_strand)."""
    from test_pair_align_cpu import edited
    rng = random.Random("polish/shapes")
    templates, reads = [], []
    for n, count in ((0, 2), (1, 1), (63, 2), (64, 7), (65, 2), (130, 7), (20, 70), (64, 0), (33, 2)):
        truth = _rand(rng, n)
        t = list(truth)
        for at in rng.sample(range(n), min(n, 4)):        # the template: exactly n bases, four of them wrong
            t[at] = rng.choice([b for b in BASES if b != t[at]])
        templates.append("".join(t))
        reads.append([edited(rng, truth, 2) for _ in range(count)])
    reads[0] = ["", "A"]                                  # the empty template: the empty read aligns, no other does
    reads[8] = [_rand(rng, 30), _rand(rng, 36)]
    strands = [[i % 2 for i in range(len(rs))] for rs in reads]
    reads = [[revcomp(r) if s else r for r, s in zip(rs, ss)] for rs, ss in zip(reads, strands)]
    assert [len(t) for t in templates] == [0, 1, 63, 64, 65, 130, 20, 64, 33]
    return templates, reads, strands


def test_shape_pool_against_the_restatement(da):
    templates, reads, strands = shape_pool(da)
    statuses, changed = set(), 0
    for name, params in models(da):
        for band in BANDS:
            got = da.consensusReads(params, templates, reads, band=band, read_strand=strands, rounds=3, host=True)
            want = consensus_py(da, params, templates, reads, band, strands, rounds=3)
            same(got, want)
            assert got.stats is None
            statuses |= set(int(s) for s in got.status)
            changed += int((got.rounds > 0).sum())
            if name == "P6-global-exact":
                assert got.status[8] == NO_VOTERS and got.strings()[8] == templates[8] and got.converged[8] == 0
    assert statuses == {OK, NO_VOTERS, NO_READS} and changed > 20
    name, params = models(da)[2]                          # no strand array: every read as given
    same(da.consensusReads(params, templates, reads, band=8, rounds=2, host=True), consensus_py(da, params, templates, reads, 8, None, 2))


T = "GATTACAGGCTCATGC"


def one(da, params, reads, rounds=1, template=T):
    got = da.consensusReads(params, [template], [reads], band=-1, rounds=rounds, host=True)
    same(got, consensus_py(da, params, [template], [reads], -1, None, rounds))
    return got.strings()[0], int(got.voters[0])


def test_hand_made_ties(da):
    from test_pair_align_cpu import make_params
    p = da.MutatorParams.fromFlags(**NOISY)
    gone = T[:4] + T[5:]                                  # T without its A at 4
    assert one(da, p, [T, gone]) == (T, 2)                # 2 D == V keeps the base
    assert one(da, p, [T, gone, gone]) == (gone, 3)
    more = T[:5] + T[4] + T[5:]                           # a tandem copy of that A
    assert one(da, p, [T, more]) == (T, 2)                # 2 N == V does not insert
    assert one(da, p, [T, more, more]) == (more, 3)
    assert T[10] == "T"
    sub = lambda b: T[:10] + b + T[11:]
    assert one(da, p, [T, sub("G")]) == (T, 2)            # a tie in M keeps the template's base
    assert one(da, p, [sub("G"), sub("C")]) == (sub("C"), 2)       # ... that excludes it: the smallest code
    assert one(da, p, [sub("G"), sub("C"), sub("G")]) == (sub("G"), 3)
    six = T[:10] + T[4:10] + T[10:]                       # a tandem copy of six bases: a run of 6, of which 4 are kept
    al = da.alignPairs(p, [T], [six], band=-1, host=True)
    assert [int(o) & 3 for o in al.ops[0]] == [0] * 10 + [2] * 6 + [0] * 6
    assert one(da, p, [six, six, six]) == (T[:10] + T[4:8] + T[10:], 3)
    tail = T + T[-2:]                                     # an insertion at gap I, after the last base
    assert one(da, p, [tail, tail, T]) == (tail, 3)
    p1 = make_params(da, [1.], pTanDup=.1)                # only duplications of one base: two adjacent ones are one run
    twice = T[:10] + T[9] + T[9] + T[10:]
    al = da.alignPairs(p1, [T], [twice], band=-1, host=True)
    assert [int(o) for o in al.ops[0]][10:12] == [2 | 1 << 2, 2 | 1 << 2]
    assert one(da, p1, [twice, twice, T]) == (twice, 3)


def two_round_cluster():
    """A template far from its reads, found by search with the restatement: the first round's template aligns the reads otherwise."""
    from test_pair_align_cpu import edited
    rng = random.Random("polish/two-rounds/%d" % TWO_ROUND_SEED)
    truth = _rand(rng, 60)
    return edited(rng, truth, 12), [edited(rng, truth, 2) for _ in range(5)]


TWO_ROUND_SEED = 4                                        # the first of 0, 1, ... whose cluster takes two rounds


def test_termination(da):
    p = da.MutatorParams.fromFlags(**NOISY)
    templates, reads, strands = shape_pool(da)
    got = da.consensusReads(p, templates, reads, band=8, read_strand=strands, rounds=0, host=True)
    assert got.strings() == templates and not got.rounds.any() and not got.converged.any() and not got.voters.any()
    assert [int(s) for s in got.status] == [NO_READS if not r else OK for r in reads]
    got = da.consensusReads(p, [T], [[T, T, T]], band=8, host=True)
    assert got.strings() == [T] and list(got.rounds) == [0] and list(got.converged) == [1] and list(got.voters) == [3]
    t, rs = two_round_cluster()
    full = da.consensusReads(p, [t], [rs], band=8, rounds=6, host=True)
    same(full, consensus_py(da, p, [t], [rs], 8, None, 6))
    assert full.rounds[0] == 2 and full.converged[0] == 1
    cut = da.consensusReads(p, [t], [rs], band=8, rounds=2, host=True)          # rounds_max reached while still changing
    assert cut.strings() == full.strings() and cut.rounds[0] == 2 and cut.converged[0] == 0
    first = da.consensusReads(p, [t], [rs], band=8, rounds=1, host=True)
    assert first.strings() != full.strings() and first.rounds[0] == 1 and first.converged[0] == 0
    again = da.consensusReads(p, first.strings(), [rs], band=8, rounds=1, host=True)   # rounds compose
    assert again.strings() == full.strings()
    empty = da.consensusReads(p, [], [], host=True)
    assert len(empty) == 0


def test_argument_errors(da):
    from test_pair_align_cpu import make_params
    p = da.MutatorParams.fromFlags(**NOISY)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.consensusReads(p, [T], [[T]], rounds=-1, host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.consensusReads(p, [T], [[T]], band=-2, host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.consensusReads(p, [np.array([0, 4, 1], dtype=np.int8)], [[T]], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.consensusReads(p, [T], [[np.array([0, -1], dtype=np.int8)]], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.consensusReads(p, [T], [[T]], read_strand=[[2]], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.consensusReads(make_params(da, [1. / 14] * 14), [T], [[T]], host=True)
    with pytest.raises(ValueError):
        da.consensusReads(p, [T, T], [[T]], host=True)
    # offsets that do not ascend: only the C ABI can be handed those
    L = da.lib.lib()
    seq = np.zeros(8, dtype=np.int8)
    i64 = lambda *x: np.array(x, dtype=np.int64)
    out, out_off = ctypes.c_void_p(), i64(0, 0, 0)
    i32, u8 = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    call = lambda toff, roff, cloff: L.dnas_cluster_consensus_host(
        ctypes.byref(p.c), 8, 2, seq.ctypes.data, toff.ctypes.data, 2, seq.ctypes.data, roff.ctypes.data, None, cloff.ctypes.data, 1,
        ctypes.byref(out), out_off.ctypes.data, i32.ctypes.data, u8.ctypes.data, i32.ctypes.data, u8.ctypes.data)
    assert call(i64(0, 4, 8), i64(0, 4, 8), i64(0, 1, 2)) == 0
    L.dnas_free(out)
    out.value = None
    for bad in ((i64(0, 5, 4), i64(0, 4, 8), i64(0, 1, 2)), (i64(0, 4, 8), i64(0, 5, 4), i64(0, 1, 2)),
                (i64(0, 4, 8), i64(0, 4, 8), i64(0, 2, 1)), (i64(1, 4, 8), i64(0, 4, 8), i64(0, 1, 2)),
                (i64(0, 4, 8), i64(0, 4, 8), i64(0, 1, 1))):
        assert call(*bad) == -1 and out.value is None
    assert {"dnas_cluster_consensus", "dnas_cluster_consensus_host", "dnas_viterbi_clusters_ex"} <= set(da.lib.declared_symbols())


def test_cli_usage(da, tmp_path):
    """--cluster-polish goes with -V and --cluster-file or --cluster-auto only; that is decided before a GPU is needed."""
    data = os.path.join(ROOT, "tests", "golden", "ref_data")
    run = lambda *args: subprocess.run([BIN, "-v0"] + list(args), capture_output=True, timeout=120)
    fa, lab = str(tmp_path / "reads.fa"), str(tmp_path / "labels.txt")
    with open(fa, "w") as f:
        f.write(">r0\nACGTACGT\n>r1\nACGTACGA\n")
    with open(lab, "w") as f:
        f.write("x\nx\n")
    mach = ["-L", os.path.join(data, "l4c4.json")]
    for args in (mach + ["-V", fa, "--cluster-polish", "3"], mach + ["--cluster-file", lab, "--cluster-polish", "3"],
                 mach + ["-d", fa, "--cluster-polish", "2"], mach + ["--cluster-reads", fa, "--cluster-polish", "2"],
                 mach + ["-V", fa, "--cluster-polish", "0"], mach + ["-V", fa, "--cluster-file", lab, "--cluster-polish", "-1"],
                 mach + ["-V", fa, "--cluster-file", lab, "--cluster-polish"]):
        r = run(*args)
        assert r.returncode == 1 and r.stdout == b"" and b"--cluster-polish" in r.stderr, args
    assert b"--cluster-polish" in run("--help").stdout
