"""Consensus by rescoring on the host (dnas_consensus_score_host, csrc/host/consensus.cpp) -- no GPU.

The expectation is built here, independently of the library's sums and pick: dnas_align_pairs_host on the expanded (candidate,
oriented read) list gives the item scores, and totals_py / pick_py below restate the definition of include/dnastore_amd.h over
them.  Every comparison is an equality; doubles are compared as uint64 bit patterns."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import BANDS, NOISY, _bits, _rand, models  # noqa: E402,F401

NEG = float("-inf")
OK, NO_PATH, NO_CANDIDATES, NO_READS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


# ---------------------------------------------------------------------------------------------------------------- cases
def shape_pool(da):
    """-> (candidates, reads, strands), one list per cluster.  Strands and reads of 0, 1, 63, 64, 65 and 130 nt; clusters of 0, 1,
    2 and 7 reads; 0, 1 and 3 candidates, one a duplicate strand; a read with strand 1 is given reverse-complemented."""
    from test_pair_align_cpu import edited
    rng = random.Random("consensus/shapes")
    s = {n: _rand(rng, n) for n in (0, 1, 63, 64, 65, 130)}
    other = _rand(rng, 130)
    ed = lambda a: edited(rng, a, 3)
    clusters = [
        # 7 reads of one 130-mer, three candidates: the strand, an unrelated one, the strand again
        ([s[130], other, s[130]], [ed(s[130]), s[130], ed(s[130]), ed(s[130]), s[130], ed(s[130]), ed(s[130])], [0, 1, 0, 1, 1, 0, 0]),
        ([s[64]], [ed(s[64]), s[64]], [1, 0]),
        ([], [s[63], s[1]], [0, 1]),                                   # no candidates
        ([s[63], s[65], s[64]], [], []),                               # no reads
        ([], [], []),
        ([s[0], s[1], s[63]], [s[1]], [0]),
        # reads of every length against candidates of 65 and 63 nt (a duplicate first and last)
        ([s[65], s[63], s[65]], [s[0], s[1], s[63], s[64], s[65], s[130], ed(s[65])], [0, 1, 1, 0, 1, 0, 1]),
        ([s[0]], [_rand(rng, 5)], [0]),                                # an empty strand explains no read: no path
        ([s[1]], [s[0]], [1]),
        ([s[0], s[63], s[1]], [ed(s[63]), s[63]], [0, 0]),             # the empty candidate is out, the others are not
        ([s[63], s[64], s[65]], [ed(s[64]), ed(s[64])], [1, 1]),
    ]
    cands = [c for c, _, _ in clusters]
    strands = [st for _, _, st in clusters]
    reads = [[da.reverse_complement(r) if f else r for r, f in zip(rs, st)] for _, rs, st in clusters]
    assert sorted(set(len(r) for r in reads)) == [0, 1, 2, 7] and sorted(set(len(c) for c in cands)) == [0, 1, 3]
    return cands, reads, strands


# ------------------------------------------------------------------------------------------------ the definition, restated
def item_list(cands, reads):
    """[(cluster, candidate, read)] in item order: candidate-major inside a cluster."""
    return [(c, j, i) for c in range(len(reads)) for j in range(len(cands[c])) for i in range(len(reads[c]))]


def totals_py(cands, reads, items, scores):
    """Per cluster the list of its candidates' totals: 0.0, then every item score added in read order."""
    totals = [[0.0] * len(cs) for cs in cands]
    for (c, j, _), sc in zip(items, scores):
        totals[c][j] = totals[c][j] + float(sc)
    return totals


def pick_py(totals, n_reads):
    """(winner, total, second, status) per cluster as include/dnastore_amd.h defines them."""
    out = []
    for ts, n in zip(totals, n_reads):
        if not ts:
            out.append((-1, NEG, NEG, NO_CANDIDATES))
            continue
        if n == 0:
            out.append((-1, NEG, NEG, NO_READS))
            continue
        best, winner = NEG, -1
        for j, t in enumerate(ts):
            if t > best:
                best, winner = t, j
        if winner < 0:
            out.append((-1, NEG, NEG, NO_PATH))
        else:
            out.append((winner, best, max([t for j, t in enumerate(ts) if j != winner] + [NEG]), OK))
    return out


def expected(da, params, cands, reads, strands, band):
    """-> (totals per cluster, pick_py's rows) through alignPairs(host=True) on the expanded list."""
    items = item_list(cands, reads)
    ins = [cands[c][j] for c, j, _ in items]
    outs = [da.reverse_complement(reads[c][i]) if strands is not None and strands[c][i] else reads[c][i] for c, _, i in items]
    scores = da.alignPairs(params, ins, outs, band=band, host=True).score if items else np.zeros(0)
    totals = totals_py(cands, reads, items, scores)
    return totals, pick_py(totals, [len(r) for r in reads])


def same_as_expected(res, totals, rows):
    assert len(res) == len(rows) and len(res.totals) == len(totals)
    for got, want in zip(res.totals, totals):
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert [int(x) for x in res.winner] == [r[0] for r in rows]
    assert np.array_equal(_bits(res.total), _bits([r[1] for r in rows]))
    assert np.array_equal(_bits(res.second), _bits([r[2] for r in rows]))
    assert [int(x) for x in res.status] == [r[3] for r in rows]


# ---------------------------------------------------------------------------------------------------------------- tests
def test_totals_and_winners_match_the_restated_definition(da):
    cands, reads, strands = shape_pool(da)
    statuses = set()
    for name, params in models(da):
        for band in BANDS:
            res = da.consensusScore(params, cands, reads, band=band, read_strand=strands, host=True)
            assert res.stats is None
            same_as_expected(res, *expected(da, params, cands, reads, strands, band))
            statuses |= set(int(x) for x in res.status)
            if name == "P6" and band == 8:                       # the reads find their strand
                assert [int(w) for w in res.winner] == [0, 0, -1, -1, -1, 1, 0, -1, 0, 1, 1]
    assert statuses == {OK, NO_PATH, NO_CANDIDATES, NO_READS}
    # read_strand = None is all forward: other scores than with the strands, the same as with zeros
    name, params = models(da)[2]
    plain = da.consensusScore(params, cands, reads, band=8, host=True)
    same_as_expected(plain, *expected(da, params, cands, reads, None, 8))
    zeros = da.consensusScore(params, cands, reads, band=8, read_strand=[[0] * len(r) for r in reads], host=True)
    same_as_expected(zeros, *expected(da, params, cands, reads, None, 8))
    assert not np.array_equal(_bits(plain.total), _bits(da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True).total))


def test_ties_and_order(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("consensus/ties")
    from test_pair_align_cpu import edited
    a, b = _rand(rng, 40), _rand(rng, 40)
    reads = [edited(rng, a, 2), a, edited(rng, a, 2)]
    # a duplicate strand: the lower index wins, the copy is the runner-up, the margin is 0
    res = da.consensusScore(params, [[b, a, a]], [reads], band=8, host=True)
    assert res.winner[0] == 1 and res.status[0] == OK and _bits(res.second)[0] == _bits(res.total)[0] and res.margin[0] == 0
    assert _bits(res.totals[0])[1] == _bits(res.totals[0])[2] and res.totals[0][0] < res.total[0]
    # the total is the sum of the alignments' scores in read order
    al = da.alignPairs(params, [a], reads, band=8, host=True).score
    assert _bits(res.total)[0] == _bits(np.array((0.0 + al[0] + al[1]) + al[2]))[0]
    # a single candidate has no runner-up
    res = da.consensusScore(params, [[a]], [reads], band=8, host=True)
    assert res.winner[0] == 0 and res.second[0] == NEG and res.margin[0] == np.inf
    # a read that is -inf against one candidate takes that candidate out, not the others: under the global exact model only
    # the very strand explains a read, and no candidate explains two different reads
    exact = da.MutatorParams.fromFlags(sub=0., dup=0., del_open=0., global_=True)
    res = da.consensusScore(exact, [[b, a], [a, b]], [[a, a], [a, b]], band=8, host=True)
    assert list(res.winner) == [1, -1] and list(res.status) == [OK, NO_PATH]
    assert res.totals[0][0] == NEG and np.isfinite(res.totals[0][1]) and list(res.totals[1]) == [NEG, NEG]
    assert res.second[0] == NEG and res.total[1] == NEG and res.margin[1] == NEG
    # the empty calls
    res = da.consensusScore(params, [], [], host=True)
    assert len(res) == 0
    res = da.consensusScore(params, [[], [a]], [[a], []], host=True)
    assert list(res.status) == [NO_CANDIDATES, NO_READS] and list(res.winner) == [-1, -1] and list(res.totals[1]) == [0.0]
    assert list(res.total) == [NEG, NEG] and list(res.second) == [NEG, NEG]


def _raw(da, n_clusters, cand_off, cl_cand, read_off, cl_read, cand_seqs=None, read_seqs=None, strand=None, band=8, params=None):
    """dnas_consensus_score_host on hand-made arrays -> the return code."""
    params = params or da.MutatorParams.fromFlags(**NOISY)
    i64 = lambda x: np.array(x, dtype=np.int64)
    cand_off, cl_cand, read_off, cl_read = i64(cand_off), i64(cl_cand), i64(read_off), i64(cl_read)
    cand_seqs = np.zeros(64, np.int8) if cand_seqs is None else np.array(cand_seqs, np.int8)
    read_seqs = np.zeros(64, np.int8) if read_seqs is None else np.array(read_seqs, np.int8)
    strand = None if strand is None else np.array(strand, np.uint8)
    winner, status = np.zeros(8, np.int64), np.zeros(8, np.uint8)
    total, second = np.zeros(8), np.zeros(8)
    return da.lib.lib().dnas_consensus_score_host(
        ctypes.byref(params.c), band, n_clusters, len(cand_off) - 1, cand_seqs.ctypes.data, cand_off.ctypes.data, cl_cand.ctypes.data,
        len(read_off) - 1, read_seqs.ctypes.data, read_off.ctypes.data, strand.ctypes.data if strand is not None else None,
        cl_read.ctypes.data, winner.ctypes.data, total.ctypes.data, second.ctypes.data, status.ctypes.data, None)


def test_argument_errors(da):
    E_INVALID, E_BAD_BASE, E_UNSUPPORTED = -1, -6, -9
    good = dict(cand_off=[0, 4, 8], cl_cand=[0, 1, 2], read_off=[0, 3, 6, 9], cl_read=[0, 2, 3])
    assert _raw(da, 2, **good) == 0
    for key, bad in (("cand_off", [0, 5, 4]), ("cand_off", [1, 4, 8]), ("read_off", [0, 4, 3, 9]), ("read_off", [2, 3, 6, 9]),
                     ("cl_cand", [0, 2, 1]), ("cl_cand", [0, 1, 1]), ("cl_cand", [1, 1, 2]), ("cl_read", [0, 3, 2]),
                     ("cl_read", [0, 2, 4]), ("cl_read", [1, 2, 3])):
        assert _raw(da, 2, **dict(good, **{key: bad})) == E_INVALID, (key, bad)
    assert _raw(da, 2, strand=[0, 1, 2], **good) == E_INVALID
    assert _raw(da, 2, band=-2, **good) == E_INVALID
    assert _raw(da, 2, cand_seqs=[0, 1, 2, 4] + [0] * 8, **good) == E_BAD_BASE
    assert _raw(da, 2, read_seqs=[0] * 8 + [4], **good) == E_BAD_BASE
    assert _raw(da, 2, read_seqs=[0] * 9 + [4], **good) == 0             # (beyond the last read)
    from test_pair_align_cpu import make_params
    assert _raw(da, 2, params=make_params(da, [1. / 14] * 14), **good) == E_UNSUPPORTED
    # ... and through the Python layer
    params = da.MutatorParams.fromFlags(**NOISY)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.consensusScore(params, [[np.array([0, 4], np.int8)]], [["ACGT"]], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.consensusScore(make_params(da, [1. / 14] * 14), [["ACGT"]], [["ACGT"]], host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.consensusScore(params, [["ACGT"]], [["ACGT"]], band=-2, host=True)


def test_cli_usage(da, tmp_path):
    """What the command line decides before it needs a GPU: --cluster-file goes with -V only, --cluster-table with
    --cluster-file only, and a label file of another length than the FASTA exits 1 with nothing on stdout."""
    import subprocess
    root = os.path.dirname(_HERE)
    exe = os.path.join(root, "dnastore_amd", "bin", "dnastore")
    data = os.path.join(root, "tests", "golden", "ref_data")
    run = lambda *args: subprocess.run([exe, "-v0"] + list(args), capture_output=True, timeout=120)
    fa, lab = str(tmp_path / "reads.fa"), str(tmp_path / "labels.txt")
    with open(fa, "w") as f:
        f.write(">r0\nACGTACGT\n>r1\nACGTACGA\n>r2\nTTGCAAGT\n")
    with open(lab, "w") as f:
        f.write("x\ny\n")
    mach = ["-L", os.path.join(data, "l4c4.json")]
    r = run(*mach, "-V", fa, "--cluster-file", lab, "--both-strands")
    assert r.returncode == 1 and r.stdout == b"" and b"2 cluster names for 3 reads" in r.stderr
    r = run(*mach, "-V", fa, "--cluster-file", str(tmp_path / "missing.txt"))
    assert r.returncode == 1 and r.stdout == b""
    for args in (mach + ["--cluster-file", lab], mach + ["-d", fa, "--cluster-file", lab], mach + ["-E", "HELLO", "--cluster-file", lab],
                 mach + ["-V", fa, "--cluster-table"]):
        r = run(*args)
        assert r.returncode == 1 and r.stdout == b"" and b"cluster" in r.stderr, args
    out = run("--help").stdout
    assert b"--cluster-file" in out and b"--cluster-table" in out
    assert {"dnas_consensus_score", "dnas_consensus_score_host", "dnas_viterbi_clusters", "dnas_model_device"} <= set(da.lib.declared_symbols())
