"""dnas_trim_reads_host (csrc/host/trim.cpp), the statement of demultiplexing and trimming, against the definition restated in pure
Python (trim_cases.py) -- no GPU.  Equalities throughout: all seven output arrays (the edits are two columns)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import trim_cases as T  # noqa: E402

ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_library_declares_the_trim_calls(da):
    assert {"dnas_trim_reads", "dnas_trim_reads_host"} <= set(da.lib.declared_symbols())
    assert all(hasattr(da.lib.lib(), s) for s in ("dnas_trim_reads", "dnas_trim_reads_host"))


def test_exhaustive_small_cases(da):
    """One pair with F and R over all strings of 1-2 bases from {A, C}, every read of 0..7 bases over {A, C}, every combination of
    the parameters."""
    short = ["".join(p) for n in (1, 2) for p in itertools.product("AC", repeat=n)]
    reads = ["".join(p) for n in range(8) for p in itertools.product("AC", repeat=n)]
    assert len(short) == 6 and len(reads) == 255
    for F, R in itertools.product(short, short):
        for max_offset, permille, anchors, min_payload in itertools.product((0, 2, -1), (0, 500, 1000), ("both", "either"), (0, 2)):
            options = dict(max_offset=max_offset, anchors=anchors, min_payload=min_payload)
            got = T.arrays(da.trimReads([(F, R)], reads, max_edit_permille=permille, host=True, **options))
            T.assert_same(got, T.trim_pool_py([(F, R)], reads, permille=permille, **options), (F, R, max_offset, permille, anchors, min_payload))


SHAPE_GRID = [(8, 250), (-1, 250), (0, 1000), (8, 0)]


@pytest.mark.parametrize("max_offset,permille", SHAPE_GRID)
def test_shape_pool(da, max_offset, permille):
    primers, reads = T.shape_pool()
    assert len(primers) == 7 and sorted({len(p) for pr in primers for p in pr}) == [1, 2, 7, 8, 9, 20, 24, 25, 63, 64]
    assert primers[3] == primers[0] and primers[4][1] == T.rc(primers[4][0])
    assert {0, 1, 63, 64, 65, 130} <= {len(r) for r in reads}
    for anchors, min_payload in itertools.product(("both", "either"), (0, 10)):
        options = dict(max_offset=max_offset, anchors=anchors, min_payload=min_payload)
        got = T.arrays(da.trimReads(primers, reads, max_edit_permille=permille, host=True, **options))
        T.assert_same(got, T.trim_pool_py(primers, reads, permille=permille, **options), (max_offset, permille, anchors, min_payload))


def test_shape_pool_holds_what_it_says(da):
    """Every pair but the duplicate wins somewhere, the duplicate ties as the runner-up, both strands and every status occur, the
    later of two exact occurrences wins, and a read lacking R is accepted under `either` only."""
    primers, reads = T.shape_pool()
    f0, r0 = primers[0]
    both = da.trimReads(primers, reads, host=True)
    assert set(both.pair.tolist()) == {-1, 0, 1, 2, 4, 5, 6}
    anywhere = da.trimReads(primers, reads, max_offset=-1, host=True)
    assert set(both.strand[both.pair >= 0].tolist()) == {0, 1} and set(anywhere.status.tolist()) == {0, 1, 2}
    exact = reads.index(f0 + r0)
    assert (both.pair[exact], both.begin[exact], both.end[exact], both.second[exact]) == (0, 20, 20, 0)       # pair 3 ties, k = 0 wins
    assert da.trimReads(primers[:1], [f0 + r0[3:]], host=True).status[0] == da.lib.TRIM_TOO_SHORT           # F and R overlap by 3
    palin = next(i for i in range(len(reads)) if both.pair[i] == 4 and both.edits[i].tolist() == [0, 0])
    assert both.strand[palin] == 0 and both.strand[reads.index(T.rc(reads[palin]))] == 0                          # R = rc(F): strand 0
    twice = next(i for i, r in enumerate(reads) if r.startswith(f0 + f0))
    assert both.begin[twice] == 20
    assert anywhere.begin[twice] == 40
    far = [i for i, r in enumerate(reads) if r[9:29] == f0]                                                     # 9 junk bases
    assert far and all(anywhere.pair[i] == 0 for i in far)
    assert all(both.pair[i] != 0 for i in far)
    no_r = next(i for i, r in enumerate(reads) if r[4:24] == f0 and r0 not in r)
    either = da.trimReads(primers[:1], reads[no_r:no_r + 1], anchors="either", host=True)   # (in the pool ("G", "TC") is cheaper)
    assert both.pair[no_r] != 0 and (either.pair[0], either.edits[0].tolist(), either.begin[0], either.end[0]) == (0, [0, -1], 24, 64)
    assert either.total[0] == 0 + 250 * 20 // 1000 + 1


def test_invalid_arguments(da):
    reads, ok = ["ACGTACGT"], [("ACG", "TTG")]
    trim = lambda primers=ok, reads=reads, **kw: da.trimReads(primers, reads, host=True, **kw)
    for bad in ([("", "A")], [("A", "")], [("A" * 65, "A")], [("A", "C" * 65)]):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            trim(bad)
    for kw in (dict(max_edit_permille=-1), dict(max_edit_permille=1001), dict(max_offset=-2), dict(min_payload=-1)):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            trim(**kw)
    with pytest.raises(ValueError):
        trim(anchors="one")
    L = da.lib.lib()
    seqs, off, out = np.zeros(8, np.int8), np.array([0, 3, 6], np.int64), np.zeros(8, np.int32)
    roff, u8 = np.array([0, 8], np.int64), np.zeros(8, np.uint8)
    args = lambda anchors=0, pseqs=seqs.ctypes.data, rseqs=seqs.ctypes.data, pair=out.ctypes.data: (
        1, pseqs, off.ctypes.data, 1, rseqs, roff.ctypes.data, 8, 250, anchors, 0, pair, u8.ctypes.data, out.ctypes.data, out.ctypes.data,
        out.ctypes.data, out.ctypes.data, u8.ctypes.data)
    assert L.dnas_trim_reads_host(*args()) == 0
    for bad in (args(anchors=2), args(anchors=-1), args(pseqs=None), args(rseqs=None), args(pair=None)):
        assert L.dnas_trim_reads_host(*bad) == -1
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        trim(reads=[np.array([0, 4], np.int8)])
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        trim([(np.array([5], np.int8), "A")])
    # the two valid empty calls
    none = trim(reads=[])
    assert len(none) == 0 and none.payloads() == [] and none.kept() == []
    bare = trim([], reads=["ACGT", ""])
    assert bare.pair.tolist() == [-1, -1] and bare.status.tolist() == [da.lib.TRIM_NO_ANCHOR] * 2 and bare.payloads() == [None, None]
    assert bare.second.tolist() == [-1, -1] and bare.edits.tolist() == [[-1, -1]] * 2 and bare.begin.tolist() == bare.end.tolist() == [0, 0]


@pytest.fixture(scope="module")
def planted():
    return T.planted_pool()


def test_planted_truth(da, planted):
    primers, reads, truth = planted
    assert len(reads) == 160
    got = da.trimReads(primers, reads, max_offset=8, max_edit_permille=250, anchors="both", min_payload=0, host=True)
    T.assert_same(T.arrays(got), T.trim_pool_py(primers, reads))
    T.planted_conditions(reads, truth, T.arrays(got))
    pay = got.payloads()
    assert all((p is None) == (got.status[i] != 0) for i, p in enumerate(pay))
    assert all(p == T.payload_py(reads[i], [int(getattr(got, f)[i]) for f in T.FIELDS[:4]]) for i, p in enumerate(pay) if p is not None)
    assert got.kept(pair=3) == [i for i in range(160) if got.pair[i] == 3] and got.stats is None
    assert got.kept(min_margin=1) == got.kept()                          # no read has a second pair accepted


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))


def _records(text):
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            out.append([line[1:], ""])
        else:
            out[-1][1] += line
    return out


def test_cli(da, planted, tmp_path):
    primers, reads, truth = planted
    pool, pfile = str(tmp_path / "pool.fa"), str(tmp_path / "primers.fa")
    _fasta(pool, ["read%d" % i for i in range(len(reads))], reads)
    _fasta(pfile, [n for k in range(8) for n in ("F%d" % k, "R%d" % k)], [p for pr in primers for p in pr])
    run = lambda args: subprocess.run([BIN, "-v0", "--trim-reads", pool] + args, capture_output=True, timeout=60)
    want = da.trimReads(primers, reads, host=True)
    pay = want.payloads()
    done = run(["--trim-primers", pfile])
    assert done.returncode == 0, done.stderr
    recs = _records(done.stdout.decode())
    kept = want.kept()
    assert [r[1] for r in recs] == [pay[i] for i in kept]
    assert [r[0] for r in recs] == ["read%d primer=F%d strand=%s edits=%d,%d" % (i, want.pair[i], "+-"[want.strand[i]], *want.edits[i])
                                    for i in kept]
    assert b"trimmed" in done.stderr
    one = run(["--trim-primers", pfile, "--trim-select", "F5"])
    assert one.returncode == 0 and [r[1] for r in _records(one.stdout.decode())] == [pay[i] for i in want.kept(pair=5)]
    assert len(want.kept(pair=5)) == 20
    loose = run(["--trim-primers", pfile, "--trim-max-offset", "-1", "--trim-max-edit", "300", "--trim-anchors", "either", "--trim-min-payload", "50"])
    other = da.trimReads(primers, reads, max_offset=-1, max_edit_permille=300, anchors="either", min_payload=50, host=True)
    assert loose.returncode == 0 and [r[1] for r in _records(loose.stdout.decode())] == [p for p in other.payloads() if p is not None]
    odd = str(tmp_path / "odd.fa")
    _fasta(odd, ["F0", "R0", "F1"], ["ACGT", "ACGT", "ACGT"])
    for args in (["--trim-primers", odd], [], ["--trim-primers", pfile, "--trim-anchors", "one"], ["--trim-primers", pfile, "--trim-select", "F9"],
                 ["--trim-primers", pfile, "--trim-max-edit", "1001"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b"" and bad.stderr, args
    assert b"--trim-reads" in subprocess.run([BIN, "--help"], capture_output=True, timeout=60).stdout
