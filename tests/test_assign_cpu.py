"""Read assignment on the host (dnas_assign_reads_host, csrc/host/assign.cpp) -- no GPU, but for the command line, which has
no host arm (like --align-pairs, it reports that there is no device and exits 2).

The expectation is built here, independently of the library's fold: dnas_align_pairs_host on the expanded (read, candidate,
strand) list gives the item scores, and fold_py below restates the definition of include/dnastore_amd.h over them."""
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
BASES = "ACGT"
NEG = float("-inf")
NOISY = dict(sub=.03, dup=.02, del_open=.02, del_ext=.2)
NOISY_FLAGS = ["--error-sub-prob", ".03", "--error-dup-prob", ".02", "--error-del-open", ".02", "--error-del-ext", ".2"]
BANDS = (-1, 0, 8)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- cases
def models(da):
    """P0, P1, P6, P13 with a zero entry, and the global exact model (no path unless the read is the original)."""
    from test_gpu_pair_align import _models
    keep = ("P0", "P1", "P6", "P13-zero", "P6-global-exact")
    return [(name, params) for name, params in _models(da) if name in keep]


def shape_pool(da):
    """K = 7 originals of 0, 1, 63, 64, 65, 130 nt and a duplicate of the 64-nt one; 24 reads: related reads of several
    originals (every other one reverse-complemented), exact copies, two unrelated reads and an empty one."""
    from test_pair_align_cpu import edited
    rng = random.Random("assign/shapes")
    originals = [_rand(rng, n) for n in (0, 1, 63, 64, 65, 130)]
    originals.append(originals[3])
    reads = []
    for k in (2, 3, 4, 5, 2, 3, 4, 5, 5, 5):
        reads += [edited(rng, originals[k], 3), originals[k]]
    reads.append(originals[1])
    reads = [da.reverse_complement(r) if i % 2 else r for i, r in enumerate(reads)]
    reads += [_rand(rng, 70), _rand(rng, 130), ""]
    assert len(originals) == 7 and len(reads) == 24
    return originals, reads


def planted_pool(da, seed="assign/planted"):
    """K = 12 originals of 120 nt; 48 reads, each edited(rng, a, 3) of a known original, a known half reverse-complemented."""
    from test_pair_align_cpu import edited
    rng = random.Random(seed)
    originals = [_rand(rng, 120) for _ in range(12)]
    truth = [(rng.randrange(12), i % 2) for i in range(48)]
    reads = [edited(rng, originals[k], 3) for k, _ in truth]
    reads = [da.reverse_complement(r) if s else r for r, (_, s) in zip(reads, truth)]
    return originals, reads, truth


# ------------------------------------------------------------------------------------------------ the definition, restated
def item_list(K, n_reads, strands, candidates=None):
    """[(read, original, strand)] in item order."""
    per = {"forward": (0,), "reverse": (1,), "both": (0, 1)}[strands]
    return [(r, k, s) for r in range(n_reads) for k in (candidates[r] if candidates is not None else range(K)) for s in per]


def fold_py(items, scores, n_reads):
    """The outputs as include/dnastore_amd.h defines them, from every item's score."""
    out = []
    for r in range(n_reads):
        mine = [(sc, k, s) for (rr, k, s), sc in zip(items, scores) if rr == r]
        best, orig, strand = NEG, -1, 0
        for sc, k, s in mine:
            if sc > best:
                best, orig, strand = sc, k, s
        second = max([sc for sc, k, _ in mine if k != orig] + [NEG]) if orig >= 0 else NEG
        status = 2 if not mine else (1 if orig < 0 else 0)
        out.append((orig, strand, best, second, status))
    return out


def expected(da, params, originals, reads, band, strands="both", candidates=None):
    """-> (item scores, fold_py's rows) through alignPairs(host=True) on the expanded list."""
    items = item_list(len(originals), len(reads), strands, candidates)
    ins = [originals[k] for _, k, _ in items]
    outs = [da.reverse_complement(reads[r]) if s else reads[r] for r, _, s in items]
    scores = da.alignPairs(params, ins, outs, band=band, host=True).score if items else np.zeros(0)
    return items, scores, fold_py(items, scores, len(reads))


def same_as_expected(res, items, scores, rows):
    assert np.array_equal(_bits(np.concatenate(res.item_scores)) if len(scores) else np.zeros(0, np.uint64), _bits(scores))
    assert [int(x) for x in res.original] == [r[0] for r in rows]
    assert [int(x) for x in res.strand] == [r[1] for r in rows]
    assert np.array_equal(_bits(res.score), _bits([r[2] for r in rows]))
    assert np.array_equal(_bits(res.second), _bits([r[3] for r in rows]))
    assert [int(x) for x in res.status] == [r[4] for r in rows]


# ---------------------------------------------------------------------------------------------------------------- tests
def test_items_match_the_host_aligner(da):
    originals, reads = shape_pool(da)
    statuses = set()
    for name, params in models(da):
        for band in BANDS:
            res = da.assignReads(params, originals, reads, band=band, strands="both", host=True, item_scores=True)
            assert res.stats is None and [len(x) for x in res.item_scores] == [14] * 24
            same_as_expected(res, *expected(da, params, originals, reads, band))
            statuses |= set(int(s) for s in res.status)
            if name == "P6" and band == 8:                       # the related reads find their original and their strand
                assert [int(x) for x in res.original[:8:2]] == [2, 3, 4, 5] and list(res.strand[:20]) == [0, 1] * 10
    assert statuses == {da.lib.ASSIGN_OK, da.lib.ASSIGN_NO_PATH}
    # one strand only
    name, params = models(da)[2]
    for strands in ("forward", "reverse"):
        res = da.assignReads(params, originals, reads, band=8, strands=strands, host=True, item_scores=True)
        same_as_expected(res, *expected(da, params, originals, reads, 8, strands))
        assert set(res.strand[res.original >= 0]) == {0 if strands == "forward" else 1}


def test_tie_break_and_runner_up(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("assign/ties")
    originals = [_rand(rng, 40) for _ in range(6)]
    originals[5] = originals[2]
    res = da.assignReads(params, originals, [originals[2]], band=8, host=True)
    assert res.original[0] == 2 and res.strand[0] == 0 and _bits(res.second)[0] == _bits(res.score)[0] and res.margin[0] == 0
    # a read that is its own reverse complement: both strands score the same, the forward one is first
    half = _rand(rng, 20)
    pal = half + da.reverse_complement(half)
    assert da.reverse_complement(pal) == pal
    res = da.assignReads(params, [_rand(rng, 40), pal], [pal], band=8, host=True, item_scores=True)
    assert res.original[0] == 1 and res.strand[0] == 0 and _bits(res.item_scores[0])[2] == _bits(res.item_scores[0])[3]
    assert res.second[0] < res.score[0] and res.second[0] == max(res.item_scores[0][:2])     # the other strand is no runner-up
    # a single original has no runner-up
    res = da.assignReads(params, [pal], [pal, half], band=8, host=True)
    assert list(res.original) == [0, 0] and (res.second == NEG).all() and (res.margin == np.inf).all()
    # no candidates, no originals, no reads
    res = da.assignReads(params, originals, [pal, half], band=8, candidates=[[], [1]], host=True, item_scores=True)
    assert res.status[0] == da.lib.ASSIGN_NO_CANDIDATES and res.original[0] == -1 and res.score[0] == NEG and res.second[0] == NEG
    assert res.margin[0] == NEG and res.status[1] == da.lib.ASSIGN_OK and res.original[1] == 1 and len(res.item_scores[0]) == 0
    res = da.assignReads(params, [], [pal, ""], host=True)
    assert list(res.status) == [da.lib.ASSIGN_NO_CANDIDATES] * 2 and list(res.original) == [-1, -1]
    res = da.assignReads(params, originals, [], host=True)
    assert len(res) == 0 and res.pairs() == ([], [], [])


def test_candidate_lists(da):
    originals, reads = shape_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    rng = random.Random("assign/candidates")
    cands = [[rng.randrange(7) for _ in range(rng.choice((0, 1, 2, 3, 5)))] for _ in reads]       # duplicates, empty lists
    cands[2], cands[4] = [6, 3, 2], [4, 4]
    full = da.assignReads(params, originals, reads, band=8, host=True)
    for strands in ("both", "forward"):
        res = da.assignReads(params, originals, reads, band=8, strands=strands, candidates=cands, host=True, item_scores=True)
        same_as_expected(res, *expected(da, params, originals, reads, 8, strands, cands))
    assert res.original[2] == 6 and full.original[2] == 3              # the listed order decides between the two copies
    assert res.second[4] == NEG and res.original[4] == 4               # a duplicate of the winner is no other original
    assert any(res.original[i] != full.original[i] for i in range(len(reads)))
    for bad in ([[7]] + [[]] * 23, [[-1]] + [[]] * 23):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.assignReads(params, originals, reads, candidates=bad, host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        from test_pair_align_cpu import make_params
        da.assignReads(make_params(da, [1. / 14] * 14), originals, reads, host=True)
    with pytest.raises(da.DnasError, match="DNAS_E_BAD_BASE"):
        da.assignReads(params, originals, [np.array([0, 4], np.int8)], host=True)


def test_planted_truth(da):
    """Every read goes back to the original and the strand it was made from, with a positive margin.  Checked with the host
    statement over the seeds assign/planted and assign/planted/0 .. 4 before this one was fixed: all met it, the smallest margin
    seen was above 200 nats (an unrelated 120-mer scores far below a read with three edits)."""
    originals, reads, truth = planted_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    res = da.assignReads(params, originals, reads, band=16, strands="both", host=True)
    assert [(int(k), int(s)) for k, s in zip(res.original, res.strand)] == truth
    assert (res.status == da.lib.ASSIGN_OK).all() and (res.margin > 0).all()
    print("smallest margin:", float(res.margin.min()))
    ins, outs, kept = res.pairs()
    assert kept == list(range(48)) and all(np.array_equal(a, da.tokenize(originals[k])) for a, (k, _) in zip(ins, truth))
    al = da.alignPairs(params, ins, outs, band=16, host=True)
    assert np.array_equal(_bits(al.score), _bits(res.score))            # the assignment's score is the alignment's
    assert res.pairs(min_margin=float(np.sort(res.margin)[10]))[2] == [i for i in range(48) if res.margin[i] >= np.sort(res.margin)[10]]


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))


@pytest.mark.gpu
def test_cli(da, tmp_path):
    originals, reads, truth = planted_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    names_o, names_r = ["strand%d" % k for k in range(12)], ["read%d" % i for i in range(48)]
    fo, fr, stk = str(tmp_path / "library.fa"), str(tmp_path / "pool.fa"), str(tmp_path / "pairs.stk")
    _fasta(fo, names_o, originals)
    _fasta(fr, names_r, reads)
    run = lambda args: subprocess.run([BIN, "-v0"] + NOISY_FLAGS + args, capture_output=True, timeout=300)
    base = ["--assign-reads", fr, "--assign-originals", fo, "--align-band", "16"]
    for strands in ("both", "forward"):
        r = run(base + ["--assign-strands", strands])
        assert r.returncode == 0, r.stderr.decode()
        res = da.assignReads(params, originals, reads, band=16, strands=strands)
        lines = [l.split("\t") for l in r.stdout.decode().splitlines()]
        assert len(lines) == 48
        for i, (name, orig, strand, score, margin) in enumerate(lines):
            assert name == names_r[i] and orig == (names_o[res.original[i]] if res.original[i] >= 0 else "*")
            assert strand == "-+"[int(res.strand[i] == 0)] and float(score) == res.score[i] and float(margin) == res.margin[i]
        if strands == "both":
            assert [l[1] for l in lines] == [names_o[k] for k, _ in truth]
    assert run(base).stdout == r.stdout                         # forward is the default
    # the database --fit-error reads: the kept reads, turned round where the strand says so, aligned to their originals
    r = run(base + ["--assign-strands", "both", "--assign-stockholm"])
    res = da.assignReads(params, originals, reads, band=16)
    ins, outs, kept = res.pairs()
    assert kept == list(range(48))
    want = da.alignPairs(params, ins, outs, band=16)
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout.decode() == want.stockholm([names_o[k] for k, _ in truth], names_r)
    with open(stk, "wb") as f:
        f.write(r.stdout)
    fit = run(["--fit-error", stk])
    assert fit.returncode == 0 and fit.stdout.decode() == da.paramsJSON(da.baumWelchParams(params, want.packed())[0])
    # a margin threshold leaves reads out and names them
    cut = float(np.sort(res.margin[:48])[5])
    r = run(base + ["--assign-strands", "both", "--assign-stockholm", "--assign-min-margin", repr(cut)])
    keep = [i for i in range(48) if res.margin[i] >= cut]
    assert r.returncode == 0 and len(keep) == 43 and r.stdout.count(b"//\n") == 43
    assert all((("read%d:" % i).encode() in r.stderr) == (i not in keep) for i in range(48))
    # without duplications (-l0) a read longer than every original has no path: unassigned, named and left out
    fo2, fr2 = str(tmp_path / "two.fa"), str(tmp_path / "three.fa")
    _fasta(fo2, ["x", "y"], ["ACGTACGT", "TTGCA"])
    _fasta(fr2, ["long", "short", "turned"], ["ACGTACGTA", "ACGTAGT", "TGCAA"])
    small = ["-l0", "--assign-reads", fr2, "--assign-originals", fo2, "--assign-strands", "both"]
    r = run(small)
    res = da.assignReads(da.MutatorParams.fromFlags(length=0, **NOISY), ["ACGTACGT", "TTGCA"], ["ACGTACGTA", "ACGTAGT", "TGCAA"])
    lines = [l.split("\t") for l in r.stdout.decode().splitlines()]
    assert r.returncode == 0 and list(res.original) == [-1, 0, 1] and list(res.status) == [da.lib.ASSIGN_NO_PATH, 0, 0]
    assert lines[0] == ["long", "*", "+", "-inf", "-inf"] and lines[1][:3] == ["short", "x", "+"] and lines[2][:3] == ["turned", "y", "-"]
    assert [float(l[3]) for l in lines[1:]] == list(res.score[1:]) and [float(l[4]) for l in lines[1:]] == list(res.margin[1:])
    r = run(small + ["--assign-stockholm"])
    assert r.returncode == 0 and b"long:" in r.stderr and b"short" not in r.stderr and r.stdout.count(b"//\n") == 2
    for args in (["--assign-reads", fr], base + ["--assign-strands", "sideways"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b""
