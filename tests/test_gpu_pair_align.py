"""dnas_align_pairs on the GPU (csrc/pair_align_kernels.hip) against its host statement dnas_align_pairs_host: score bits, op
bytes and status must be identical, whatever the shapes, the band, the batching and the number of devices."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")
BASES = "ACGT"
NOISY = dict(sub=.03, dup=.02, del_open=.02, del_ext=.2)
NOISY_FLAGS = ["--error-sub-prob", ".03", "--error-dup-prob", ".02", "--error-del-open", ".02", "--error-del-ext", ".2"]

SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (63, 63), (64, 64), (65, 60), (129, 140), (70, 40), (40, 70))
BANDS = (-1, 0, 3, 8, 70)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _related(rng, a, O):
    """A read of exactly O bases that the model explains from a: substitutions, short deletions and tandem copies, then the
    length made up by a deletion block or tandem copies where the shape asks for another length."""
    from test_pair_align_cpu import edited
    b = edited(rng, a, 3) if a else ""
    while len(b) > O:                               # too long: a block goes
        at = rng.randrange(len(b))
        b = b[:at] + b[at + min(len(b) - O, 9):]
    while len(b) < O:                               # too short: tandem copies (or, from nothing, anything)
        if not b:
            b = _rand(rng, O)
            break
        at = rng.randrange(len(b))
        k = min(rng.randint(1, 3), at + 1, O - len(b))
        b = b[:at + 1] + b[at + 1 - k:at + 1] + b[at + 1:]
    return b


def _models(da):
    from test_pair_align_cpu import make_params
    zero = [1. / 12] * 13
    zero[4] = 0.
    return (("P0", make_params(da, [])),
            ("P1", make_params(da, [1.], pTanDup=.1)),
            ("P6", da.MutatorParams.fromFlags(**NOISY)),
            ("P13-zero", make_params(da, zero, pDelOpen=.05, pTanDup=.1)),
            ("P6-no-transversion", make_params(da, [1. / 6] * 6, pTransversion=0.)),
            ("P6-global-exact", da.MutatorParams.fromFlags(sub=0., dup=0., del_open=0., global_=True)))


def _shape_list(seed):
    """Every shape of SHAPES with a related and an unrelated read, and a few more related pairs: 35 pairs."""
    rng = random.Random(seed)
    ins, outs = [], []
    for I, O in SHAPES:
        a = _rand(rng, I)
        ins += [a, a]
        outs += [_related(rng, a, O), _rand(rng, O)]
    for I in (5, 17, 62, 63, 64, 65, 100, 127, 128, 130, 150, 190, 33, 96, 200):
        a = _rand(rng, I)
        ins.append(a)
        outs.append(_related(rng, a, max(0, I + rng.randint(-4, 4))))
    return ins, outs


def _same(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got.status, want.status), (got.status, want.status)
    assert np.array_equal(got.score.view(np.uint64), want.score.view(np.uint64)), np.flatnonzero(got.score.view(np.uint64) != want.score.view(np.uint64))
    for i in range(len(want)):
        assert np.array_equal(got.ops[i], want.ops[i]), i


@pytest.fixture(scope="module")
def shape_cases(da):
    """[(name, params, ins, outs, {band: host result})], the host results computed once."""
    out = []
    for k, (name, params) in enumerate(_models(da)):
        ins, outs = _shape_list("gpu-pair-align/%d" % k)
        out.append((name, params, ins, outs, {band: da.alignPairs(params, ins, outs, band=band, host=True) for band in BANDS}))
    return out


def test_every_shape_model_and_band(da, shape_cases, monkeypatch):
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves over 35 pairs: every wave walks several pairs
    pairs = 0
    statuses = set()
    for name, params, ins, outs, want in shape_cases:
        for band in BANDS:
            got = da.alignPairs(params, ins, outs, band=band)
            _same(got, want[band])
            assert got.stats["batches"] == 1 and got.stats["pairs_too_large"] == 0 and got.stats["cells"] > 0
            statuses |= set(int(s) for s in got.status)
        pairs += len(ins)
    assert pairs >= 200 and statuses == {da.lib.ALIGN_OK, da.lib.ALIGN_NO_PATH}
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid as shipped, all models in one list per band
    name, params, ins, outs, want = shape_cases[2]
    for band in (-1, 8):
        _same(da.alignPairs(params, ins * 4, outs * 4, band=band), da.alignPairs(params, ins * 4, outs * 4, band=band, host=True))


def test_boundary_row_beyond_lds(da):
    """Reads of more than 1015 bases: the stripes hand their last row on through HBM instead of LDS."""
    rng = random.Random("gpu-pair-align/long")
    params = da.MutatorParams.fromFlags(**NOISY)
    a = _rand(rng, 1100)
    ins = [a, _rand(rng, 130), a[:200]]
    outs = [_related(rng, a, 1104), _rand(rng, 1100), _related(rng, a[:200], 198)]
    for band in (8, -1):
        _same(da.alignPairs(params, ins, outs, band=band), da.alignPairs(params, ins, outs, band=band, host=True))


def test_batching(da):
    rng = random.Random("gpu-pair-align/batches")
    params = da.MutatorParams.fromFlags(**NOISY)
    ins = [_rand(rng, rng.randint(90, 110)) for _ in range(40)]
    outs = [_related(rng, a, len(a) + rng.randint(-3, 3)) for a in ins]
    want = da.alignPairs(params, ins, outs, band=8, host=True)
    one = da.alignPairs(params, ins, outs, band=8)
    _same(one, want)
    assert one.stats["batches"] == 1
    # a pair's record is 2 stripes x at most 149 steps x 128 bytes: 300 000 bytes hold at most 8 of them
    split = da.alignPairs(params, ins, outs, band=8, arena_bytes=300000)
    _same(split, want)
    assert split.stats["batches"] >= 3 and split.stats["cells"] == one.stats["cells"]
    _same(da.alignPairs(params, ins, outs, band=8, arena_bytes=300000), split)           # the same call again
    # one pair of 2000 bases (32 stripes: 585 000 bytes) among them
    big = _rand(rng, 2000)
    ins2, outs2 = ins[:7] + [big] + ins[7:], outs[:7] + [_related(rng, big, 2000)] + outs[7:]
    got = da.alignPairs(params, ins2, outs2, band=8, arena_bytes=300000)
    assert got.status[7] == da.lib.ALIGN_TOO_LARGE and len(got.ops[7]) == 0 and np.isnan(got.score[7]) and got.skipped == [7]
    assert got.stats["pairs_too_large"] == 1
    keep = [i for i in range(len(ins2)) if i != 7]
    assert np.array_equal(got.status[keep], want.status) and np.array_equal(got.score[keep].view(np.uint64), want.score.view(np.uint64))
    assert all(np.array_equal(got.ops[i], want.ops[j]) for j, i in enumerate(keep))
    whole = da.alignPairs(params, ins2, outs2, band=8)                                   # with room, the long pair is aligned too
    assert whole.status[7] == da.lib.ALIGN_OK and whole.rows(7)[0].replace("-", "") == big
    empty = da.alignPairs(params, [], [])
    assert len(empty) == 0 and empty.stats["batches"] == 0 and empty.stats["cells"] == 0


def test_viterbi_path_is_in_the_forward_sum(da):
    from synth import synthetic_alignment
    rng = random.Random("gpu-pair-align/estep")
    params = da.MutatorParams.fromFlags(**NOISY)
    rows = [synthetic_alignment(rng, rng.randint(90, 110), sub=.03, dele=.02, dup=.02) for _ in range(24)]
    ins, outs = [r[0][1].replace("-", "") for r in rows], [r[1][1].replace("-", "") for r in rows]
    res = da.alignPairs(params, ins, outs, band=32)
    assert not res.skipped and params.c.n_len == 6
    fb = da.ForwardBackward(res.packed(), device=0)
    for strict in (True, False):
        _, _, per = fb.expectedCounts(params, strict=strict)
        slack = per - (res.score - 1e-6 * np.maximum(1., np.abs(res.score)))
        print("strict" if strict else "loose", "smallest surplus of the forward log-likelihood over the Viterbi score:",
              float(np.min((per - res.score) / np.maximum(1., np.abs(res.score)))))
        assert (slack >= 0).all(), (strict, per, res.score)
    fb.close()


def test_all_devices(da, monkeypatch):
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    rng = random.Random("gpu-pair-align/devices")
    params = da.MutatorParams.fromFlags(**NOISY)
    ins = [_rand(rng, rng.choice([0, 3, 40, 64, 100, 150, 260])) for _ in range(50)]
    outs = [_related(rng, a, max(0, len(a) + rng.randint(-3, 3))) for a in ins]
    one = da.alignPairs(params, ins, outs, band=8, device=0)
    many = da.alignPairs(params, ins, outs, band=8, device=-1)
    _same(many, one)
    _same(many, da.alignPairs(params, ins, outs, band=8, host=True))
    assert many.stats["cells"] == one.stats["cells"] and many.stats["batches"] == 3
    two = da.alignPairs(params, ins[:2], outs[:2], band=8, device=-1)                    # fewer pairs than devices
    _same(two, da.alignPairs(params, ins[:2], outs[:2], band=8, host=True))
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.alignPairs(params, ins, outs, device=-2)


def _fasta(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))


def test_cli(da, tmp_path):
    rng = random.Random("gpu-pair-align/cli")
    params = da.MutatorParams.fromFlags(**NOISY)
    ins = [_rand(rng, rng.randint(30, 90)) for _ in range(12)]
    outs = [_related(rng, a, len(a) + rng.randint(-2, 2)) for a in ins]
    names_in, names_out = ["strand%d" % i for i in range(12)], ["read%d" % i for i in range(11)] + ["strand11"]
    fa, fr, stk = str(tmp_path / "originals.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "pairs.stk")
    _fasta(fa, names_in, ins)
    _fasta(fr, names_out, outs)
    run = lambda args: subprocess.run([BIN, "-v0"] + args, capture_output=True, timeout=300)
    r = run(NOISY_FLAGS + ["--align-pairs", fa, "--align-reads", fr, "--align-band", "16"])
    res = da.alignPairs(params, ins, outs, band=16)
    assert r.returncode == 0 and r.stdout.decode() == res.stockholm(names_in, names_out), r.stderr.decode()
    assert "strand11/read " in r.stdout.decode()
    with open(stk, "wb") as f:
        f.write(r.stdout)
    r = run(NOISY_FLAGS + ["--error-counts", stk])
    counts, _, _ = da.expectedCounts(params, res.packed())
    assert r.returncode == 0 and r.stdout.decode() == da.countsJSON(counts, params.c.n_len), r.stderr.decode()
    # one original with all reads; the default band
    one = str(tmp_path / "one.fa")
    _fasta(one, ["origin"], [ins[0]])
    reads = [_related(rng, ins[0], len(ins[0]) + d) for d in (-1, 0, 2)]
    _fasta(fr, ["r0", "r1", "r2"], reads)
    r = run(NOISY_FLAGS + ["--align-pairs", one, "--align-reads", fr])
    assert r.returncode == 0 and r.stdout.decode() == da.alignPairs(params, [ins[0]], reads).stockholm(["origin"], ["r0", "r1", "r2"])
    # a pair without a path is named and left out; a count mismatch is an error
    r = run(["-l0", "--align-pairs", one, "--align-reads", fr])
    want = da.alignPairs(da.MutatorParams.fromFlags(length=0), [ins[0]], reads)
    assert want.skipped == [2] and r.returncode == 0 and b"r2" in r.stderr and b"r1" not in r.stderr
    assert r.stdout.decode() == want.stockholm(["origin"], ["r0", "r1", "r2"])
    r = run(["--align-pairs", fa, "--align-reads", fr])
    assert r.returncode == 1 and r.stdout == b"" and b"12 originals for 3 reads" in r.stderr
