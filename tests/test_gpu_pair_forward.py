"""The forward pair-HMM score on the GPU (paForwardScorePair of csrc/pair_forward_device.h behind dnas_pair_likelihoods and the
forward mode of dnas_consensus_score_ex / dnas_viterbi_clusters_scored) against its host statement.

Every comparison with the host statement is an equality of uint64 bit patterns with host=True in table mode; test D holds the
GPU to the exact references of pair_forward_cases.py directly, under the derived bound of the table."""
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

import pair_forward_cases as C  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402
from test_assign_cpu import BANDS as CONSENSUS_BANDS, NOISY, _rand, models as consensus_models  # noqa: E402
from test_cluster_cpu import band_cells, source_constant  # noqa: E402
from test_consensus_cpu import OK, NO_PATH, NO_CANDIDATES, NO_READS, item_list, shape_pool  # noqa: E402
from test_gpu_consensus import BAND, MACHINE, PLANTED, PLANTED_FLAGS, planted_pool  # noqa: E402
from test_gpu_pair_align import SHAPES, _models, _related  # noqa: E402
from test_gpu_pair_hmm_edges import crossover_pairs, dealt_to_four_waves, in_hbm, transitions  # noqa: E402

FORWARD_BANDS = (-1, 0, 1, 32)
# I in {0, 1, 63, 64, 65, 130}: one stripe, a boundary row written and never read, then two and three stripes; O includes 0
FORWARD_SHAPES = SHAPES + ((1, 0), (1, 4), (63, 0), (64, 70), (65, 65), (130, 127), (130, 0))
LDS_COLS = (source_constant("pair_align_device.h", "kPaLdsDoubles") - 16) // 2
TOP = LDS_COLS - 1                                      # the longest read whose boundary row stays in LDS


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def forward_models(da):
    """_models of test_gpu_pair_align.py and three more, so that P covers 0, 1, 2, 3, 6, 7 and 13: both sides of every edge of
    paDispatchKP (KP = 2 up to P = 2, 6 up to P = 6, then 13)."""
    from test_pair_align_cpu import make_params
    more = (("P2", make_params(da, [.7, .3])), ("P3", make_params(da, [.5, .3, .2], pTanDup=.08)),
            ("P7", make_params(da, [.3, .2, .15, .15, .1, .05, .05], pTanDup=.06)))
    out = tuple(_models(da)) + more
    assert sorted(set(p.c.n_len for _, p in out)) == [0, 1, 2, 3, 6, 7, 13]
    return out


def shape_list(seed):
    """Every shape of FORWARD_SHAPES with a related and an unrelated read; every third read is given reverse-complemented and
    flagged: (originals, reads, read_strand)."""
    rng = random.Random(seed)
    ins, outs = [], []
    for I, O in FORWARD_SHAPES:
        a = _rand(rng, I)
        ins += [a, a]
        outs += [_related(rng, a, O), _rand(rng, O)]
    strand = [int(i % 3 == 1) for i in range(len(ins))]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    outs = ["".join(comp[c] for c in reversed(b)) if s else b for b, s in zip(outs, strand)]
    return ins, outs, strand


def same_bits(got, want):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))


# ------------------------------------------------------------------------------------------------ A. shapes, models and bands
@pytest.fixture(scope="module")
def shape_cases(da):
    """[(name, params, ins, outs, strand, {band: host result})], the host results computed once."""
    out = []
    for k, (name, params) in enumerate(forward_models(da)):
        ins, outs, strand = shape_list("gpu-pair-forward/%d" % k)
        out.append((name, params, ins, outs, strand,
                    {band: da.pairLikelihoods(params, ins, outs, band=band, read_strand=strand, host=True) for band in FORWARD_BANDS}))
    return out


def test_every_shape_model_and_band(da, shape_cases, monkeypatch):
    assert {I for I, _ in FORWARD_SHAPES} >= {0, 1, 63, 64, 65, 130} and 0 in {O for _, O in FORWARD_SHAPES}
    n = 2 * len(FORWARD_SHAPES)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves: every wave walks several pairs
    monkeypatch.setenv("DNAS_FORWARD_CHUNK", "7")          # a prime: launches of 7 pairs and a ragged last one
    finite = no_path = 0
    for name, params, ins, outs, strand, want in shape_cases:
        for band in FORWARD_BANDS:
            got = da.pairLikelihoods(params, ins, outs, band=band, read_strand=strand)
            same_bits(got, want[band])
            st = da.pairLikelihoods.last_stats
            assert st["items"] == n and st["chunks"] == -(-n // 7) and st["score_ms"] > 0
            assert st["cells"] == sum(band_cells(len(a), len(b), band) for a, b in zip(ins, outs))
            assert not np.isnan(got).any()
            finite += int(np.isfinite(got).sum())
            no_path += int((got == NEG).sum())
    assert finite >= 400 and no_path >= 50
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the chunk as shipped
    monkeypatch.delenv("DNAS_FORWARD_CHUNK")
    for name, params, ins, outs, strand, want in shape_cases:
        for band in FORWARD_BANDS:
            same_bits(da.pairLikelihoods(params, ins, outs, band=band, read_strand=strand), want[band])
            assert da.pairLikelihoods.last_stats["chunks"] == 1
    name, params, ins, outs, strand, want = shape_cases[2]      # no strand array: every read as given
    same_bits(da.pairLikelihoods(params, ins, outs, band=32), da.pairLikelihoods(params, ins, outs, band=32, host=True))
    empty = da.pairLikelihoods(params, [], [])
    assert empty.shape == (0,) and da.pairLikelihoods.last_stats["chunks"] == 0


# ------------------------------------------------------------------------------------------------ B. the LDS / HBM crossover
@pytest.mark.parametrize("name", ("P2", "P6", "P13-zero"))
def test_the_lds_hbm_crossover(da, monkeypatch, name):
    """The 26 pairs around O = TOP, the longest read whose boundary row stays in LDS, dealt so that under one work-group every
    wave alternates between a row in LDS and one in its HBM scratch, and meets a shorter HBM row after a longer one."""
    from test_cluster_cpu import cluster_models
    params = dict(cluster_models(da))[name]
    full = dealt_to_four_waves(crossover_pairs())
    assert len(full) == 26 and max(len(b) for _, b, _ in full) == TOP + 2 and sum(in_hbm(p) for p in full) == 13
    for w in range(4):
        assert transitions(full[w::4]) == {"LDS>HBM", "HBM>LDS", "HBM>shorter HBM"}, w
    ins, outs, related = [p[0] for p in full], [p[1] for p in full], np.array([p[2] for p in full])
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "1")
    for band in (-1, 8):
        want = da.pairLikelihoods(params, ins, outs, band=band, host=True)
        assert np.isfinite(want[related]).all()
        same_bits(da.pairLikelihoods(params, ins, outs, band=band), want)
        assert da.pairLikelihoods.last_stats["cells"] == sum(band_cells(len(a), len(b), band) for a, b in zip(ins, outs))


# ------------------------------------------------------------------------------------------------ C. devices
def test_all_devices(da, monkeypatch):
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    rng = random.Random("gpu-pair-forward/devices")
    params = da.MutatorParams.fromFlags(**NOISY)
    ins = [_rand(rng, rng.choice([0, 3, 40, 64, 100, 150, 260])) for _ in range(50)]
    outs = [_related(rng, a, max(0, len(a) + rng.randint(-3, 3))) for a in ins]
    strand = [rng.randrange(2) for _ in ins]
    one = da.pairLikelihoods(params, ins, outs, band=8, read_strand=strand, device=0)
    cells = da.pairLikelihoods.last_stats["cells"]
    many = da.pairLikelihoods(params, ins, outs, band=8, read_strand=strand, device=-1)
    st = da.pairLikelihoods.last_stats
    same_bits(many, one)
    same_bits(many, da.pairLikelihoods(params, ins, outs, band=8, read_strand=strand, host=True))
    assert st["cells"] == cells and st["items"] == 50 and st["chunks"] == 3
    two = da.pairLikelihoods(params, ins[:2], outs[:2], band=8, device=-1)                    # fewer pairs than devices
    same_bits(two, da.pairLikelihoods(params, ins[:2], outs[:2], band=8, host=True))
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.pairLikelihoods(params, ins, outs, device=-2)


# ------------------------------------------------------------------------------------------------ D. the exact references
def _inside_table_bounds(name, pairs, want, got):
    worst = 0.
    for i, (a, b) in enumerate(pairs):
        if want[i] == NEG:
            assert got[i] == NEG, (name, i, got[i])
            continue
        lo, hi = C.table_bounds(want[i], len(a), len(b))
        assert lo <= got[i] <= hi, (name, i, got[i], want[i], lo, hi)
        worst = max(worst, abs(got[i] - want[i]))
    return worst


def test_against_the_exact_references(da):
    """Without the host statement in the loop: the tiny and the medium pairs on the GPU against the mpmath forward pass over the
    model's moves (on the tiny pairs test_pair_forward_cpu.py holds that pass to the sum over every enumerated path)."""
    worst, n = 0., 0
    for name, plain, pairs in C.tiny_cases():
        a, b = C.seqs(pairs)
        want = np.array([C.exact_forward(plain, x, y) for x, y in pairs])
        worst = max(worst, _inside_table_bounds(name, pairs, want, da.pairLikelihoods(C.lib_params(da, plain), a, b, band=-1)))
        n += len(pairs)
    print("tiny: largest |GPU - exact| = %.3g nats over %d pairs" % (worst, n))
    assert n == 160
    worst = 0.
    for name, plain, pairs, want in C.medium_exact():
        a, b = C.seqs(pairs)
        for band in C.MEDIUM_BANDS:
            got = da.pairLikelihoods(C.lib_params(da, plain), a, b, band=band)
            worst = max(worst, _inside_table_bounds("%s/band%d" % (name, band), pairs, want[band], got))
    print("medium: largest |GPU - exact| = %.3g nats" % worst)


# ------------------------------------------------------------------------------------------------ E. error-model edges
def test_error_model_edges(da):
    """Probabilities of exactly 0 and 1, of 1e-300 and of 1 - 2^-53 on the GPU: the bits of the host statement, never NaN."""
    n = finite = 0
    for name, plain, pairs in C.boundary_cases():
        p = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        got = da.pairLikelihoods(p, a, b, band=-1)
        assert not np.isnan(got).any(), name
        same_bits(got, da.pairLikelihoods(p, a, b, band=-1, host=True))
        n += 1
        finite += int(np.isfinite(got).sum())
    assert n == 4 * 14 and finite >= 300


# ------------------------------------------------------------------------------------------------ F. consensus, forward mode
def same_consensus(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got.winner, want.winner), (got.winner, want.winner)
    assert np.array_equal(got.status, want.status)
    assert np.array_equal(bits(got.total), bits(want.total)) and np.array_equal(bits(got.second), bits(want.second))
    assert np.array_equal(bits(got.confidence), bits(want.confidence))
    for c, (a, b) in enumerate(zip(got.totals, want.totals)):
        assert np.array_equal(bits(a), bits(b)), (c, a, b)
    for c, (a, b) in enumerate(zip(got.posterior, want.posterior)):
        assert np.array_equal(bits(a), bits(b)), (c, a, b)


def test_consensus_forward_mode(da, monkeypatch):
    cands, reads, strands = shape_pool(da)
    n_items = len(item_list(cands, reads))
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    monkeypatch.setenv("DNAS_CONSENSUS_CHUNK", "37")
    statuses, want = set(), {}
    for name, params in consensus_models(da):
        for band in CONSENSUS_BANDS:
            want[name, band] = da.consensusScore(params, cands, reads, band=band, read_strand=strands, host=True, score="forward")
            got = da.consensusScore(params, cands, reads, band=band, read_strand=strands, score="forward")
            same_consensus(got, want[name, band])
            assert got.stats["chunks"] == -(-n_items // 37) > 1 and got.stats["items"] == n_items and got.stats["cells"] > 0
            statuses |= set(int(s) for s in got.status)
    assert statuses == {OK, NO_PATH, NO_CANDIDATES, NO_READS}
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the chunk as shipped
    monkeypatch.delenv("DNAS_CONSENSUS_CHUNK")
    for name, params in consensus_models(da):
        for band in CONSENSUS_BANDS:
            got = da.consensusScore(params, cands, reads, band=band, read_strand=strands, score="forward")
            same_consensus(got, want[name, band])
            assert got.stats["chunks"] == 1
    # the modes differ, and the default call is the one it was
    name, params = consensus_models(da)[2]
    plain = da.consensusScore(params, cands, reads, band=8, read_strand=strands)
    assert not hasattr(plain, "posterior") and not np.array_equal(bits(plain.total), bits(want[name, 8].total))
    host_plain = da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True)
    assert np.array_equal(bits(plain.total), bits(host_plain.total)) and np.array_equal(plain.winner, host_plain.winner)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        post = np.zeros(4)
        import ctypes
        z = np.zeros(4, np.int64)
        da.lib.check(da.lib.lib().dnas_consensus_score_ex(ctypes.byref(params.c), 8, 0, 0, None, None, z.ctypes.data, 0, None, None, None,
                                                          z.ctypes.data, 0, da.lib.SCORE_VITERBI, None, None, None, None, None,
                                                          post.ctypes.data, None))
    # three devices
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    many = da.consensusScore(params, cands, reads, band=8, read_strand=strands, device=-1, score="forward")
    same_consensus(many, want[name, 8])
    assert many.stats["chunks"] == 3 and many.stats["items"] == n_items


# ------------------------------------------------------------------------------------------------ G. decode_clusters
@pytest.fixture(scope="module")
def planted(da, ref_data):
    machine = da.Machine.fromFile(os.path.join(ref_data, MACHINE))
    messages, reads, labels = planted_pool(da, machine)
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    dec = da.ViterbiDecoder(machine, params, device=0)
    plain = dec.decode_clusters(reads, labels, strands="both", band=BAND)
    fwd = dec.decode_clusters(reads, labels, strands="both", band=BAND, score="forward")
    dec.close()
    return machine, params, messages, reads, labels, plain, fwd


def host_candidates(da, machine, reads, labels, per_read):
    """dnas_viterbi_clusters' step 2 over the decodes of a call -> per cluster (candidate strands, proposers, member reads,
    strands)."""
    out_sym, _, status, strand = per_read
    names = list(dict.fromkeys(labels))
    rows = []
    for n in names:
        members = [i for i, lab in enumerate(labels) if lab == n]
        strands_of, prop = [], []
        for i in members:
            if status[i] != 0 or out_sym[i] == "":
                continue
            try:
                s = machine.encodeSymbols(out_sym[i])
            except da.DnasError:
                continue
            if s not in strands_of:
                strands_of.append(s)
                prop.append(i)
        rows.append((strands_of, prop, [reads[i] for i in members], [int(strand[i]) for i in members]))
    return rows


def test_decode_clusters_forward_mode(da, planted):
    machine, params, messages, reads, labels, plain, fwd = planted
    assert not hasattr(plain, "confidence") and fwd.confidence.shape == (40,)
    for got, want in zip(fwd.per_read, plain.per_read):      # the decode is the default call's
        if isinstance(want, list):
            assert list(got) == list(want)
        else:
            assert np.array_equal(np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8))
    rows = host_candidates(da, machine, reads, labels, plain.per_read)
    host = da.consensusScore(params, [r[0] for r in rows], [r[2] for r in rows], band=BAND, read_strand=[r[3] for r in rows], host=True,
                             score="forward")
    assert [int(x) for x in fwd.n_candidates] == [len(r[0]) for r in rows]
    for c, (cands, prop, _, _) in enumerate(rows):
        assert fwd.status[c] == host.status[c] == OK
        w = int(np.argmax(host.totals[c]))
        assert w == host.winner[c] and fwd.read[c] == prop[w]
        assert bits(fwd.total[c]) == bits(host.totals[c][w]) and bits(fwd.second[c]) == bits(host.second[c])
        assert bits(fwd.confidence[c]) == bits(host.posterior[c][w]) and 0 < fwd.confidence[c] <= 1
    named = sum(s == m for s, m in zip(fwd.symbols, messages))
    print("forward mode names the planted message in %d of 40 clusters (default: %d); confidence from %.6g to %.6g"
          % (named, sum(s == m for s, m in zip(plain.symbols, messages)), fwd.confidence.min(), fwd.confidence.max()))
    assert fwd.stats["items"] == plain.stats["items"] and fwd.stats["chunks"] == 1
    assert not np.array_equal(bits(fwd.total), bits(plain.total))


# ------------------------------------------------------------------------------------------------ H. command line
def test_cli(da, planted, ref_data, tmp_path):
    machine, params, messages, reads, labels, _, _ = planted
    n = 3 * 8
    reads, labels = reads[:n], labels[:n]
    fa, lab = str(tmp_path / "pool.fa"), str(tmp_path / "labels.txt")
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">read%d\n%s\n" % (i, r))
    with open(lab, "w") as f:
        f.write("".join(l + "\n" for l in labels))
    dec = da.ViterbiDecoder(machine, params, device=0)
    plain = dec.decode_clusters(reads, labels, strands="both", band=BAND)
    fwd = dec.decode_clusters(reads, labels, strands="both", band=BAND, score="forward")
    dec.close()
    base = ["-L", os.path.join(ref_data, MACHINE), "-V", fa, "--cluster-file", lab, "--both-strands", "--error-global", "--align-band", str(BAND)]
    run = lambda args: subprocess.run([BIN, "-v0"] + PLANTED_FLAGS + args, capture_output=True, timeout=300)
    r = run(base + ["--cluster-table", "--cluster-score", "forward"])
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    lines = [l.split("\t") for l in r.stdout.decode().splitlines()]
    assert len(lines) == 8
    for c, (name, n_reads, n_cand, votes, total, margin, sym, conf) in enumerate(lines):
        assert name == fwd.labels[c] and int(n_reads) == 3 and int(n_cand) == fwd.n_candidates[c] and int(votes) == fwd.votes[c]
        assert float(total) == fwd.total[c] and float(margin) == fwd.margin[c] and sym == fwd.symbols[c]
        assert conf == "%.17g" % fwd.confidence[c] and float(conf) == fwd.confidence[c]
    # without the flag: the table of the default call, seven columns, and --cluster-score viterbi prints the same bytes
    r = run(base + ["--cluster-table"])
    assert r.returncode == 0 and r.stdout == run(base + ["--cluster-table", "--cluster-score", "viterbi"]).stdout
    lines = [l.split("\t") for l in r.stdout.decode().splitlines()]
    assert len(lines) == 8
    for c, (name, n_reads, n_cand, votes, total, margin, sym) in enumerate(lines):
        assert name == plain.labels[c] and float(total) == plain.total[c] and float(margin) == plain.margin[c] and sym == plain.symbols[c]
    r = run(base + ["-r", "--cluster-score", "forward"])                # without the table: the messages only
    assert r.returncode == 0 and r.stdout.decode().splitlines() == list(fwd.symbols)
    for args in (base + ["--cluster-score", "posterior"], [a for a in base if a not in ("--cluster-file", lab)] + ["--cluster-score", "forward"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b"" and b"--cluster-score" in bad.stderr
