"""Posterior move counts over the whole band on the GPU (pair_counts_kernel of csrc/pair_counts_kernels.hip behind
dnas_pair_counts and dnas_baum_welch_pairs) against the host statement in table mode: pair_ll and pair_ll_backward uint64-equal,
status equal, per-pair counts and totals to rtol=1e-9, atol=1e-300 (the guided E-step's tolerance: the only difference is the
device's exp and the order in which non-negative terms are added).  The exact-reference test holds the GPU to
pair_counts_cases.py directly, inside the derived bounds of the CPU tests."""
import json
import math
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

import pair_counts_cases as K  # noqa: E402
import pair_forward_cases as C  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402
from test_assign_cpu import NOISY, _rand  # noqa: E402
from test_cluster_cpu import band_cells, source_constant  # noqa: E402
from test_gpu_pair_align import _related  # noqa: E402
from test_gpu_pair_forward import FORWARD_BANDS, FORWARD_SHAPES, forward_models, shape_list  # noqa: E402
from test_gpu_pair_hmm_edges import crossover_pairs, dealt_to_four_waves, record_words  # noqa: E402

# kPcLdsCols of pair_counts_device.h: the [16][64] substitution counters share a wave's LDS with the boundary row
COUNTS_LDS_COLS = (source_constant("pair_align_device.h", "kPaLdsDoubles") - 16 - 16 * 64) // 2
TOP = COUNTS_LDS_COLS - 1                               # the longest read whose backward boundary row stays in LDS


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def same_as_host(got, want, label=""):
    assert np.array_equal(got.status, want.status), (label, np.flatnonzero(got.status != want.status))
    assert np.array_equal(bits(got.pair_ll), bits(want.pair_ll)), (label, np.flatnonzero(bits(got.pair_ll) != bits(want.pair_ll)))
    assert np.array_equal(bits(got.pair_ll_backward), bits(want.pair_ll_backward)), \
        (label, np.flatnonzero(bits(got.pair_ll_backward) != bits(want.pair_ll_backward)))
    assert not np.isnan(got.pair_counts).any() and not np.isnan(got.counts).any(), label
    np.testing.assert_allclose(got.pair_counts, want.pair_counts, rtol=1e-9, atol=1e-300, err_msg=label)
    np.testing.assert_allclose(got.counts, want.counts, rtol=1e-9, atol=1e-300, err_msg=label)
    np.testing.assert_allclose(got.ll, want.ll, rtol=1e-9, atol=1e-300, err_msg=label)


def scratch_bytes(I, O, band, P):
    """What a pair asks of the wave that takes it: PaGeom::words() doubles for each of S, D and T_0 .. T_{P-1}."""
    return record_words(I, O, band) * (P + 2) * 8


# ------------------------------------------------------------------------------------------------ A. shapes, models and bands
@pytest.fixture(scope="module")
def shape_cases(da):
    """[(name, params, ins, outs, strand, {band: host result})], the host results computed once."""
    out = []
    for k, (name, params) in enumerate(forward_models(da)):
        ins, outs, strand = shape_list("gpu-pair-counts/%d" % k)
        out.append((name, params, ins, outs, strand,
                    {band: da.pairCounts(params, ins, outs, band=band, read_strand=strand, host=True) for band in FORWARD_BANDS}))
    return out


def test_every_shape_model_and_band(da, shape_cases, monkeypatch):
    assert {I for I, _ in FORWARD_SHAPES} >= {0, 1, 63, 64, 65, 130} and 0 in {O for _, O in FORWARD_SHAPES}
    assert sorted(set(p.c.n_len for _, p, *_ in shape_cases)) == [0, 1, 2, 3, 6, 7, 13] and FORWARD_BANDS == (-1, 0, 1, 32)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves: every wave walks several pairs and reuses its scratch
    monkeypatch.setenv("DNAS_COUNTS_CHUNK", "7")           # a prime: launches of 7 pairs and a ragged last one
    ok = no_path = 0
    for name, params, ins, outs, strand, want in shape_cases:
        n = len(ins)
        for band in FORWARD_BANDS:
            got = da.pairCounts(params, ins, outs, band=band, read_strand=strand)
            same_as_host(got, want[band], (name, band))
            st = got.stats
            assert st["chunks"] == -(-n // 7) and st["kernel_ms"] > 0 and st["pairs_too_large"] == 0 and 1 <= st["waves"] <= 8
            assert st["cells"] == sum(band_cells(len(a), len(b), band) for a, b in zip(ins, outs))
            ok += int((got.status == K.COUNTS_OK).sum())
            no_path += int((got.status == K.COUNTS_NO_PATH).sum())
            assert (got.pair_counts[got.status == K.COUNTS_NO_PATH] == 0).all()
    assert ok >= 400 and no_path >= 50
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the chunk as shipped
    monkeypatch.delenv("DNAS_COUNTS_CHUNK")
    for name, params, ins, outs, strand, want in shape_cases:
        for band in FORWARD_BANDS:
            got = da.pairCounts(params, ins, outs, band=band, read_strand=strand)
            same_as_host(got, want[band], (name, band, "shipped"))
            assert got.stats["chunks"] == 1
    name, params, ins, outs, strand, want = shape_cases[2]      # no strand array: every read as given
    same_as_host(da.pairCounts(params, ins, outs, band=32), da.pairCounts(params, ins, outs, band=32, host=True))
    empty = da.pairCounts(params, [], [])
    assert empty.pair_ll.shape == (0,) and empty.stats["chunks"] == 0 and empty.ll == 0 and (empty.counts == 0).all()


# ------------------------------------------------------------------------------------------------ B. the LDS / HBM crossover
def own_crossover_pairs():
    """Pairs around O = TOP, this kernel's crossover, one, two and three stripes, ordered so that under one work-group every wave
    goes LDS > HBM > shorter HBM > LDS."""
    rng = random.Random("gpu-pair-counts/crossover")
    order = [TOP] * 4 + [TOP + 2] * 4 + [TOP + 1] * 4 + [TOP - 1] * 4
    rows = [63, 64, 70, 130] * 4
    pairs = []
    for I, O in zip(rows, order):
        a = _rand(rng, I)
        pairs.append((a, _related(rng, a, O)))
    return pairs


@pytest.mark.parametrize("name", ("P2", "P6", "P13-zero"))
def test_the_lds_hbm_crossover(da, monkeypatch, name):
    """The backward boundary row crosses between LDS and the wave's HBM row both ways: the 26 crossover pairs of
    test_gpu_pair_hmm_edges.py (whose short reads stay in LDS among long ones in HBM here) and 16 pairs around this kernel's own
    crossover, each list dealt to the four waves of one work-group."""
    from test_cluster_cpu import cluster_models
    params = dict(cluster_models(da))[name]
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "1")
    own = own_crossover_pairs()
    for w in range(4):
        walk = [len(b) > TOP for _, b in own[w::4]]
        assert walk == [False, True, True, False]
    full = dealt_to_four_waves(crossover_pairs())
    lists = ((own, (-1, 8)), ([(a, b) for a, b, _ in full], (8,)))
    for pairs, bands in lists:
        ins, outs = [p[0] for p in pairs], [p[1] for p in pairs]
        assert min(len(b) for b in outs) <= TOP < max(len(b) for b in outs)
        for band in bands:
            want = da.pairCounts(params, ins, outs, band=band, host=True)
            assert (want.status == K.COUNTS_OK).sum() >= len(pairs) - 5
            got = da.pairCounts(params, ins, outs, band=band)
            same_as_host(got, want, (name, band))
            assert got.stats["waves"] == 4


# ------------------------------------------------------------------------------------------------ C. the arena
@pytest.fixture(scope="module")
def arena_case(da):
    rng = random.Random("gpu-pair-counts/arena")
    params = da.MutatorParams.fromFlags(**NOISY)
    lengths = [40, 150, 64, 150, 10, 130, 150, 90, 65, 150, 0, 120] * 2
    ins = [_rand(rng, n) for n in lengths]
    outs = [_related(rng, a, max(0, len(a) + rng.randint(-3, 3))) for a in ins]
    ins.append(_rand(rng, 200))                            # the largest pair, alone in its size
    outs.append(_related(rng, ins[-1], 204))
    band = 8
    return params, ins, outs, band, da.pairCounts(params, ins, outs, band=band, host=True)


def test_small_arena_cuts_the_grid(da, arena_case):
    params, ins, outs, band, want = arena_case
    P = params.c.n_len
    per_wave = max(scratch_bytes(len(a), len(b), band, P) for a, b in zip(ins, outs))
    got = da.pairCounts(params, ins, outs, band=band, arena_bytes=2 * per_wave)
    same_as_host(got, want)
    assert got.stats["waves"] == 2 and got.stats["scratch_bytes"] == 2 * per_wave and got.stats["pairs_too_large"] == 0
    wide = da.pairCounts(params, ins, outs, band=band)
    assert wide.stats["waves"] > 2
    assert np.array_equal(bits(wide.pair_counts), bits(got.pair_counts))     # a pair's counts do not depend on the grid


def test_small_arena_one_pair_too_large(da, arena_case):
    params, ins, outs, band, want = arena_case
    P = params.c.n_len
    sizes = [scratch_bytes(len(a), len(b), band, P) for a, b in zip(ins, outs)]
    big = int(np.argmax(sizes))
    assert big == len(ins) - 1 and sorted(sizes)[-2] < sizes[big]
    got = da.pairCounts(params, ins, outs, band=band, arena_bytes=sizes[big] - 1)
    assert got.status[big] == K.COUNTS_TOO_LARGE and np.isnan(got.pair_ll[big]) and np.isnan(got.pair_ll_backward[big])
    assert (got.pair_counts[big] == 0).all() and got.stats["pairs_too_large"] == 1
    rest = da.pairCounts(params, ins[:big], outs[:big], band=band, host=True)
    keep = np.arange(len(ins)) != big
    assert np.array_equal(got.status[keep], rest.status)
    assert np.array_equal(bits(got.pair_ll[keep]), bits(rest.pair_ll))
    assert np.array_equal(bits(got.pair_ll_backward[keep]), bits(rest.pair_ll_backward))
    np.testing.assert_allclose(got.pair_counts[keep], rest.pair_counts, rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(got.counts, rest.counts, rtol=1e-9, atol=1e-300)       # the totals are over the rest
    np.testing.assert_allclose(got.ll, rest.ll, rtol=1e-9)
    assert not np.isnan(got.counts).any() and not math.isnan(got.ll)


# ------------------------------------------------------------------------------------------------ D. totals
def test_totals_do_not_depend_on_grid_or_devices(da, arena_case, monkeypatch):
    params, ins, outs, band, want = arena_case
    strand = [i % 2 for i in range(len(ins))]
    outs = [da.reverse_complement(b) if s and b else b for b, s in zip(outs, strand)]
    shipped = da.pairCounts(params, ins, outs, band=band, read_strand=strand)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "1")
    one = da.pairCounts(params, ins, outs, band=band, read_strand=strand)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    three = da.pairCounts(params, ins, outs, band=band, read_strand=strand, device=-1)
    assert one.stats["waves"] == 4 and shipped.stats["waves"] > 4 and three.stats["chunks"] == 3
    for other in (one, three):
        assert np.array_equal(bits(other.counts), bits(shipped.counts)) and bits(other.ll) == bits(shipped.ll)
        assert np.array_equal(bits(other.pair_counts), bits(shipped.pair_counts))
    # ... because they are sums in pair order of the per-pair values
    total = np.zeros_like(shipped.counts)
    ll = 0.
    for i in range(len(ins)):
        if shipped.status[i] == K.COUNTS_OK:
            total += shipped.pair_counts[i]
            ll += shipped.pair_ll[i]
    assert np.array_equal(bits(total), bits(shipped.counts)) and ll == shipped.ll
    same_as_host(three, da.pairCounts(params, ins, outs, band=band, read_strand=strand, host=True))


# ------------------------------------------------------------------------------------------------ E. the exact references
def _inside_table_bound(label, params, pairs, exact_rows, got):
    worst = 0.
    P = params.c.n_len
    for i, ((a, b), (ll, counts)) in enumerate(zip(pairs, exact_rows)):
        if counts is None:
            assert got.status[i] == K.COUNTS_NO_PATH and got.pair_ll[i] == NEG and (got.pair_counts[i] == 0).all(), (label, i)
            continue
        assert got.status[i] == K.COUNTS_OK, (label, i)
        lo, hi = C.table_bounds(ll, len(a), len(b))
        assert lo <= got.pair_ll[i] <= hi, (label, i)
        lo, hi = K.backward_table_bounds(ll, len(a), len(b), P)
        assert lo <= got.pair_ll_backward[i] <= hi, (label, i)
        e = K.table_log_bound(len(a), len(b), P)
        g = got.pair_counts[i]
        assert (g >= counts * math.exp(-e) - 1e-300).all() and (g <= counts * math.exp(e) + 1e-300).all(), (label, i, g, counts)
        worst = max(worst, float(np.abs(g - counts).max()))
    return worst


GPU_MEDIUM_BANDS = (8, 0)      # the banded mpmath passes cost a tenth of the full matrix, which test_pair_counts_cpu.py covers


def test_against_the_exact_references(da):
    """The tiny pairs (the mpmath pass over the whole matrix, which test_pair_counts_cpu.py holds to the enumeration of every
    path) and the medium pairs inside bands 8 and 0."""
    worst = 0.
    for name, plain, pairs, rows in K.tiny_passed():
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        worst = max(worst, _inside_table_bound(name, params, pairs, rows, da.pairCounts(params, a, b, band=-1)))
    for name, plain, pairs, by_band in K.medium_exact(GPU_MEDIUM_BANDS):
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        for band in GPU_MEDIUM_BANDS:
            worst = max(worst, _inside_table_bound((name, band), params, pairs, by_band[band], da.pairCounts(params, a, b, band=band)))
    print("GPU counts against the exact references: largest |count - exact| = %.3g" % worst)


def test_the_boundary_models(da):
    """Probabilities of 0, 1, 1e-300 and 1 - 2^-53: no NaN, NO_PATH exactly where the mpmath pass finds no path, the counts of
    zero-probability moves exactly 0, everything else inside the table bound."""
    n = 0
    for name, plain, pairs, rows in K.boundary_exact():
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        got = da.pairCounts(params, a, b, band=-1)
        same_as_host(got, da.pairCounts(params, a, b, band=-1, host=True), name)
        _inside_table_bound(name, params, pairs, rows, got)
        assert (got.pair_counts[:, K.zero_moves(plain)] == 0).all(), name
        n += 1
    assert n == 56


# ------------------------------------------------------------------------------------------------ F. the fit
def test_fit_follows_the_host_em(da):
    ins, outs = K.em_pairs()
    start = K.em_start(da)
    fitted, iters, trace = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, max_iterations=3)
    assert iters == 3 and len(trace) == 3
    assert K.params_dict(trace[0][0]) == K.params_dict(start)
    for step in range(3):
        p, ll = trace[step]
        assert p.pLen == [.25] * 4
        host = da.pairCounts(p, ins, outs, band=K.EM_BAND, host=True)
        assert ll == pytest.approx(host.ll + K.log_prior(p, 4), rel=1e-9)
        want = K.m_step(host.counts)
        nxt = trace[step + 1][0] if step < 2 else fitted
        assert K.params_dict(nxt) == pytest.approx(want, rel=1e-9), step
    full, n_gpu, _ = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND)
    host_full, n_host, _ = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, host=True)
    assert n_gpu == n_host and 1 <= n_gpu < 100          # stopped by the 1e-3 rule, both after the same number of steps
    assert K.params_dict(full) == pytest.approx(K.params_dict(host_full), rel=1e-6)


def _fasta(path, seqs, prefix):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">%s%d\n%s\n" % (prefix, i, s))


def test_command_line(da, tmp_path):
    """--count-pairs and --fit-pairs print what pairCounts and baumWelchPairs return."""
    ins, outs = K.em_pairs()
    _fasta(tmp_path / "originals.fa", ins, "o")
    _fasta(tmp_path / "reads.fa", outs, "r")
    flags = ["--error-sub-prob", ".03", "--error-dup-prob", ".01", "--error-del-open", ".01", "--error-del-ext", ".1", "--length", "4"]
    start = da.MutatorParams.fromFlags(sub=.03, dup=.01, del_open=.01, del_ext=.1, length=4)
    files = [str(tmp_path / "originals.fa"), "--align-reads", str(tmp_path / "reads.fa"), "--align-band", str(K.EM_BAND)]
    r = subprocess.run([BIN] + flags + ["--count-pairs"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = da.pairCounts(start, ins, outs, band=K.EM_BAND)
    assert start.c.n_len == 2 and r.stdout == da.countsJSON(want.counts, start.c.n_len)      # --length 4: two duplication lengths
    r = subprocess.run([BIN] + flags + ["--fit-pairs"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fitted, _, _ = da.baumWelchPairs(start, ins, outs, band=K.EM_BAND)
    assert r.stdout == da.paramsJSON(fitted) and json.loads(r.stdout)
