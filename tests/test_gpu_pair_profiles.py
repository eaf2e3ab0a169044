"""Pair-HMM row profiles on the GPU (pair_profile_kernel of csrc/pair_profile_kernels.hip behind dnas_pair_profiles) against the
host statement in table mode: pair_ll uint64-equal, status equal, every per-pair block, the aggregate and the counts agreement
to rtol=1e-9 (the project's contract for the counts: only the device's exp differs, and all terms are non-negative) with atol
the smallest normal double (in case the device's exp flushes a subnormal), the coverage exact.  The exact-reference test holds
the GPU to pair_profile_cases.py directly, inside the table bound of the CPU tests."""
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
import pair_profile_cases as R  # noqa: E402
from pair_forward_cases import NEG, bits  # noqa: E402
from test_assign_cpu import NOISY, _rand  # noqa: E402
from test_cluster_cpu import source_constant  # noqa: E402
from test_gpu_pair_align import _related  # noqa: E402
from test_gpu_pair_forward import forward_models  # noqa: E402
from test_gpu_pair_hmm_edges import record_words  # noqa: E402

# kPpLdsCols of pair_counts_device.h: the [4][64] match counters share a wave's LDS with the boundary row
PROFILE_LDS_COLS = (source_constant("pair_align_device.h", "kPaLdsDoubles") - 16 - 4 * 64) // 2
TOP = PROFILE_LDS_COLS - 1                              # the longest read whose backward boundary row stays in LDS
TOL = dict(rtol=1e-9, atol=R.TINY)
STRIPE_BANDS = (-1, 8, 0)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def same_as_host(got, want, label=""):
    assert np.array_equal(got.status, want.status), (label, np.flatnonzero(got.status != want.status))
    assert np.array_equal(bits(got.pair_ll), bits(want.pair_ll)), (label, np.flatnonzero(bits(got.pair_ll) != bits(want.pair_ll)))
    assert len(got.pair_profiles) == len(want.pair_profiles)
    for i, (g, w) in enumerate(zip(got.pair_profiles, want.pair_profiles)):
        assert g.shape == w.shape and not np.isnan(g).any(), (label, i)
        np.testing.assert_allclose(g, w, err_msg="%s pair %d" % (label, i), **TOL)
        if got.status[i] != K.COUNTS_OK:
            assert (g == 0).all(), (label, i)
    assert np.array_equal(got.coverage, want.coverage), label
    assert not np.isnan(got.profile).any(), label
    np.testing.assert_allclose(got.profile, want.profile, err_msg=str(label), **TOL)


def same_bits(got, want):
    assert np.array_equal(bits(got.profile), bits(want.profile)) and np.array_equal(got.coverage, want.coverage)
    assert np.array_equal(bits(got.pair_ll), bits(want.pair_ll)) and np.array_equal(got.status, want.status)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got.pair_profiles, want.pair_profiles))


def scratch_bytes(I, O, band, P):
    """What a pair asks of the wave that takes it: PaGeom::words() doubles for each of S and D, whatever P (the backward pass of
    this kernel never meets a parked T lane again, so none is parked)."""
    return record_words(I, O, band) * 2 * 8


# ------------------------------------------------------------------------------------------------ A. stripe edges, every instance
STRIPE_MODELS = ("P0", "P1", "P2", "P3", "P6", "P7", "P13-zero")


def test_stripe_edges_every_kernel_instance_and_band(da, monkeypatch):
    """I + 1 rows around one, two and three stripes of 64, both read strands, under P of 0, 1, 2, 3, 6, 7 and 13: both sides of
    every edge of the dispatch on the duplication lengths (KP = 2, 6, 13)."""
    models = [(name, p) for name, p in forward_models(da) if name in STRIPE_MODELS]
    assert sorted(p.c.n_len for _, p in models) == [0, 1, 2, 3, 6, 7, 13]
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves: every wave walks several pairs and reuses its scratch
    n = 0
    for k, (name, params) in enumerate(models):
        ins, outs, strand = R.stripe_pairs("gpu-pair-profiles/%d" % k, longer=params.c.n_len > 0)
        assert {len(a) for a in ins} >= set(R.STRIPE_ROWS) and "" in outs and 0 in strand and 1 in strand
        assert all(abs(len(a) - len(b)) <= 8 for a, b in zip(ins, outs))
        for band in STRIPE_BANDS:
            keep = [i for i in range(len(ins)) if band != 0 or len(ins[i]) == len(outs[i])]
            a, b, s = [ins[i] for i in keep], [outs[i] for i in keep], [strand[i] for i in keep]
            assert {len(x) for x in a} >= set(R.STRIPE_ROWS)
            want = da.pairProfiles(params, a, b, band=band, read_strand=s, host=True)
            assert (want.status == K.COUNTS_OK).all(), (name, band, np.flatnonzero(want.status != K.COUNTS_OK))
            for anchor in ("start", "end") if band == 8 else ("start",):
                got = da.pairProfiles(params, a, b, band=band, read_strand=s, anchor=anchor)
                same_as_host(got, want if anchor == "start" else da.pairProfiles(params, a, b, band=band, read_strand=s, host=True, anchor="end"),
                             (name, band, anchor))
                assert got.stats["chunks"] == 1 and got.stats["kernel_ms"] > 0 and got.stats["pairs_too_large"] == 0
                assert 1 <= got.stats["waves"] <= 8
            n += len(keep)
    assert n >= 7 * 40
    name, params = models[4]
    empty = da.pairProfiles(params, [], [])
    assert empty.pair_ll.shape == (0,) and empty.stats["chunks"] == 0 and empty.profile.shape == (5 + params.c.n_len, 0)


# ------------------------------------------------------------------------------------------------ B. the LDS / HBM crossover
def crossover_pairs():
    """16 pairs around O = TOP, this kernel's own crossover, one, two and three stripes, ordered so that under one work-group
    every wave goes LDS > HBM > shorter HBM > LDS."""
    rng = random.Random("gpu-pair-profiles/crossover")
    order = [TOP] * 4 + [TOP + 2] * 4 + [TOP + 1] * 4 + [TOP - 1] * 4
    rows = [63, 64, 70, 130] * 4
    pairs = []
    for I, O in zip(rows, order):
        a = _rand(rng, I)
        pairs.append((a, _related(rng, a, O)))
    return pairs


@pytest.mark.parametrize("name", ("P2", "P6", "P13-zero"))
def test_the_lds_hbm_crossover(da, monkeypatch, name):
    """The backward boundary row crosses between LDS and the wave's HBM row both ways, at this kernel's constant: beyond the
    counts kernel's, so every one of these rows is in HBM there."""
    from test_cluster_cpu import cluster_models
    params = dict(cluster_models(da))[name]
    counts_cols = (source_constant("pair_align_device.h", "kPaLdsDoubles") - 16 - 16 * 64) // 2
    assert counts_cols < TOP - 1 and 4 * (16 + 2 * PROFILE_LDS_COLS + 4 * 64) * 8 <= 64 * 1024
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "1")
    pairs = crossover_pairs()
    for w in range(4):
        assert [len(b) + 1 > PROFILE_LDS_COLS for _, b in pairs[w::4]] == [False, True, True, False]
    ins, outs = [p[0] for p in pairs], [p[1] for p in pairs]
    want = da.pairProfiles(params, ins, outs, band=8, host=True)
    assert (want.status == K.COUNTS_OK).sum() >= len(pairs) - 5
    got = da.pairProfiles(params, ins, outs, band=8)
    same_as_host(got, want, name)
    assert got.stats["waves"] == 4


# ------------------------------------------------------------------------------------------------ C. grid, chunks, devices, arena
@pytest.fixture(scope="module")
def arena_case(da):
    rng = random.Random("gpu-pair-profiles/arena")
    params = da.MutatorParams.fromFlags(**NOISY)
    lengths = [40, 150, 64, 150, 10, 130, 150, 90, 65, 150, 0, 120] * 2
    ins = [_rand(rng, n) for n in lengths]
    outs = [_related(rng, a, max(0, len(a) + rng.randint(-3, 3))) if a else "" for a in ins]
    ins.append(_rand(rng, 200))                            # the largest pair, alone in its size
    outs.append(_related(rng, ins[-1], 204))
    strand = [i % 2 for i in range(len(ins))]
    outs = [da.reverse_complement(b) if s and b else b for b, s in zip(outs, strand)]
    band = 8
    return params, ins, outs, strand, band, da.pairProfiles(params, ins, outs, band=band, read_strand=strand, host=True, anchor="end")


def test_blocks_and_aggregate_do_not_depend_on_grid_chunks_or_devices(da, arena_case, monkeypatch):
    params, ins, outs, strand, band, want = arena_case
    shipped = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end")
    same_as_host(shipped, want)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    monkeypatch.setenv("DNAS_COUNTS_CHUNK", "7")           # a prime: launches of 7 pairs and a ragged last one
    cut = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end")
    alone = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end", per_pair=False)
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")
    monkeypatch.delenv("DNAS_COUNTS_CHUNK")
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    three = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end", device=-1)
    three_alone = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end", device=-1, per_pair=False)
    assert cut.stats["chunks"] == -(-len(ins) // 7) and 1 <= cut.stats["waves"] <= 8
    assert shipped.stats["chunks"] == 1 and shipped.stats["waves"] > 8 and three.stats["chunks"] == 3
    for other in (cut, three):
        same_bits(other, shipped)
    for other in (alone, three_alone):                     # the aggregate formed chunk by chunk, no per-pair output
        assert other.pair_profiles is None and np.array_equal(bits(other.profile), bits(shipped.profile))
        assert np.array_equal(other.coverage, shipped.coverage)
    # ... because the aggregate is the sum in pair order of the per-pair blocks
    codes = [da.tokenize(a) for a in ins]
    total, cover = R.fold(shipped.pair_profiles, codes, shipped.status, "end", shipped.profile.shape[1])
    assert np.array_equal(cover, shipped.coverage)
    np.testing.assert_allclose(shipped.profile, total, rtol=1e-13, atol=0)


def test_small_arena_cuts_the_grid(da, arena_case):
    params, ins, outs, strand, band, want = arena_case
    P = params.c.n_len
    per_wave = max(scratch_bytes(len(a), len(b), band, P) for a, b in zip(ins, outs))
    got = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end", arena_bytes=2 * per_wave)
    same_as_host(got, want)
    assert got.stats["waves"] == 2 and got.stats["scratch_bytes"] == 2 * per_wave and got.stats["pairs_too_large"] == 0
    wide = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end")
    assert wide.stats["waves"] > 2
    same_bits(wide, got)                                   # a pair's block does not depend on the grid


def test_small_arena_one_pair_too_large(da, arena_case):
    params, ins, outs, strand, band, want = arena_case
    P = params.c.n_len
    sizes = [scratch_bytes(len(a), len(b), band, P) for a, b in zip(ins, outs)]
    big = int(np.argmax(sizes))
    assert big == len(ins) - 1 and sorted(sizes)[-2] < sizes[big]
    got = da.pairProfiles(params, ins, outs, band=band, read_strand=strand, anchor="end", arena_bytes=sizes[big] - 1)
    assert got.status[big] == K.COUNTS_TOO_LARGE and np.isnan(got.pair_ll[big]) and (got.pair_profiles[big] == 0).all()
    assert got.pair_profiles[big].shape == (6 + P, 201) and got.stats["pairs_too_large"] == 1
    rest = da.pairProfiles(params, ins[:big], outs[:big], band=band, read_strand=strand[:big], host=True, anchor="end")
    assert np.array_equal(got.status[:big], rest.status) and np.array_equal(bits(got.pair_ll[:big]), bits(rest.pair_ll))
    for g, w in zip(got.pair_profiles[:big], rest.pair_profiles):
        np.testing.assert_allclose(g, w, **TOL)
    # the aggregate is over the rest: the positions only the large pair has are not covered
    n_rest = rest.profile.shape[1]
    assert np.array_equal(got.coverage[:n_rest], rest.coverage) and (got.coverage[n_rest:] == 0).all()
    np.testing.assert_allclose(got.profile[:, :n_rest], rest.profile, **TOL)
    assert (got.profile[:, n_rest:] == 0).all() and not np.isnan(got.profile).any()


# ------------------------------------------------------------------------------------------------ D. the references
def test_the_boundary_models(da):
    """Probabilities of 0, 1, 1e-300 and 1 - 2^-53: no NaN, NO_PATH where the host says so, the planes of zero-probability moves
    exactly 0."""
    n = no_path = 0
    for name, plain, pairs in C.boundary_cases():
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        want = da.pairProfiles(params, a, b, band=-1, host=True)
        got = da.pairProfiles(params, a, b, band=-1)
        same_as_host(got, want, name)
        zero = R.zero_planes(plain)
        assert all((blk[zero] == 0).all() for blk in got.pair_profiles), (name, zero)
        no_path += int((got.status == K.COUNTS_NO_PATH).sum())
        n += 1
    assert n == 56 and no_path > 0


GPU_MEDIUM_BANDS = (8, 0)      # the banded mpmath passes cost a tenth of the full matrix, which test_pair_profiles_cpu.py covers


def _inside_table_bound(label, params, pairs, exact_rows, got):
    worst = 0.
    P = params.c.n_len
    for i, ((a, b), (ll, want)) in enumerate(zip(pairs, exact_rows)):
        if want is None:
            assert got.status[i] == K.COUNTS_NO_PATH and got.pair_ll[i] == NEG and (got.pair_profiles[i] == 0).all(), (label, i)
            continue
        assert got.status[i] == K.COUNTS_OK, (label, i)
        lo, hi = C.table_bounds(ll, len(a), len(b))
        assert lo <= got.pair_ll[i] <= hi, (label, i)
        e = K.table_log_bound(len(a), len(b), P)
        g = got.pair_profiles[i]
        assert (g >= want * math.exp(-e) - 1e-300).all() and (g <= want * math.exp(e) + 1e-300).all(), (label, i)
        worst = max(worst, float(np.abs(g - want).max()))
    return worst


def test_against_the_exact_references(da):
    """Without the host statement in the loop: the tiny pairs over the whole matrix and the medium pairs inside bands 8 and 0
    against the mpmath pass of pair_profile_cases.py."""
    worst = 0.
    for name, plain, pairs, rows in R.tiny_exact():
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        worst = max(worst, _inside_table_bound(name, params, pairs, rows, da.pairProfiles(params, a, b, band=-1)))
    for name, plain, pairs, by_band in R.medium_exact(GPU_MEDIUM_BANDS):
        params = C.lib_params(da, plain)
        a, b = C.seqs(pairs)
        for band in GPU_MEDIUM_BANDS:
            worst = max(worst, _inside_table_bound((name, band), params, pairs, by_band[band], da.pairProfiles(params, a, b, band=band)))
    print("GPU profiles against the exact references: largest |value - exact| = %.3g" % worst)


def test_rows_sum_to_the_counts_on_the_gpu(da, arena_case):
    params, ins, outs, strand, band, want = arena_case
    got = da.pairProfiles(params, ins, outs, band=band, read_strand=strand)
    counts = da.pairCounts(params, ins, outs, band=band, read_strand=strand)
    assert np.array_equal(got.status, counts.status) and np.array_equal(bits(got.pair_ll), bits(counts.pair_ll))
    assert (got.status == K.COUNTS_OK).sum() >= len(ins) - 2
    for blk, c in zip(got.pair_profiles, counts.pair_counts):
        rows = np.concatenate(([blk[:R.DEL_OPEN].sum()], blk[R.DEL_OPEN:].sum(axis=1)))
        np.testing.assert_allclose(rows, np.concatenate(([c[2], c[0], c[3]], c[21:])), **TOL)


# ------------------------------------------------------------------------------------------------ E. the decoder and the tool
def test_decode_clusters_with_support(da, ref_data):
    from test_gpu_consensus import BAND, MACHINE, PLANTED, planted_pool
    machine = da.Machine.fromFile(os.path.join(ref_data, MACHINE))
    messages, reads, labels = planted_pool(da, machine, n_clusters=6)
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    dec = da.ViterbiDecoder(machine, params, device=0)
    plain = dec.decode_clusters(reads, labels, band=BAND)
    got = dec.decode_clusters(reads, labels, band=BAND, support=True)
    dec.close()
    assert not hasattr(plain, "support") and len(got.support) == 6 and got.support_reads.shape == (6,)
    # every other field is the default call's
    assert got.labels == plain.labels and got.symbols == plain.symbols and np.array_equal(got.read, plain.read)
    for f in ("total", "second", "margin"):
        assert np.array_equal(bits(getattr(got, f)), bits(getattr(plain, f))), f
    for f in ("votes", "n_candidates", "status", "source"):
        assert np.array_equal(getattr(got, f), getattr(plain, f)), f
    assert got.per_read[0] == plain.per_read[0] and all(np.array_equal(g, w) for g, w in zip(got.per_read[1:], plain.per_read[1:]))
    # the support is the host statement's, restated from the public calls
    won = 0
    for c, lab in enumerate(got.labels):
        mine = [i for i, x in enumerate(labels) if x == lab]
        if plain.read[c] < 0:
            assert got.support[c].shape == (0,) and got.support_reads[c] == 0
            continue
        s = da.tokenize(machine.encodeSymbols(plain.symbols[c]))
        host = da.pairProfiles(params, [s] * len(mine), [reads[i] for i in mine], band=BAND, host=True,
                               read_strand=[int(plain.per_read[3][i]) for i in mine])
        ok = [j for j in range(len(mine)) if host.status[j] == K.COUNTS_OK]
        assert got.support_reads[c] == len(ok) and got.support[c].shape == (len(s),)
        mean = sum(host.pair_profiles[j][R.MATCH + s, np.arange(len(s))] for j in ok) / len(ok)
        np.testing.assert_allclose(got.support[c], mean, **TOL)
        assert (got.support[c] >= 0).all() and (got.support[c] <= 1 + 1e-6).all()
        won += 1
    assert won >= 5


def _fasta(path, seqs, prefix):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">%s%d\n%s\n" % (prefix, i, s))


@pytest.mark.parametrize("anchor", ("start", "end"))
def test_command_line(da, tmp_path, anchor):
    """--profile-pairs prints what pairProfiles returns."""
    ins, outs = K.em_pairs()
    _fasta(tmp_path / "originals.fa", ins, "o")
    _fasta(tmp_path / "reads.fa", outs, "r")
    flags = ["--error-sub-prob", ".03", "--error-dup-prob", ".01", "--error-del-open", ".01", "--error-del-ext", ".1", "--length", "4"]
    start = da.MutatorParams.fromFlags(sub=.03, dup=.01, del_open=.01, del_ext=.1, length=4)
    cmd = [BIN] + flags + ["--profile-pairs", str(tmp_path / "originals.fa"), "--align-reads", str(tmp_path / "reads.fa"),
                           "--align-band", str(K.EM_BAND)] + (["--profile-anchor", "end"] if anchor == "end" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    want = da.pairProfiles(start, ins, outs, band=K.EM_BAND, host=True, anchor=anchor)
    n_pos = max(len(a) for a in ins) + 1
    assert start.c.n_len == 2 and out["anchor"] == anchor and out["positions"] == n_pos and out["coverage"] == list(want.coverage)
    for j, key in enumerate(("same", "transition", "transversion", "delOpen", "delExtend")):
        np.testing.assert_allclose(out[key], want.profile[j], err_msg=key, **TOL)
    assert len(out["dup"]) == 2
    for k in range(2):
        np.testing.assert_allclose(out["dup"][k], want.profile[R.SUM_DUP + k], **TOL)
