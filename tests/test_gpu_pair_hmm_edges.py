"""The pair-HMM wavefront (paWalkForward / paScoreChunk of csrc/pair_align_device.h) and the sketch and filter kernels of
csrc/cluster_kernels.hip at the shapes where they change path: the last boundary row that stays in LDS and the first that goes
through HBM, waves that alternate between the two, bands at and beyond the clip to the full matrix, pools of more than two filter
tiles, and a sketch grid that goes round twice.

Every comparison is an equality against the host=True call with the same arguments (the host statements are held to exact
references by test_pair_align_cpu.py, test_assign_cpu.py, test_consensus_cpu.py and test_cluster_cpu.py): doubles as uint64 bit
patterns, op bytes, statuses, winners, edges and the counts of the stats as they are.  The shapes are built from the two
constants of the source, read below; every condition a case relies on is asserted on host-side data before the GPU call."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY, _rand  # noqa: E402
from test_cluster_cpu import K, band_cells, cluster_models, one_edit, pool_t, same_results, source_constant  # noqa: E402
from test_gpu_assign import _same as same_assignments  # noqa: E402
from test_gpu_consensus import _same as same_consensus  # noqa: E402
from test_gpu_pair_align import SHAPES, _models, _related, _same as same_alignments  # noqa: E402

LDS_DOUBLES = source_constant("pair_align_device.h", "kPaLdsDoubles")      # a wave's LDS: 16 substitution scores, then the row
TILE = source_constant("cluster_kernels.hip", "kClTile")                   # rows and columns of a filter tile
LDS_COLS = (LDS_DOUBLES - 16) // 2                                         # kPaLdsCols: the columns (O + 1) a row in LDS holds
C = LDS_COLS - 1                                                           # the longest read whose boundary row stays in LDS
NEG = float("-inf")
INT32_MAX = 2 ** 31 - 1
CROSSOVER_BANDS = (-1, 8)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


# ------------------------------------------------------------------------------------------- A. the LDS / HBM crossover: pairs
def crossover_pairs():
    """[(original, read, related)]: 21 related pairs -- I in {63, 64, 70, 130} (one stripe, whose boundary row is written and
    never read, two and three stripes) with O in {C - 1, C, C + 1, C + 2}, (C, C), (C + 1, C + 1), (C + 1, 64), (5, C + 1),
    (64, 200) -- and 5 unrelated pairs of the same lengths: 26 pairs."""
    rng = random.Random("pair-hmm-edges/crossover")
    shapes = [(I, O) for I in (63, 64, 70, 130) for O in (C - 1, C, C + 1, C + 2)]
    shapes += [(C, C), (C + 1, C + 1), (C + 1, 64), (5, C + 1), (64, 200)]
    pairs = []
    for I, O in shapes:
        a = _rand(rng, I)
        pairs.append((a, _related(rng, a, O), True))
    pairs += [(_rand(rng, I), _rand(rng, O), False) for I, O in ((64, C), (130, C + 1), (63, C + 2), (70, C - 1), (C, C + 1))]
    assert all((len(a), len(b)) == s for (a, b, _), s in zip(pairs, shapes))
    return pairs


def in_hbm(pair):
    return len(pair[1]) > C


def dealt_to_four_waves(pairs):
    """The pairs in an order in which, under DNAS_ALIGN_BLOCKS=1 (4 waves, wave w walks the pairs w, w + 4, ...), every wave
    starts LDS, HBM with O = C + 2, HBM with O = C + 1, LDS; the rest follow shuffled."""
    lds = [p for p in pairs if not in_hbm(p)]
    far = [p for p in pairs if len(p[1]) == C + 2]
    near = [p for p in pairs if len(p[1]) == C + 1]
    assert len(lds) >= 8 and len(far) >= 4 and len(near) >= 4 and len(lds) + len(far) + len(near) == len(pairs)
    rest = lds[8:] + far[4:] + near[4:]
    random.Random("pair-hmm-edges/rest").shuffle(rest)
    return lds[:4] + far[:4] + near[:4] + lds[4:8] + rest


def transitions(walk):
    """What a wave meets between one pair and its next."""
    met = set()
    for p, q in zip(walk, walk[1:]):
        if not in_hbm(p) and in_hbm(q):
            met.add("LDS>HBM")
        if in_hbm(p) and not in_hbm(q):
            met.add("HBM>LDS")
        if in_hbm(p) and in_hbm(q) and len(q[1]) < len(p[1]):
            met.add("HBM>shorter HBM")
    return met


def record_words(I, O, band):
    """PaGeom::words: the 16-bit choice words the fill kernel files for a pair (to size an arena that splits the list)."""
    b = I + O + 1 if band < 0 or band > I + O + 1 else band
    lo, hi = min(O - I, 0) - b, max(O - I, 0) + b
    return (I // 64 + 1) * min(hi - lo + 1 + 126, O + 64) * 64


@pytest.fixture(scope="module")
def crossover():
    full = dealt_to_four_waves(crossover_pairs())
    short = [p for p in full if not in_hbm(p)]
    return full, short


@pytest.mark.parametrize("name", ("P2", "P6", "P13-zero"))
def test_align_pairs_at_the_crossover(da, crossover, monkeypatch, name):
    """alignPairs (the recording fill kernel and its traceback) on 26 pairs around O = C, the last read whose boundary row stays
    in LDS (1015): a list of 13 pairs whose longest read is exactly C (the row fills the wave's LDS to its last double, no HBM
    scratch at all) and the full list of 26, where 13 pairs go through HBM.  With the grid as shipped a wave owns a pair; with
    one work-group each of the 4 waves walks 6 or 7 pairs and meets LDS > HBM, HBM > LDS and HBM > a shorter HBM row (its scratch
    row reused with the stale columns of a longer pair)."""
    params = dict(cluster_models(da))[name]
    full, short = crossover
    assert max(len(b) for _, b, _ in short) == C and max(len(b) for _, b, _ in full) == C + 2
    assert sum(len(b) == C for _, b, _ in full) >= 5 and sum(len(b) == C + 1 for _, b, _ in full) >= 5
    for w in range(4):                                     # the condition of the one-work-group runs, on the list itself
        assert transitions(full[w::4]) == {"LDS>HBM", "HBM>LDS", "HBM>shorter HBM"}, w
    for pairs in (short, full):
        ins, outs, related = [p[0] for p in pairs], [p[1] for p in pairs], np.array([p[2] for p in pairs])
        for band in CROSSOVER_BANDS:
            want = da.alignPairs(params, ins, outs, band=band, host=True)
            assert (want.status[related] == da.lib.ALIGN_OK).all() and np.isfinite(want.score[related]).all()
            got = da.alignPairs(params, ins, outs, band=band)
            same_alignments(got, want)
            assert got.stats["batches"] == 1 and got.stats["pairs_too_large"] == 0
            assert got.stats["cells"] == sum(band_cells(len(a), len(b), band) for a, b in zip(ins, outs))
            monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "1")
            same_alignments(da.alignPairs(params, ins, outs, band=band), want)
            if name == "P6" and band == 8 and pairs is full:   # ... and the alternation across the batches of a small arena
                words = [record_words(len(a), len(b), band) for a, b in zip(ins, outs)]
                arena = max(2 * max(words), 2 * sum(words) // 4)
                split = da.alignPairs(params, ins, outs, band=band, arena_bytes=arena)
                same_alignments(split, want)
                assert split.stats["batches"] >= 3 and split.stats["pairs_too_large"] == 0
                assert split.stats["cells"] == got.stats["cells"]
            monkeypatch.delenv("DNAS_ALIGN_BLOCKS")


# ---------------------------------------------------------------------------- A. the crossover: the three score entry points
def score_sequences(da, top):
    """-> (originals, reads, strands): originals of 63, top, 130 and 5 nt; six reads, the longest exactly top nt -- two of top, one
    of top - 1 and one of top - 2 nt (related to the originals of 63, top, top and 130 nt), one of 200 and one of 64 nt; a read
    with strand 1 is given reverse-complemented."""
    rng = random.Random("pair-hmm-edges/score/%d" % (top - C))
    a63, along, a130, a5, a64 = (_rand(rng, n) for n in (63, top, 130, 5, 64))
    made = [(_related(rng, a63, top), 0), (_related(rng, along, top), 1), (_related(rng, a64, 200), 0),
            (_related(rng, along, top - 1), 1), (_related(rng, along, 64), 1), (_related(rng, a130, top - 2), 0)]
    reads = [da.reverse_complement(r) if s else r for r, s in made]
    assert max(map(len, reads)) == top and sorted(map(len, reads))[-3:] == [top - 1, top, top]
    return [a63, along, a130, a5], reads, [s for _, s in made], a64


SCORE_CASES = [(top, name) for top in (C, C + 1) for name in ("P2", "P6", "P13-zero")]
SCORE_IDS = ["%s-%s" % ("C" if top == C else "C+1", name) for top, name in SCORE_CASES]


def eight_waves(monkeypatch, chunk_env):
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves ...
    monkeypatch.setenv(chunk_env, "37")                    # ... over chunks of a prime number of items: every wave walks several


@pytest.mark.parametrize("top,name", SCORE_CASES, ids=SCORE_IDS)
def test_assign_reads_at_the_crossover(da, monkeypatch, top, name):
    """assignReads, 4 originals x 6 reads x both strands = 48 items.  Longest read C: the score kernel's dynamic LDS holds a
    full-size row and there is no HBM scratch; longest read C + 1: the two reads of C + 1 nt go through HBM between items that
    stay in LDS.  The reverse strand is read in place (b[O - 1 - j]) at O = C and O = C + 1."""
    params = dict(cluster_models(da))[name]
    originals, reads, strands, _ = score_sequences(da, top)
    eight_waves(monkeypatch, "DNAS_ASSIGN_CHUNK")
    for band in CROSSOVER_BANDS:
        want = da.assignReads(params, originals, reads, band=band, host=True, item_scores=True)
        assert (want.status == da.lib.ASSIGN_OK).all() and [(int(want.original[r]), int(want.strand[r])) for r in (1, 3)] == [(1, 1)] * 2
        got = da.assignReads(params, originals, reads, band=band, item_scores=True)
        same_assignments(got, want)
        assert got.stats["items"] == 48 and got.stats["chunks"] == 2
        assert got.stats["cells"] == 2 * sum(band_cells(len(a), len(b), band) for a in originals for b in reads)


@pytest.mark.parametrize("top,name", SCORE_CASES, ids=SCORE_IDS)
def test_consensus_score_at_the_crossover(da, monkeypatch, top, name):
    """consensusScore on the same sequences as candidates and reads: three clusters, 18 + 6 + 16 = 40 items."""
    params = dict(cluster_models(da))[name]
    (a63, along, a130, a5), reads, strands, a64 = score_sequences(da, top)
    pick = lambda xs, idx: [xs[i] for i in idx]
    members = (range(6), (1, 2, 3), (0, 2, 4, 5))
    cands = [[a63, along, a130], [along, a5], [a5, a63, a64, a130]]
    groups, flags = [pick(reads, m) for m in members], [pick(strands, m) for m in members]
    assert max(len(r) for g in groups for r in g) == top
    eight_waves(monkeypatch, "DNAS_CONSENSUS_CHUNK")
    for band in CROSSOVER_BANDS:
        want = da.consensusScore(params, cands, groups, band=band, read_strand=flags, host=True)
        got = da.consensusScore(params, cands, groups, band=band, read_strand=flags)
        same_consensus(got, want)
        assert got.stats["items"] == 40 and got.stats["chunks"] == 2 and got.stats["candidates"] == 9
        assert got.stats["cells"] == sum(band_cells(len(c), len(r), band) for cs, g in zip(cands, groups) for c in cs for r in g)


def crossover_pool(da, top):
    """24 reads: families of 5 to 130 nt (a founder, an edited copy, an edited copy turned round), one read of 200 nt, and two long
    ones -- of top - 1 nt at index 8 and of top nt at index 19, so that 19 rows end in an item with O = top."""
    rng = random.Random("pair-hmm-edges/pool/%d" % (top - C))
    short = []
    for n in (5, 20, 63, 64, 65, 100, 130):
        a = _rand(rng, n)
        short += [a, _related(rng, a, n + rng.randint(-2, 2)), da.reverse_complement(_related(rng, a, n + rng.randint(0, 3)))]
    short.append(_rand(rng, 200))
    rng.shuffle(short)
    along = _rand(rng, top)
    reads = short[:8] + [da.reverse_complement(_related(rng, along, top - 1))] + short[8:18] + [along] + short[18:]
    assert len(reads) == 24 and max(map(len, reads)) == top == len(reads[19]) and len(reads[8]) == top - 1 and min(map(len, reads)) > 0
    return reads


@pytest.mark.parametrize("top,name", SCORE_CASES, ids=SCORE_IDS)
def test_cluster_reads_at_the_crossover(da, monkeypatch, top, name):
    """clusterReads on a pool of 24 reads with every pair scored on both strands (276 pairs, 552 items), no floor: the edge list
    is the candidate list with every pair's better score."""
    params = dict(cluster_models(da))[name]
    reads = crossover_pool(da, top)
    eight_waves(monkeypatch, "DNAS_CLUSTER_CHUNK")
    for band in CROSSOVER_BANDS:
        opts = dict(band=band, k=K, min_shared=0, min_score_per_nt=NEG, edges=True)
        want = da.clusterReads(params, reads, host=True, **opts)
        assert want.stats["candidates"] == want.stats["edges"] == 276
        got = da.clusterReads(params, reads, **opts)
        same_results(got, want)
        assert got.stats["chunks"] == -(-276 // 37)
        assert got.stats["cells"] == 2 * sum(band_cells(len(reads[i]), len(reads[j]), band) for i in range(24) for j in range(i + 1, 24))


# ---------------------------------------------------------------------------------------------------------- B. the band's limits
LIMIT_SHAPES = ((63, 63), (65, 60), (129, 140), (70, 40), (40, 70))       # one stripe, two, three; I > O and O > I


def limit_bands(I, O):
    """The widest band that is not clipped, the clip itself, the first band beyond it, and the largest int32."""
    return (I + O, I + O + 1, I + O + 2, INT32_MAX)


def test_band_limits_align_pairs(da):
    """alignPairs under all six models at band = I + O, I + O + 1, I + O + 2 and 2^31 - 1 (PaGeom clips a band beyond I + O + 1 to
    the full matrix; the last one stands on the 64-bit arithmetic of stepsMax): the host at the same band, and -- every one of
    these bands holds every cell -- the GPU's own result at band = -1, cells included.  3 pairs per shape."""
    assert set(LIMIT_SHAPES) <= set(SHAPES)
    for m, (name, params) in enumerate(_models(da)):
        for I, O in LIMIT_SHAPES:
            rng = random.Random("pair-hmm-edges/limits/%d/%d/%d" % (m, I, O))
            a = _rand(rng, I)
            ins, outs = [a, a, a], [_related(rng, a, O), _rand(rng, O), a[:O] + a[:max(0, O - I)]]
            full = da.alignPairs(params, ins, outs, band=-1)
            same_alignments(full, da.alignPairs(params, ins, outs, band=-1, host=True))
            assert full.stats["cells"] == 3 * (I + 1) * (O + 1)
            for band in limit_bands(I, O):
                got = da.alignPairs(params, ins, outs, band=band)
                same_alignments(got, da.alignPairs(params, ins, outs, band=band, host=True))
                same_alignments(got, full)
                assert got.stats["cells"] == full.stats["cells"], (name, I, O, band)


def test_band_limits_assign_reads(da):
    """The same bands through a score kernel: assignReads under P6, two originals x three reads x both strands per shape."""
    params = da.MutatorParams.fromFlags(**NOISY)
    for I, O in LIMIT_SHAPES:
        rng = random.Random("pair-hmm-edges/limits/assign/%d/%d" % (I, O))
        a = _rand(rng, I)
        originals = [_rand(rng, I), a]
        reads = [_related(rng, a, O), da.reverse_complement(_related(rng, a, O)), _rand(rng, O)]
        full = da.assignReads(params, originals, reads, band=-1, item_scores=True)
        same_assignments(full, da.assignReads(params, originals, reads, band=-1, host=True, item_scores=True))
        assert list(full.original[:2]) == [1, 1] and list(full.strand[:2]) == [0, 1] and full.stats["cells"] == 12 * (I + 1) * (O + 1)
        for band in limit_bands(I, O):
            got = da.assignReads(params, originals, reads, band=band, item_scores=True)
            same_assignments(got, da.assignReads(params, originals, reads, band=band, host=True, item_scores=True))
            same_assignments(got, full)
            assert got.stats["cells"] == full.stats["cells"] and got.stats["items"] == 12


# ------------------------------------------------------------------------------------------ C. the filter beyond two tiles
T_OPTS = dict(band=4, k=K, edges=True)
T_SETTINGS = [(sketch, min_shared) for sketch in (16, 32, 64) for min_shared in (1, 2)]


def row_offsets(ij, n):
    """-> (candidates per row, the position of every row's first candidate in the list) of a candidate list in (i, j) order."""
    per_row = np.bincount(ij[:, 0], minlength=n)
    return per_row, np.concatenate([[0], np.cumsum(per_row)])


def band_rows(row_off, cap):
    """[(lo, rowFirst, rowEnd)] of the bands of cap pairs the list is scored in: the rows an emit launch walks."""
    total = int(row_off[-1])
    return [(lo, int(np.searchsorted(row_off, lo, side="right")) - 1, int(np.searchsorted(row_off, min(total, lo + cap), side="left")))
            for lo in range(0, total, cap)]


def filter_conditions(ij, n):
    """What pool T is for: rows that overflow a tile's columns over three or more column tiles, rows with a few candidates and
    rows with none, and enough candidates for 8 bands of 37."""
    per_row, _ = row_offsets(ij, n)
    assert per_row.max() > TILE and int((per_row == 0).sum()) >= TILE // 2 and len(ij) >= 8 * 37
    assert int(((per_row > 0) & (per_row < 8)).sum()) >= TILE // 2
    fullest = ij[ij[:, 0] == per_row.argmax(), 1]
    assert len(set(int(j) // TILE for j in fullest)) >= 3
    return per_row


@pytest.fixture(scope="module")
def pool(da):
    """(reads of pool T, P6, {(sketch, min_shared, floor): the host's result}), computed once.  Without a floor the edge list is
    the candidate list; that it is the list of clusterCandidates is checked for one setting."""
    reads = pool_t(da, TILE)
    params = da.MutatorParams.fromFlags(**NOISY)
    host = {}
    for sketch, min_shared in T_SETTINGS:
        for floor in (NEG, 0.0):
            host[sketch, min_shared, floor] = da.clusterReads(params, reads, sketch=sketch, min_shared=min_shared, min_score_per_nt=floor,
                                                              host=True, **T_OPTS)
        listed = host[sketch, min_shared, NEG]
        assert listed.stats["edges"] == listed.stats["candidates"] == len(listed.edges[0])
        assert 0 < host[sketch, min_shared, 0.0].stats["edges"] < listed.stats["edges"]
        filter_conditions(listed.edges[0], len(reads))
    ij, _ = da.clusterCandidates(params, reads, band=4, k=K, sketch=16, min_shared=2)
    assert np.array_equal(ij, host[16, 2, NEG].edges[0])
    return reads, params, host


def test_filter_on_five_tiles(da, pool):
    """Pool T (257 reads: four full row tiles and one of a single row) with the grid as shipped, every sketch size, min_shared 1
    and 2, without a floor (the filter alone: the candidate list in order, with both scores of every pair folded into its edge)
    and with the floor 0.  Candidates of the 32 896 pairs, as the host finds them (min_shared 1 / 2): sketch 16: 2907 / 2802,
    sketch 32: 3068 / 2874, sketch 64: 3143 / 3002; the fullest row has 72 and 35 to 61 rows have none; the floor leaves 2782 to
    2784 edges and 62 clusters."""
    reads, params, host = pool
    assert len(reads) == 4 * TILE + 1
    for (sketch, min_shared, floor), want in host.items():
        got = da.clusterReads(params, reads, sketch=sketch, min_shared=min_shared, min_score_per_nt=floor, **T_OPTS)
        same_results(got, want)
        assert got.stats["chunks"] == 1


def test_filter_bands_inside_rows(da, pool, monkeypatch):
    """The list of pool T scored in bands of 37 pairs (the emit kernel starts and ends inside rows of every tile; 8 waves walk a
    band's 74 items) and in bands of a third of the list (an emit grid of three or more row tiles from a rowFirst that is no
    multiple of the tile)."""
    reads, params, host = pool
    n = len(reads)
    listed = host[16, 2, NEG]
    candidates = listed.stats["candidates"]
    _, row_off = row_offsets(listed.edges[0], n)
    inside = set(first // TILE for lo, first, _ in band_rows(row_off, 37) if row_off[first] < lo)
    assert inside >= set(range(4))                         # a band starts inside a row of each of the four full tiles
    third = -(-candidates // 3)
    wide = [(first, end) for _, first, end in band_rows(row_off, third) if end - first > 2 * TILE]
    assert wide and any(first % TILE for first, _ in wide)
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")
    for cap in (37, third):
        monkeypatch.setenv("DNAS_CLUSTER_CHUNK", str(cap))
        for floor in (NEG, 0.0):
            got = da.clusterReads(params, reads, sketch=16, min_shared=2, min_score_per_nt=floor, **T_OPTS)
            same_results(got, host[16, 2, floor])
            assert got.stats["chunks"] == -(-candidates // cap)


@pytest.mark.parametrize("workers", (2, 3))
def test_filter_tiles_dealt_to_workers(da, pool, monkeypatch, workers):
    """Five row tiles over 2 or 3 workers: a worker's count grid owns the tiles w and w + W (blockIdx.x >= 1 with a tile stride
    above 1), and the bands of the list are dealt."""
    reads, params, host = pool
    assert -(-len(reads) // TILE) > workers
    monkeypatch.setenv("DNAS_FAKE_DEVICES", str(workers))
    for sketch, min_shared, floor in ((16, 2, NEG), (32, 1, 0.0)):
        opts = dict(sketch=sketch, min_shared=min_shared, min_score_per_nt=floor, **T_OPTS)
        one = da.clusterReads(params, reads, device=0, **opts)
        every = da.clusterReads(params, reads, device=-1, **opts)
        same_results(every, one)
        same_results(every, host[sketch, min_shared, floor])
        assert every.stats["chunks"] > one.stats["chunks"] == 1


def test_filter_last_tile_full_and_of_one_row(da, pool, monkeypatch):
    """Prefixes of pool T that end with a tile exactly full (64, 128, 192 reads) and with a tile of one row (65, 129), on one
    device and dealt to two workers; 141, 156, 682, 716 and 1614 candidates at sketch 16, min_shared 1."""
    reads, params, _ = pool
    for n in (TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE):
        opts = dict(sketch=16, min_shared=1, min_score_per_nt=NEG, **T_OPTS)
        want = da.clusterReads(params, reads[:n], host=True, **opts)
        assert want.stats["candidates"] == want.stats["edges"] > n // 4
        same_results(da.clusterReads(params, reads[:n], **opts), want)
        monkeypatch.setenv("DNAS_FAKE_DEVICES", "2")
        same_results(da.clusterReads(params, reads[:n], device=-1, **opts), want)
        monkeypatch.delenv("DNAS_FAKE_DEVICES")


def test_every_pair_on_four_tiles(da, monkeypatch):
    """min_shared = 0 on 3 tiles + 1 reads of 19 to 29 nt (193 reads, band 0): every one of the 18 528 pairs is a candidate, every
    row but the last few overflows the tile in every column tile it meets."""
    rng = random.Random("pair-hmm-edges/every-pair")
    n = 3 * TILE + 1
    reads = []
    for i in range(n):
        r = one_edit(rng, reads[rng.randrange(len(reads))]) if i % 3 == 2 else _rand(rng, rng.randint(21, 27))
        reads.append(r if 20 <= len(r) <= 28 else _rand(rng, 24))
    reads = [da.reverse_complement(r) if i % 4 == 1 else r for i, r in enumerate(reads)]
    params = da.MutatorParams.fromFlags(**NOISY)
    for floor in (NEG, 0.0):
        opts = dict(band=0, k=K, min_shared=0, min_score_per_nt=floor, edges=True)
        want = da.clusterReads(params, reads, host=True, **opts)
        assert want.stats["candidates"] == n * (n - 1) // 2 and (want.stats["edges"] == want.stats["candidates"]) == (floor == NEG)
        same_results(da.clusterReads(params, reads, **opts), want)
        monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
        every = da.clusterReads(params, reads, device=-1, **opts)
        monkeypatch.delenv("DNAS_FAKE_DEVICES")
        same_results(every, want)
        assert every.stats["chunks"] > 1


def test_sketch_grid_goes_round_twice(da, monkeypatch):
    """32 CUs + 3 reads of 10 to 16 nt: the sketch grid has 32 CUs waves, its last three reads are signed in a wave's second trip.
    With min_shared = sketch = 16 only reads with one signature are candidates, so the candidate list witnesses the signatures:
    about one read in a hundred is a planted copy (every other one turned round, which has the same signature), one pair of
    them lies beyond the first trip and one straddles it."""
    import torch
    first_trip = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    n = first_trip + 3
    rng = random.Random("pair-hmm-edges/sketch-stride")
    reads = [_rand(rng, rng.randint(10, 16)) for _ in range(n)]
    spots = rng.sample(range(6, n - 3), 2 * (n // 100))
    planted = [(n - 3, n - 1), (5, n - 2)] + [tuple(sorted(spots[2 * i:2 * i + 2])) for i in range(n // 100)]
    for q, (src, dst) in enumerate(planted):
        reads[dst] = da.reverse_complement(reads[src]) if q % 2 else reads[src]
    params = da.MutatorParams.fromFlags(**NOISY)
    opts = dict(band=0, k=K, sketch=16, min_shared=16, min_score_per_nt=NEG, edges=True)
    want = da.clusterReads(params, reads, host=True, **opts)
    listed = set((int(i), int(j)) for i, j in want.edges[0])
    assert set(planted) <= listed and want.stats["candidates"] == len(listed) < 4 * len(planted)
    assert any(i >= first_trip for i, _ in planted) and any(i < first_trip <= j for i, j in planted)
    print("sketch stride: %d reads, %d planted pairs, %d candidates" % (n, len(planted), len(listed)))
    same_results(da.clusterReads(params, reads, **opts), want)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    same_results(da.clusterReads(params, reads, device=-1, **opts), want)
