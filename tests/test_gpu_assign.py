"""dnas_assign_reads on the GPU (csrc/assign_kernels.hip) against its host statement dnas_assign_reads_host: item scores,
winners, runners-up and statuses must be bit-identical, whatever the shapes, the band, the grid, the chunking and the number of
devices."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import BANDS, NOISY, _bits, _rand, models, planted_pool, shape_pool  # noqa: E402


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _same(got, want, items=True):
    assert len(got) == len(want)
    assert np.array_equal(got.original, want.original), (got.original, want.original)
    assert np.array_equal(got.strand, want.strand) and np.array_equal(got.status, want.status)
    assert np.array_equal(_bits(got.score), _bits(want.score)), np.flatnonzero(_bits(got.score) != _bits(want.score))
    assert np.array_equal(_bits(got.second), _bits(want.second)), np.flatnonzero(_bits(got.second) != _bits(want.second))
    if items:
        assert len(got.item_scores) == len(want.item_scores)
        for i, (a, b) in enumerate(zip(got.item_scores, want.item_scores)):
            assert np.array_equal(_bits(a), _bits(b)), (i, np.flatnonzero(_bits(a) != _bits(b)))


@pytest.fixture(scope="module")
def planted(da):
    """(originals, reads, truth, params, the host's result at band 16), computed once."""
    originals, reads, truth = planted_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    return originals, reads, truth, params, da.assignReads(params, originals, reads, band=16, host=True, item_scores=True)


def test_every_shape_model_and_band(da, monkeypatch):
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves over 336 items: every wave walks many
    monkeypatch.setenv("DNAS_ASSIGN_CHUNK", "37")          # a prime: chunks end inside reads' item runs and between strands
    originals, reads = shape_pool(da)
    statuses = set()
    for name, params in models(da):
        for band in BANDS:
            want = da.assignReads(params, originals, reads, band=band, host=True, item_scores=True)
            got = da.assignReads(params, originals, reads, band=band, item_scores=True)
            _same(got, want)
            assert got.stats["chunks"] == -(-336 // 37) > 1 and got.stats["items"] == 336 and got.stats["cells"] > 0
            statuses |= set(int(s) for s in got.status)
    assert statuses == {da.lib.ASSIGN_OK, da.lib.ASSIGN_NO_PATH}
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the chunk as shipped, one strand at a time
    monkeypatch.delenv("DNAS_ASSIGN_CHUNK")
    name, params = models(da)[2]
    for strands in ("forward", "reverse", "both"):
        got = da.assignReads(params, originals, reads, band=8, strands=strands, item_scores=True)
        _same(got, da.assignReads(params, originals, reads, band=8, strands=strands, host=True, item_scores=True))
        assert got.stats["chunks"] == 1


def test_boundary_row_beyond_lds(da):
    """An original and a read of more than 1015 bases: the stripes hand their last row on through HBM instead of LDS."""
    from test_gpu_pair_align import _related
    rng = random.Random("gpu-assign/long")
    params = da.MutatorParams.fromFlags(**NOISY)
    a = _rand(rng, 1100)
    originals = [_rand(rng, 1100), a, a[:200]]
    reads = [da.reverse_complement(_related(rng, a, 1104)), _related(rng, a[:200], 198)]
    got = da.assignReads(params, originals, reads, band=8, item_scores=True)
    _same(got, da.assignReads(params, originals, reads, band=8, host=True, item_scores=True))
    assert list(got.original) == [1, 2] and list(got.strand) == [1, 0]


def test_score_is_the_alignments(da, planted):
    originals, reads, truth, params, want = planted
    got = da.assignReads(params, originals, reads, band=16)
    _same(got, want, items=False)
    assert [(int(k), int(s)) for k, s in zip(got.original, got.strand)] == truth and (got.margin > 0).all()
    ins, outs, kept = got.pairs()
    assert kept == list(range(len(reads)))
    assert np.array_equal(_bits(da.alignPairs(params, ins, outs, band=16).score), _bits(got.score))


def test_all_devices(da, planted, monkeypatch):
    originals, reads, truth, params, want = planted
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    one = da.assignReads(params, originals, reads, band=16, device=0, item_scores=True)
    many = da.assignReads(params, originals, reads, band=16, device=-1, item_scores=True)
    _same(many, one)
    _same(many, want)
    assert many.stats["cells"] == one.stats["cells"] and many.stats["items"] == one.stats["items"] and many.stats["chunks"] == 3
    cands = [[(i + d) % 12 for d in range(i % 4)] for i in range(len(reads))]               # lists of 0 to 3, dealt with their reads
    _same(da.assignReads(params, originals, reads, band=16, device=-1, candidates=cands, item_scores=True),
          da.assignReads(params, originals, reads, band=16, candidates=cands, host=True, item_scores=True))
    two = da.assignReads(params, originals, reads[:2], band=16, device=-1, item_scores=True)  # fewer reads than devices
    _same(two, da.assignReads(params, originals, reads[:2], band=16, host=True, item_scores=True))
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.assignReads(params, originals, reads, device=-2)


def test_handle_reuse(da, planted):
    originals, reads, truth, params, want = planted
    h = da.Assigner(params, originals, band=16)
    cands = [[truth[i][0], (i * 5) % 12, 3] for i in range(20)]
    calls = ((reads, "both", None), (reads[:7], "forward", None), (reads[5:25], "reverse", cands), (reads, "both", None))
    for sub, strands, cand in calls:
        got = h.assign(sub, strands=strands, candidates=cand, item_scores=True)
        _same(got, da.assignReads(params, originals, sub, band=16, strands=strands, candidates=cand, item_scores=True))
        _same(got, da.assignReads(params, originals, sub, band=16, strands=strands, candidates=cand, host=True, item_scores=True))
    _same(got, want)
    empty = h.assign([])
    assert len(empty) == 0 and empty.stats["chunks"] == 0 and empty.stats["items"] == 0
    h.close()
    none = da.assignReads(params, [], reads[:3])
    assert list(none.status) == [da.lib.ASSIGN_NO_CANDIDATES] * 3 and none.stats["chunks"] == 0
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.assignReads(params, originals, reads[:1], candidates=[[12]])
