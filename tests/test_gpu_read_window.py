"""How the read reaches the tier-A / tier-C fill kernel (csrc/viterbi_tiera.hip): a window of bases in scalar registers -- the
last bases as one packed word, the next ones out of an aligned 4-byte word of the caller's `bases` buffer that is loaded a
column before its first byte is used, and only if it holds a byte of the read.  The window can go wrong at its boundaries: reads
shorter than the duplication depth, refills at every 4th byte, reads that start at every residue mod 8 of the buffer, the first
and the last word of a buffer, a lattice segment that starts inside the read, a work-group that walks several reads.

Every comparison is an equality with the CPU oracle: decoded string, fp64 log-likelihood bits, status and every lattice cell as
uint64 -- except where no whole lattice exists by construction (bounded-memory segments, both-strand calls)."""
import os
import re

import numpy as np
import pytest

from random_machines import random_read, width_case, write_params

pytestmark = pytest.mark.gpu

FLAGS = dict(dup=.05, sub=.02, del_open=.02, del_ext=.1)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 70)     # history shorter than D; refills fall at multiples of 4 (and of 8)
NO_PATH = 1
_cases = {}        # D -> (machine text, library machine, library params, oracle, long read)
_reference = {}    # (D or machine name, read) -> oracle result, computed once and shared


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq))


def _case(da, O, tmp, D):
    """A width-case machine of 150 states with D duplication lanes (global alignment), and one read of 90 bases or more with a
    duplication of every length 1..D in it; the reads of the tests are pieces of it."""
    if D not in _cases:
        text, pLen = width_case(D, 70 + D, 150)
        dp, op, _ = write_params(tmp, da, O, pLen, global_=True, **FLAGS)
        orc = O.ViterbiOracle(O.Machine.from_json(text), op)
        assert orc.D == D
        long_ = ""
        for seed in range(400):
            long_ += random_read(9000 + 100 * D + seed, text, max_len=60, noise=.06, dups=D)
            if len(long_) >= 90:
                break
        assert len(long_) >= 90
        _cases[D] = (text, da.Machine.fromJSON(text), dp, orc, long_)
    return _cases[D]


def _want(key, orc, read, lattice):
    k = (key, read)
    if k not in _reference or (lattice and _reference[k][2] is None):
        _reference[k] = orc.decode(read, want_lattice=True) if lattice else orc.decode(read) + (None,)
    return _reference[k]


def _check(dec, key, orc, reads, got, lattice=True):
    out, ll, st = got[:3]
    for i, r in enumerate(reads):
        s, oll, olat = _want(key, orc, r, lattice)
        assert out[i] == s and _bits(ll[i]) == _bits(oll), (i, r, out[i], s, ll[i], oll)
        assert st[i] == (NO_PATH if oll == -np.inf else 0), (i, r, st[i], oll)
        if lattice:
            lat = np.ascontiguousarray(dec.lattice(i, len(r)).transpose(0, 2, 1))      # [L+1][N][lanes], the oracle's layout
            assert lat.shape == olat.shape and not np.isnan(lat).any(), (i, r)
            assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64)), (i, r)


def _tier_a(dec, D, two_per_cu):
    assert dec.tier.startswith("tier A"), dec.tier
    shape = re.search(r"T(\d+)K(\d+)D(\d+)S", dec.tier)
    assert int(shape.group(1)) == 1024 and int(shape.group(3)) == D, dec.tier
    assert (int(shape.group(2)) <= 8) == two_per_cu, dec.tier      # programs of at most 8 rows: two work-groups to a CU


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("read_window")


@pytest.mark.parametrize("D", [4, 8])
def test_lengths(da, oracle_mod, tmp, D):
    """Reads of 0 .. 17 and 70 bases in one call, at D = 4 and at D = 8 (the widest window: nine bases of history and look-ahead).
    The program has at most 8 rows: two work-groups share a CU."""
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    reads = [long_[:n] for n in LENGTHS]
    dec = da.ViterbiDecoder(m, dp, options="tier=A")
    _tier_a(dec, D, True)
    _check(dec, D, orc, reads, dec.decode(reads))
    dec.close()


@pytest.mark.parametrize("D", [4, 8])
def test_every_start_alignment(da, oracle_mod, tmp, D):
    """Reads of odd lengths packed back to back: the reads start at every residue mod 8 of the buffer, so the first word of a read
    holds 8, 7, .. 1 of its bases and the refills fall at every column residue."""
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    lens = [9, 17, 9, 25, 17, 9, 9, 17, 11]
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    assert set(int(s) % 8 for s in starts) == set(range(8))
    reads = [long_[3 * i:3 * i + n] for i, n in enumerate(lens)]
    dec = da.ViterbiDecoder(m, dp, options="tier=A")
    _check(dec, D, orc, reads, dec.decode(reads))
    dec.close()


def test_first_and_last_word_of_the_buffer(da, oracle_mod, tmp):
    """Device pointers as a caller hands them over: a buffer allocated at exactly the packed size, the first read at its first
    byte, the last read ending with its last byte (in the middle of an aligned word: 9 + 17 + 12 = 38 bytes)."""
    import torch
    from dnastore_amd import pack_reads
    D = 4
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    reads = [long_[:9], long_[20:37], long_[40:52]]
    off, bases = pack_reads(reads)
    assert bases.nbytes == 38 and int(off[-1]) == 38
    k = len(reads)
    cap = int(np.diff(off).max()) * 4 + 64
    out_off = np.arange(k + 1, dtype=np.uint64) * np.uint64(cap)
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
    assert d_bases.numel() == 38
    d_sym = torch.zeros(k * cap, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(k, dtype=torch.int32, device=dev)
    d_ll = torch.zeros(k, dtype=torch.float64, device=dev)
    d_st = torch.zeros(k, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()    # torch's copies / fills are done before the library's own streams touch the buffers
    dec = da.ViterbiDecoder(m, dp, options="tier=A")
    dec.decode_device(off, d_bases.data_ptr(), d_sym.data_ptr(), out_off, d_len.data_ptr(), d_ll.data_ptr(), d_st.data_ptr())
    dec.sync()
    sym, olen = d_sym.cpu().numpy(), d_len.cpu().numpy()
    out = [sym[i * cap:i * cap + int(olen[i])].tobytes().decode() for i in range(k)]
    _check(dec, D, orc, reads, (out, d_ll.cpu().numpy(), d_st.cpu().numpy()))
    dec.close()


@pytest.mark.parametrize("D,seg", [(4, 6), (4, 9), (8, 10), (8, 13)])
def test_segments_start_anywhere(da, oracle_mod, tmp, D, seg):
    """Bounded-memory decode in short segments (the minimum width D + 2, and an odd one): a launch starts at a column c0 > 0 and
    takes up x_{c0} .. x_{c0-D+1}; with segments of 9 and 13 columns c0 meets every residue mod 8, and the reads start at
    different residues of the buffer besides.  No whole lattice exists: strings, log-likelihood bits and status."""
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    reads = [long_[:85], long_[1:12], long_[2:40], "", long_[5:6], long_[7:80]]
    dec = da.ViterbiDecoder(m, dp, options="tier=A,checkpoint=always,segment=%d" % seg)
    _tier_a(dec, D, True)
    got = dec.decode(reads)
    assert dec.stats()["checkpointed_reads"] == len(reads)
    _check(dec, D, orc, reads, got, lattice=False)
    dec.close()


def test_both_strands(da, oracle_mod, tmp):
    """Both orientations of every read: the reverse complements are written by a kernel of the call's prologue, ahead of the
    fills that read them through the scalar cache."""
    D = 4
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    given = [long_[:n] for n in (1, 7, 8, 9, 17, 70)] + [_revcomp(long_[3:44]), _revcomp(long_[10:19])]
    dec = da.ViterbiDecoder(m, dp, options="tier=A")
    out, ll, st, strand = dec.decode(given, strands="both")
    for i, g in enumerate(given):
        f = _want(D, orc, g, False)
        b = _want(D, orc, _revcomp(g), False)
        rev = b[1] > f[1]
        s, oll = (b if rev else f)[:2]
        assert out[i] == s and _bits(ll[i]) == _bits(oll) and strand[i] == int(rev), (i, g, out[i], s, ll[i], oll, strand[i])
        assert st[i] == (NO_PATH if oll == -np.inf else 0), (i, st[i])
    dec.close()


def test_one_work_group_per_cu(da, oracle_mod, ref_data):
    """The 14-row program of the 12 361-state machine (one work-group per CU, the shape bench.py runs): short reads over the
    window's seams, every lattice cell."""
    O = oracle_mod
    path = os.path.join(ref_data, "s16h74l4c4.json")
    m = da.Machine.fromFile(path)
    orc = O.ViterbiOracle(O.Machine.from_file(path), O.MutatorParams.from_cli(global_=True))
    dna = list(m.encodeBytes(b"MI"))
    dna[7] = "ACGT"[("ACGT".index(dna[7]) + 1) % 4]
    dna = "".join(dna)
    reads = [dna[:n] for n in (0, 1, 5, 8, 9, 17)]
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True))
    _tier_a(dec, 4, False)
    _check(dec, "s16h74l4c4", orc, reads, dec.decode(reads))
    dec.close()


@pytest.mark.parametrize("D", [4, 8])
def test_cluster_of_two(da, oracle_mod, tmp, D):
    """A cluster of two work-groups (tier C) on the same reads: every member keeps its own window."""
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    reads = [long_[:n] for n in LENGTHS]
    dec = da.ViterbiDecoder(m, dp, options="tier=C,cluster=2")
    assert dec.tier.startswith("tier C: 2 work-groups"), dec.tier
    _check(dec, D, orc, reads, dec.decode(reads))
    dec.close()


def test_cluster_fixture_machine(da, oracle_mod, ref_data):
    """The small cluster fixture of test_gpu_tier_c.py (l4c4, two members of 512 threads) on its golden read."""
    O = oracle_mod
    path = os.path.join(ref_data, "l4c4.json")
    flags = dict(sub=0., del_open=0., global_=True)
    dec = da.ViterbiDecoder(da.Machine.fromFile(path), da.MutatorParams.fromFlags(**flags), options="tier=C,cluster=2,threads=512")
    assert dec.tier.startswith("tier C: 2 work-groups"), dec.tier
    orc = O.ViterbiOracle(O.Machine.from_file(path), O.MutatorParams.from_cli(**flags))
    read = da.read_fastseqs(os.path.join(ref_data, "hello.dup.fa"))[0][1]
    reads = [read, read[3:20], read[:8]]
    _check(dec, "l4c4", orc, reads, dec.decode(reads))
    dec.close()


def test_one_cluster_walks_several_reads(da, oracle_mod, tmp):
    """One cluster, seven reads in one launch: the work-groups go from read to read, and the window (like the early-offer state) is
    set up again for each -- a long read, then short ones whose whole length is less than what the window held."""
    D = 4
    text, m, dp, orc, long_ = _case(da, oracle_mod, tmp, D)
    reads = [long_[:70], long_[5:8], "", long_[11:28], long_[2:3], long_[30:85], long_[1:10]]
    dec = da.ViterbiDecoder(m, dp, options="tier=C,cluster=2,max_clusters=1")
    assert dec.tier.startswith("tier C: 2 work-groups"), dec.tier
    got = dec.decode(reads)
    assert dec.cluster_census()[0] == 1
    _check(dec, D, orc, reads, got)
    dec.close()
