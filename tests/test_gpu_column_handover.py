"""How the tier-A fill kernel hands a lattice column over to the next one (csrc/viterbi_tiera.hip, one work-group per read): the
emit offers of column p + 1 are made inside phase C of column p, an arrival counter in LDS says when all waves have made theirs,
and the take runs in front of the single barrier that separates the two columns.  Column 0, the first column of a lattice
segment, the last column and every cluster keep the offers-barrier-take-barrier route.  The cases here sit on the seams between
the two routes: reads so short that the first early-offered column is the last but one, history shorter than the duplication
depth, segments of the minimum width, several reads of different lengths per launch and a second call on the same model.

Every comparison is an equality with the CPU oracle: decoded string, fp64 log-likelihood bits, and every lattice cell as uint64
(dnas_model_read_lattice) -- except in the segment case, where no whole lattice exists by construction (test_gpu_checkpoint.py)
and the string and the log-likelihood carry the check."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHORT = (0, 1, 2, 3, 4, 5, 9)          # D = 4: first and last column, history shorter than D, the first full history
_reference = {}                        # (machine, global_, read) -> oracle result, computed once and shared
_oracles = {}                          # (machine, global_) -> oracle


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq))


def _machines(da, O, ref_data, mach):
    path = os.path.join(ref_data, mach)
    return da.Machine.fromFile(path), O.Machine.from_file(path)


def _want(O, omach, mach, global_, read, lattice=True, params=None):
    """global_: True or False for the default error model in that mode, or -- with params, an oracle MutatorParams -- the name
    under which the two caches know that model."""
    key = (mach, global_, read)
    if key not in _reference or (lattice and _reference[key][2] is None):
        if (mach, global_) not in _oracles:
            _oracles[(mach, global_)] = O.ViterbiOracle(omach, params or O.MutatorParams.from_cli(global_=global_))
        orc = _oracles[(mach, global_)]
        _reference[key] = orc.decode(read, want_lattice=True) if lattice else orc.decode(read) + (None,)
    return _reference[key]


def _check(dec, O, omach, mach, global_, reads, got, lattice=True, params=None):
    out, ll, st = got[:3]
    for i, r in enumerate(reads):
        s, oll, olat = _want(O, omach, mach, global_, r, lattice, params)
        assert out[i] == s and bits(ll[i]) == bits(oll), (i, r, out[i], s, ll[i], oll)
        assert st[i] == (1 if s == "" and np.isinf(oll) else 0), (i, r, st[i])
        if lattice:
            lat = np.ascontiguousarray(dec.lattice(i, len(r)).transpose(0, 2, 1))      # [L+1][N][lanes], the oracle's layout
            assert lat.shape == olat.shape
            assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64)), (i, r)


def _message(m, payload, flip):
    """An encoded payload with one substituted base."""
    dna = list(m.encodeBytes(payload))
    dna[flip] = "ACGT"[("ACGT".index(dna[flip]) + 1) % 4]
    return "".join(dna)


def _tier_a(dec, two_per_cu):
    assert dec.tier.startswith("tier A"), dec.tier
    shape = re.search(r"T(\d+)K(\d+)", dec.tier)
    assert int(shape.group(1)) == 1024, dec.tier
    # programs of at most 8 rows run in 64 registers, two work-groups to a CU (host/plan.cpp); the 12 361-state machine's has 14
    assert (int(shape.group(2)) <= 8) == two_per_cu, dec.tier


@pytest.mark.parametrize("global_", [True, False], ids=["global", "local"])
@pytest.mark.parametrize("mach,two_per_cu", [("s16h74l4c4.json", False), ("h74l4c4.json", True)])
def test_short_reads(da, oracle_mod, ref_data, mach, two_per_cu, global_):
    """0, 1, 2, 3, 4, 5 and 9 nt: at 1 nt the only early-offered column is column 0, at 2 nt the first one taken early is the last."""
    m, om = _machines(da, oracle_mod, ref_data, mach)
    dna = _message(m, b"MI", 7)
    reads = [dna[:n] for n in SHORT]
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=global_))
    _tier_a(dec, two_per_cu)
    _check(dec, oracle_mod, om, mach, global_, reads, dec.decode(reads))
    dec.close()


def _forty(m):
    dna = _message(m, b"Hi", 11)
    assert 30 <= len(dna) <= 60, len(dna)
    return dna


def test_whole_read_global_and_local(da, oracle_mod, ref_data):
    """One read of about 40 nt, whole lattice, in both alignment modes."""
    mach = "s16h74l4c4.json"
    m, om = _machines(da, oracle_mod, ref_data, mach)
    read = _forty(m)
    for global_ in (True, False):
        dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=global_))
        _tier_a(dec, False)
        _check(dec, oracle_mod, om, mach, global_, [read], dec.decode([read]))
        dec.close()


def test_minimum_segments(da, oracle_mod, ref_data):
    """The same read in lattice segments of the minimum width (D + 2 columns): c0 and c1 inside the read, the hand-over parked
    behind a segment and picked up by the next launch, whose arrival counter starts at zero again."""
    mach = "s16h74l4c4.json"
    m, om = _machines(da, oracle_mod, ref_data, mach)
    read = _forty(m)
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True), options="checkpoint=always,segment=6")
    assert dec.max_dup_len == 4
    _tier_a(dec, False)
    got = dec.decode([read])
    stats = dec.stats()
    assert stats["checkpointed_reads"] == 1 and stats["fill_launches"] >= len(read) // 6
    _check(dec, oracle_mod, om, mach, True, [read], got, lattice=False)
    dec.close()


def test_both_strands(da, oracle_mod, ref_data):
    mach = "s16h74l4c4.json"
    m, om = _machines(da, oracle_mod, ref_data, mach)
    read = _forty(m)
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True))
    for given in (read, _revcomp(read)):
        out, ll, st, strand = dec.decode([given], strands="both")
        f = _want(oracle_mod, om, mach, True, given, lattice=False)
        b = _want(oracle_mod, om, mach, True, _revcomp(given), lattice=False)
        rev = b[1] > f[1]
        s, oll = (b if rev else f)[:2]
        assert out[0] == s and bits(ll[0]) == bits(oll) and strand[0] == int(rev), (out[0], s, ll[0], oll, strand[0])
    dec.close()


def test_several_reads_per_launch_and_a_second_call(da, oracle_mod, ref_data):
    """Three reads of different lengths in one launch, then a second call on the same model: every read's counter starts at zero
    and counts its own columns."""
    mach = "s16h74l4c4.json"
    m, om = _machines(da, oracle_mod, ref_data, mach)
    long_ = _forty(m)
    reads = [long_, long_[:9], long_[:23]]
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True))
    _check(dec, oracle_mod, om, mach, True, reads, dec.decode(reads))
    again = [reads[2], reads[0]]
    _check(dec, oracle_mod, om, mach, True, again, dec.decode(again))
    dec.close()


def test_cluster_route_unchanged(da, oracle_mod, ref_data):
    """A cluster of two work-groups (tier C) keeps barrier, fold, take, barrier: one read, every cell against the oracle."""
    mach = "s16h74l4c4.json"
    m, om = _machines(da, oracle_mod, ref_data, mach)
    read = _forty(m)
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True), options="tier=C,cluster=2")
    assert dec.tier.startswith("tier C"), dec.tier
    _check(dec, oracle_mod, om, mach, True, [read], dec.decode([read]))
    dec.close()
