"""Phase C's per-state constants in the tier-A / tier-C fill kernel (csrc/viterbi_tiera.hip): what the duplication chain needs of
a state's meta word -- its own duplication depth mdl, its context bases, "this slot holds a real state" -- is loaded once per
work-group and kept in registers for the whole launch, two rows of 16 bits per register (PK, packed along the lattice's row
pairs), and the vote "every state of this wave's row has a full context" is one bit per row in a scalar register.  The
64-register programs (two work-groups of 1024 threads per CU, W8 in the plan key), the programs of more than 16 rows and the
widths D > 4 (a row's constants no longer fit 16 bits) keep one load per row and column.  Here both forms meet what a packing
mistake would get wrong: states of every depth 0 .. D in one row, a pair with one dead row, slots without a state next to
slots with one, every width D = 1 .. 8, a cluster whose rows are paired by the plan, a lattice segment that starts inside the
read, and a work-group that walks several reads with the same registers.

Every comparison is an equality with the CPU oracle: decoded string, fp64 log-likelihood bits, status and every lattice cell as
uint64 -- except in lattice segments, where no whole lattice exists by construction."""
import json
import os

import numpy as np
import pytest

import tiera_census as tc
from random_machines import random_machine, random_read, width_case, write_params

pytestmark = pytest.mark.gpu

FLAGS = dict(dup=.05, sub=.02, del_open=.02, del_ext=.1)
NO_PATH = 1      # DNAS_READ_NO_PATH
PLAN_ENV = ("DNAS_THREADS", "DNAS_PLAN_PICK", "DNAS_PLAN_ORDER", "DNAS_PLAN_SLACK", "DNAS_PLAN_REMOTE_ROWS", "DNAS_PLAN_OCCUPANCY")
_models = {}     # key -> (machine text, library machine, library params, oracle, reads)
_reference = {}  # (key, read) -> oracle result, computed once and shared


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("meta_registers")


@pytest.fixture(autouse=True)
def _plan_environment(monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _reads(text, D, n, seed):
    """n reads of 20 .. 60 bases -- longer than D, so that the first D columns, the wave-uniform chain and the general chain all
    run --, each with a tandem duplication of every length 1 .. D."""
    reads = []
    for i in range(200 * n):
        r = random_read(seed + i, text, max_len=56 - D, noise=.06, dups=D)
        if 20 <= len(r) <= 60:
            reads.append(r)
            if len(reads) == n:
                return reads
    raise AssertionError("the machine's walks are too short")


def _width_model(da, O, tmp, D, n_states, n_reads=3):
    """A width-case machine (most contexts D wide, the rest of every width below: mdl = 0 .. D side by side in one row; '*'
    contexts at D = 3, 5, 7) under a global error model with a non-uniform pLen."""
    key = ("width", D, n_states)
    if key not in _models:
        text, pLen = width_case(D, 70 + D, n_states)
        dp, op, _ = write_params(tmp, da, O, pLen, global_=True, **FLAGS)
        orc = O.ViterbiOracle(O.Machine.from_json(text), op)
        assert orc.D == D
        _models[key] = (text, da.Machine.fromJSON(text), dp, orc, _reads(text, D, n_reads, 7000 + 100 * D))
    return (key,) + _models[key]


def _fuzz_model(da, O, seed, n_states):
    """random_machine(seed): contexts of width 0, 1, 2 and 4 (D = 4), the CLI's default pLen, global alignment."""
    key = ("fuzz", seed, n_states)
    if key not in _models:
        text = random_machine(seed, n_states)
        flags = dict(FLAGS, global_=True)
        orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**flags))
        assert orc.D == 4
        _models[key] = (text, da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**flags), orc, _reads(text, 4, 3, 8000 + 100 * seed))
    return (key,) + _models[key]


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


def _program(dec, tier, D, packed):
    """The program the decoder compiled; packed: its constants sit in registers (D <= 4, at most 16 rows, not a 64-register
    program)."""
    assert dec.tier.startswith("tier " + tier), dec.tier
    prog = tc.program_of_model(dec)
    assert prog.D == D, dec.tier
    w8 = tc.KEY.search(dec.tier).group(11) == "8"
    assert packed == (D <= 4 and prog.K <= 16 and not w8), dec.tier
    return prog


def _depths(text):
    """The duplication depths of the machine's states: the width of the left context without its '*' prefix."""
    return set(len(st["l"].lstrip("*")) for st in json.loads(text)["state"])


def test_mixed_depths_in_full_pairs(da, oracle_mod, tmp):
    """1100 states over four rows of 512 threads, two whole pairs: depths 0 .. 4 side by side in every row, so no wave takes the
    wave-uniform chain for all of its rows and every field of both halves of a register is used."""
    key, text, m, dp, orc, reads = _width_model(da, oracle_mod, tmp, 4, 1100)
    assert _depths(text) == {0, 1, 2, 3, 4}
    dec = da.ViterbiDecoder(m, dp, options="tier=A,threads=512")
    prog = _program(dec, "A", 4, True)
    assert prog.K == 4 and all(r[0] >= 0 for r in prog.rows), dec.tier
    _check(dec, key, orc, reads, dec.decode(reads))
    dec.close()


def test_last_pair_with_a_dead_row(da, oracle_mod, tmp):
    """1300 states plan to three live rows and an empty one: the last pair's register holds one row's constants and a half-word
    of zeros, and every live row has slots without a state (the machine fills 55 % of them)."""
    key, text, m, dp, orc, reads = _width_model(da, oracle_mod, tmp, 4, 1300)
    dec = da.ViterbiDecoder(m, dp, options="tier=A,threads=512")
    prog = _program(dec, "A", 4, True)
    dead = [k for k, r in enumerate(prog.rows) if r[0] < 0]
    assert prog.K == 4 and len(dead) == 1 and prog.pairs_identity, dec.tier
    _check(dec, key, orc, reads, dec.decode(reads))
    dec.close()


@pytest.mark.parametrize("seed,n_states", [(1, 150), (2, 300), (3, 400)])
def test_holes_in_every_row(da, oracle_mod, seed, n_states):
    """The fuzz machines of at most 400 states on 512 threads: one live row with more empty slots than states, paired with a dead
    row -- invalid slots (constants 0: never valid, depth 0) in the same waves as valid ones, of depths 0, 1, 2 and 4."""
    key, text, m, dp, orc, reads = _fuzz_model(da, oracle_mod, seed, n_states)
    dec = da.ViterbiDecoder(m, dp, options="tier=A,threads=512")
    prog = _program(dec, "A", 4, True)
    assert prog.K == 2 and prog.rows[1][0] < 0, dec.tier
    _check(dec, key, orc, reads, dec.decode(reads))
    dec.close()


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_width(da, oracle_mod, tmp, D):
    """D = 1 .. 8 on 700 states in one pair of rows of 512 threads.  Up to D = 4 the context (2 D bits) fits the packed form; D > 4
    keeps the per-column loads -- both against every lattice cell."""
    key, text, m, dp, orc, reads = _width_model(da, oracle_mod, tmp, D, 700, n_reads=2)
    dec = da.ViterbiDecoder(m, dp, options="tier=A,threads=512")
    prog = _program(dec, "A", D, D <= 4)
    assert prog.K == 2 and all(r[0] >= 0 for r in prog.rows), dec.tier
    _check(dec, key, orc, reads, dec.decode(reads))
    dec.close()


def test_cluster_with_planned_pairs(oracle_mod, monkeypatch):
    """The fan2-c2 shape of tests/tiera_census.py: two members whose rows the plan pairs by fill (DNAS_PAIRS is not the identity),
    so a register's halves are rows that are no neighbours, and the mask of live pairs (pairValid) comes from the same loads."""
    import dnastore_amd as da
    case = {c.id: c for c in tc.SHAPED_CASES}["fan2-c2"]
    monkeypatch.setenv("DNAS_THREADS", str(case.threads))
    text = tc.shaped_text(case)
    flags = dict(sub=.02, dup=.01, del_open=.02, del_ext=.1, global_=True)
    dec = da.ViterbiDecoder(da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**flags), options=tc.model_options(case))
    prog = _program(dec, "C", 4, True)
    assert prog.G == 2 and not prog.pairs_identity, dec.tier
    orc = oracle_mod.ViterbiOracle(oracle_mod.Machine.from_json(text), oracle_mod.MutatorParams.from_cli(**flags))
    reads = [r for r in tc.shaped_reads(text) if 20 <= len(r) <= 60]
    assert len(reads) == 2
    _check(dec, "fan2-c2", orc, reads, dec.decode(reads, out_cap=4096))
    dec.close()


def test_two_work_groups_per_cu(da, oracle_mod, ref_data):
    """h74l4c4 (six rows, 64 registers, two work-groups of 1024 threads per CU): the form that keeps the loads."""
    O = oracle_mod
    path = os.path.join(ref_data, "h74l4c4.json")
    m = da.Machine.fromFile(path)
    orc = O.ViterbiOracle(O.Machine.from_file(path), O.MutatorParams.from_cli(global_=True))
    dna = list(m.encodeBytes(b"MI355X"))
    dna[7] = "ACGT"[("ACGT".index(dna[7]) + 1) % 4]
    dna[20:20] = dna[17:20]      # a tandem duplication of three bases
    dna = "".join(dna)
    reads = [dna[:24], dna[:41]]
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True))
    prog = _program(dec, "A", 4, False)
    assert prog.T == 1024 and prog.K <= 8, dec.tier
    _check(dec, "h74l4c4", orc, reads, dec.decode(reads))
    dec.close()


def test_segment_starts_inside_the_read(da, oracle_mod, tmp):
    """Bounded-memory decode (the DNAS_SEGMENTS=1 compile) in segments of 6 and 9 columns: every launch but a read's first starts
    at a column c0 > 0 with registers it loaded itself.  No whole lattice exists: strings, log-likelihood bits and status."""
    key, text, m, dp, orc, reads = _width_model(da, oracle_mod, tmp, 4, 1300)
    for seg in (6, 9):
        dec = da.ViterbiDecoder(m, dp, options="tier=A,threads=512,checkpoint=always,segment=%d" % seg)
        _program(dec, "A", 4, True)
        got = dec.decode(reads)
        assert dec.stats()["checkpointed_reads"] == len(reads)
        _check(dec, key, orc, reads, got, lattice=False)
        dec.close()


def test_one_work_group_walks_several_reads(da, oracle_mod, tmp):
    """One cluster of two work-groups, five reads in one launch: the registers are loaded in front of the read loop and must be
    what they were when the second, third ... read is filled (a long read, short ones, an empty one in between)."""
    key, text, m, dp, orc, reads = _width_model(da, oracle_mod, tmp, 4, 1300)
    reads = [reads[0], reads[1][:21], "", reads[2], reads[0][3:30]]
    dec = da.ViterbiDecoder(m, dp, options="tier=C,cluster=2,threads=512,max_clusters=1")
    _program(dec, "C", 4, True)
    got = dec.decode(reads)
    assert dec.cluster_census()[0] == 1
    _check(dec, key, orc, reads, got)
    dec.close()
