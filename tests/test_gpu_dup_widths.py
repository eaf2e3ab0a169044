"""Every duplication width against the oracle.  The fill tiers, both tracebacks, the node records and the bounded-memory
segments are compiled for one width D = min(widest left context, len(pLen)) (host/model.cpp); the fixture machines all give
D = 4.  Here random machines (60-400 states, tests/random_machines.py WIDTH_CASES) with contexts of every width up to 32, some
'*'-prefixed, run under non-uniform pLen (strictly decreasing, strictly increasing, one entry 0) read from one JSON file by
both sides, on reads that carry a tandem duplication of every length 1..D.  Decoded strings, fp64 log-likelihood bits,
status and every lattice cell (all D + 2 lanes, as uint64) are held to the oracle."""
import json
import re

import numpy as np
import pytest

from random_machines import random_read, width_case, write_params

pytestmark = pytest.mark.gpu

FLAGS = dict(dup=.05, sub=.02, del_open=.02, del_ext=.1)
TIER_OPTIONS = {"A": "tier=A", "B": "tier=B", "C": "tier=C,cluster=%d"}
NO_PATH = 1      # DNAS_READ_NO_PATH


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _model(da, O, tmp_path, D, global_, n_states=150, seed=None, shape=None, no_t=False, **flags):
    text, pLen = width_case(D, 70 + D if seed is None else seed, n_states, shape)
    if no_t:
        text = _without_t(text)
    dp, op, _ = write_params(tmp_path, da, O, pLen, global_=global_, **dict(FLAGS, **flags))
    m = da.Machine.fromJSON(text)
    orc = O.ViterbiOracle(O.Machine.from_json(text), op)
    assert orc.D == D
    return text, m, dp, orc


def _reads(text, D, n, seed, max_len=30, noise=.06):
    """n reads of 12 bases or more (walks that end early are passed over), each with a duplication of every length 1..D."""
    reads = []
    for i in range(50 * n):
        r = random_read(seed + i, text, max_len=max_len, noise=noise, dups=D)
        if len(r) >= 12:
            reads.append(r)
            if len(reads) == n:
                return reads
    raise AssertionError("the machine's walks are too short")


def _without_t(text):
    """The machine with every T it emits, and every T of its contexts, made an A: under sub = 0 a read with a T has no path (no
    edge emits it, and a duplication copies context bases)."""
    j = json.loads(text)
    for st in j["state"]:
        st["l"] = st["l"].replace("T", "A")
        for t in st["trans"]:
            if t.get("out") == "T":
                t["out"] = "A"
    return json.dumps(j)


def _options(tier, D):
    return TIER_OPTIONS[tier] % (2 + D % 2) if tier == "C" else TIER_OPTIONS[tier]


def _assert_tier(dec, tier, D):
    note = dec.tier
    assert note.startswith("tier " + tier), note
    if tier == "B":
        assert note.endswith("(D%d)" % D), note
    else:
        assert re.search(r"K\d+D%dS" % D, note), note


def _same_ll(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _check(dec, orc, reads, lattice=True, where=None):
    out, ll, st = dec.decode(reads)
    for i, r in enumerate(reads):
        if lattice:
            s, oll, olat = orc.decode(r, want_lattice=True)
        else:
            s, oll = orc.decode(r)
        assert out[i] == s and _same_ll(ll[i], oll), (where, i, r, out[i], s, ll[i], oll)
        assert st[i] == (NO_PATH if oll == -np.inf else 0), (where, i, st[i], oll)
        if lattice:
            lat = np.ascontiguousarray(dec.lattice(i, len(r)).transpose(0, 2, 1))
            assert lat.shape == olat.shape and not np.isnan(lat).any(), where
            assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64)), (where, i)
    return out, ll, st


@pytest.mark.parametrize("D", [0, 1, 2, 3, 5, 6, 7, 8])
@pytest.mark.parametrize("tier", ["A", "B", "C"])
def test_every_dup_width_on_every_tier(da, oracle_mod, tmp_path, D, tier):
    """D = 0..8 on tiers A, B and C (a cluster of 2 or 3), local and global: the width cases take D from the contexts at some widths
    and from pLen (contexts wider than P) at others, carry wildcard contexts (the general chain) at D = 3, 5, 7, and mostly full
    contexts (the wave-uniform chain) everywhere."""
    for global_ in (False, True):
        text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, global_)
        dec = da.ViterbiDecoder(m, dp, options=_options(tier, D))
        _assert_tier(dec, tier, D)
        _check(dec, orc, _reads(text, D, 6, 1000 * D), where=(D, tier, global_))
        dec.close()


@pytest.mark.parametrize("D", [9, 12, 16, 32])
def test_widths_beyond_tier_a(da, oracle_mod, tmp_path, D):
    """D = 9..32: tier B alone.  The default falls back to it; tier A or a cluster asked for by name are refused; tier B is bit-exact."""
    for global_ in (False, True):
        text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, global_, n_states=100)
        for opts in ("tier=A", "tier=C,cluster=2"):
            with pytest.raises(da.DnasError, match="more than 8 duplication lanes"):
                da.ViterbiDecoder(m, dp, options=opts)
        dec = da.ViterbiDecoder(m, dp)
        _assert_tier(dec, "B", D)
        _check(dec, orc, _reads(text, D, 3, 2000 * D, max_len=24), where=(D, global_))
        dec.close()


def test_plen_of_33_entries_is_refused(da, oracle_mod, tmp_path):
    """The library's limit: 33 pLen entries are refused with a message naming the 32-entry limit (the oracle has no such limit)."""
    text, pLen = width_case(32, 5, 60)
    with pytest.raises(da.DnasError, match="32 entries"):
        write_params(tmp_path, da, oracle_mod, pLen + [0.01])


@pytest.mark.parametrize("D", [1, 3, 5, 8])
def test_tracebacks_at_other_widths(da, oracle_mod, tmp_path, D, monkeypatch):
    """Both traceback kernels, from the node records (D <= 4) and through the CSR arrays (DNAS_NO_NODE_RECORDS; the only way at
    D > 4): the oracle's strings and log-likelihood bits, local and global."""
    for global_ in (False, True):
        text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, global_)
        reads = _reads(text, D, 24, 3000 * D)
        for records in (True, False):
            if records:
                monkeypatch.delenv("DNAS_NO_NODE_RECORDS", raising=False)
            else:
                monkeypatch.setenv("DNAS_NO_NODE_RECORDS", "1")
            for opts in (None, "traceback=thread"):
                dec = da.ViterbiDecoder(m, dp, options=opts)
                _check(dec, orc, reads, lattice=False, where=(D, global_, records, opts))
                dec.close()


def test_duplication_events_at_width_6(da, oracle_mod, tmp_path):
    """The level-3 event log at D = 6: the wave and thread kernels give the same events; on reads built with a duplication of every
    length 1..6 and no other change, the duplication events fit in the read, are 1..6 bases long, and every built length shows up."""
    D = 6
    text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, False, shape="down")
    logs, reads = [], []
    for i in range(16):
        log = []
        reads.append(random_read(4000 + i, text, max_len=30, noise=0., dups=D, dup_log=log))
        logs.append(log)
    got = []
    for opts in (None, "traceback=thread"):
        dec = da.ViterbiDecoder(m, dp, options=opts)
        dec.set_event_log(True)
        _check(dec, orc, reads, lattice=False, where=opts)
        got.append([dec.events(i) for i in range(len(reads))])
        dec.close()
    assert got[0] == got[1]
    lens = []
    for r, evs in zip(reads, got[0]):
        for ev in evs:
            mt = re.fullmatch(r"Duplication at (\d+): ([ACGT]+)", ev)
            if mt:
                p, k = int(mt.group(1)), len(mt.group(2))
                assert 1 <= k <= D and p + k <= len(r), (r, ev)
                lens.append(k)
    # (the decoder may explain an inserted copy otherwise -- a substitution, another walk -- so the count is held loosely, but every
    #  length 1..D the reads were built with must show up, 5 and 6 among them: past what a node record holds)
    built = [j for log in logs for _, j in log]
    assert set(lens) == set(built) == set(range(1, D + 1)), (sorted(lens), sorted(built))
    assert 2 * len(lens) >= len(built), (sorted(lens), sorted(built))


@pytest.mark.parametrize("D,tiers", [(0, "ABC"), (1, "ABC"), (3, "ABC"), (6, "ABC"), (8, "ABC"), (12, "B")])
def test_segments_at_other_widths(da, oracle_mod, tmp_path, D, tiers):
    """The bounded-memory decode keeps D + 1 history columns and needs segments of D + 2 or more: checkpoint=always with segments of
    D + 2 and D + 5 columns, every read through segments, strings, status and ll bits as the oracle's."""
    for global_ in (False, True):
        text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, global_, n_states=120)
        reads = _reads(text, D, 6, 5000 * D, max_len=40) + [""]
        for tier in tiers:
            for seg in (D + 2, D + 5):
                dec = da.ViterbiDecoder(m, dp, options=_options(tier, D) + ",checkpoint=always,segment=%d" % seg)
                _assert_tier(dec, tier, D)
                _check(dec, orc, reads, lattice=False, where=(D, tier, seg, global_))
                assert dec.stats()["checkpointed_reads"] == len(reads)
                dec.close()


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("edge", ["no_dup_no_del", "no_sub"])
def test_error_model_edges(da, oracle_mod, tmp_path, D, edge):
    """Zero probabilities give -inf scores: no duplications or deletions at all with a zero pLen entry besides, and no substitutions on
    a machine that never emits a T (reads with a T then have no path: empty string, NO_PATH, -inf as the oracle).  Every tier,
    every lattice cell, no NaN."""
    flags = dict(dup=0., del_open=0., del_ext=0.) if edge == "no_dup_no_del" else dict(sub=0., no_t=True)
    for global_ in (False, True):
        text, m, dp, orc = _model(da, oracle_mod, tmp_path, D, global_, n_states=100, shape="zero", **flags)
        reads = _reads(text, D, 6, 6000 * D)
        if edge == "no_sub":                 # ... and reads with a T in them
            reads += [r[:len(r) // 2] + "T" + r[len(r) // 2:] for r in reads[:3]]
        for tier in "ABC":
            dec = da.ViterbiDecoder(m, dp, options=_options(tier, D))
            _assert_tier(dec, tier, D)
            _, ll, st = _check(dec, orc, reads, where=(D, edge, tier, global_))
            dec.close()
        if edge == "no_sub":
            assert (st == NO_PATH).any() and np.isinf(ll[st == NO_PATH]).all()
