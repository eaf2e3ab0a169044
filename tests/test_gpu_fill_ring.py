"""Tier A, calls of three or more fill launches: the launches go down two streams into a ring of three arena slices (DESIGN.md
3.6; option fill_overlap), so that two fills are in flight while a third batch is traced back.  Which slice a batch fills, which
traceback it waits for and which stream it runs on change nothing about the answers: every call here is held to the CPU oracle
and to the same call with fill_overlap=0 (two arena halves, one fill stream), bit for bit.

Shapes: max_slots=2 and 2 .. 13 reads of 40-120 nt of unequal lengths, so that the slices hold lattices of different sizes and
the last batch is partial -- batch 3 is the first to reuse a slice, batch 6 opens the second lap.  Machines: s16h74l4c4 (one
work-group per CU) and l4c4 at 1024 threads (two per CU)."""
import math
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

# id: machine, error-model flags, options beside max_slots, payload bytes of the pool's reads (-> 40-120 nt)
MACHINES = {
    "one-per-cu": ("s16h74l4c4.json", dict(), "", (2, 5, 3, 6, 4)),
    "two-per-cu": ("l4c4.json", dict(global_=True), ",threads=1024", (5, 12, 8, 14, 6, 10)),
}
POOL = 13
BATCHES_OF = {2: 1, 3: 2, 5: 3, 7: 4, 13: 7}        # reads -> fill launches under max_slots=2


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq.upper()))


def same(a, b):
    assert list(a[0]) == list(b[0])
    for x, y in zip(a[1:], b[1:]):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def column_bytes(dec):
    """Arena bytes of one lattice column of a tier-A model (plan_call: the S and D lanes of the plan's T x K slots)."""
    shape = re.search(r"T(\d+)K(\d+)", dec.tier)
    return 8 * 2 * int(shape.group(1)) * int(shape.group(2))


def lattice_bytes(col, read):
    return col * (len(read) + 1) + 64             # + the spare cell plan_call adds to every lattice


class Case:
    """One machine: its pool of reads, the oracle's answers (computed once, shared by the tests) and the models made so far."""

    def __init__(self, da, O, ref_data, key):
        mach, flags, extra, nbytes = MACHINES[key]
        path = os.path.join(ref_data, mach)
        self.da, self.machine, self.params = da, da.Machine.fromFile(path), da.MutatorParams.fromFlags(**flags)
        self.extra = extra
        self.oracle = O.ViterbiOracle(O.Machine.from_file(path), O.MutatorParams.from_cli(**flags))
        om = O.Machine.from_file(path)
        self.reads = [synth.synthetic_reads(om, 1, nbytes[i % len(nbytes)], 4100 + i, sub=.02, dele=.01, dup=.01)[0] for i in range(POOL)]
        lens = [len(r) for r in self.reads]
        assert min(lens) >= 40 and max(lens) <= 120 and len(set(lens)) >= 5, lens
        self._want, self._want_rc, self._models = {}, {}, {}

    def want(self, reads, cache=None, flip=False):
        """(strings, log-likelihoods, status) as the oracle has them."""
        cache = self._want if cache is None else cache
        for r in reads:
            if r not in cache:
                cache[r] = self.oracle.decode(revcomp(r) if flip else r)
        return ([cache[r][0] for r in reads], np.array([cache[r][1] for r in reads], dtype=np.float64),
                np.array([1 if cache[r][0] == "" and math.isinf(cache[r][1]) else 0 for r in reads], dtype=np.uint8))

    def want_both(self, reads):
        f, r = self.want(reads), self.want(reads, self._want_rc, flip=True)
        rev = [bool(r[1][i] > f[1][i]) for i in range(len(reads))]
        pick = lambda k: [(r if rev[i] else f)[k][i] for i in range(len(reads))]
        return pick(0), np.array(pick(1), dtype=np.float64), np.array(pick(2), dtype=np.uint8), np.array(rev, dtype=np.uint8)

    def model(self, options="", arena_bytes=0):
        key = (options, arena_bytes)
        if key not in self._models:
            self._models[key] = self.da.ViterbiDecoder(self.machine, self.params, arena_bytes=arena_bytes,
                                                       options="max_slots=2" + self.extra + options)
            tier = self._models[key].tier
            assert tier.startswith("tier A: T"), tier
            assert ("2 work-groups per CU" in tier) == (self.extra != ""), tier
        return self._models[key]

    def close(self):
        for dec in self._models.values():
            dec.close()


@pytest.fixture(scope="module", params=list(MACHINES))
def case(request, da, oracle_mod, ref_data):
    c = Case(da, oracle_mod, ref_data, request.param)
    yield c
    c.close()


def sorted_order(reads):
    """The order plan_call decodes in: longest first, ties in the caller's order."""
    return sorted(range(len(reads)), key=lambda i: -len(reads[i]))


# ---- 1. ring boundaries -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(BATCHES_OF))
def test_ring_boundaries(case, n):
    reads = case.reads[:n]
    ring, plain = case.model(), case.model(",fill_overlap=0")
    got = ring.decode(reads)
    st = ring.stats()
    ref = plain.decode(reads)
    st0 = plain.stats()
    same(got, case.want(reads))
    same(got, ref)
    assert st0["fill_launches"] == BATCHES_OF[n] and st["fill_launches"] == st0["fill_launches"]
    assert st0["arena_slices"] == min(2, BATCHES_OF[n])
    assert st["arena_slices"] == (3 if BATCHES_OF[n] >= 3 else st0["arena_slices"])
    assert st["columns"] == st0["columns"] and st["lattice_bytes"] == st0["lattice_bytes"]


# ---- 2. an arena of the caller's ---------------------------------------------------------------------------------------------

def test_explicit_arena_falls_back_or_is_cut_again(case):
    reads = case.reads[:7]
    want = case.want(reads)
    col = column_bytes(case.model())
    sizes = sorted((lattice_bytes(col, r) for r in reads), reverse=True)
    half = sizes[0] + sizes[1]                       # any batch of two fits half the arena; three of the largest batch do not fit it
    assert 3 * sizes[0] <= 2 * half                  # (a third of it still holds the longest read)
    dec = case.model(arena_bytes=2 * half)
    same(dec.decode(reads), want)
    assert dec.stats()["arena_slices"] == 2 and dec.stats()["fill_launches"] == 4
    cut = case.model(",fill_overlap=2", arena_bytes=2 * half)
    same(cut.decode(reads), want)
    assert cut.stats()["arena_slices"] == 3 and cut.stats()["fill_launches"] > 4      # the two longest reads no longer share a slice
    # an arena whose third does not hold the longest read: two halves as ever, whatever the option says
    small = 2 * sizes[0] + sizes[0] // 2
    assert small // 3 < sizes[0] <= small // 2
    for options in ("", ",fill_overlap=2"):
        dec = case.model(options, arena_bytes=small)
        same(dec.decode(reads), want)
        st = dec.stats()
        assert st["arena_slices"] == 2 and st["checkpointed_reads"] == 0 and st["fill_launches"] >= 4, st


# ---- 3. both strands ---------------------------------------------------------------------------------------------------------

def test_both_strands_over_the_ring(case):
    reads = [revcomp(r) if i % 3 == 1 else r for i, r in enumerate(case.reads[:7])]      # a pair per launch: 7 launches
    want = case.want_both(reads)
    assert want[3].any() and not want[3].all()
    ring, plain = case.model(), case.model(",fill_overlap=0")
    got = ring.decode(reads, strands="both")
    st, ss = ring.stats(), ring.strand_stats()
    ref = plain.decode(reads, strands="both")
    same(got, want)
    same(got, ref)
    assert st["fill_launches"] == 7 == plain.stats()["fill_launches"]
    assert st["arena_slices"] == 3 and plain.stats()["arena_slices"] == 2
    assert ss == plain.strand_stats() and ss["reads"] == 7 and ss["reverse_won"] == int(want[3].sum())


# ---- 4. segments, then the ring ------------------------------------------------------------------------------------------------

def test_segments_in_front_of_the_ring(case):
    shorts = sorted(case.reads, key=len)[:6]
    payload = bytes(8)
    while len(case.machine.encodeBytes(payload)) < 300:
        payload = bytes((7 * k + 3) % 256 for k in range(len(payload) + 1))
    long_read = case.machine.encodeBytes(payload)
    reads = shorts[:2] + [long_read] + shorts[2:]
    col = column_bytes(case.model())
    sizes = sorted((lattice_bytes(col, r) for r in shorts), reverse=True)
    arena = 3 * (sizes[0] + sizes[1])                # three of the largest batch side by side ...
    assert lattice_bytes(col, long_read) > arena // 2    # ... and the long read does not fit half of it: segments
    # segments of 64 columns: five of them, filled twice but for the last
    ring, plain = case.model(",segment=64", arena_bytes=arena), case.model(",segment=64,fill_overlap=0", arena_bytes=arena)
    got, st = ring.decode(reads), ring.stats()
    ref, st0 = plain.decode(reads), plain.stats()
    same(got, ref)
    same((got[0][:2] + got[0][3:], np.delete(got[1], 2), np.delete(got[2], 2)), case.want(shorts))
    assert got[0][2] != "" and got[2][2] == 0
    assert st["checkpointed_reads"] == 1 == st0["checkpointed_reads"]
    assert st["fill_launches"] == st0["fill_launches"] == 3 + 2 * ((len(long_read) + 1 + 63) // 64) - 1
    assert st["arena_slices"] == 3 and st0["arena_slices"] == 2


# ---- 5. one model, changing calls ------------------------------------------------------------------------------------------------

def test_one_model_through_ring_calls_of_changing_shape(case):
    dec = case.da.ViterbiDecoder(case.machine, case.params, options="max_slots=2" + case.extra)
    fresh = case.da.ViterbiDecoder(case.machine, case.params, options="max_slots=2" + case.extra)
    try:
        for n, slices in ((7, 3), (1, 1), (13, 3), (5, 3)):        # the timing and sync events grow, and are trimmed
            reads = case.reads[:n]
            same(dec.decode(reads), case.want(reads))
            assert dec.stats()["arena_slices"] == slices and dec.stats()["fill_launches"] == (n + 1) // 2
        reads = case.reads[3:12]
        dec.set_event_log(True)
        fresh.set_event_log(True)
        got, ref = dec.decode(reads), fresh.decode(reads)
        same(got, case.want(reads))
        same(got, ref)
        assert dec.stats()["arena_slices"] == 3 and dec.stats()["fill_launches"] == 5
        events = [dec.events(i) for i in range(len(reads))]
        assert events == [fresh.events(i) for i in range(len(reads))] and any(events)
        dec.set_event_log(False)
        same(dec.decode(case.reads[:7]), case.want(case.reads[:7]))
    finally:
        dec.close()
        fresh.close()


# ---- 6. lattices after a ring call -------------------------------------------------------------------------------------------------

def test_lattices_after_a_ring_call(case):
    """dnas_model_read_lattice after a 4-batch ring call: the lattices of the last two batches, each in its own slice, are the
    oracle's; the batches before them are refused.  (The ring still holds the lattices of a third batch, but
    test_gpu_viterbi.py::test_device_entry_point_rejects_bad_bases_and_stale_lattices pins "the last two batches" for a default
    model of exactly this shape, so the rule stays what it was.)"""
    reads = case.reads[:7]
    dec = case.model()
    same(dec.decode(reads), case.want(reads))
    assert dec.stats()["arena_slices"] == 3 and dec.stats()["fill_launches"] == 4
    order = sorted_order(reads)                      # batches: order[0:2], [2:4], [4:6], [6:7] in slices 0, 1, 2, 0
    for at in (4, 5, 6):
        i = order[at]
        _, _, lat = case.oracle.decode(reads[i], want_lattice=True)
        got = np.ascontiguousarray(dec.lattice(i, len(reads[i])).transpose(0, 2, 1))      # [L+1][lanes][N] -> the oracle's [L+1][N][lanes]
        assert np.array_equal(got.view(np.uint64), lat.view(np.uint64)), at
    for at in (0, 1, 2, 3):
        with pytest.raises(case.da.DnasError) as e:
            dec.lattice(order[at], len(reads[order[at]]))
        assert "overwritten" in str(e.value)


# ---- 7. fill_ms --------------------------------------------------------------------------------------------------------------------

def test_fill_ms_is_the_union_of_the_launches(case):
    reads = case.reads[:13]
    figures = {}
    for options in (",fill_overlap=0", ""):
        dec = case.model(options)
        dec.decode(reads)                            # (warm: the arena and the buffers are there)
        t0 = time.perf_counter()
        dec.decode(reads)                            # decode + sync + copies
        wall_ms = (time.perf_counter() - t0) * 1e3
        st = dec.stats()
        print("fill_overlap%s: fill_ms %.3f traceback_ms %.3f launches %d wall %.3f ms" %
              (options[-2:] if options else "=1", st["fill_ms"], st["traceback_ms"], st["fill_launches"], wall_ms))
        assert 0 < st["fill_ms"] <= wall_ms, (options, st, wall_ms)
        assert 0 < st["traceback_ms"]
        figures[options] = st
    serial, ring = figures[",fill_overlap=0"], figures[""]
    assert ring["arena_slices"] == 3 and serial["arena_slices"] == 2 and ring["fill_launches"] == serial["fill_launches"] == 7
    # loosely: the union is at least its longest launch, the sum at most seven of them (a factor of four for the noise of two runs)
    per_launch = serial["fill_ms"] / serial["fill_launches"]
    assert per_launch / 4 <= ring["fill_ms"] <= 4 * serial["fill_ms"], (ring, serial)
