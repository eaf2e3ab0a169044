"""One ViterbiDecoder taken through a script of calls of different shapes, as bench.py, the CLI and ABI callers use it: a model
is made once and called again and again, and between calls it keeps state that only grows or is replaced on demand (the
lattice arena, the scheduling arrays, the host-entry I/O buffers, the timing events, the tier-C watchdog copies, probe word and
sync-word placement, the segment kernel, the event-log buffers).  Every step is held to the oracle and to a fresh model, bit
for bit, and asserts the path it was meant to take (launches, segmented reads, the tier-C probe, the occupancy note).

  S1  one short read R0 (the variant's reference fixture read): string, log-likelihood and the whole lattice are the oracle's
  S2  7 reads in 4 launches (an empty and a 1-base read among them): the scheduling, event, watchdog and I/O state grow
  S3  R0 alone again, one launch after the growth: identical to S1, lattice included
  S4  a ~500-nt read that does not fit half the arena beside two short ones: segments (the segment kernel's first use)
  S5  S2's reads through the device entry point
  S6  the event log on, then off again
  S7  a call with no reads: no stats, lattice or events of the call before survive it, on either entry point
  S8  R0 once more"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DUP_GC = "duplication of GC"
# id: machine, error-model flags, reference fixture read, options, environment, R0's events where the flags are those of
# test_gpu_decode_fastseqs.py::test_traceback_event_log
VARIANTS = {
    "tierA": ("s16h74l4c4.json", dict(global_=True), "hello.s16h74.del.fa", "max_slots=2", {}, None),
    "tierA-thread-traceback": ("s16h74l4c4.json", dict(), "hello.s16h74.del.fa", "max_slots=2,traceback=thread", {},
                               ["Deletion between 28 and 29: G"]),
    "tierA-two-per-cu": ("l4c4.json", dict(sub=0., del_open=0., global_=True), "hello.dup.fa", "max_slots=2,threads=1024",
                         {"DNAS_PLAN_OCCUPANCY": "2"}, DUP_GC),
    "tierB": ("h74l4c4.json", dict(), "hello.h74.sub.fa", "tier=B,max_slots=2", {}, ["Substitution at 25: A -> G"]),
    "tierC-compact": ("s16h74l4c4.json", dict(global_=True), "hello.s16h74.del.fa",
                      "tier=C,cluster=3,threads=512,cluster_spread=0,max_slots=2", {}, None),
    "tierC-single-read-shape": ("s16h74l4c4.json", dict(global_=True), "hello.s16h74.del.fa",
                                "tier=C,cluster=14,threads=1024,cluster_spread=0,max_slots=2", {}, None),
    "tierC-spread": ("s16h74l4c4.json", dict(), "hello.s16h74.del.fa", "tier=C,cluster=4,cluster_spread=1,max_slots=2", {},
                     ["Deletion between 28 and 29: G"]),
}


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def column_bytes(dec):
    """Arena bytes of one lattice column of this model (plan_call: 8 * storedLanes * Npad): tier B stores every lane of the
    states rounded up to 32, tiers A and C the S and D lanes of the plan's slots -- T x K per work-group, G work-groups per
    read on tier C -- as the tier note names them."""
    if dec.tier.startswith("tier B"):
        return 8 * (dec.max_dup_len + 2) * ((dec.n_states + 31) // 32 * 32)
    shape = re.search(r"T(\d+)K(\d+)", dec.tier)
    cluster = re.match(r"tier C: (\d+) work-groups per read", dec.tier)
    members = int(cluster.group(1)) if cluster else 1
    return 8 * 2 * members * int(shape.group(1)) * int(shape.group(2))


def lattice_bytes(col, read):
    return col * (len(read) + 1) + 64             # + the spare cell plan_call adds to every lattice


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    (oa, la, sa), (ob, lb, sb) = a, b
    assert list(oa) == list(ob)
    assert np.array_equal(_bits(la), _bits(lb))
    assert np.array_equal(np.asarray(sa), np.asarray(sb))


def _part(res, idx):
    return [res[0][i] for i in idx], np.asarray(res[1])[list(idx)], np.asarray(res[2])[list(idx)]


def _as_oracle_lattice(lat):
    return np.ascontiguousarray(lat.transpose(0, 2, 1)).view(np.uint64)      # [L+1][lanes][N] -> the oracle's [L+1][N][lanes]


def _decode_device(dec, torch, reads):
    from dnastore_amd import pack_reads
    off, bases = pack_reads(reads)
    k = len(reads)
    cap = int(np.diff(off).max()) * 4 + 64
    out_off = np.arange(k + 1, dtype=np.uint64) * np.uint64(cap)
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
    d_sym = torch.zeros(k * cap, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
    d_ll = torch.zeros(max(k, 1), dtype=torch.float64, device=dev)
    d_st = torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()    # torch's copies / fills are done before the library's own streams touch the buffers
    dec.decode_device(off, d_bases.data_ptr(), d_sym.data_ptr(), out_off, d_len.data_ptr(), d_ll.data_ptr(), d_st.data_ptr())
    dec.sync()
    sym, olen = d_sym.cpu().numpy(), d_len.cpu().numpy()
    return ([sym[i * cap:i * cap + int(olen[i])].tobytes().decode() for i in range(k)], d_ll.cpu().numpy()[:k],
            d_st.cpu().numpy()[:k])


def _script_reads(m, flags):
    """S2's 7 reads (encoded payloads of 1-5 bytes, a tandem duplication and -- where the model allows them -- a substitution and a
    deletion in some, an empty read and a 1-base read) and S4's ~500-nt read."""
    enc = [m.encodeBytes(bytes((37 * i + 11 * k) % 256 for k in range(n))) for i, n in enumerate((3, 1, 5, 2, 4))]
    enc[0] = enc[0][:12] + enc[0][9:12] + enc[0][12:]                    # a tandem duplication of 3 bases
    if flags.get("sub", 1.) > 0:
        c = enc[2][20]
        enc[2] = enc[2][:20] + {"A": "C", "C": "G", "G": "T", "T": "A"}[c] + enc[2][21:]
    if flags.get("del_open", 1.) > 0:
        enc[4] = enc[4][:15] + enc[4][16:]
    reads = [enc[0], enc[1], "", enc[2], "G", enc[3], enc[4]]
    payload = bytes(8)
    while len(m.encodeBytes(payload)) < 480:
        payload = bytes((7 * k + 3) % 256 for k in range(len(payload) + 1))
    return reads, m.encodeBytes(payload)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_model_through_calls_of_changing_shape(da, oracle_mod, ref_data, monkeypatch, capfd, variant):
    import torch
    mach, flags, fa, options, env, r0_events = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    compact_c = options.startswith("tier=C") and "cluster_spread=0" in options
    path = os.path.join(ref_data, mach)
    m = da.Machine.fromFile(path)
    params = da.MutatorParams.fromFlags(**flags)
    orc = oracle_mod.ViterbiOracle(oracle_mod.Machine.from_file(path), oracle_mod.MutatorParams.from_cli(**flags))
    r0 = da.read_fastseqs(os.path.join(ref_data, fa))[0][1]
    s2, long_read = _script_reads(m, flags)
    s4 = [s2[0], long_read, r0]

    # the model with a large arena sizes the others (and is S4's whole-lattice reference)
    big = da.ViterbiDecoder(m, params, options=options)
    col = column_bytes(big)
    pairs = sorted((lattice_bytes(col, r) for r in s2 + [r0]), reverse=True)
    half = max(pairs[0] + pairs[1], 160 * col)          # a batch of 2 of S1-S3 and S6 fits half the arena; S4's long read does not
    assert lattice_bytes(col, long_read) > half and 450 <= len(long_read) <= 700
    arena = 2 * half
    dec = da.ViterbiDecoder(m, params, arena_bytes=arena, options=options)
    fresh = da.ViterbiDecoder(m, params, arena_bytes=arena, options=options)
    try:
        tier = dec.tier
        assert column_bytes(dec) == col and column_bytes(fresh) == col, (tier, big.tier)
        if variant.startswith("tierA"):
            assert tier.startswith("tier A: T")
        if variant == "tierA-two-per-cu":
            assert "2 work-groups per CU" in tier and "T1024K" in tier, tier
        if variant == "tierB":
            assert tier.startswith("tier B"), tier
        if variant.startswith("tierC"):
            members = int(re.search(r"cluster=(\d+)", options).group(1))
            assert tier.startswith("tier C: %d work-groups per read" % members), tier
            assert ("dealt over the XCDs" in tier) == (not compact_c), tier
        if compact_c:
            assert "sync words at" in tier, tier          # placement was measured: small launches run the probe
        if variant.startswith("tierC"):
            monkeypatch.setenv("DNAS_SYNC_DEBUG", "1")    # the probe says where it ran on stderr

        # references: the oracle, and a fresh model with the same options and arena (event log on) for R0 + S2's reads
        o_r0, o_ll0, o_lat0 = orc.decode(r0, want_lattice=True)
        o_s2 = [orc.decode(r) for r in s2]
        fresh.set_event_log(True)
        ref = fresh.decode([r0] + s2)
        assert fresh.stats()["fill_launches"] == 4
        ref_events = [fresh.events(i) for i in range(1 + len(s2))]
        ref_s2 = _part(ref, range(1, 1 + len(s2)))
        assert ref[0][0] == o_r0 and _bits(ref[1][0]) == _bits(o_ll0)
        assert [s for s, _ in o_s2] == ref_s2[0] and np.array_equal(_bits([ll for _, ll in o_s2]), _bits(ref_s2[1]))
        assert list(ref_s2[2]) == [1 if np.isneginf(ll) else 0 for _, ll in o_s2]    # DNAS_READ_NO_PATH exactly where the oracle has none
        if r0_events == DUP_GC:
            assert len(ref_events[0]) == 1 and re.fullmatch(r"Duplication at \d+: GC", ref_events[0][0]), ref_events[0]
        elif r0_events is not None:
            assert ref_events[0] == r0_events
        ref_s4 = big.decode(s4)
        assert big.stats()["checkpointed_reads"] == 0

        def check_r0(step):
            got = dec.decode([r0])
            st = dec.stats()
            assert st["fill_launches"] == 1 and st["checkpointed_reads"] == 0, (step, st)
            _same(got, _part(ref, [0]))
            assert np.array_equal(_as_oracle_lattice(dec.lattice(0, len(r0))), o_lat0.view(np.uint64)), step
            return got

        def probed(launches):
            # DNAS_SYNC_DEBUG=1: a line per probe.  The compact tier-C plans probe before every launch of at most 8 clusters;
            # nothing else probes (clusters dealt over the XCDs have no "next XCD" to ask for)
            n = capfd.readouterr().err.count("probe on XCC")
            assert n >= launches if compact_c else n == 0, (launches, n)

        # S1
        capfd.readouterr()
        s1 = check_r0("S1")
        assert s1[2][0] == 0
        probed(1)
        # S2: 4 launches of at most 2 reads (2 clusters on tier C): every watchdog, event, scheduling and I/O buffer grows
        capfd.readouterr()
        got2 = dec.decode(s2)
        assert dec.stats()["fill_launches"] == 4 and dec.stats()["checkpointed_reads"] == 0
        probed(4)
        _same(got2, ref_s2)
        # S3: one launch after the growth (on the compact tier-C plans: the probe word S1 allocated)
        check_r0("S3")
        probed(1)
        # S4: the long read through segments (the segment kernel is compiled here), the short ones whole
        got4 = dec.decode(s4)
        st4 = dec.stats()
        assert st4["checkpointed_reads"] == 1 and st4["fill_launches"] >= 3, st4
        _same(got4, ref_s4)
        with pytest.raises(da.DnasError):
            dec.lattice(1, len(long_read))
        assert np.array_equal(_as_oracle_lattice(dec.lattice(2, len(r0))), o_lat0.view(np.uint64))
        # S5: the device entry point, S2's reads
        got5 = _decode_device(dec, torch, s2)
        assert dec.stats()["fill_launches"] == 4
        _same(got5, ref_s2)
        # S6: the event log on -- every read's events are the fresh model's -- and off again
        dec.set_event_log(True)
        got6 = dec.decode([r0] + s2)
        assert dec.stats()["fill_launches"] == 4
        _same(got6, ref)
        assert [dec.events(i) for i in range(1 + len(s2))] == ref_events
        dec.set_event_log(False)
        _same(dec.decode([r0] + s2), ref)
        with pytest.raises(da.DnasError):
            dec.events(0)
        # S7: a call with no reads is the last call: its stats are zero, and no lattice or event of the call before stays readable
        dec.set_event_log(True)
        for entry in ("host", "device"):
            check_r0("S7 " + entry)
            assert dec.events(0) == ref_events[0]
            if entry == "host":
                out, ll, st = dec.decode([])
                assert out == [] and len(ll) == 0 and len(st) == 0
            else:
                dec.decode_device(np.zeros(1, np.uint64), 0, 0, np.zeros(1, np.uint64), 0, 0, 0)
                dec.sync()
            assert all(v == 0 for v in dec.stats().values()), dec.stats()
            with pytest.raises(da.DnasError):
                dec.lattice(0, len(r0))
            with pytest.raises(da.DnasError):
                dec.events(0)
        dec.set_event_log(False)
        # S8
        capfd.readouterr()
        check_r0("S8")
        probed(1)
    finally:
        dec.close()
        fresh.close()
        big.close()
