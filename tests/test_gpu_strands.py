"""Reads of unknown orientation: strand modes forward / reverse / both of dnas_viterbi_batch_strands,
dnas_decode_fastseqs_strands and the Python layer above them.

The contract: per read, F = the decode of the read and R = the decode of its reverse complement; mode "both" returns R
with strand 1 iff R's log-likelihood is strictly larger (fp64), else F with strand 0.  Expected values come from the CPU
oracle applied to the read and to its reverse complement, which is computed here in plain Python -- never from the entry
points under test.  Two exceptions: the oracle has no event log and no bounded-memory path, so there the yardstick is the
library's forward entry point (itself pinned to the oracle by the rest of the suite).  Symbols, status and strand are
compared for equality, log-likelihoods as uint64 bit patterns.

stats() of a "both" call counts orientations: `columns` is 2 * sum(L + 1) and `checkpointed_reads` 2 per read that went
through segments; strand_stats() counts the caller's reads."""
import ctypes
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402
from viterbi_cases import NOERRS, VITERBI_GOLDENS  # noqa: E402

pytestmark = pytest.mark.gpu

# SURVEY.md Appendix B (as tests/test_gpu_tier_c.py builds its machines)
DROPDOT = ('{"state":[{"n":0,"id":"S","trans":[{"in":"^","out":"^","to":1}]},{"n":1,"id":"T","trans":[{"in":"0","out":"0","to":1},'
           '{"in":"1","out":"1","to":1},{"in":".","to":1},{"in":"$","out":"$","to":2}]},{"n":2,"id":"U","trans":[]}]}')
FIXED = ["", "A", "AT", "ACGT", "AATT"]


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq.upper()))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def expected(orc, read):
    """The rule, from two oracle decodes: (symbols, loglike, status, strand, loglike forward, loglike reverse)."""
    f, r = orc.decode(read), orc.decode(revcomp(read))
    rev = r[1] > f[1]
    s, ll = r if rev else f
    return s, ll, (1 if s == "" and math.isinf(ll) else 0), int(rev), f[1], r[1]


def check_against(got, want):
    out, ll, st, strand = got
    assert list(out) == [w[0] for w in want]
    assert np.array_equal(bits(ll), bits([w[1] for w in want]))
    assert list(st) == [w[2] for w in want]
    assert list(strand) == [w[3] for w in want]


def counts(want):
    """reverse_won, ties, both_no_path as strand_stats defines them."""
    return (sum(w[3] for w in want), sum(1 for w in want if w[4] == w[5]),
            sum(1 for w in want if math.isinf(w[4]) and math.isinf(w[5]) and w[4] < 0 and w[5] < 0))


def check_stats(dec, reads, want, segmented=False):
    cols = sum(len(r) + 1 for r in reads)
    s = dec.strand_stats()
    rev, ties, none = counts(want)
    assert s["reads"] == len(reads) and s["tracebacks"] == len(reads) and s["fill_columns"] == 2 * cols
    assert s["reverse_won"] + s["ties"] <= len(reads)
    assert (s["reverse_won"], s["ties"], s["both_no_path"]) == (rev, ties, none)
    assert s["pass2_columns"] == (cols if segmented else 0)


def mixed_reads(O, mach_path, seed, n=24, max_bytes=12, max_len=None, errors=True):
    """n synthetic reads of ragged lengths, each flipped by a seeded coin (-> reads, flipped flags), then the fixed reads and
    one 40-nt uniformly random read."""
    om = O.Machine.from_file(mach_path)
    rng = random.Random(seed)
    reads, flipped = [], []
    for i in range(n):
        nbytes = 1 + i % max_bytes
        kw = dict(sub=.02, dele=.01, dup=.01) if errors else dict(sub=0.)
        r = synth.synthetic_reads(om, 1, nbytes, seed * 1000 + i, **kw)[0]
        if max_len is not None and len(r) > max_len:
            r = synth.synthetic_reads(om, 1, 1 + i % 3, seed * 1000 + i, **kw)[0]
        flip = rng.random() < 0.5
        reads.append(revcomp(r) if flip else r)
        flipped.append(flip)
    reads += FIXED + ["".join(rng.choice("ACGT") for _ in range(40))]
    return reads, flipped


_CACHE = {}


def mixed_case(O, ref_data, mach, flags_key, flags, errors=True):
    """(reads, expected) of a machine and error model, the oracle run once per session."""
    key = (mach, flags_key, errors)
    if key not in _CACHE:
        path = os.path.join(ref_data, mach)
        reads, _ = mixed_reads(O, path, 7 + len(mach), max_len=130 if mach.startswith("s16") else None, errors=errors)
        orc = O.ViterbiOracle(O.Machine.from_file(path), O.MutatorParams.from_cli(**flags))
        _CACHE[key] = (reads, [expected(orc, r) for r in reads])
    return _CACHE[key]


# ---- 1. the reference's goldens, flipped ----------------------------------------------------------------------------------

def _strands_forward(da, fa, m, params):
    """dnas_decode_fastseqs_strands(..., DNAS_STRAND_FORWARD) -> [(name, symbols, loglike)], strands."""
    L = da.lib.lib()
    h = ctypes.c_void_p()
    da.lib.check(L.dnas_decode_fastseqs_strands(str(fa).encode(), m._h, ctypes.byref(params.c), 0, 0, da.lib.STRAND_FORWARD, ctypes.byref(h)))
    n = L.dnas_decoded_count(h)
    recs = [(L.dnas_decoded_name(h, i).decode(), L.dnas_decoded_seq(h, i).decode(), L.dnas_decoded_loglike(h, i)) for i in range(n)]
    strands = [L.dnas_decoded_strand(h, i) for i in range(n)]
    L.dnas_decoded_free(h)
    return recs, strands


@pytest.mark.parametrize("mach,fa,flags,golden,loglike", VITERBI_GOLDENS)
def test_reference_goldens_flipped(da, ref_data, tmp_path, mach, fa, flags, golden, loglike):
    m = da.Machine.fromFile(os.path.join(ref_data, mach))
    params = da.MutatorParams.fromFlags(**flags)
    src = os.path.join(ref_data, fa)
    recs = da.read_fastseqs(src)
    assert len(recs) == 1
    flipped = tmp_path / "flipped.fa"
    flipped.write_text("".join(">%s\n%s\n" % (n, revcomp(s)) for n, s in recs))
    want = open(os.path.join(ref_data, golden)).read().strip()
    for path, mode, strand in ((flipped, "both", 1), (src, "both", 0), (flipped, "reverse", 1)):
        info = {}
        got = da.decode_fastseqs(path, m, params, strands=mode, info=info)
        assert [(n, s) for n, s, _ in got] == [(recs[0][0], want)], (mode, strand)
        assert bits([got[0][2]])[0] == bits([loglike])[0]
        assert info["strand"] == [strand]
    fwd, strands = _strands_forward(da, src, m, params)
    assert fwd == da.decode_fastseqs(src, m, params) and strands == [0]


# ---- 2. a mixed batch against the oracle, all tiers -----------------------------------------------------------------------

@pytest.mark.parametrize("options", [None, "tier=A", "tier=B"])
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("mach", ["l4c4.json", "mr2l4c4.json", "h74l4c4.json", "s16mr2l4c4.json", "s16h74l4c4.json"])
def test_mixed_batch_matches_oracle(da, oracle_mod, ref_data, mach, local, options):
    flags = dict(global_=not local)
    reads, want = mixed_case(oracle_mod, ref_data, mach, "local" if local else "global", flags)
    assert len(reads) >= 24 + 6
    # the input covers the cases: reverse won, forward won strictly, an exact tie
    assert any(w[3] == 1 for w in want) and any(w[3] == 0 and w[4] > w[5] for w in want) and any(w[4] == w[5] for w in want)
    dec = da.ViterbiDecoder(da.Machine.fromFile(os.path.join(ref_data, mach)), da.MutatorParams.fromFlags(**flags), options=options)
    if options:
        assert dec.tier.startswith("tier " + options[-1])
    check_against(dec.decode(reads, strands="both"), want)
    check_stats(dec, reads, want)
    st = dec.stats()
    assert st["columns"] == 2 * sum(len(r) + 1 for r in reads) and st["checkpointed_reads"] == 0
    with pytest.raises(da.DnasError) as e:
        dec.lattice(0, len(reads[0]))
    assert "DNAS_E_UNSUPPORTED" in str(e.value)
    dec.close()


@pytest.mark.parametrize("options", [None, "tier=B"])
@pytest.mark.parametrize("mach", ["l4c4.json", "h74l4c4.json"])
def test_no_errors_model_losers_without_a_path(da, oracle_mod, ref_data, mach, options):
    """NOERRS, global: an error-free read has a path as written and none reversed; the empty read and a random read have none
    either way (DNAS_READ_NO_PATH, strand 0, empty string)."""
    reads, want = mixed_case(oracle_mod, ref_data, mach, "noerrs", NOERRS, errors=False)
    assert any(math.isinf(w[4]) != math.isinf(w[5]) and math.isfinite(w[1]) for w in want)          # loser -inf, winner finite
    assert any(w[3] == 1 and math.isinf(w[4]) for w in want) and any(w[3] == 0 and math.isinf(w[5]) and math.isfinite(w[4]) for w in want)
    assert any(math.isinf(w[4]) and math.isinf(w[5]) and w[2] == 1 and w[3] == 0 and w[0] == "" for w in want)   # both -inf
    dec = da.ViterbiDecoder(da.Machine.fromFile(os.path.join(ref_data, mach)), da.MutatorParams.fromFlags(**NOERRS), options=options)
    check_against(dec.decode(reads, strands="both"), want)
    check_stats(dec, reads, want)
    dec.close()


# ---- 3. more than one batch, odd counts ------------------------------------------------------------------------------------

def test_pairs_stay_together_across_batches(da, oracle_mod, ref_data):
    flags = dict(global_=True)
    reads, want = mixed_case(oracle_mod, ref_data, "h74l4c4.json", "global", flags)
    reads, want = reads[:25], want[:25]
    m = da.Machine.fromFile(os.path.join(ref_data, "h74l4c4.json"))
    whole = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(**flags))
    ref = whole.decode(reads, strands="both")
    whole.close()
    check_against(ref, want)
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(**flags), options="max_slots=6")
    got = dec.decode(reads, strands="both")
    assert dec.stats()["fill_launches"] > 1
    check_against(got, want)
    assert got[0] == ref[0] and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[1:], ref[1:]))
    check_stats(dec, reads, want)
    dec.close()


def test_pairs_stay_together_when_the_arena_cuts(da, oracle_mod, ref_data):
    """An arena whose half holds 400 lattice columns: the batches of a "both" call are cut by the arena, in front of a pair only;
    with checkpoint=always the bounded-memory groups are halved until they fit, in whole pairs; an arena too small for the
    segments of one pair is an error that says what the pair would take."""
    import re
    flags = dict(global_=True)
    reads, want = mixed_case(oracle_mod, ref_data, "h74l4c4.json", "global", flags)
    m = da.Machine.fromFile(os.path.join(ref_data, "h74l4c4.json"))
    params = da.MutatorParams.fromFlags(**flags)
    whole = da.ViterbiDecoder(m, params)
    shape = re.search(r"T(\d+)K(\d+)", whole.tier)                 # tier A: K rows x T threads of lattice slots, S and D lanes
    col = 2 * int(shape.group(1)) * int(shape.group(2)) * 8
    whole.close()
    cols = sum(len(r) + 1 for r in reads)
    assert 2 * (max(len(r) for r in reads) + 1) < 400 < cols
    dec = da.ViterbiDecoder(m, params, arena_bytes=2 * 400 * col)
    check_against(dec.decode(reads, strands="both"), want)
    st = dec.stats()
    assert st["checkpointed_reads"] == 0 and st["fill_launches"] >= 2 * cols // 400 > 2
    check_stats(dec, reads, want)
    dec.close()
    dec = da.ViterbiDecoder(m, params, arena_bytes=2 * 400 * col, options="checkpoint=always,segment=16")
    check_against(dec.decode(reads, strands="both"), want)
    check_stats(dec, reads, want, segmented=True)
    assert dec.stats()["checkpointed_reads"] == 2 * len(reads)
    dec.close()
    tiny = da.ViterbiDecoder(m, params, arena_bytes=8 * col)
    with pytest.raises(da.DnasError) as e:
        tiny.decode(reads[:1], strands="both")
    assert "DNAS_E_NOMEM" in str(e.value) and "checkpoints" in str(e.value)
    tiny.close()


# ---- 4. tier C -------------------------------------------------------------------------------------------------------------

def _compose(da, ref_data, *parts):
    ms = [p if isinstance(p, da.Machine) else da.Machine.fromFile(os.path.join(ref_data, p)) for p in parts]
    m = ms[-1]
    for a in reversed(ms[:-1]):
        m = da.Machine.compose(a, m)
    return m


def _substitute(rng, dna, rate):
    out = list(dna)
    for i, c in enumerate(out):
        if rng.random() < rate:
            out[i] = rng.choice([b for b in "ACGT" if b != c])
    return "".join(out)


@pytest.mark.parametrize("options", ["tier=C,cluster=2,max_clusters=5", "tier=C,cluster=2,max_clusters=1", "tier=C,cluster=2"])
def test_tier_c_fixture_machine(da, oracle_mod, ref_data, options):
    """The 12 361-state fixture forced onto clusters of two work-groups; an odd number of clusters and a single one (a pair then
    shares it)."""
    flags = dict(global_=True)
    reads, want = mixed_case(oracle_mod, ref_data, "s16h74l4c4.json", "global", flags)
    dec = da.ViterbiDecoder(da.Machine.fromFile(os.path.join(ref_data, "s16h74l4c4.json")), da.MutatorParams.fromFlags(**flags), options=options)
    assert dec.tier.startswith("tier C: 2 work-groups")
    check_against(dec.decode(reads, strands="both"), want)
    check_stats(dec, reads, want)
    dec.close()


@pytest.mark.parametrize("options", [None, "max_clusters=3"])
def test_tier_c_cluster_machine(da, oracle_mod, ref_data, options):
    """BASELINE configs[1], flusher * mixradar6 * l4c4 (46 670 states: does not fit one CU), three ~100-nt reads, one flipped."""
    O = oracle_mod
    m = _compose(da, ref_data, "flusher.json", "mixradar6.json", "l4c4.json")
    assert m.nStates() == 46670
    rng = random.Random(7)
    reads = [_substitute(rng, m.encodeBytes(bytes(rng.randrange(256) for _ in range(12))), 0.01) for _ in range(3)]
    reads[1] = revcomp(reads[1])
    key = "composite"
    if key not in _CACHE:
        orc = O.ViterbiOracle(O.Machine.from_json(m.toJSON()), O.MutatorParams.from_cli(global_=True))
        _CACHE[key] = [expected(orc, r) for r in reads]
    want = _CACHE[key]
    assert [w[3] for w in want] == [0, 1, 0]
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(global_=True), options=options)
    assert dec.tier.startswith("tier C")
    check_against(dec.decode(reads, strands="both"), want)
    check_stats(dec, reads, want)
    dec.close()


# ---- 5. the bounded-memory path --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("mach,options", [("s16h74l4c4.json", ""), ("h74l4c4.json", "tier=B"), ("s16h74l4c4.json", "tier=C,cluster=2,max_clusters=3")])
def test_segments_match_whole_lattice(da, oracle_mod, ref_data, mach, options, local):
    """checkpoint=always: equal to the whole-lattice "both" result bit for bit; the second pass fills and traces back the
    winners only (pass2_columns = sum(L + 1) over the caller's reads, fill_columns twice that), and stats().checkpointed_reads
    counts orientations."""
    flags = dict(global_=not local)
    reads, want = mixed_case(oracle_mod, ref_data, mach, "local" if local else "global", flags)
    m = da.Machine.fromFile(os.path.join(ref_data, mach))
    params = da.MutatorParams.fromFlags(**flags)
    whole = da.ViterbiDecoder(m, params, options=options or None)
    assert whole.tier.startswith("tier " + (options[5] if options else "A"))
    ref = whole.decode(reads, strands="both")
    assert whole.stats()["checkpointed_reads"] == 0
    min_seg = whole.max_dup_len + 2
    whole.close()
    check_against(ref, want)
    for seg in (min_seg, 16, 64):
        dec = da.ViterbiDecoder(m, params, options=",".join(x for x in (options, "checkpoint=always,segment=%d" % seg) if x))
        got = dec.decode(reads, strands="both")
        assert got[0] == ref[0] and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[1:], ref[1:])), seg
        check_stats(dec, reads, want, segmented=True)
        assert dec.stats()["checkpointed_reads"] == 2 * len(reads)
        # a forward call over the same handle afterwards is today's call
        fwd = dec.decode(reads[:7])
        assert dec.strand_stats() == dict.fromkeys(dec.strand_stats(), 0) and dec.stats()["checkpointed_reads"] == 7
        assert len(fwd) == 3
        dec.close()


# ---- 6. the event log ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [None, "checkpoint=always,segment=9"])
def test_event_log_of_a_flipped_read(da, oracle_mod, ref_data, options):
    flags = dict(global_=True)
    reads, want = mixed_case(oracle_mod, ref_data, "s16h74l4c4.json", "global", flags)
    m = da.Machine.fromFile(os.path.join(ref_data, "s16h74l4c4.json"))
    dec = da.ViterbiDecoder(m, da.MutatorParams.fromFlags(**flags), options=options)
    dec.set_event_log(True)
    oriented = [revcomp(r) if w[3] else r for r, w in zip(reads, want)]      # every read as the winner was decoded
    dec.decode(oriented)
    ref = [dec.events(i) for i in range(len(reads))]
    got = dec.decode(reads, strands="both")
    check_against(got, want)
    assert [dec.events(i) for i in range(len(reads))] == ref
    assert any(ref[i] for i, w in enumerate(want) if w[3] == 1)              # flipped reads with events are among them
    dec.close()


# ---- 7. the device entry point, and a model reused across modes -----------------------------------------------------------

def test_device_entry_point_and_model_reuse(da, oracle_mod, ref_data):
    import torch
    flags = dict(global_=True)
    reads, want = mixed_case(oracle_mod, ref_data, "h74l4c4.json", "global", flags)
    m = da.Machine.fromFile(os.path.join(ref_data, "h74l4c4.json"))
    params = da.MutatorParams.fromFlags(**flags)
    dec = da.ViterbiDecoder(m, params)
    dev = torch.device("cuda", 0)

    def on_device(rs, mode):
        off, bases = da.pack_reads(rs)
        k = len(rs)
        cap = int(np.diff(off).max()) + 64
        out_off = np.arange(k + 1, dtype=np.uint64) * np.uint64(cap)
        d_bases = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
        d_sym = torch.zeros(k * cap, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(k, dtype=torch.int32, device=dev)
        d_ll = torch.zeros(k, dtype=torch.float64, device=dev)
        d_st = torch.full((k,), 9, dtype=torch.uint8, device=dev)
        d_strand = torch.full((k,), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        dec.decode_device(off, d_bases.data_ptr(), d_sym.data_ptr(), out_off, d_len.data_ptr(), d_ll.data_ptr(), d_st.data_ptr(),
                          strands=mode, d_strand_ptr=d_strand.data_ptr())
        dec.sync()
        sym, olen = d_sym.cpu().numpy(), d_len.cpu().numpy()
        return ([sym[i * cap:i * cap + int(olen[i])].tobytes().decode() for i in range(k)], d_ll.cpu().numpy(), d_st.cpu().numpy(),
                d_strand.cpu().numpy())

    fresh = da.ViterbiDecoder(m, params)
    for rs, ws, mode in ((reads[:9], want[:9], "forward"), (reads, want, "both"), (reads[3:20], want[3:20], "forward"), (reads[5:16], want[5:16], "both"),
                         (reads[:4], want[:4], "reverse")):
        got = on_device(rs, mode)
        if mode == "both":
            check_against(got, ws)
            check_stats(dec, rs, ws)
        else:
            ref = fresh.decode([revcomp(r) for r in rs] if mode == "reverse" else rs)
            assert got[0] == ref[0] and np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(got[2], ref[2])
            assert list(got[3]) == [1 if mode == "reverse" else 0] * len(rs)
            assert dec.strand_stats()["reverse_won"] == 0
    fresh.close()
    dec.close()


def test_one_model_through_strand_calls_of_changing_shape(da, oracle_mod, ref_data):
    """One decoder, host entry point, an arena whose half holds 400 lattice columns: the buffers per virtual read and the
    both-strand bases grow (steps 1-2), the winners' per-segment tables come into use and grow (3-4: a ~500-nt and a ~600-nt read
    go through segments, pair by pair), then a reverse, a forward and an empty call, and the first call again.  Every step equals
    a fresh decoder given that call alone bit for bit, and the rule worked out from the oracle."""
    import re
    from test_gpu_model_reuse import _script_reads
    flags = dict(global_=True)
    short, want_short = mixed_case(oracle_mod, ref_data, "h74l4c4.json", "global", flags)
    path = os.path.join(ref_data, "h74l4c4.json")
    m = da.Machine.fromFile(path)
    params = da.MutatorParams.fromFlags(**flags)
    orc = oracle_mod.ViterbiOracle(oracle_mod.Machine.from_file(path), oracle_mod.MutatorParams.from_cli(**flags))
    r500 = _script_reads(m, flags)[1]
    payload = bytes(8)
    while len(m.encodeBytes(payload)) < 580:
        payload = bytes((5 * k + 1) % 256 for k in range(len(payload) + 1))
    r600 = revcomp(m.encodeBytes(payload))                      # (this one arrives flipped)
    assert 450 <= len(r500) <= 560 < len(r600) <= 650
    want_long = {r: expected(orc, r) for r in (r500, r600)}
    assert want_long[r500][3] == 0 and want_long[r600][3] == 1
    whole = da.ViterbiDecoder(m, params)
    shape = re.search(r"T(\d+)K(\d+)", whole.tier)              # as test_pairs_stay_together_when_the_arena_cuts
    col = 2 * int(shape.group(1)) * int(shape.group(2)) * 8
    whole.close()
    arena = 2 * 400 * col
    assert 2 * (max(len(r) for r in short) + 1) < 400 < 2 * (len(r500) + 1)

    def pick(ids, *long):
        return [short[i] for i in ids] + list(long), [want_short[i] for i in ids] + [want_long[r] for r in long]

    script = [("both",) + pick(range(3)), ("both",) + pick(range(3, 15)), ("both",) + pick((20, 7), r500),
              ("both",) + pick((9, 24), r500, r600), ("reverse",) + pick(range(11, 15)), ("forward",) + pick(range(15, 19)),
              ("both", [], []), ("both",) + pick(range(3))]
    dec = da.ViterbiDecoder(m, params, arena_bytes=arena)
    for step, (mode, reads, want) in enumerate(script, 1):
        got = dec.decode(reads, strands=mode)
        fresh = da.ViterbiDecoder(m, params, arena_bytes=arena)
        ref = fresh.decode(reads, strands=mode)
        fresh.close()
        assert len(got) == len(ref) == (3 if mode == "forward" else 4), step
        assert got[0] == ref[0] and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[1:], ref[1:])), step
        if mode == "both":
            check_against(got, want)
            if step in (3, 4):                                  # the winners of the long reads, and only they, walk a second pass
                assert dec.strand_stats()["pass2_columns"] == sum(len(r) + 1 for r in reads if len(r) > 400), step
            elif reads:
                check_stats(dec, reads, want)
        else:                                                   # one orientation: its log-likelihood as the oracle gave it
            assert np.array_equal(bits(got[1]), bits([w[5 if mode == "reverse" else 4] for w in want])), step
            assert mode == "forward" or list(got[3]) == [1] * len(reads)
        assert (dec.stats()["checkpointed_reads"] > 0) == (step in (3, 4)), step
    dec.close()


# ---- 8. every GPU of a node ------------------------------------------------------------------------------------------------

def test_all_devices_both_strands(da, ref_data, tmp_path, monkeypatch):
    m = da.Machine.fromFile(os.path.join(ref_data, "h74l4c4.json"))
    params = da.MutatorParams.fromFlags(global_=True)
    rng = random.Random(3)
    fa = tmp_path / "reads.fa"
    flipped = []
    with open(fa, "w") as f:
        for i in range(44):
            dna = m.encodeBytes(bytes(rng.randrange(256) for _ in range(1 + i % 7)))
            flipped.append(rng.random() < 0.5)
            f.write(">read%d some comment\n%s\n" % (i, revcomp(dna) if flipped[-1] else dna))
        f.write(">empty\n\n")
    one_info, all_info = {}, {}
    one = da.decode_fastseqs(fa, m, params, device=0, info=one_info, strands="both", events=True)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")               # three host threads / models share the GPUs there are
    everywhere = da.decode_fastseqs(fa, m, params, device=-1, info=all_info, strands="both", events=True)
    assert everywhere == one and len(one) == 45
    assert one_info["devices"] == 1 and all_info["devices"] == 3
    assert all_info["strand"] == one_info["strand"] and set(one_info["strand"]) == {0, 1} and one_info["strand"][-1] == 0
    assert one[0][0] == "read0" and flipped.count(True) > 0
