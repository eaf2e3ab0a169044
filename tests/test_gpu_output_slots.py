"""Where a traceback puts what it found: the caller's output slot and the library's event log (the closing lines of the two
kernels of csrc/viterbi_kernels.hip, and what the callers inside the library make of them).

1. The slot contract of include/dnastore_amd.h, through dnas_viterbi_batch_device.  A dozen reads whose decoded lengths n_i the
   oracle gives lie side by side in one device buffer of sentinel bytes, in slots of n_i, n_i - 1, 0, n_i + 1, 1 and n_i + 37
   symbols dealt so that every kind of slot has every other kind as a neighbour (KIND_WALK), between guard bytes, at an odd
   address.  Status, length, string, log-likelihood bits, the needed length an overflowed read leaves, the guards.  Routes: the
   wave-per-read traceback (the default) and the thread-per-read one (traceback=thread), both from the node records and through
   the CSR arrays (DNAS_NO_NODE_RECORDS=1); walks parked and resumed across lattice segments (checkpoint=always,segment=6);
   tier=B; tier=C,cluster=2; a both-strand call (dnas_viterbi_batch_strands_device, mode both); and a call with the event log on
   (which runs the tracebacks a second time when a log was too small).  Machines: l4c4.json, random_machine(3, 150), and a chain
   of 100 emitting edges, which decodes every read, the empty one too, to 100 symbols.
2. Strings longer than the 4 L + 64 symbols the library's own callers start from: decode, decode_packed, both strands,
   decode_fastseqs, decode_clusters (with and without consensus reads) and the command line's -V on the chain machine.
3. Event lists longer than the 3 L + 64 events the log starts from: on the chain machine without substitutions and
   duplications a read of L bases is 100 - L deletions and nothing else, whatever the code under test says; all routes that log.

The reference of every comparison is the C oracle (oracle/), bit for bit; the event counts follow from the model."""
import contextlib
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from random_machines import random_machine, random_read, shaped_machine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")
REF_DATA = os.path.join(ROOT, "tests", "golden", "ref_data")

SENTINEL = 0xA5
GUARD = 61                              # bytes in front of the first slot and behind the last: the slots start at an odd address
ROOMY = 37
KINDS = ("fit", "one short", "none", "one over", "one", "roomy")
# a walk over the six kinds of slot on which every two kinds are neighbours somewhere; a call deals a window of it over its reads
KIND_WALK = (0, 1, 2, 3, 4, 5, 0, 2, 4, 0, 3, 5, 1, 4, 2, 5, 3, 1)

CHAIN_LEN = 100
CHAIN_FLAGS = dict(global_=True, sub=.02, dup=.01, del_open=.02, del_ext=.5)
CHAIN_CLI = ["--error-global", "--error-sub-prob", ".02", "--error-dup-prob", ".01", "--error-del-open", ".02", "--error-del-ext", ".5"]
EXACT_FLAGS = dict(global_=True, sub=0., dup=0., del_open=.02, del_ext=.5)    # no substitutions, no duplications

ROUTES = {                              # name -> (model options, DNAS_NO_NODE_RECORDS, both strands, event log)
    "wave": (None, False, False, False),
    "thread": ("traceback=thread", False, False, False),
    "wave-csr": (None, True, False, False),
    "thread-csr": ("traceback=thread", True, False, False),
    "segments": ("checkpoint=always,segment=6", False, False, False),
    "tierB": ("tier=B", False, False, False),
    "tierC": ("tier=C,cluster=2", False, False, False),
    "both-strands": (None, False, True, False),
    "event-log": (None, False, False, True),
}


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def revcomp(s):
    return s.upper()[::-1].translate(str.maketrans("ACGT", "TGCA"))


def chain_text():
    return shaped_machine(1, [("E", 1, "01")], CHAIN_LEN)


def chain_bases():
    """The 100 bases the chain emits, in order: its only path."""
    return "".join(s["trans"][0]["out"] for s in json.loads(chain_text())["state"][:-1])


def _machine_case(da, name):
    """-> (machine text, error model flags, reads): an empty read, a read without a path where the parameters leave one, reads
    of different decoded lengths; at most 30 bases each."""
    if name == "l4c4":
        # no substitutions and no deletions: a read is a message as the machine writes it, with a duplication or two, or it has no
        # path (the empty read has none either)
        text = open(os.path.join(REF_DATA, "l4c4.json")).read()
        m = da.Machine.fromJSON(text)
        msgs = [m.encodeSymbols(b) for b in ("", "0", "10", "0110", "1011010", "110100101", "00101101110", "1110001011010")]
        dup = lambda r, at, k: r[:at] + r[at - k:at] + r[at:]
        reads = ["", "GGATCACAGTCT"] + msgs + [dup(msgs[3], 9, 2), dup(msgs[5], 14, 1), dup(dup(msgs[2], 6, 1), 11, 3)]
        return text, dict(global_=True, sub=0., dup=.01, del_open=0.), reads
    if name == "random3":
        # the noisy model of test_gpu_fuzz_machines.py.  Under it every base string has a path (deletions reach anything: none of
        # 900 random reads lacked one), so this machine's reads all decode; the slots of reads without a path are the other two's
        text = random_machine(3, 150)
        reads = ["", "A"] + [random_read(300 + k, text, max_len=30) for k in range(10)]
        return text, dict(global_=True, sub=.02, dup=.01, del_open=.02, del_ext=.1), reads
    # the chain: deletions only, so a read is a subsequence of the 100 bases or has no path, and every decode is 100 symbols
    c = chain_bases()
    reads = ["", "G" * 30, c[7], c[3:13], c[::4], c[:30], c[70:], c[1::9], "CCGGCCCCTGAGTCCGAGGAGAGGGTGCTT", c[40:46], c[5:95:3], c[-1]]
    return chain_text(), EXACT_FLAGS, reads


_cases = {}


def _case(da, O, name):
    """The machine's case with the oracle's answers, computed once: per read (string, loglike) forward, and for the both-strand
    route (string, loglike, strand) of the orientation with the strictly larger log-likelihood."""
    if name not in _cases:
        text, flags, reads = _machine_case(da, name)
        assert len(reads) >= 11 and max(len(r) for r in reads) <= 30 and "" in reads
        orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**flags))
        fwd = [orc.decode(r) for r in reads]
        both = []
        for r, f in zip(reads, fwd):
            b = orc.decode(revcomp(r))
            both.append((b + (1,)) if b[1] > f[1] else (f + (0,)))
        lengths = {len(s) for s, ll in fwd if not math.isinf(ll)}
        if name == "random3":
            assert not any(math.isinf(ll) for _, ll in fwd) and len(lengths) >= 5
        else:
            assert sum(math.isinf(ll) for _, ll in fwd) >= 2            # reads without a path
            assert lengths == {CHAIN_LEN} if name == "chain" else len(lengths) >= 5
        _cases[name] = (text, flags, reads, fwd, both)
    return _cases[name]


def _capacities(want, first):
    """One slot per read, its kind from KIND_WALK[first:]; -> (capacities, kind per read)."""
    caps, kinds = [], []
    for i, (s, ll) in enumerate(want):
        k = KIND_WALK[first + i]
        n = len(s)
        caps.append((n, max(n - 1, 0), 0, n + 1, 1, n + ROOMY)[k])
        kinds.append(k)
    return caps, kinds


def test_every_kind_of_slot_meets_every_other():
    """The two windows of KIND_WALK that the contract test deals over its 12 reads hold every pair of kinds as neighbours."""
    pairs = set()
    for first in (0, len(KIND_WALK) - 12):
        w = KIND_WALK[first:first + 12]
        pairs |= {frozenset(p) for p in zip(w, w[1:])}
    assert pairs == {frozenset((a, b)) for a in range(6) for b in range(a)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["l4c4", "random3", "chain"])
def test_slot_contract(da, oracle_mod, monkeypatch, name, route):
    """Every read of every layout: status 0 exactly where the slot holds the string, else 2 (1 without a path); out_len the
    string's length or 0; the string; the log-likelihood bits, overflowed or not; the length an overflowed read needs at the front
    of a slot of 8 bytes or more; not a byte changed outside the slots."""
    import torch
    options, csr, both, log = ROUTES[route]
    text, flags, reads, fwd, both_want = _case(da, oracle_mod, name)
    reads = reads[:12]
    want = (both_want if both else fwd)[:12]
    monkeypatch.delenv("DNAS_NO_NODE_RECORDS", raising=False)
    if csr:
        monkeypatch.setenv("DNAS_NO_NODE_RECORDS", "1")
    dev = torch.device("cuda", 0)
    off, bases = da.pack_reads(reads)
    k = len(reads)
    with contextlib.closing(da.ViterbiDecoder(da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**flags), options=options)) as dec:
        if options and options.startswith("tier="):
            assert dec.tier.startswith("tier " + options[5]), dec.tier
        dec.set_event_log(log)
        d_bases = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
        for first in (0, len(KIND_WALK) - 12):
            caps, kinds = _capacities([w[:2] for w in want], first)
            out_off = np.zeros(k + 1, dtype=np.uint64)
            out_off[0] = GUARD
            out_off[1:] = GUARD + np.cumsum(caps)
            total = int(out_off[-1]) + GUARD
            d_sym = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
            d_len = torch.full((k,), 77, dtype=torch.int32, device=dev)
            d_ll = torch.zeros(k, dtype=torch.float64, device=dev)
            d_st = torch.full((k,), 9, dtype=torch.uint8, device=dev)
            d_strand = torch.full((k,), 9, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            dec.decode_device(off, d_bases.data_ptr(), d_sym.data_ptr(), out_off, d_len.data_ptr(), d_ll.data_ptr(), d_st.data_ptr(),
                              strands="both" if both else "forward", d_strand_ptr=d_strand.data_ptr() if both else None)
            dec.sync()
            sym, olen, ll, st = d_sym.cpu().numpy(), d_len.cpu().numpy(), d_ll.cpu().numpy(), d_st.cpu().numpy()
            strand = d_strand.cpu().numpy()
            if route == "segments":
                assert dec.stats()["checkpointed_reads"] == k
            # not a byte outside the slots: the guards at both ends (the slots are contiguous between them)
            assert (sym[:GUARD] == SENTINEL).all() and (sym[int(out_off[-1]):] == SENTINEL).all(), (name, route, first)
            for i, w in enumerate(want):
                s, oll = w[:2]
                what = (name, route, first, i, reads[i], KINDS[kinds[i]], caps[i], len(s))
                no_path = math.isinf(oll)
                status = 1 if no_path else 0 if caps[i] >= len(s) else 2
                slot = sym[int(out_off[i]):int(out_off[i + 1])]
                print(what, "status", st[i], "len", olen[i], "ll", ll[i])
                assert st[i] == status, what
                assert olen[i] == (len(s) if status == 0 else 0), what
                assert bits(ll[i]) == bits(oll), what + (ll[i], oll)
                if status == 0:
                    assert slot[:len(s)].tobytes().decode() == s, what
                if status == 2 and caps[i] >= 8:
                    assert da.slot_needed(sym, out_off, i) == len(s), what
                if status == 1 or caps[i] == 0:
                    assert (slot == SENTINEL).all(), what                    # nothing to write, nothing written
                if both:
                    assert strand[i] == w[2], what


# ---------------------------------------------------------------------------------------------- strings longer than the guess
def _long_reads():
    c = chain_bases()
    return ["", "A", c[3:13], c[20:50]]


@pytest.fixture(scope="module")
def chain_long(da, oracle_mod):
    """The chain machine under the noisy global model: (library machine, params, reads, the oracle's (string, loglike) per read and
    per reverse complement)."""
    O = oracle_mod
    text = chain_text()
    orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**CHAIN_FLAGS))
    reads = _long_reads()
    fwd = [orc.decode(r) for r in reads]
    back = [orc.decode(revcomp(r)) for r in reads]
    for r, (s, ll) in zip(reads, fwd):
        assert len(s) == CHAIN_LEN and math.isfinite(ll)
    assert [4 * len(r) + 64 < CHAIN_LEN for r in reads] == [True, True, False, False]     # two beyond their slot, two inside
    return da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**CHAIN_FLAGS), reads, fwd, back


def _same(got_strings, got_ll, want, what):
    for i, (s, ll) in enumerate(want):
        print(what, i, len(got_strings[i]), got_ll[i], ll)
    for i, (s, ll) in enumerate(want):
        assert got_strings[i] == s and bits(got_ll[i]) == bits(ll), (what, i, got_strings[i], s, got_ll[i], ll)


def test_decode_delivers_strings_longer_than_its_slots(da, chain_long):
    """decode and decode_packed with the slots they size themselves, forward and both strands; out_cap=8 keeps its contract."""
    m, params, reads, fwd, back = chain_long
    with contextlib.closing(da.ViterbiDecoder(m, params)) as dec:
        out, ll, st = dec.decode(reads)
        assert list(st) == [0] * len(reads)
        _same(out, ll, fwd, "decode")
        off, bases = da.pack_reads(reads)
        sym, ooff, olen, ll, st = dec.decode_packed(off, bases)
        assert list(st) == [0] * len(reads) and (np.diff(ooff).astype(np.int64) >= olen).all()
        _same([sym[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes().decode() for i in range(len(reads))], ll, fwd, "decode_packed")
        out, ll, st, strand = dec.decode(reads, strands="both")
        want = [b if b[1] > f[1] else f for f, b in zip(fwd, back)]
        assert list(st) == [0] * len(reads) and list(strand) == [int(b[1] > f[1]) for f, b in zip(fwd, back)]
        _same(out, ll, want, "decode both")
        sym, ooff, olen, ll, st, strand = dec.decode_packed(off, bases, strands="both")
        _same([sym[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes().decode() for i in range(len(reads))], ll, want, "decode_packed both")
        out, ll, st = dec.decode(reads, out_cap=8)                   # the caller's own slots: the status, and no string
        assert list(st) == [2] * len(reads) and out == [""] * len(reads)
        assert np.array_equal(bits(ll), bits([w[1] for w in fwd]))


def _fasta(tmp_path, reads):
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    return str(fa)


def test_decode_fastseqs_and_cli_deliver_long_strings(da, chain_long, tmp_path):
    m, params, reads, fwd, back = chain_long
    fa = _fasta(tmp_path, reads)
    got = da.decode_fastseqs(fa, m, params)
    assert [g[0] for g in got] == ["r%d" % i for i in range(len(reads))]
    _same([g[1] for g in got], [g[2] for g in got], fwd, "decode_fastseqs")
    info = {}
    got = da.decode_fastseqs(fa, m, params, strands="both", info=info)
    want = [b if b[1] > f[1] else f for f, b in zip(fwd, back)]
    _same([g[1] for g in got], [g[2] for g in got], want, "decode_fastseqs both")
    assert info["strand"] == [int(b[1] > f[1]) for f, b in zip(fwd, back)]
    # the command line prints the strings (it has no output for the log-likelihood)
    mpath = tmp_path / "chain.json"
    mpath.write_text(chain_text())
    r = subprocess.run([BIN, "-v0", "-L", str(mpath), "-V", fa, "--raw"] + CHAIN_CLI, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().split("\n")[:-1] == [s for s, ll in fwd]


def test_decode_clusters_delivers_long_strings(da, oracle_mod, chain_long, tmp_path):
    """decode_clusters, every read a cluster of its own: the per-read decodes; with polish=1 also the decodes of the consensus
    reads, whose slots are a guess of the same kind.  And the command line's cluster decode, which prints messages only."""
    m, params, reads, fwd, back = chain_long
    labels = ["c%d" % i for i in range(len(reads))]
    orc = oracle_mod.ViterbiOracle(oracle_mod.Machine.from_json(chain_text()), oracle_mod.MutatorParams.from_cli(**CHAIN_FLAGS))
    with contextlib.closing(da.ViterbiDecoder(m, params)) as dec:
        out = dec.decode_clusters(reads, labels, strands="forward", band=-1)
        assert list(out.per_read[2]) == [0] * len(reads)
        _same(out.per_read[0], out.per_read[1], fwd, "decode_clusters")
        out = dec.decode_clusters(reads, labels, strands="forward", band=-1, polish=1)
        _same(out.per_read[0], out.per_read[1], fwd, "decode_clusters polish")
        ctext, cll, cst = out.consensus_decodes
        assert list(cst) == [0] * len(reads)
        _same(ctext, cll, [orc.decode(r) for r in out.consensus_reads], "consensus decodes")
        assert any(4 * len(r) + 64 < CHAIN_LEN for r in out.consensus_reads)
    fa = _fasta(tmp_path, reads)
    lab = tmp_path / "labels.txt"
    lab.write_text("".join(l + "\n" for l in labels))
    mpath = tmp_path / "chain.json"
    mpath.write_text(chain_text())
    r = subprocess.run([BIN, "-v0", "-L", str(mpath), "-V", fa, "--cluster-file", str(lab), "--align-band", "-1", "--raw"] + CHAIN_CLI,
                       capture_output=True, timeout=120)
    # (the chain's messages lack the end symbol the encoder wants, so no cluster has a candidate to print: the call decodes every
    # read, the two long ones a second time, and ends well)
    assert r.returncode == 0 and r.stdout == b"\n" * len(reads), (r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------- events beyond the log's guess
EVENT_ROUTES = (None, "traceback=thread", "checkpoint=always,segment=9")


def _event_reads():
    c = chain_bases()
    return ["", c[7], c[3:13], c[::4], c[60:90], c[98:]]


def _events(da, dec, reads, strands="forward"):
    """decode with the log on -> per read the event lines; dnas_model_read_events asked for the count first says what it then
    delivers."""
    L = da.lib.lib()
    got = dec.decode(reads, strands=strands)
    lists = []
    for i in range(len(reads)):
        n, n2 = ctypes.c_int64(-1), ctypes.c_int64(-1)
        da.lib.check(L.dnas_model_read_events(dec._h, i, None, 0, ctypes.addressof(n)))
        buf = np.full(n.value + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        da.lib.check(L.dnas_model_read_events(dec._h, i, buf.ctypes.data, len(buf), ctypes.addressof(n2)))
        assert n.value == n2.value and (buf[n.value:] == 0xFFFFFFFFFFFFFFFF).all() and (buf[:n.value] != 0xFFFFFFFFFFFFFFFF).all(), (i, n.value, n2.value)
        lists.append(dec.events(i))
        assert len(lists[-1]) == n.value
    return got, lists


def test_event_log_holds_every_deletion(da, oracle_mod, tmp_path):
    """No substitutions, no duplications, global: a path emits the chain's 100 bases and a read of L bases keeps L of them, so
    the walk logs exactly 100 - L deletions and nothing else -- 100, 99 and 90 of them in logs that start at 64, 67 and 94
    events.  The wave kernel, the thread kernel and parked walks give the same lists; decode_fastseqs hands out the same."""
    O = oracle_mod
    text = chain_text()
    reads = _event_reads()
    assert [3 * len(r) + 64 < CHAIN_LEN - len(r) for r in reads] == [True, True, False, False, False, True]
    orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**EXACT_FLAGS))
    want = [orc.decode(r) for r in reads]
    m, params = da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**EXACT_FLAGS)
    ref = None
    for options in EVENT_ROUTES:
        with contextlib.closing(da.ViterbiDecoder(m, params, options=options)) as dec:
            dec.set_event_log(True)
            (out, ll, st), lists = _events(da, dec, reads)
            _same(out, ll, want, ("events", options))
            for r, ev in zip(reads, lists):
                print(options, len(r), len(ev))
            for r, ev in zip(reads, lists):
                assert len(ev) == CHAIN_LEN - len(r) and all(e.startswith("Deletion between ") for e in ev), (options, r, len(ev))
            ref = ref or lists
            assert lists == ref, options
    got = da.decode_fastseqs(_fasta(tmp_path, reads), m, params, events=True)
    _same([g[1] for g in got], [g[2] for g in got], want, "decode_fastseqs events")
    assert [g[3] for g in got] == ref


def test_event_log_with_substitutions(da, oracle_mod):
    """sub = .02: still no duplications, so a path still emits 100 bases for L of the read -- at least 100 - L deletions, and a
    substitution wherever the walk says so.  The three routes agree; both strands log the winner's walk."""
    O = oracle_mod
    text = chain_text()
    flags = dict(EXACT_FLAGS, sub=.02)
    c = chain_bases()
    reads = _event_reads() + ["A", c[3:8] + "T" + c[9:13]]
    orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**flags))
    want = [orc.decode(r) for r in reads]
    m, params = da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**flags)
    ref = None
    for options in EVENT_ROUTES:
        with contextlib.closing(da.ViterbiDecoder(m, params, options=options)) as dec:
            dec.set_event_log(True)
            (out, ll, st), lists = _events(da, dec, reads)
            _same(out, ll, want, ("events sub", options))
            for r, ev in zip(reads, lists):
                n_del = sum(e.startswith("Deletion between ") for e in ev)
                print(options, len(r), len(ev), n_del)
                assert n_del == CHAIN_LEN - len(r) and len(ev) >= n_del, (options, r, len(ev), n_del)
                assert all(e.startswith(("Deletion between ", "Substitution at ")) for e in ev), (options, r)
            ref = ref or lists
            assert lists == ref, options
            if options != "traceback=thread":                     # both strands: the log of a read is the log of the winner's walk
                given = [revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
                flipped = [orc.decode(revcomp(r))[1] > orc.decode(r)[1] for r in given]
                got, lists_both = _events(da, dec, given, strands="both")
                assert list(got[3]) == [int(f) for f in flipped]
                for i, r in enumerate(given):
                    if (revcomp(r) if flipped[i] else r) == reads[i]:
                        assert lists_both[i] == ref[i], (options, i)
                assert sum((revcomp(r) if f else r) == w for r, f, w in zip(given, flipped, reads)) >= len(reads) - 2
