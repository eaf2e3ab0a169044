"""Every route of the library on poisoned device memory with guarded allocations (DNAS_DEBUG_ALLOC, csrc/device_buffer.hpp).

The other GPU tests hold a kernel's answer to the host statement or the oracle; that catches wrong arithmetic.  It cannot catch
a kernel that reads device memory nobody wrote -- what hipMalloc hands back is often zeros, and a zero count, flag or score looks
initialised -- nor one that stores a little past the end of its buffer.  Here every device and pinned allocation of a route is
filled with a byte and followed by a guard band of 256 bytes of it:

    0xFF    NaN as fp64, -1 as int32, 255 as a byte: the general case
    0x55    0x5555555555555555 ~ 1.19e103 as fp64, finite and positive: a max-plus kernel hides NaN (fmax(NaN, x) = x), so a
            poisoned score has to WIN a maximum to be seen

Each case sets the variable, creates every handle inside it, runs the smallest shape that reaches the route, holds the answer
to the reference that does not depend on device memory (host=True where a host statement exists, the oracle for the Viterbi and
forward-backward kernels; bit for bit, an equality wherever the existing test of the route is one), closes the handles, and
asserts from debugAllocStats() that guarded allocations were made (the seam was live), that every one of them was checked at
its free, and that no guard band had changed.  "unset" runs the route with the variable unset; the poisoned answer must also be
the unpoisoned one, bit for bit.

Cases and helpers are those of the existing case modules.  LDS cannot be poisoned from the host, and a DevBuf that is reused
without growing is not refilled (tests/test_gpu_model_reuse.py is the guard for stale contents)."""
import gc
import os
import random
import struct
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

pytestmark = pytest.mark.gpu

BYTES = (None, "0xFF", "0x55")
# the testing aids a route may set: none of them leaks from one route (or from the caller's environment) into another
AIDS = ("DNAS_TIER", "DNAS_THREADS", "DNAS_PLAN_PICK", "DNAS_PLAN_ORDER", "DNAS_PLAN_SLACK", "DNAS_PLAN_REMOTE_ROWS", "DNAS_FB_STREAMING",
        "DNAS_FB_NO_NARROW", "DNAS_ALIGN_BLOCKS", "DNAS_COUNTS_CHUNK", "DNAS_FORWARD_CHUNK", "DNAS_ASSIGN_CHUNK", "DNAS_CONSENSUS_CHUNK",
        "DNAS_POLISH_LDS_POSITIONS", "DNAS_CLUSTER_GATE_WORDS", "DNAS_CLUSTER_CHUNK", "DNAS_CLUSTERER_SEGMENTS", "DNAS_TRIM_PAIR_CHUNK",
        "DNAS_SIMULATE_THREAD_PER_READ", "DNAS_SIMULATE_BLOCKS", "DNAS_FAKE_DEVICES", "DNAS_CHECKPOINT", "DNAS_SEGMENT")
ROUTES = {}
_references = {}     # computed once (host statements, oracle decodes, pools) and left unchanged
_unpoisoned = {}     # route -> (frozen answer, allocation stats) of its run with the variable unset


def route(fn):
    ROUTES[fn.__name__] = fn
    return fn


def once(key, make):
    if key not in _references:
        _references[key] = make()
    return _references[key]


def frozen(x):
    """An answer as nested tuples of bytes: two answers are the same bit for bit iff their frozen forms are equal."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (float, np.floating)):
        return struct.pack("<d", float(x))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    if x is None or isinstance(x, (bool, int, str, bytes, np.integer)):
        return x
    raise TypeError("cannot freeze %r" % type(x))


class Context:
    def __init__(self, da, O, ref_data, env):
        self.da, self.O, self.ref_data, self.env = da, O, ref_data, env


def run(name, byte, O, ref_data):
    """-> (the route's frozen answer, debugAllocStats of the run)."""
    import dnastore_amd as da
    with pytest.MonkeyPatch.context() as env:
        for aid in AIDS:
            env.delenv(aid, raising=False)
        if byte is None:
            env.delenv("DNAS_DEBUG_ALLOC", raising=False)
        else:
            env.setenv("DNAS_DEBUG_ALLOC", byte)
        gc.collect()                                       # (a handle an earlier test dropped is freed before the count starts)
        da.debugAllocStats(reset=True)
        answer = ROUTES[name](Context(da, O, ref_data, env))
        gc.collect()
        stats = da.debugAllocStats(reset=True)
    return frozen(answer), stats


def unpoisoned(name, O, ref_data):
    if name not in _unpoisoned:
        _unpoisoned[name] = run(name, None, O, ref_data)
    return _unpoisoned[name]


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def noisy(da):
    from test_assign_cpu import NOISY
    return da.MutatorParams.fromFlags(**NOISY)


# ------------------------------------------------------------------------------------------------ Viterbi fill and traceback
@route
def viterbi_tier_a(c):
    """l4c4.json on hello.fa and hello.dup.fa: the goldens' strings and log-likelihoods."""
    from viterbi_cases import VITERBI_GOLDENS
    out = []
    for mach, fa, flags, golden, loglike in VITERBI_GOLDENS[:2]:
        assert mach == "l4c4.json" and fa in ("hello.fa", "hello.dup.fa")
        dec = c.da.ViterbiDecoder(c.da.Machine.fromFile(os.path.join(c.ref_data, mach)), c.da.MutatorParams.fromFlags(**flags))
        assert dec.tier.startswith("tier A"), dec.tier
        sym, ll, st = dec.decode([s for _, s in c.da.read_fastseqs(os.path.join(c.ref_data, fa))])
        dec.close()
        assert sym == [open(os.path.join(c.ref_data, golden)).read().strip()] and st[0] == 0 and ll[0] == loglike, (fa, sym, ll)
        out.append((sym, ll, st))
    return out


@route
def viterbi_tier_c(c):
    """A shaped machine cut over two work-groups: strings, log-likelihoods, status and every lattice cell are the oracle's."""
    import test_gpu_row_shapes as RS
    case = RS.CASES["chain-c2"]
    assert case.members > 1
    dec, orc, reads = RS._setup(c.env, c.O, case, False)
    sym, ll, st = dec.decode(reads, out_cap=RS.OUT_CAP)
    lattices = []
    for i, r in enumerate(reads):
        s, oll, olat = once(("tier C", i), lambda: orc.decode(r, want_lattice=True))
        assert sym[i] == s and bits(ll[i]) == bits(oll) and st[i] == (RS.NO_PATH if oll == -np.inf else 0), (i, sym[i], s, ll[i], oll)
        lat = np.ascontiguousarray(dec.lattice(i, len(r)).transpose(0, 2, 1))
        assert lat.shape == olat.shape and np.array_equal(lat.view(np.uint64), olat.view(np.uint64)), i
        lattices.append(lat)
    dec.close()
    return sym, ll, st, lattices


@route
def viterbi_tier_b(c):
    """The general kernel, as test_gpu_tier_b.py reaches it, with its whole lattice."""
    flags = dict(sub=0., del_open=0., global_=True)
    c.env.setenv("DNAS_TIER", "B")
    path = os.path.join(c.ref_data, "l4c4.json")
    dec = c.da.ViterbiDecoder(c.da.Machine.fromFile(path), c.da.MutatorParams.fromFlags(**flags))
    assert dec.tier.startswith("tier B"), dec.tier
    read = c.da.read_fastseqs(os.path.join(c.ref_data, "hello.dup.fa"))[0][1]
    sym, ll, st = dec.decode([read])
    s, oll, olat = once("tier B", lambda: c.O.ViterbiOracle(c.O.Machine.from_file(path), c.O.MutatorParams.from_cli(**flags))
                        .decode(read, want_lattice=True))
    lat = np.ascontiguousarray(dec.lattice(0, len(read)).transpose(0, 2, 1))
    dec.close()
    assert sym[0] == s and ll[0] == oll and st[0] == 0
    assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64))
    return sym, ll, st, lat


@route
def viterbi_segments(c):
    """The bounded-memory decode at the shortest segment (D + 2 columns) on the smallest reads test_gpu_checkpoint.py segments:
    the empty read, one base, D + 1 .. D + 3 bases and a one-byte payload."""
    flags = dict(sub=0., del_open=0., global_=True)
    path = os.path.join(c.ref_data, "l4c4.json")
    machine = c.da.Machine.fromFile(path)
    reads = ["", "A", "ACGTA", "ACGTAC", "ACGTACG", machine.encodeBytes(b"\x5a")]
    dec = c.da.ViterbiDecoder(machine, c.da.MutatorParams.fromFlags(**flags), options="checkpoint=always,segment=6")
    assert dec.max_dup_len == 4
    sym, ll, st = dec.decode(reads)
    assert dec.stats()["checkpointed_reads"] == len(reads)
    dec.close()
    orc = once("segments oracle", lambda: c.O.ViterbiOracle(c.O.Machine.from_file(path), c.O.MutatorParams.from_cli(**flags)))
    for i, r in enumerate(reads):
        s, oll = once(("segments", i), lambda: orc.decode(r))
        assert sym[i] == s and bits(ll[i]) == bits(oll) and st[i] == (1 if s == "" and oll == -np.inf else 0), (i, sym[i], s, ll[i], oll)
    assert st[-1] == 0 and sym[-1] != ""
    return sym, ll, st


def ring_case(c):
    import test_gpu_fill_ring as FR
    case = once("ring case", lambda: FR.Case(c.da, c.O, c.ref_data, "two-per-cu"))
    case._models = {}
    return FR, case


@route
def viterbi_ring(c):
    """Five reads under max_slots=2: three fill launches into the ring of three arena slices."""
    FR, case = ring_case(c)
    reads = case.reads[:5]
    assert FR.BATCHES_OF[5] == 3
    try:
        dec = case.model()
        got = dec.decode(reads)
        st = dec.stats()
    finally:
        case.close()
    assert st["arena_slices"] == 3 and st["fill_launches"] == 3, st
    FR.same(got, case.want(reads))
    return got


@route
def viterbi_both_strands(c):
    FR, case = ring_case(c)
    reads = [FR.revcomp(r) if i % 3 == 1 else r for i, r in enumerate(case.reads[:4])]
    want = case.want_both(reads)
    assert want[3].any() and not want[3].all()
    dec = c.da.ViterbiDecoder(case.machine, case.params)
    got = dec.decode(reads, strands="both")
    ss = dec.strand_stats()
    dec.close()
    FR.same(got, want)
    assert ss["reads"] == 4 and ss["reverse_won"] == int(want[3].sum())
    return got


@route
def decode_clusters_polished_with_support(c):
    """Six clusters of three reads, polish=1, support=True: the definition restated over the oracle's decodes, and the support
    the host statement of pairProfiles gives."""
    import pair_counts_cases as K
    import pair_profile_cases as R
    from test_gpu_consensus import BAND, MACHINE, PLANTED, oracle_decodes, planted_pool
    from test_gpu_pair_profiles import TOL
    from test_gpu_polish import check_polished, expected_polished
    da = c.da
    machine = da.Machine.fromFile(os.path.join(c.ref_data, MACHINE))
    flags = dict(global_=True, **PLANTED)
    params = da.MutatorParams.fromFlags(**flags)

    def reference():
        messages, reads, labels = planted_pool(da, machine, n_clusters=6)
        orc = c.O.ViterbiOracle(c.O.Machine.from_file(os.path.join(c.ref_data, MACHINE)), c.O.MutatorParams.from_cli(**flags))
        decodes = oracle_decodes(c.O, c.ref_data, reads, flags)
        return reads, labels, decodes, expected_polished(da, orc, machine, params, reads, labels, decodes, BAND, 1)

    reads, labels, decodes, (rows, cons, cons_dec, refused, _, cands) = once("decode_clusters", reference)
    dec = da.ViterbiDecoder(machine, params, device=0)
    got = dec.decode_clusters(reads, labels, strands="both", band=BAND, polish=1, support=True)
    dec.close()
    check_polished(got, rows, cons, cons_dec)
    sym, ll, st, strand = got.per_read
    assert list(sym) == [d[0] for d in decodes] and np.array_equal(bits(ll), bits([d[1] for d in decodes]))
    assert [int(x) for x in st] == [d[2] for d in decodes] and [int(x) for x in strand] == [d[3] for d in decodes]
    assert got.stats["encode_failures"] == refused and got.stats["candidates"] == sum(len(x) for x in cands)
    assert len(got.support) == 6 and got.support_reads.shape == (6,)
    for k, lab in enumerate(got.labels):
        if got.read[k] < 0 and not got.source[k]:
            assert got.support[k].shape == (0,) and got.support_reads[k] == 0
            continue
        mine = [i for i, x in enumerate(labels) if x == lab]
        s = da.tokenize(machine.encodeSymbols(got.symbols[k]))
        host = once(("support", k), lambda: da.pairProfiles(params, [s] * len(mine), [reads[i] for i in mine], band=BAND, host=True,
                                                            read_strand=[decodes[i][3] for i in mine]))
        ok = [j for j in range(len(mine)) if host.status[j] == K.COUNTS_OK]
        assert got.support_reads[k] == len(ok) and got.support[k].shape == (len(s),)
        np.testing.assert_allclose(got.support[k], sum(host.pair_profiles[j][R.MATCH + s, np.arange(len(s))] for j in ok) / len(ok), **TOL)
    return (got.labels, got.symbols, got.read, got.total, got.second, got.votes, got.n_candidates, got.status, got.source,
            got.consensus_reads, list(got.consensus_decodes), list(got.per_read), got.support, got.support_reads)


# ------------------------------------------------------------------------------------------------ forward-backward E-step
def fb_pair(c, kind, mode=None):
    """One pair of an on-chip kind through the E-step: the oracle's numbers, the routing the census predicts."""
    import fb_census as C
    import fb_edge_pairs as E
    from test_gpu_fwdback_edges import _against_oracle, _triple
    P = E.KIND_P
    pairs = once(("fb pairs", kind), lambda: E.short_kind_pairs("poisoned", kind, 1, P))
    assert C.route(pairs[0], P)[:2] == (kind, True)
    want = once(("fb", kind), lambda: c.O.expected_counts(c.O.MutatorParams.from_cli(length=2 * P), pairs))
    if mode:
        c.env.setenv(mode, "1")
    params = c.da.MutatorParams.fromFlags(length=2 * P)
    fb = c.da.ForwardBackward(c.O.pack_pairs(pairs), device=0)
    got = fb.expectedCounts(params)
    st = fb.stats()
    fb.close()
    assert _triple(st) == C.predict(pairs, P, no_narrow=mode == "DNAS_FB_NO_NARROW", streaming=mode == "DNAS_FB_STREAMING"), st
    _against_oracle(got, want, (kind, mode))
    return list(got)


@route
def fwdback_onchip_kind0(c):
    return fb_pair(c, 0)


@route
def fwdback_onchip_kind1(c):
    return fb_pair(c, 1)


@route
def fwdback_onchip_kind2(c):
    return fb_pair(c, 2)


@route
def fwdback_onchip_kind3(c):
    return fb_pair(c, 3)


@route
def fwdback_streaming(c):
    return fb_pair(c, 1, "DNAS_FB_STREAMING")


@route
def fwdback_no_narrow(c):
    return fb_pair(c, 0, "DNAS_FB_NO_NARROW")


# ------------------------------------------------------------------------------------------------ pair HMM
def align_pool(c):
    from test_gpu_pair_align import _shape_list
    return once("align pool", lambda: _shape_list("poisoned/pair-align"))


def aligned(c, ins, outs, band, key, **gpu):
    from test_gpu_pair_align import _same
    params = noisy(c.da)
    got = c.da.alignPairs(params, ins, outs, band=band, **gpu)
    _same(got, once(("align", key, band), lambda: c.da.alignPairs(params, ins, outs, band=band, host=True)))
    assert got.stats["pairs_too_large"] == 0 and got.stats["cells"] > 0
    return got.score, got.status, got.ops, got.stats["batches"]


@route
def align_pairs_band8(c):
    return aligned(c, *align_pool(c), 8, "pool")


@route
def align_pairs_full(c):
    return aligned(c, *align_pool(c), c.da.lib.ALIGN_FULL, "pool")


@route
def align_pairs_boundary_row_in_hbm(c):
    """The pairs of test_gpu_pair_align.py::test_boundary_row_beyond_lds: a read of more than 1015 bases."""
    from test_gpu_pair_align import _rand, _related

    def pairs():
        rng = random.Random("gpu-pair-align/long")
        a = _rand(rng, 1100)
        return [a, _rand(rng, 130), a[:200]], [_related(rng, a, 1104), _rand(rng, 1100), _related(rng, a[:200], 198)]

    ins, outs = once("align long", pairs)
    assert max(map(len, outs)) > 1015
    return aligned(c, ins, outs, 8, "long")


@route
def align_pairs_two_blocks(c):
    """Eight waves over 35 pairs: a wave's scratch is reused across items."""
    c.env.setenv("DNAS_ALIGN_BLOCKS", "2")
    return aligned(c, *align_pool(c), 8, "pool")


@route
def pair_likelihoods(c):
    from test_gpu_pair_forward import same_bits, shape_list
    ins, outs, strand = once("forward pool", lambda: shape_list("poisoned/pair-forward"))
    params = noisy(c.da)
    got = c.da.pairLikelihoods(params, ins, outs, band=32, read_strand=strand)
    same_bits(got, once("forward host", lambda: c.da.pairLikelihoods(params, ins, outs, band=32, read_strand=strand, host=True)))
    assert not np.isnan(got).any() and np.isfinite(got).any()
    return got


@route
def pair_counts_in_chunks(c):
    """DNAS_COUNTS_CHUNK=1, its smallest multi-chunk value: a launch per pair."""
    from test_gpu_pair_counts import same_as_host
    from test_gpu_pair_forward import shape_list
    ins, outs, strand = once("counts pool", lambda: shape_list("poisoned/pair-counts"))
    params = noisy(c.da)
    c.env.setenv("DNAS_COUNTS_CHUNK", "1")
    got = c.da.pairCounts(params, ins, outs, band=32, read_strand=strand)
    same_as_host(got, once("counts host", lambda: c.da.pairCounts(params, ins, outs, band=32, read_strand=strand, host=True)))
    assert got.stats["chunks"] == len(ins) > 1 and got.stats["pairs_too_large"] == 0
    return got.counts, got.ll, got.pair_counts, got.pair_ll, got.pair_ll_backward, got.status


@route
def pair_profiles(c):
    import pair_profile_cases as R
    from test_gpu_pair_profiles import same_as_host
    ins, outs, strand = once("profile pool", lambda: R.stripe_pairs("poisoned/pair-profiles", longer=True))
    params = noisy(c.da)
    got = c.da.pairProfiles(params, ins, outs, band=8, read_strand=strand)
    same_as_host(got, once("profile host", lambda: c.da.pairProfiles(params, ins, outs, band=8, read_strand=strand, host=True)))
    assert got.stats["pairs_too_large"] == 0
    return got.profile, got.coverage, got.pair_profiles, got.pair_ll, got.status


@route
def baum_welch_pairs_one_iteration(c):
    """The fit follows the host's EM (to the tolerance of test_gpu_pair_counts.py::test_fit_follows_the_host_em)."""
    import pair_counts_cases as K
    ins, outs = once("em pairs", K.em_pairs)
    start = K.em_start(c.da)
    fitted, iters, trace = c.da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, max_iterations=1)
    host, host_iters, host_trace = once("em host", lambda: c.da.baumWelchPairs(start, ins, outs, band=K.EM_BAND, max_iterations=1, host=True))
    assert iters == host_iters == 1 and len(trace) == len(host_trace) == 1
    assert K.params_dict(trace[0][0]) == K.params_dict(start) and trace[0][1] == pytest.approx(host_trace[0][1], rel=1e-9)
    assert K.params_dict(fitted) == pytest.approx(K.params_dict(host), rel=1e-9)
    return sorted(K.params_dict(fitted).items()), trace[0][1]


# ------------------------------------------------------------------------------------------------ assignment
def assigned(c, key, originals, reads, **options):
    from test_gpu_assign import _same
    params = noisy(c.da)
    h = c.da.Assigner(params, originals, band=8)
    got = h.assign(reads, item_scores=True, **options)
    h.close()
    _same(got, once(("assign", key), lambda: c.da.assignReads(params, originals, reads, band=8, host=True, item_scores=True, **options)))
    return got, (got.original, got.strand, got.score, got.second, got.status, got.item_scores)


@route
def assign_reads_in_chunks(c):
    from test_assign_cpu import shape_pool
    originals, reads = once("assign pool", lambda: shape_pool(c.da))
    c.env.setenv("DNAS_ASSIGN_CHUNK", "37")                # a prime: chunks end inside reads' item runs and between strands
    got, answer = assigned(c, "chunks", originals, reads)
    assert got.stats["chunks"] == -(-got.stats["items"] // 37) > 1
    return answer


@route
def assign_reads_candidate_lists(c):
    """Lists of 0 to 3 candidates per read."""
    from test_assign_cpu import planted_pool
    originals, reads, _ = once("assign planted", lambda: planted_pool(c.da))
    cands = [[(i + d) % len(originals) for d in range(i % 4)] for i in range(len(reads))]
    got, answer = assigned(c, "lists", originals, reads, candidates=cands)
    assert c.da.lib.ASSIGN_NO_CANDIDATES in got.status and c.da.lib.ASSIGN_OK in got.status
    return answer


@route
def assign_reads_no_candidates(c):
    """Every candidate list is empty: no item, no score kernel."""
    from test_assign_cpu import planted_pool
    originals, reads, _ = once("assign planted", lambda: planted_pool(c.da))
    got, answer = assigned(c, "empty", originals, reads[:5], candidates=[[]] * 5)
    assert list(got.status) == [c.da.lib.ASSIGN_NO_CANDIDATES] * 5 and got.stats["items"] == 0
    return answer


# ------------------------------------------------------------------------------------------------ consensus and polish
def consensus_scored(c, score):
    from test_consensus_cpu import shape_pool
    cands, reads, strands = once("consensus pool", lambda: shape_pool(c.da))
    params = noisy(c.da)
    got = c.da.consensusScore(params, cands, reads, band=8, read_strand=strands, score=score)
    want = once(("consensus", score), lambda: c.da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True, score=score))
    if score == "forward":
        from test_gpu_pair_forward import same_consensus
        same_consensus(got, want)
        return got.winner, got.status, got.total, got.second, got.totals, got.confidence, got.posterior
    from test_gpu_consensus import _same
    _same(got, want)
    return got.winner, got.status, got.total, got.second, got.totals


@route
def consensus_score_viterbi(c):
    return consensus_scored(c, "viterbi")


@route
def consensus_score_forward(c):
    return consensus_scored(c, "forward")


def polished(c, key, templates, reads, strands, rounds):
    from test_polish_cpu import same_result
    params = noisy(c.da)
    got = c.da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=rounds)
    same_result(got, once(("polish", key), lambda: c.da.consensusReads(params, templates, reads, band=8, read_strand=strands, rounds=rounds,
                                                                       host=True)))
    return got, (got.strings(), got.rounds, got.converged, got.voters, got.status,
                 [got.stats[k] for k in ("rounds", "pairs", "batches", "lds_clusters", "hbm_clusters")])


@route
def consensus_reads_template_grows(c):
    """The clusters of test_gpu_polish_columns.py that drop out one by one; the second one's template grows by a base in its
    first round and is read where that round left it in the second."""
    from test_gpu_polish_columns import shrinking_call
    templates, reads = shrinking_call()
    got, answer = polished(c, "grows", templates, reads, None, 6)
    assert len(got.strings()[1]) == len(templates[1]) + 1 and got.rounds[1] == 1 and got.stats["rounds"] == 3
    return answer


@route
def consensus_reads_tables_in_hbm(c):
    """DNAS_POLISH_LDS_POSITIONS=0, the smallest cap: the table of every non-empty template leaves LDS."""
    from test_polish_cpu import shape_pool
    templates, reads, strands = once("polish pool", lambda: shape_pool(c.da))
    c.env.setenv("DNAS_POLISH_LDS_POSITIONS", "0")
    got, answer = polished(c, "hbm", templates, reads, strands, 3)
    assert got.stats["hbm_clusters"] > 0 and got.stats["lds_clusters"] <= got.stats["rounds"]     # (the empty template alone stays)
    return answer


# ------------------------------------------------------------------------------------------------ clustering
CLUSTER_OPTIONS = dict(band=16, sketch=32, min_shared=2, max_edit_permille=230)
CLUSTER_COUNTS = ("pairs", "candidates", "items", "cells", "edges", "chunks", "clusters", "strand_conflicts")
GATE_COUNTS = ("tested", "passed", "long_pairs", "word_steps")


def cluster_answer(got):
    return (got.cluster, got.root, got.strand, got.status, list(got.edges), [got.stats[k] for k in CLUSTER_COUNTS],
            [got.gate[k] for k in GATE_COUNTS])


def cluster_pool(c):
    from test_cluster_cpu import K, shape_pool
    reads = once("cluster pool", lambda: shape_pool(c.da))
    want = once("cluster host", lambda: c.da.clusterReads(noisy(c.da), reads, host=True, edges=True, k=K, **CLUSTER_OPTIONS))
    assert 0 < want.gate["passed"] < want.gate["tested"] and want.stats["edges"] > 0
    return reads, want, K


def clustered(c, words):
    from test_cluster_cpu import same_results
    reads, want, K = cluster_pool(c)
    c.env.setenv("DNAS_CLUSTER_GATE_WORDS", str(words))
    c.env.setenv("DNAS_CLUSTER_CHUNK", "37")               # a prime: bands end inside rows
    got = c.da.clusterReads(noisy(c.da), reads, edges=True, k=K, **CLUSTER_OPTIONS)
    same_results(got, want)
    assert all(got.gate[k] == want.gate[k] for k in ("tested", "passed", "word_steps"))
    assert got.stats["chunks"] > 1 and got.gate["long_pairs"] > want.gate["long_pairs"]   # (the host counts the shipped route's)
    return cluster_answer(got)


@route
def cluster_reads_gate_one_word(c):
    return clustered(c, 1)


@route
def cluster_reads_gate_two_words(c):
    return clustered(c, 2)


@route
def clusterer_three_adds(c):
    """Batches of 10, 20 and 37 reads with two row segments: the handle's buffers grow by reserveKeep at every add."""
    from test_gpu_clusterer import cut, same_pool
    reads, want, K = cluster_pool(c)
    c.env.setenv("DNAS_CLUSTERER_SEGMENTS", "2")
    c.env.setenv("DNAS_CLUSTER_CHUNK", "37")
    batches = cut(reads, (10, 20))
    assert [len(b) for b in batches] == [10, 20, 37]
    with c.da.Clusterer(noisy(c.da), k=K, **CLUSTER_OPTIONS) as h:
        for batch in batches:
            h.add(batch)
        got = h.result(edges=True)
    same_pool(got, want)
    answer = cluster_answer(got)
    return answer[:5] + ([got.stats[k] for k in CLUSTER_COUNTS if k != "chunks"],) + answer[6:]


@route
def edit_distances_across_the_word_edge(c):
    """The pairs of test_cluster_gate_cpu.py: patterns (the shorter read) of 63 and 64 bases, one word, of 128 and 129, two words and
    three, and the longer ones."""
    from test_cluster_gate_cpu import distance_cases
    reads, pairs, _ = once("distance cases", lambda: distance_cases(c.da))
    assert {63, 64, 128, 129} <= {min(len(reads[i]), len(reads[j])) for i, j in pairs}
    got = c.da.editDistances(reads, pairs)
    assert got.dtype == np.int32 and np.array_equal(got, once("distance host", lambda: c.da.editDistances(reads, pairs, host=True)))
    return got


# ------------------------------------------------------------------------------------------------ trim
def trimmed(c, reads, what, **options):
    import trim_cases as T
    from test_gpu_trim import columns, same
    primers, _ = once("trim pool", T.shape_pool)
    got = same(c.da, primers, reads, what, **options)
    assert got.stats["columns"] == columns(primers, reads, 8)
    return got, (T.arrays(got), [got.stats[k] for k in ("items", "columns", "trimmed", "chunks", "devices")])


def trim_primers(c):
    import trim_cases as T
    return once("trim pool", T.shape_pool)[0]


def trim_reads(c):
    import trim_cases as T
    return once("trim pool", T.shape_pool)[1]


@route
def trim_reads_pair_chunks_of_one(c):
    c.env.setenv("DNAS_TRIM_PAIR_CHUNK", "1")
    got, answer = trimmed(c, trim_reads(c), "chunks of one pair")
    assert got.stats["chunks"] == len(trim_primers(c)) > 1
    return answer


@route
def trim_reads_one_read(c):
    return trimmed(c, trim_reads(c)[7:8], "one read")[1]


@route
def trim_reads_ragged_last_wave(c):
    reads = trim_reads(c) * 5
    assert len(reads) > 64 and len(reads) % 64 != 0
    return trimmed(c, reads, "pool x 5")[1]


# ------------------------------------------------------------------------------------------------ simulation
def sim_case(c, name="noisy"):
    import simulate_model as S
    strands = once("sim strands", lambda: S.random_strands(S.STRAND_LENGTHS + S.CHUNK_EDGE_LENGTHS, 11))
    assert {63, 64, 65, 127, 128, 129} <= set(map(len, strands))
    return S, S.make_params(c.da, S.PARAM_SETS[name], S.p_len_of(3))[0], strands


def sim_answer(got):
    return got.reads, got.strand, got.reversed, got.ops, got.status, [got.stats[k] for k in ("batches", "bases_in", "bases_out", "ops",
                                                                                              "reads_too_large", "devices")]


SIM_OPTIONS = dict(coverage=4, seed=0x1234567890abcdef, first_index=2 ** 32 - 3, reverse_prob=.5)


def simulated(c, thread_per_read, batches):
    from test_gpu_simulate import same
    S, mp, strands = sim_case(c)
    if thread_per_read:
        c.env.setenv("DNAS_SIMULATE_THREAD_PER_READ", "1")
    options = dict(SIM_OPTIONS)
    if batches:
        host = once("sim host", lambda: c.da.simulateReads(mp, strands, host=True, **SIM_OPTIONS))
        options["arena_bytes"] = sum(len(r) + len(o) for r, o in zip(host.reads, host.ops)) // 4 - 1
    got = same(c.da, mp, strands, (thread_per_read, batches), **options)
    assert got.stats["batches"] >= 4 if batches else got.stats["batches"] == 1
    return sim_answer(got)


@route
def simulate_wave_route(c):
    return simulated(c, False, False)


@route
def simulate_wave_route_in_batches(c):
    return simulated(c, False, True)


@route
def simulate_thread_per_read_route(c):
    return simulated(c, True, False)


@route
def simulate_thread_per_read_route_in_batches(c):
    return simulated(c, True, True)


@route
def simulate_reads_too_large(c):
    """pTanDup = .9 and an arena of the median read's bytes: the larger reads are DNAS_SIM_TOO_LARGE with length 0 and no ops,
    every other read is what the host statement gives."""
    S, mp, strands = sim_case(c, "dup-.9")
    whole = once("sim dup host", lambda: c.da.simulateReads(mp, strands, host=True, **SIM_OPTIONS))
    need = np.array([len(r) + len(o) for r, o in zip(whole.reads, whole.ops)])
    arena = int(np.median(need))
    large = need > arena
    got = c.da.simulateReads(mp, strands, arena_bytes=arena, **SIM_OPTIONS)
    assert 0 < large.sum() < len(need) and got.stats["reads_too_large"] == large.sum()
    assert np.array_equal(got.status, np.where(large, c.da.lib.SIM_TOO_LARGE, c.da.lib.SIM_OK)) and np.array_equal(got.reversed, whole.reversed)
    for i in range(len(need)):
        if large[i]:
            assert len(got.reads[i]) == 0 and len(got.ops[i]) == 0
        else:
            assert np.array_equal(got.reads[i], whole.reads[i]) and np.array_equal(got.ops[i], whole.ops[i])
    return sim_answer(got)


# ------------------------------------------------------------------------------------------------ several devices
@route
def three_devices_align_pairs(c):
    c.env.setenv("DNAS_FAKE_DEVICES", "3")
    answer = aligned(c, *align_pool(c), 8, "pool", device=-1)
    assert answer[3] == 3                                  # a batch per worker
    return answer[:3]


@route
def three_devices_trim_reads(c):
    c.env.setenv("DNAS_FAKE_DEVICES", "3")
    got, answer = trimmed(c, trim_reads(c) * 5, "three workers", device=-1)
    assert got.stats["devices"] == 3
    return answer[0], answer[1][1:3]


# ------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("byte", BYTES, ids=["unset" if b is None else b for b in BYTES])
@pytest.mark.parametrize("name", list(ROUTES))
def test_route(oracle_mod, ref_data, name, byte):
    if byte is None:
        _, stats = unpoisoned(name, oracle_mod, ref_data)
        assert stats == dict(allocations=0, frees_checked=0, violations=0, first_bytes=0, first_offset=0), stats
        return
    answer, stats = run(name, byte, oracle_mod, ref_data)
    print(name, byte, stats)
    assert stats["allocations"] > 0, "no guarded allocation: the mode was not live (a stale library?)"
    assert stats["frees_checked"] == stats["allocations"], stats
    assert stats["violations"] == 0, stats
    assert answer == unpoisoned(name, oracle_mod, ref_data)[0], "the poisoned answer is not the unpoisoned one"
