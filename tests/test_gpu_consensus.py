"""Consensus on the GPU (csrc/consensus_kernels.hip): dnas_consensus_score against its host statement
dnas_consensus_score_host, and dnas_viterbi_clusters / ViterbiDecoder.decode_clusters / the command line's --cluster-file
against an expectation made of the CPU oracle's decodes, Machine.encodeSymbols, dnas_align_pairs_host and the Python restatement
of the definition in test_consensus_cpu.py -- never of the call under test.  Every comparison is an equality; doubles are
compared as uint64 bit patterns."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")

import synth  # noqa: E402
from test_assign_cpu import BANDS, NOISY, _bits, _rand, models  # noqa: E402
from test_consensus_cpu import NEG, OK, NO_PATH, NO_CANDIDATES, NO_READS, item_list, pick_py, shape_pool, totals_py  # noqa: E402

MACHINE = "h74l4c4.json"
PLANTED = dict(sub=.04, dup=.01, del_open=.02, del_ext=.2, length=4)
PLANTED_FLAGS = ["--error-sub-prob", ".04", "--error-dup-prob", ".01", "--error-del-open", ".02", "--error-del-ext", ".2", "-l4"]
BAND = 16


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _same(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got.winner, want.winner), (got.winner, want.winner)
    assert np.array_equal(got.status, want.status)
    assert np.array_equal(_bits(got.total), _bits(want.total)), np.flatnonzero(_bits(got.total) != _bits(want.total))
    assert np.array_equal(_bits(got.second), _bits(want.second)), np.flatnonzero(_bits(got.second) != _bits(want.second))
    assert len(got.totals) == len(want.totals)
    for c, (a, b) in enumerate(zip(got.totals, want.totals)):
        assert np.array_equal(_bits(a), _bits(b)), (c, a, b)


# --------------------------------------------------------------------------------------------- the kernels vs the host statement
def test_every_shape_model_and_band(da, monkeypatch):
    cands, reads, strands = shape_pool(da)
    n_items = len(item_list(cands, reads))
    assert n_items == 61
    monkeypatch.setenv("DNAS_ALIGN_BLOCKS", "2")           # 8 waves over 61 items: every wave walks several
    monkeypatch.setenv("DNAS_CONSENSUS_CHUNK", "37")       # a prime: chunks end inside a candidate's reads and between clusters
    statuses = set()
    want = {}
    for name, params in models(da):
        for band in BANDS:
            want[name, band] = da.consensusScore(params, cands, reads, band=band, read_strand=strands, host=True)
            got = da.consensusScore(params, cands, reads, band=band, read_strand=strands)
            _same(got, want[name, band])
            assert got.stats["chunks"] == -(-n_items // 37) > 1 and got.stats["items"] == n_items and got.stats["cells"] > 0
            assert got.stats["candidates"] == sum(len(c) for c in cands)
            statuses |= set(int(s) for s in got.status)
    assert statuses == {OK, NO_PATH, NO_CANDIDATES, NO_READS}
    monkeypatch.delenv("DNAS_ALIGN_BLOCKS")                # ... and the grid and the chunk as shipped
    monkeypatch.delenv("DNAS_CONSENSUS_CHUNK")
    for name, params in models(da):
        for band in BANDS:
            got = da.consensusScore(params, cands, reads, band=band, read_strand=strands)
            _same(got, want[name, band])
            assert got.stats["chunks"] == 1
    name, params = models(da)[2]                           # no strand array: every read as given
    _same(da.consensusScore(params, cands, reads, band=8), da.consensusScore(params, cands, reads, band=8, host=True))
    empty = da.consensusScore(params, [], [])
    assert len(empty) == 0 and empty.stats["chunks"] == 0 and empty.stats["items"] == 0
    none = da.consensusScore(params, [[], ["ACGT"]], [["ACGT"], []])       # clusters, and not one item
    assert list(none.status) == [NO_CANDIDATES, NO_READS] and none.stats["chunks"] == 0 and list(none.totals[1]) == [0.0]


def band_cells(I, O, band):
    """Cells (ip, op), 0 <= ip <= I, 0 <= op <= O, with min(0, O - I) - band <= op - ip <= max(0, O - I) + band."""
    lo, hi = min(0, O - I) - band, max(0, O - I) + band
    return sum(min(ip + hi, O) - max(ip + lo, 0) + 1 for ip in range(I + 1))


def test_boundary_row_beyond_lds(da):
    """A candidate and two reads of about 1100 bases, one reverse-complemented: the stripes hand their last row on through HBM
    instead of LDS."""
    from test_gpu_pair_align import _related
    rng = random.Random("gpu-consensus/long")
    params = da.MutatorParams.fromFlags(**NOISY)
    a = _rand(rng, 1100)
    cands = [[_rand(rng, 1100), a]]
    reads = [[da.reverse_complement(_related(rng, a, 1104)), _related(rng, a, 1096)]]
    got = da.consensusScore(params, cands, reads, band=8, read_strand=[[1, 0]])
    _same(got, da.consensusScore(params, cands, reads, band=8, read_strand=[[1, 0]], host=True))
    assert list(got.winner) == [1] and np.isfinite(got.total[0])
    assert got.stats["cells"] == sum(band_cells(len(c), len(r), 8) for c in cands[0] for r in reads[0])
    # ... and of 2100: the cell count of the stats leaves its table of lengths for the map
    b = _rand(rng, 2100)
    cands, reads = [[b]], [[_related(rng, b, 2100)]]
    got = da.consensusScore(params, cands, reads, band=8)
    _same(got, da.consensusScore(params, cands, reads, band=8, host=True))
    assert got.stats["cells"] == band_cells(2100, 2100, 8) and np.isfinite(got.total[0])


def test_all_devices(da, monkeypatch):
    cands, reads, strands = shape_pool(da)
    params = da.MutatorParams.fromFlags(**NOISY)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    want = da.consensusScore(params, cands, reads, band=8, read_strand=strands, host=True)
    one = da.consensusScore(params, cands, reads, band=8, read_strand=strands, device=0)
    many = da.consensusScore(params, cands, reads, band=8, read_strand=strands, device=-1)
    _same(many, one)
    _same(many, want)
    assert many.stats["cells"] == one.stats["cells"] and many.stats["items"] == one.stats["items"] and many.stats["chunks"] == 3
    _same(da.consensusScore(params, cands, reads, band=8, device=-1), da.consensusScore(params, cands, reads, band=8, host=True))
    two = da.consensusScore(params, cands[:2], reads[:2], band=8, read_strand=strands[:2], device=-1)    # fewer clusters than devices
    _same(two, da.consensusScore(params, cands[:2], reads[:2], band=8, read_strand=strands[:2], host=True))
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.consensusScore(params, cands, reads, device=-2)


# ------------------------------------------------------------------------------------------------- decode_clusters vs the oracle
def planted_pool(da, machine, n_clusters=40, n_reads=3):
    """The generator of the measurements in DESIGN.md 3.9 -> (messages, reads, labels): per cluster a 6-byte payload, its strand,
    n_reads mutated copies, each flipped (reverse-complemented) by a coin.  Reads are in cluster order."""
    rng = random.Random("consensus/planted")
    messages, reads, labels = [], [], []
    for k in range(n_clusters):
        payload = bytes(rng.randrange(256) for _ in range(6))
        message = synth.bytes_to_symbols(payload)
        strand = machine.encodeSymbols(message)
        mine = [synth.mutate(strand, rng, sub=.04, dele=.02, dup=.01) for _ in range(n_reads)]
        flip = [rng.random() < .5 for _ in range(n_reads)]
        messages.append(message)
        reads += [da.reverse_complement(r) if f else r for r, f in zip(mine, flip)]
        labels += ["cluster%d" % k] * n_reads
    return messages, reads, labels


def oracle_decodes(O, ref_data, reads, flags):
    """Per read what dnas_viterbi_batch_strands in mode both has to return, from two oracle decodes: (symbols, loglike, status,
    strand)."""
    orc = O.ViterbiOracle(O.Machine.from_file(os.path.join(ref_data, MACHINE)), O.MutatorParams.from_cli(**flags))
    out = []
    for r in reads:
        f, b = orc.decode(r), orc.decode(synth_revcomp(r))
        rev = b[1] > f[1]
        s, ll = b if rev else f
        out.append((s, ll, 1 if s == "" and ll == NEG else 0, int(rev)))
    return out


def synth_revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq.upper()))


def expected_clusters(da, machine, params, reads, labels, decodes, band):
    """The definition of dnas_viterbi_clusters restated over the oracle's decodes -> per cluster (label, symbols, read, total,
    second, votes, n_candidates, status), the list of every cluster's totals, and the number of messages the encoder refused."""
    names = list(dict.fromkeys(labels))
    members = {n: [i for i, lab in enumerate(labels) if lab == n] for n in names}
    cands, props, votes, groups, strands, refused = [], [], [], [], [], 0
    for n in names:
        strand_of, prop, vote = [], [], []
        for i in members[n]:
            sym, _, status, _ = decodes[i]
            if status != 0 or sym == "":
                continue
            try:
                s = machine.encodeSymbols(sym)
            except da.DnasError:                       # not a message of this machine: no candidate
                refused += 1
                continue
            if s in strand_of:
                vote[strand_of.index(s)] += 1
            else:
                strand_of.append(s)
                prop.append(i)
                vote.append(1)
        cands.append(strand_of)
        props.append(prop)
        votes.append(vote)
        groups.append([reads[i] for i in members[n]])
        strands.append([decodes[i][3] for i in members[n]])
    items = item_list(cands, groups)
    ins = [cands[c][j] for c, j, _ in items]
    outs = [synth_revcomp(groups[c][i]) if strands[c][i] else groups[c][i] for c, _, i in items]
    scores = da.alignPairs(params, ins, outs, band=band, host=True).score if items else np.zeros(0)
    totals = totals_py(cands, groups, items, scores)
    rows = []
    for c, (w, total, second, status) in enumerate(pick_py(totals, [len(g) for g in groups])):
        rows.append((names[c], decodes[props[c][w]][0] if w >= 0 else "", props[c][w] if w >= 0 else -1, total, second,
                     votes[c][w] if w >= 0 else 0, len(cands[c]), status))
    return rows, totals, refused


def check_clusters(res, rows, decodes):
    assert list(res.labels) == [r[0] for r in rows]
    assert list(res.symbols) == [r[1] for r in rows]
    assert [int(x) for x in res.read] == [r[2] for r in rows]
    assert np.array_equal(_bits(res.total), _bits([r[3] for r in rows]))
    assert np.array_equal(_bits(res.second), _bits([r[4] for r in rows]))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(_bits(res.margin), _bits([r[3] - r[4] if r[2] >= 0 else NEG for r in rows]))
    assert [int(x) for x in res.votes] == [r[5] for r in rows]
    assert [int(x) for x in res.n_candidates] == [r[6] for r in rows]
    assert [int(x) for x in res.status] == [r[7] for r in rows]
    out, ll, st, strand = res.per_read
    assert list(out) == [d[0] for d in decodes] and np.array_equal(_bits(ll), _bits([d[1] for d in decodes]))
    assert [int(x) for x in st] == [d[2] for d in decodes] and [int(x) for x in strand] == [d[3] for d in decodes]


@pytest.fixture(scope="module")
def planted(da, oracle_mod, ref_data):
    """(machine, messages, reads, labels, the oracle's decodes under the global model), computed once."""
    machine = da.Machine.fromFile(os.path.join(ref_data, MACHINE))
    messages, reads, labels = planted_pool(da, machine)
    return machine, messages, reads, labels, oracle_decodes(oracle_mod, ref_data, reads, dict(global_=True, **PLANTED))


def plurality(messages):
    """The message a unique plurality of the non-empty decoded strings names, or None."""
    count = {}
    for m in messages:
        if m:
            count[m] = count.get(m, 0) + 1
    top = sorted(count.values(), reverse=True)
    if not top or (len(top) > 1 and top[0] == top[1]):
        return None
    return max(count, key=count.get)


def test_decode_clusters_against_the_oracle(da, planted):
    """40 clusters x 3 reads on h74l4c4.json, both strands, global model, band 16.  Measured with the host statement before
    this test was fixed: all 120 orientations recovered, 96 of 120 single reads decode to the planted message, it is among the
    candidates of all 40 clusters, rescoring picks it in 40 of 40 (smallest margin 6.14 nats, no two totals equal), a unique
    plurality of the decoded strings in 36 of 40."""
    machine, messages, reads, labels, decodes = planted
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    rows, totals, refused = expected_clusters(da, machine, params, reads, labels, decodes, BAND)
    dec = da.ViterbiDecoder(machine, params, device=0)
    res = dec.decode_clusters(reads, labels, strands="both", band=BAND)
    check_clusters(res, rows, decodes)
    assert refused == 0 and res.stats["encode_failures"] == 0 and res.stats["candidates"] == sum(len(t) for t in totals)
    assert res.stats["items"] == 3 * res.stats["candidates"] and res.stats["chunks"] == 1
    assert dec.stats()["columns"] == 2 * sum(len(r) + 1 for r in reads)      # the decode's stats stay readable through the model
    # the properties measured on the CPU
    assert list(res.symbols) == messages
    assert (res.margin > 0).all() and (res.status == OK).all()
    by_vote = sum(plurality([decodes[3 * k + i][0] for i in range(3)]) == messages[k] for k in range(40))
    print("plurality names the planted message in %d of 40 clusters; smallest margin %r" % (by_vote, float(res.margin.min())))
    assert by_vote < 40
    # labels in any order: the clusters come in order of first appearance, the reads keep their order inside a cluster
    perm = list(range(len(reads)))
    random.Random("consensus/shuffle").shuffle(perm)
    shuffled = dec.decode_clusters([reads[i] for i in perm], [labels[i] for i in perm], strands="both", band=BAND)
    want, _, _ = expected_clusters(da, machine, params, [reads[i] for i in perm], [labels[i] for i in perm], [decodes[i] for i in perm], BAND)
    check_clusters(shuffled, want, [decodes[i] for i in perm])
    assert sorted(zip(shuffled.labels, shuffled.symbols)) == sorted(zip(res.labels, res.symbols))
    # forward only: the flipped reads decode to something else, the call still equals its definition
    fwd = dec.decode_clusters(reads[:9], labels[:9], strands="forward", band=BAND)
    assert list(fwd.per_read[3]) == [0] * 9 and len(fwd) == 3
    empty = dec.decode_clusters([], [])
    assert len(empty) == 0 and empty.stats["candidates"] == 0
    dec.close()


def test_local_model_candidates_are_strands(da, oracle_mod, ref_data, planted):
    """Under the local model (the command line's default) a message can come back without its leading '^'; it encodes to the
    strand of the full message, so the two are ONE candidate: no cluster has two candidates with bit-equal totals."""
    machine, messages, reads, labels, _ = planted
    n = 3 * 6
    reads, labels = reads[:n], labels[:n]
    decodes = oracle_decodes(oracle_mod, ref_data, reads, PLANTED)
    params = da.MutatorParams.fromFlags(**PLANTED)
    rows, totals, refused = expected_clusters(da, machine, params, reads, labels, decodes, BAND)
    for ts in totals:
        assert len(set(_bits(ts).tolist())) == len(ts)
    dec = da.ViterbiDecoder(machine, params, device=0)
    res = dec.decode_clusters(reads, labels, strands="both", band=BAND)
    check_clusters(res, rows, decodes)
    assert [int(x) for x in res.n_candidates] == [len(ts) for ts in totals] and res.stats["encode_failures"] == refused
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli(da, planted, ref_data, tmp_path):
    machine, messages, reads, labels, decodes = planted
    n = 3 * 8
    reads, labels = reads[:n], labels[:n]
    order = [i for k in range(3) for i in range(k, n, 3)]             # the clusters interleaved: the FASTA is not grouped
    reads, labels = [reads[i] for i in order], [labels[i] for i in order]
    fa, lab, short = str(tmp_path / "pool.fa"), str(tmp_path / "labels.txt"), str(tmp_path / "short.txt")
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">read%d\n%s\n" % (i, r))
    with open(lab, "w") as f:
        f.write("".join(l + "\n" for l in labels))
    with open(short, "w") as f:
        f.write("".join(l + "\n" for l in labels[:-1]))
    params = da.MutatorParams.fromFlags(global_=True, **PLANTED)
    dec = da.ViterbiDecoder(machine, params, device=0)
    res = dec.decode_clusters(reads, labels, strands="both", band=BAND)
    dec.close()
    assert list(res.symbols) == messages[:8]
    base = ["-L", os.path.join(ref_data, MACHINE), "-V", fa, "--cluster-file", lab, "--both-strands", "--error-global", "--align-band", str(BAND)]
    run = lambda args: subprocess.run([BIN, "-v0"] + PLANTED_FLAGS + args, capture_output=True, timeout=300)
    r = run(base)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    want = []
    for name, sym in zip(res.labels, res.symbols):
        want += [">" + name] + [sym[i:i + 50] for i in range(0, len(sym), 50)]
    assert r.stdout.decode().splitlines() == want
    r = run(base + ["-r"])
    assert r.returncode == 0 and r.stdout.decode().splitlines() == list(res.symbols)
    r = run(base + ["--cluster-table"])
    assert r.returncode == 0
    lines = [l.split("\t") for l in r.stdout.decode().splitlines()]
    assert len(lines) == 8
    for c, (name, n_reads, n_cand, votes, total, margin, sym) in enumerate(lines):
        assert name == res.labels[c] and int(n_reads) == 3 and int(n_cand) == res.n_candidates[c] and int(votes) == res.votes[c]
        assert float(total) == res.total[c] and float(margin) == res.margin[c] and sym == res.symbols[c]
    # forward only: another result, the same as the library's
    dec = da.ViterbiDecoder(machine, params, device=0)
    fwd = dec.decode_clusters(reads, labels, strands="forward", band=BAND)
    dec.close()
    r = run([a for a in base if a != "--both-strands"] + ["-r"])
    assert r.returncode == 0 and r.stdout.decode().split("\n")[:-1] == list(fwd.symbols) and list(fwd.symbols) != list(res.symbols)
    for c in range(8):                                                  # a cluster without a winner is named
        assert (("No consensus for %s:" % fwd.labels[c]).encode() in r.stderr) == (fwd.read[c] < 0)
    bad = run(["-L", os.path.join(ref_data, MACHINE), "-V", fa, "--cluster-file", short, "--both-strands", "--error-global"])
    assert bad.returncode == 1 and bad.stdout == b"" and b"cluster names" in bad.stderr
    for args in (["-L", os.path.join(ref_data, MACHINE), "--cluster-file", lab], [a for a in base if a not in ("--cluster-file", lab)] + ["--cluster-table"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b""
