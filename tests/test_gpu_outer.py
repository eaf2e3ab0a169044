"""The pipeline's last stage end to end, with an outcome that is certain: a file through OuterCode and the inner code, exact reads
of both orientations with strands lost and strands replaced by valid frames of wrong bodies, the reads decoded on the GPU and the
messages assembled by decode_messages (dnas_outer_decode over dnas_rs_decode) -- the file comes back, the replaced strands are
named, a block beyond repair is named, and the statement (host=True) says the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import rs_exact as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, K, BODY = 12, 8, 10
MISSING = {0: (1, 9), 1: (0, 11), 2: (3, 4), 3: (0, 2, 5, 7, 10), 4: (7, 8), 6: (2, 6)}       # block -> strands without reads
REPLACED = {0: 4, 1: 5, 2: 11, 4: 0, 6: 9}                                                    # block -> the strand that arrives wrong
# The inner decoder's error model.  Under the default one the most likely message of an exact read is not always the message that
# was written: a run of zero bytes (the length prefix, the padding of the last block) comes back a byte shorter, explained as a
# duplication.  With rare duplications and deletions every exact read of this fixture decodes to its record (checked against the
# CPU oracle when the fixture was chosen), which is what makes the outcome certain.
MODEL = dict(sub=1e-3, dup=1e-6, del_open=1e-6, global_=True)


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def fixture(da, ref_data):
    machine = da.Machine.fromFile(os.path.join(ref_data, "l4c4.json"))
    code = da.OuterCode(N, K, BODY)
    data = np.random.default_rng(500).integers(0, 256, size=500, dtype=np.uint8).tobytes()
    records, B = code.encode(data, host=True)
    assert B == 7 and len(records) == 84
    sent = list(records)
    for b, p in REPLACED.items():
        s = b * N + p
        other = bytes(x ^ 0x5A for x in records[s][4:])        # wrong in every byte: every column of the block sees the error
        sent[s] = code.frame(s, other)
        assert sent[s] == R.frame(s, other)
    strands = [machine.encodeBytes(rec) for rec in sent]
    # the inner code carries a record byte for byte: every exact read decodes to its record (the CPU restatement)
    for rec, dna in zip(sent, strands):
        assert da.symbolsToBytes(machine.decodeExact(dna)) == rec
    return machine, code, data, records, sent, strands, B


def reads_of(da, strands, missing):
    """Two exact copies of every strand that has reads, every second read of the pool reverse-complemented."""
    reads = []
    for s, dna in enumerate(strands):
        if s % N in missing.get(s // N, ()):
            continue
        for _ in range(2):
            reads.append(da.reverse_complement(dna) if len(reads) % 2 else dna)
    return reads


def assemble(da, fixture, missing):
    machine, code, data, records, sent, strands, B = fixture
    reads = reads_of(da, strands, missing)
    dec = da.ViterbiDecoder(machine, da.MutatorParams.fromFlags(**MODEL), device=0)
    messages, loglike, status, strand = dec.decode(reads, strands="both")
    dec.close()
    assert strand.tolist() == [i % 2 for i in range(len(reads))] and not status.any()
    gpu = code.decode_messages(messages, B)
    host = code.decode_messages(messages, B, host=True)
    assert gpu.data == host.data and gpu.status == host.status and gpu.failed_ranges == host.failed_ranges
    for name in ("present", "column_status", "fixed"):
        assert np.array_equal(getattr(gpu, name), getattr(host, name)), name
    assert {k: v for k, v in gpu.stats.items() if k != "rs"} == {k: v for k, v in host.stats.items() if k != "rs"}
    assert gpu.stats["rs"]["columns"] == B * BODY and gpu.stats["rs"]["devices"] == 1
    return gpu


def fixed_want(B):
    fixed = np.zeros((B, N), dtype=np.int32)
    for b, p in REPLACED.items():
        fixed[b, p] = BODY
    return fixed


def test_damaged_pool_names_what_it_lost_and_returns_the_rest(da, fixture):
    machine, code, data, records, sent, strands, B = fixture
    out = assemble(da, fixture, MISSING)
    lo, hi = 3 * K * BODY - 8, 4 * K * BODY - 8
    assert out.status == da.lib.OUTER_DAMAGED and out.failed_ranges == [(lo, hi)] and len(out.data) == len(data)
    assert out.data[:lo] == data[:lo] and out.data[hi:] == data[hi:]
    want = bytearray(data[lo:hi])                              # block 3: what was received, zeros where nothing was
    for p in MISSING[3]:
        if p < K:
            want[p * BODY:(p + 1) * BODY] = bytes(BODY)
    assert out.data[lo:hi] == bytes(want)
    assert np.array_equal(out.fixed, fixed_want(B))
    assert out.present.tolist() == [[int(p not in MISSING.get(b, ())) for p in range(N)] for b in range(B)]
    assert (out.column_status[3] == R.RS_FAILED).all() and not out.column_status[5].any()
    assert (out.column_status[[0, 1, 2, 4, 6]] == R.RS_CORRECTED).all()
    assert out.stats["erased"] == 15 and out.stats["strands_fixed"] == 5 and out.stats["dropped"] == 0 and out.stats["conflicts"] == 0


def test_pool_within_capacity_returns_the_file(da, fixture):
    machine, code, data, records, sent, strands, B = fixture
    out = assemble(da, fixture, {b: m for b, m in MISSING.items() if b != 3})
    assert out.data == data and out.status == da.lib.OUTER_OK and out.failed_ranges == []
    assert np.array_equal(out.fixed, fixed_want(B)) and out.stats["erased"] == 10 and out.stats["columns_failed"] == 0


def test_command_line_round_trip(da, fixture, ref_data, tmp_path):
    """dnastore --outer-encode, the same damage to the FASTA, -V --both-strands --outer-decode: the file and the report."""
    machine, code, data, records, sent, strands, B = fixture
    exe = os.path.join(os.path.dirname(_HERE), "dnastore_amd", "bin", "dnastore")
    base = [exe, "-L", os.path.join(ref_data, "l4c4.json"), "--outer-code", "%d,%d,%d" % (N, K, BODY)]
    (tmp_path / "file.bin").write_bytes(data)
    enc = subprocess.run(base + ["--outer-encode", str(tmp_path / "file.bin")], capture_output=True, text=True, timeout=120)
    assert enc.returncode == 0 and "--outer-blocks %d" % B in enc.stderr, enc.stderr
    missing = {b: m for b, m in MISSING.items() if b != 3}
    with open(tmp_path / "reads.fa", "w") as fa:
        for i, read in enumerate(reads_of(da, strands, missing)):
            fa.write(">r%d\n%s\n" % (i, read))
    flags = ["--error-sub-prob", "0.001", "--error-dup-prob", "1e-6", "--error-del-open", "1e-6", "--error-global"]
    for extra in ([], ["--device", "-1"]):
        out = tmp_path / "out.bin"
        dec = subprocess.run(base + flags + extra + ["-V", str(tmp_path / "reads.fa"), "--both-strands", "--outer-decode", str(out),
                                                     "--outer-blocks", str(B)], capture_output=True, text=True, timeout=300)
        assert dec.returncode == 0, dec.stderr
        report = json.loads(dec.stdout)
        assert out.read_bytes() == data and report["status"] == "ok" and report["erased"] == 10 and report["failedRanges"] == []
        assert report["fixed"] == [[b * N + p, BODY] for b, p in sorted(REPLACED.items())] and report["present"] == [10, 10, 10, 12, 10, 12, 10]
