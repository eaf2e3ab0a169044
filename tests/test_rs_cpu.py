"""dnas_rs_encode_host / dnas_rs_decode_host (csrc/host/rs.cpp), the statement of the outer code, and the strand frame and file
layer over it (csrc/host/outer.cpp, host=True), against the code's definition restated in pure Python (rs_exact.py): the published
generator and parity values, an exhaustive decoder over all codewords of eight small codes, planted codewords of the large ones --
no GPU.  Equalities throughout."""
import os
import sys

import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import rs_exact as R  # noqa: E402

LARGE_CODES = [(255, 223), (255, 191), (65, 1), (64, 33), (129, 128)]


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_library_declares_the_outer_code(da):
    names = {"dnas_rs_encode", "dnas_rs_decode", "dnas_rs_encode_host", "dnas_rs_decode_host", "dnas_outer_encode", "dnas_outer_decode",
             "dnas_outer_frame", "dnas_outer_crc8", "dnas_outer_blocks"}
    assert names <= set(da.lib.declared_symbols())
    assert all(hasattr(da.lib.lib(), s) for s in names)


def test_generator_of_seven_parity_symbols_is_the_published_one(da):
    want = [0, 87, 229, 146, 149, 238, 102, 21]
    assert [int(R.LOG[c]) for c in R.generator(7)] == want
    # x^7 modulo g is g without its leading term: the parity of the one data symbol 1
    word = da.rsEncode(np.array([[[1]]], dtype=np.uint8), 8, 1, host=True)[0, :, 0]
    assert [int(R.LOG[c]) for c in word] == [0] + want[1:]


def test_published_parity_of_sixteen_data_bytes(da):
    data = [32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17]
    parity = [196, 35, 39, 119, 235, 215, 231, 226, 93, 23]
    assert R.encode(data, 10) == data + parity
    got = da.rsEncode(np.array(data, dtype=np.uint8).reshape(1, 16, 1), 26, 16, host=True)
    assert got[0, :, 0].tolist() == data + parity
    # ... and as one column among others of a wider block
    wide = np.zeros((16, 3), dtype=np.uint8)
    wide[:, 1] = data
    got = da.rsEncode(wide, 26, 16, host=True)
    assert got[:, 1].tolist() == data + parity and not got[:, 0].any() and not got[:, 2].any()


@pytest.mark.parametrize("n,k", LARGE_CODES)
def test_encode_is_the_long_division(da, n, k):
    rng = np.random.default_rng(n * 256 + k)
    data = rng.integers(0, 256, size=(2, k, 3), dtype=np.uint8)
    got = da.rsEncode(data, n, k, host=True)
    assert np.array_equal(got, R.encode_blocks(data, n - k))
    assert not R.syndromes(got, n - k).any()
    assert got[0, :, 1].tolist() == R.encode(data[0, :, 1], n - k)


def test_parameters_outside_the_code_are_unsupported(da):
    one = np.zeros((1, 1, 1), dtype=np.uint8)
    for n, k in ((1, 1), (256, 200), (255, 190), (4, 4), (4, 0)):
        with pytest.raises(da.DnasError) as err:
            da.rsEncode(np.zeros((1, max(k, 0), 1), dtype=np.uint8) if k else one[:, :0], n, k, host=True)
        assert err.value.code == -9, (n, k)
    with pytest.raises(da.DnasError) as err:
        da.rsDecode(np.zeros((1, 255, 1), dtype=np.uint8), np.ones((1, 255), dtype=np.uint8), 255, 190, host=True)
    assert err.value.code == -9


@pytest.mark.parametrize("n,k", R.SMALL_CODES)
def test_small_codes_equal_the_exhaustive_decoder(da, n, k):
    """Every case its own block of one column, so that every case has its own erasure set."""
    r = n - k
    rng = np.random.default_rng(1000 * n + k)
    words, present = R.small_cases(n, k, rng, 360)
    got = da.rsDecode(words[:, :, None], present, n, k, host=True)
    seen = set()
    for c in range(len(words)):
        out, status, e = R.decode_exhaustive(words[c], present[c], n, k)
        assert got.blocks[c, :, 0].tolist() == out.tolist() and got.status[c, 0] == status and got.errors[c, 0] == e, (c, words[c], present[c])
        changed = (out != words[c]) & present[c].astype(bool) if status == R.RS_CORRECTED else np.zeros(n, dtype=bool)
        assert got.fixed[c].tolist() == changed.astype(int).tolist()
        seen.add(status)
    assert seen == {R.RS_OK, R.RS_FAILED} | ({R.RS_CORRECTED} if r >= 2 else set())


@pytest.mark.parametrize("n,k", LARGE_CODES)
def test_planted_codewords_within_capacity_come_back(da, n, k):
    r = n - k
    fs = [0, 1, r - 1, r]
    rng = np.random.default_rng(n + k)
    clean, received, present = R.planted_blocks(n, k, 2, fs, rng)
    got = da.rsDecode(received, present, n, k, host=True)
    assert np.array_equal(got.blocks, clean)
    for b, f in enumerate(fs):
        e = (r - f) // 2
        assert got.errors[b].tolist() == [e, e] and got.status[b].tolist() == [R.RS_CORRECTED if e else R.RS_OK] * 2
        wrong = ((received[b] != clean[b]) & (present[b][:, None] != 0)).sum(axis=1)
        assert got.fixed[b].tolist() == wrong.tolist()


def test_corrected_columns_are_codewords_within_the_distance_bound(da):
    """Errors from none to beyond capacity: whatever the statement calls corrected is a codeword that differs from the received
    word in e present positions, 2 e + f <= r; what it calls failed is the received word."""
    n, k, L = 40, 28, 24
    r = n - k
    fs = [0, 3, 4, 12]
    rng = np.random.default_rng(5)
    clean, received, present = R.planted_blocks(n, k, L, fs, rng, errors=lambda b, j, f: j % 10)
    got = da.rsDecode(received, present, n, k, host=True)
    syn = R.syndromes(got.blocks, r)
    for b, f in enumerate(fs):
        here = present[b] != 0
        for j in range(L):
            e = j % 10
            st = got.status[b, j]
            if 2 * e + f <= r:
                assert st == (R.RS_CORRECTED if e else R.RS_OK) and got.errors[b, j] == e and np.array_equal(got.blocks[b, :, j], clean[b, :, j])
            if st != R.RS_FAILED:
                diff = int((got.blocks[b, here, j] != received[b, here, j]).sum())
                assert not syn[b, :, j].any() and diff == got.errors[b, j] and 2 * diff + f <= r
            else:
                assert got.errors[b, j] == 0 and np.array_equal(got.blocks[b, :, j], np.where(here, received[b, :, j], 0))
    assert {R.RS_OK, R.RS_CORRECTED, R.RS_FAILED} == set(got.status.ravel().tolist())


@pytest.mark.parametrize("n,k", [(255, 223), (64, 33), (3, 2)])
def test_more_erasures_than_parity_fail_in_every_column(da, n, k):
    r = n - k
    rng = np.random.default_rng(3)
    clean, received, present = R.planted_blocks(n, k, 3, [r + 1, n, 0], rng, errors=lambda b, j, f: 0)
    got = da.rsDecode(received, present, n, k, host=True)
    for b in (0, 1):
        assert got.status[b].tolist() == [R.RS_FAILED] * 3 and not got.errors[b].any() and not got.fixed[b].any()
        assert np.array_equal(got.blocks[b], np.where(present[b][:, None] != 0, received[b], 0))
    assert got.status[2].tolist() == [R.RS_OK] * 3 and np.array_equal(got.blocks[2], clean[2])


def test_bytes_at_erased_positions_are_never_read(da):
    n, k, L = 31, 20, 9
    rng = np.random.default_rng(8)
    clean, received, present = R.planted_blocks(n, k, L, [0, 2, 5, 11, 12, 31], rng, errors=lambda b, j, f: j % 7)
    results = []
    for fill in (0, 255, None):
        r2 = received.copy()
        gone = present == 0
        r2[gone] = rng.integers(0, 256, size=(int(gone.sum()), L), dtype=np.uint8) if fill is None else fill
        results.append(da.rsDecode(r2, present, n, k, host=True))
    for other in results[1:]:
        for name in ("blocks", "status", "errors", "fixed"):
            assert np.array_equal(getattr(other, name), getattr(results[0], name)), name


def test_no_blocks_is_a_valid_call(da):
    got = da.rsDecode(np.zeros((0, 5, 3), dtype=np.uint8), np.zeros((0, 5), dtype=np.uint8), 5, 2, host=True)
    assert got.blocks.shape == (0, 5, 3) and got.status.shape == (0, 3)
    assert da.rsEncode(np.zeros((0, 2, 3), dtype=np.uint8), 5, 2, host=True).shape == (0, 5, 3)


# ---- the strand frame and the file layer ------------------------------------------------------------------------------------------

N, K, BODY = 12, 8, 10


def _file(length, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=length, dtype=np.uint8).tobytes()


def test_crc_and_frame_follow_the_definition(da):
    assert R.crc8(b"123456789") == 0xF4                       # the check value of CRC-8 (0x07, init 0, not reflected)
    code = da.OuterCode(N, K, BODY)
    body = bytes(range(BODY))
    for s in (0, 1, 255, 256, 65535, 65536, (1 << 24) - 1):
        assert code.frame(s, body) == R.frame(s, body)
    buf = np.frombuffer(b"123456789", dtype=np.uint8)
    assert da.lib.lib().dnas_outer_crc8(buf.ctypes.data, len(buf)) == 0xF4


@pytest.mark.parametrize("length", [0, 1, K * BODY - 8, K * BODY - 7, 3001])
def test_file_round_trip(da, length):
    code = da.OuterCode(N, K, BODY)
    data = _file(length, seed=length)
    records, B = code.encode(data, host=True)
    stream, wantB = R.stream_of(data, K, BODY)
    assert B == wantB == code.n_blocks(length) and len(records) == B * N
    blocks = R.encode_blocks(np.frombuffer(stream, dtype=np.uint8).reshape(B, K, BODY), N - K)
    assert records == [R.frame(s, blocks[s // N, s % N].tobytes()) for s in range(B * N)]
    out = code.decode(records, B, host=True)
    assert out.data == data and out.status == da.lib.OUTER_OK and out.failed_ranges == []
    assert out.present.all() and not out.fixed.any() and not out.column_status.any()
    assert out.stats["records"] == B * N and out.stats["dropped"] == 0 and out.stats["erased"] == 0
    # shuffled, with the copies of a few records, and four strands of every block gone
    rng = np.random.default_rng(length + 1)
    pool = [rec for s, rec in enumerate(records) if s % N not in (1, 5, 8, 11)]
    pool = pool + pool[::7]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    out = code.decode(pool, B, host=True)
    assert out.data == data and out.status == da.lib.OUTER_OK and out.stats["erased"] == 4 * B
    assert out.present.tolist() == [[int(p not in (1, 5, 8, 11)) for p in range(N)]] * B


def test_invalid_records_are_dropped(da):
    code = da.OuterCode(N, K, BODY)
    data = _file(150)
    records, B = code.encode(data, host=True)
    assert B == 2
    bad_crc = bytearray(records[3])
    bad_crc[7] ^= 1
    bad_number = bytearray(records[4])
    bad_number[2] ^= 1
    beyond = R.frame(B * N, bytes(BODY))                      # a valid frame of a strand the pool does not have
    pool = [r for s, r in enumerate(records) if s not in (3, 4)] + [bytes(bad_crc), bytes(bad_number), beyond, records[0][:-1], records[1] + b"\0",
                                                                    b""]
    out = code.decode(pool, B, host=True)
    assert out.stats["dropped"] == 6 and out.stats["erased"] == 2
    assert out.present.ravel().tolist() == [int(s not in (3, 4)) for s in range(B * N)]
    assert out.data == data and out.status == da.lib.OUTER_OK


def test_duplicates_weights_and_ties(da):
    code = da.OuterCode(N, K, BODY)
    data = _file(60)
    records, B = code.encode(data, host=True)
    assert B == 1
    wrong = [code.frame(s, bytes(b ^ 0xFF for b in records[s][4:])) for s in range(N)]     # valid frames, every body byte wrong
    # slot 0: two against one; slots 1 and 3: one against one, ties; slot 2: the wrong one is heavier by count
    pool = records[4:] + [records[0], wrong[0], records[0]] + [records[1], wrong[1]] + [wrong[2], records[2], wrong[2]] + [records[3], wrong[3]]
    out = code.decode(pool, B, host=True)
    assert out.stats["conflicts"] == 4 and out.stats["ties"] == 2 and out.stats["erased"] == 2
    assert out.present[0].tolist() == [1, 0, 1, 0] + [1] * 8
    assert out.fixed[0].tolist() == [0, 0, BODY, 0] + [0] * 8 and out.data == data       # 2 erasures + 2 x 1 error = r
    weights = [1.0] * len(pool)
    assert pool[17] == wrong[3] and pool[11] == records[1]
    weights[17] = 1.5                                          # wrong[3] outweighs records[3] ...
    weights[11] = 1.25                                         # ... and slot 1's tie is broken the right way
    out = code.decode(pool, B, weights=weights, host=True)
    assert out.stats["ties"] == 0 and out.present.all()
    assert out.fixed[0].tolist() == [0, 0, BODY, BODY] + [0] * 8 and out.data == data and out.status == da.lib.OUTER_OK
    # weights add up in a group: three records of 0.5 beat one of 1.25
    pool2 = records[1:] + [wrong[0], records[0], records[0], records[0]]
    out = code.decode(pool2, B, weights=[1.0] * (N - 1) + [1.25, 0.5, 0.5, 0.5], host=True)
    assert not out.fixed.any() and out.present.all() and out.data == data


def test_a_lost_length_prefix_returns_the_raw_stream(da):
    code = da.OuterCode(N, K, BODY)
    data = _file(150)
    records, B = code.encode(data, host=True)
    stream, _ = R.stream_of(data, K, BODY)
    pool = [r for s, r in enumerate(records) if not (s < N and s % N in (0, 2, 4, 6, 8))]     # block 0 loses five strands: r = 4
    out = code.decode(pool, B, host=True)
    assert out.status == da.lib.OUTER_NO_LENGTH and len(out.data) == B * K * BODY
    assert out.failed_ranges == [(0, K * BODY)]                # every byte of a failed column, received or not
    got = np.frombuffer(out.data, dtype=np.uint8)
    want = np.frombuffer(stream, dtype=np.uint8).copy()
    for p in (0, 2, 4, 6):
        want[p * BODY:(p + 1) * BODY] = 0
    assert np.array_equal(got, want)
    assert (out.column_status[0] == R.RS_FAILED).all() and not out.column_status[1].any()
    # a length that exceeds the stream
    forged = R.encode_blocks(np.frombuffer((1 << 40).to_bytes(8, "little") + bytes(K * BODY - 8), dtype=np.uint8).reshape(1, K, BODY), N - K)
    out = code.decode([R.frame(s, forged[0, s].tobytes()) for s in range(N)], 1, host=True)
    assert out.status == da.lib.OUTER_BAD_LENGTH and len(out.data) == K * BODY and out.failed_ranges == []


def test_a_failed_block_past_the_prefix_names_its_ranges(da):
    code = da.OuterCode(N, K, BODY)
    data = _file(500)
    records, B = code.encode(data, host=True)
    assert B == 7
    pool = [r for s, r in enumerate(records) if not (s // N == 3 and s % N < 5)]
    out = code.decode(pool, B, host=True)
    lo = 3 * K * BODY - 8
    assert out.status == da.lib.OUTER_DAMAGED and out.failed_ranges == [(lo, lo + K * BODY)] and len(out.data) == 500
    want = bytearray(data)
    want[lo:lo + 5 * BODY] = bytes(5 * BODY)
    assert out.data == bytes(want)


def test_command_line_prints_the_strands_of_a_file(da, ref_data, tmp_path):
    """--outer-encode without a GPU runs the host statement: the records of OuterCode.encode, each through the machine's byte
    encoder, named s<number>."""
    machine_file = os.path.join(ref_data, "l4c4.json")
    data = _file(150)
    path = tmp_path / "file.bin"
    path.write_bytes(data)
    exe = os.path.join(os.path.dirname(_HERE), "dnastore_amd", "bin", "dnastore")
    run = subprocess.run([exe, "-L", machine_file, "--outer-code", "%d,%d,%d" % (N, K, BODY), "--outer-encode", str(path)], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    names, seqs = [], []
    for line in run.stdout.splitlines():
        if line.startswith(">"):
            names.append(line[1:])
            seqs.append("")
        else:
            seqs[-1] += line
    machine = da.Machine.fromFile(machine_file)
    records, B = da.OuterCode(N, K, BODY).encode(data, host=True)
    assert names == ["s%d" % s for s in range(B * N)] and seqs == [machine.encodeBytes(r) for r in records]
    assert "--outer-blocks %d" % B in run.stderr
    for args in (["--outer-encode", str(path)], ["--outer-code", "12,8"], ["--outer-code", "12,8,10", "-V", "x.fa", "--outer-decode", "out"]):
        bad = subprocess.run([exe, "-L", machine_file] + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 1 and bad.stdout == "", args


def test_statement_and_file_layer_under_sanitizers(tmp_path):
    """The statement, the solver the second kernel shares with it, and the file layer in a stand-alone host program built with
    -fsanitize=address,undefined (tools/rs_host_check.cpp)."""
    root = os.path.dirname(_HERE)
    exe = str(tmp_path / "rs_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tools", "rs_host_check.cpp"), os.path.join(root, "dnastore_amd", "csrc", "host", "rs.cpp"),
                    os.path.join(root, "dnastore_amd", "csrc", "host", "outer.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"rs host check: ok" in r.stdout, r.stderr.decode()
