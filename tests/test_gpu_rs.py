"""dnas_rs_encode / dnas_rs_decode (csrc/rs_kernels.hip) against the statement (host=True) in every output array, over the
smallest shapes at which the kernels can go wrong: code sizes around a wave and at the limits, strand lengths around a dword, a
wave and the LDS tile of 128 columns, a different erasure set and erasure count per block, errors at the ends of the data and
parity parts, adjacent columns with no, one, the most and too many errors; the small codes also against the exhaustive decoder
of rs_exact.py.  Equalities throughout."""
import gc
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import rs_exact as R  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (2, 3, 63, 64, 65, 128, 255)
RS = (1, 2, 3, 32, 63, 64)
LS = (1, 3, 4, 5, 63, 64, 65, 257, 129)                        # 129: one column beyond the LDS tile; 257: two tiles and one column
CODES = [(n, n - r) for n in NS for r in RS if r < n]
ARRAYS = ("blocks", "status", "errors", "fixed")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def same(got, want, what=""):
    for name in ARRAYS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, name, np.argwhere(a != b)[:5].tolist())


def ladder(r):
    """Adjacent columns of one block with no error, one, the most the block's erasures leave room for, and one more."""
    return lambda b, j, f: (0, 1, (r - f) // 2, (r - f) // 2 + 1)[j % 4]


_HOST = {}


def host_of(da, key, received, present, n, k):
    """The statement's answer, computed once per input."""
    if key not in _HOST:
        _HOST[key] = da.rsDecode(received, present, n, k, host=True)
    return _HOST[key]


@pytest.mark.parametrize("n,k", CODES, ids=["%d-%d" % c for c in CODES])
def test_shape_grid(da, n, k):
    r = n - k
    rng = np.random.default_rng(n * 1000 + k)
    for L in LS:
        fs = [(n + L) % (r + 1), r if L % 2 else max(r - 2, 0)]
        clean, received, present = R.planted_blocks(n, k, L, fs, rng, errors=ladder(r))
        got = da.rsDecode(received, present, n, k)
        same(got, da.rsDecode(received, present, n, k, host=True), (n, k, L))
        assert got.stats["columns"] == 2 * L and got.stats["devices"] == 1
        for b, f in enumerate(fs):                           # what the rule promises, whoever decodes
            within = np.array([2 * ladder(r)(b, j, f) + f <= r for j in range(L)])
            assert np.array_equal(got.blocks[b][:, within], clean[b][:, within]) and (got.status[b][within] != R.RS_FAILED).all()
        data = clean[:, :k]
        enc = da.rsEncode(data, n, k)
        assert np.array_equal(enc, da.rsEncode(data, n, k, host=True)) and np.array_equal(enc, clean), (n, k, L)


@pytest.mark.parametrize("n,k,L", [(65, 33, 5), (255, 223, 3), (3, 2, 64), (64, 1, 4)])
def test_many_blocks_each_with_its_own_erasures(da, n, k, L):
    """257 blocks, f = 0 .. r + 1 in turn and the positions drawn per block: nothing of one block may reach another."""
    r = n - k
    rng = np.random.default_rng(n + k + L)
    fs = [b % (r + 2) for b in range(257)]
    clean, received, present = R.planted_blocks(n, k, L, fs, rng, errors=ladder(r))
    got = da.rsDecode(received, present, n, k)
    same(got, host_of(da, ("many", n, k, L), received, present, n, k))
    for b, f in enumerate(fs):
        if f > r:
            assert (got.status[b] == R.RS_FAILED).all() and np.array_equal(got.blocks[b], np.where(present[b][:, None] != 0, received[b], 0))
    assert np.array_equal(da.rsEncode(clean[:, :k], n, k), clean)


def test_no_blocks(da):
    got = da.rsDecode(np.zeros((0, 5, 3), dtype=np.uint8), np.zeros((0, 5), dtype=np.uint8), 5, 2)
    assert got.blocks.shape == (0, 5, 3) and got.status.shape == (0, 3) and got.fixed.shape == (0, 5)
    assert da.rsEncode(np.zeros((0, 2, 3), dtype=np.uint8), 5, 2).shape == (0, 5, 3)


@pytest.mark.parametrize("n,k", [(3, 1), (64, 32), (65, 1), (255, 223), (255, 191)])
def test_errors_at_the_ends_of_data_and_parity(da, n, k):
    """Column j has one wrong byte at position 0, k - 1, k or n - 1 in turn; the last four columns have all of them wrong that
    the code can correct."""
    r = n - k
    spots = [0, k - 1, k, n - 1]
    L = 12
    rng = np.random.default_rng(n ^ k)
    clean = R.encode_blocks(rng.integers(0, 256, size=(1, k, L), dtype=np.uint8), r)
    received = clean.copy()
    for j in range(L):
        for p in sorted(set([spots[j % 4]] if j < 8 else spots[:r // 2])):
            received[0, p, j] ^= rng.integers(1, 256)
    present = np.ones((1, n), dtype=np.uint8)
    got = da.rsDecode(received, present, n, k)
    same(got, da.rsDecode(received, present, n, k, host=True))
    assert np.array_equal(got.blocks, clean) and (got.status == R.RS_CORRECTED).all()
    assert got.fixed[0].tolist() == (received[0] != clean[0]).sum(axis=1).tolist()


def test_a_hopeless_block_between_two_good_ones(da):
    n, k, L = 20, 12, 70
    rng = np.random.default_rng(11)
    clean, received, present = R.planted_blocks(n, k, L, [1, 9, 2], rng, errors=lambda b, j, f: 1)
    got = da.rsDecode(received, present, n, k)
    same(got, da.rsDecode(received, present, n, k, host=True))
    assert np.array_equal(got.blocks[[0, 2]], clean[[0, 2]]) and (got.status[[0, 2]] == R.RS_CORRECTED).all()
    assert (got.status[1] == R.RS_FAILED).all() and not got.fixed[1].any()
    assert np.array_equal(got.blocks[1], np.where(present[1][:, None] != 0, received[1], 0))


@pytest.mark.parametrize("n,k,L", [(255, 223, 130), (40, 8, 65)])
def test_every_column_in_error_at_once(da, n, k, L):
    r = n - k
    rng = np.random.default_rng(L)
    clean, received, present = R.planted_blocks(n, k, L, [3, 0], rng)          # every column at capacity
    got = da.rsDecode(received, present, n, k)
    same(got, da.rsDecode(received, present, n, k, host=True))
    assert np.array_equal(got.blocks, clean) and (got.status == R.RS_CORRECTED).all()
    assert got.stats["columns_solved"] == 2 * L
    assert got.errors[0].tolist() == [(r - 3) // 2] * L and got.errors[1].tolist() == [r // 2] * L


def test_a_pool_without_errors_never_enters_the_solver(da):
    n, k, L = 255, 223, 37
    rng = np.random.default_rng(2)
    clean, received, present = R.planted_blocks(n, k, L, [0, 5, 32, 31], rng, errors=lambda b, j, f: 0)
    got = da.rsDecode(received, present, n, k)
    same(got, da.rsDecode(received, present, n, k, host=True))
    assert np.array_equal(got.blocks, clean) and not got.status.any() and got.stats["columns_solved"] == 0


def test_bytes_at_erased_positions_do_not_matter(da):
    n, k, L = 65, 40, 67
    rng = np.random.default_rng(4)
    clean, received, present = R.planted_blocks(n, k, L, [0, 7, 25, 26, 65], rng, errors=ladder(n - k))
    results = []
    for fill in (0x00, 0xFF):
        filled = received.copy()
        filled[present == 0] = fill
        results.append(da.rsDecode(filled, present, n, k))
    same(results[0], results[1])
    same(results[0], da.rsDecode(received, present, n, k, host=True))


@pytest.fixture(scope="module")
def pool():
    n, k, L = 65, 33, 37
    rng = np.random.default_rng(9)
    fs = [b % (n - k + 2) for b in range(11)]
    clean, received, present = R.planted_blocks(n, k, L, fs, rng, errors=ladder(n - k))
    return n, k, clean, received, present


@pytest.mark.parametrize("env,device,launches,devices", [({"DNAS_RS_CHUNK": "1"}, 0, 11, 1), ({"DNAS_RS_CHUNK": "3"}, 0, 4, 1),
                                                         ({"DNAS_FAKE_DEVICES": "3"}, -1, 3, 3),
                                                         ({"DNAS_FAKE_DEVICES": "3", "DNAS_RS_CHUNK": "3"}, -1, 5, 3)],
                         ids=["chunk1", "chunk3", "devices3", "devices3-chunk3"])
def test_launches_and_devices_change_nothing(da, pool, monkeypatch, env, device, launches, devices):
    n, k, clean, received, present = pool
    want = host_of(da, "pool", received, present, n, k)
    same(da.rsDecode(received, present, n, k), want, "plain")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    got = da.rsDecode(received, present, n, k, device=device)
    same(got, want, env)
    assert got.stats["launches"] == launches and got.stats["devices"] == devices
    assert np.array_equal(da.rsEncode(clean[:, :k], n, k, device=device), clean)


@pytest.mark.parametrize("n,k", R.SMALL_CODES)
def test_small_codes_equal_the_exhaustive_decoder(da, n, k):
    rng = np.random.default_rng(77 * n + k)
    words, present = R.small_cases(n, k, rng, 120)
    # a block per case (its own erasure set), and the same cases again as the columns of blocks that share one
    got = da.rsDecode(words[:, :, None], present, n, k)
    for c in range(len(words)):
        out, status, e = R.decode_exhaustive(words[c], present[c], n, k)
        assert got.blocks[c, :, 0].tolist() == out.tolist() and got.status[c, 0] == status and got.errors[c, 0] == e, (c, words[c], present[c])
    shared = np.unique(present, axis=0)
    for mask in shared:
        cols = words[(present == mask).all(axis=1)]
        got = da.rsDecode(np.ascontiguousarray(cols.T)[None], mask[None], n, k)
        for j in range(len(cols)):
            out, status, e = R.decode_exhaustive(cols[j], mask, n, k)
            assert got.blocks[0, :, j].tolist() == out.tolist() and got.status[0, j] == status and got.errors[0, j] == e


@pytest.mark.parametrize("byte", ["0xFF", "0x55"])
def test_on_poisoned_memory_with_guarded_allocations(da, pool, byte):
    n, k, clean, received, present = pool
    want = host_of(da, "pool", received, present, n, k)
    with pytest.MonkeyPatch.context() as env:
        env.setenv("DNAS_DEBUG_ALLOC", byte)
        gc.collect()
        da.debugAllocStats(reset=True)
        got = da.rsDecode(received, present, n, k)
        enc = da.rsEncode(clean[:, :k], n, k)
        odd = da.rsDecode(received[:, :, :5], present, n, k)                     # the byte path: L is no multiple of 4
        stats = da.debugAllocStats(reset=True)
    same(got, want, byte)
    same(odd, da.rsDecode(received[:, :, :5], present, n, k, host=True), byte)
    assert np.array_equal(enc, clean)
    assert stats["allocations"] > 0 and stats["frees_checked"] == stats["allocations"] and stats["violations"] == 0, stats
