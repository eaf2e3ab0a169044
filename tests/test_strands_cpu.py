"""Both-strand decode, the parts that need no GPU: the new symbols of the C ABI, the host helper
dnas_reverse_complement, argument checking of dnas_viterbi_batch_strands, the command line's --both-strands /
--reverse-strand, and shard.gather_results with a strand tensor (gloo)."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")
D = os.path.join(ROOT, "tests", "golden", "ref_data")

NEW_SYMBOLS = ["dnas_viterbi_batch_strands", "dnas_viterbi_batch_strands_device", "dnas_reverse_complement",
               "dnas_model_last_strand_stats", "dnas_decode_fastseqs_strands", "dnas_decoded_strand"]


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_new_symbols_are_declared_and_exported(da):
    L = da.lib.lib()
    declared = da.lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    header = open(da.lib.HEADER_PATH).read()
    for word in ("#define DNAS_STRAND_FORWARD 0", "#define DNAS_STRAND_REVERSE 1", "#define DNAS_STRAND_BOTH 2", "dnas_strand_stats"):
        assert word in header
    assert (da.lib.STRAND_FORWARD, da.lib.STRAND_REVERSE, da.lib.STRAND_BOTH) == (0, 1, 2)
    assert [k for k, _ in da.lib.StrandStatsC._fields_] == ["reads", "reverse_won", "ties", "both_no_path", "tracebacks", "fill_columns",
                                                           "pass2_columns"]
    assert ctypes.sizeof(da.lib.StrandStatsC) == 7 * 8 and ctypes.sizeof(da.lib.BatchStatsC) == 7 * 8      # dnas_batch_stats keeps its layout


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 10000])
def test_reverse_complement_helper(da, n):
    L = da.lib.lib()
    rng = np.random.default_rng(n)
    seq = rng.integers(0, 4, size=n, dtype=np.uint8)
    want = np.array([3 - int(b) for b in reversed(seq.tolist())], dtype=np.uint8)       # the restatement
    out = np.full(max(n, 1), 9, dtype=np.uint8)
    assert L.dnas_reverse_complement(seq.ctypes.data if n else None, n, out.ctypes.data) == 0
    assert np.array_equal(out[:n], want)
    back = np.full(max(n, 1), 9, dtype=np.uint8)
    assert L.dnas_reverse_complement(out.ctypes.data, n, back.ctypes.data) == 0 and np.array_equal(back[:n], seq)   # an involution
    # the Python layer: arrays of codes and strings
    assert np.array_equal(da.reverse_complement(seq), want)
    text = "".join("ACGT"[b] for b in seq)
    assert da.reverse_complement(text) == "".join("ACGT"[b] for b in want)
    assert da.reverse_complement(text.lower()) == da.reverse_complement(text)
    if n:
        bad = seq.copy()
        bad[n // 2] = 4
        assert L.dnas_reverse_complement(bad.ctypes.data, n, out.ctypes.data) == -6                               # DNAS_E_BAD_BASE
        assert b"base code > 3" in L.dnas_last_error()


def test_palindromes(da):
    for s in ("", "AT", "ACGT", "AATT", "GAATTC"):
        assert da.reverse_complement(s) == s
    assert da.reverse_complement("A") == "T" and da.reverse_complement("AAC") == "GTT"


def test_batch_strands_argument_checks(da):
    """The mode and out_strand are checked before anything else (DNAS_E_INVALID); a valid call without a GPU answers
    DNAS_E_DEVICE as every device entry point does (with one, the null model is what is wrong)."""
    L = da.lib.lib()
    strand = np.zeros(4, dtype=np.uint8)
    for fn in (L.dnas_viterbi_batch_strands, L.dnas_viterbi_batch_strands_device):
        assert fn(None, 0, None, None, 3, None, None, None, None, None, strand.ctypes.data) == -1
        assert b"strand_mode" in L.dnas_last_error()
        assert fn(None, 0, None, None, -1, None, None, None, None, None, strand.ctypes.data) == -1
        assert fn(None, 0, None, None, da.lib.STRAND_BOTH, None, None, None, None, None, None) == -1
        assert b"out_strand" in L.dnas_last_error()
        rc = fn(None, 0, None, None, da.lib.STRAND_BOTH, None, None, None, None, None, strand.ctypes.data)
        assert rc == (-7 if L.dnas_device_count() == 0 else -1)
    h = ctypes.c_void_p()
    m = da.Machine.fromFile(os.path.join(D, "l4c4.json"))
    p = da.MutatorParams.fromFlags()
    assert L.dnas_decode_fastseqs_strands(os.path.join(D, "hello.fa").encode(), m._h, ctypes.byref(p.c), 0, 0, 3, ctypes.byref(h)) == -1
    assert L.dnas_decoded_strand(None, 0) == 0
    with pytest.raises(ValueError):
        da.lib.strand_mode("sideways")
    assert [da.lib.strand_mode(x) for x in ("forward", "reverse", "both", 2)] == [0, 1, 2, 2]


def _cli(*args):
    r = subprocess.run([BIN] + list(args), capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_cli_strand_flags(da):
    base = ["-L", os.path.join(D, "l4c4.json"), "-V", os.path.join(D, "hello.fa")]
    plain = _cli(*base)
    for flag in ("--both-strands", "--reverse-strand"):
        got = _cli(*(base + [flag]))
        if da.lib.lib().dnas_device_count() == 0:
            assert got == plain and got[0] != 0 and got[1] == b""       # ends as the same command without the flag does: no GPU
        else:
            assert got[0] == plain[0] == 0
    # usage errors: with another action, and both together
    for args in (["-L", os.path.join(D, "l4c4.json"), "-d", os.path.join(D, "hello.fa"), "--both-strands"],
                 ["-L", os.path.join(D, "l4c4.json"), "--both-strands"],
                 ["-L", os.path.join(D, "l4c4.json"), "-E", "HELLO", "--reverse-strand"],
                 base + ["--both-strands", "--reverse-strand"]):
        rc, out, err = _cli(*args)
        assert rc == 1 and out == b"" and b"strand" in err, args
    rc, out, err = _cli("--help")
    assert b"--both-strands" in out and b"--reverse-strand" in out
    # without the flags nothing changed
    rc, out, err = _cli("-L", os.path.join(D, "l4c4.json"), "-d", os.path.join(D, "hello.fa"))
    assert rc == 0 and out == open(os.path.join(D, "hello.txt"), "rb").read()


# ---- shard.gather_results(..., strand=t) over gloo ------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_results(rank, world, n, cap):
    """What rank `rank` holds of a job of n reads dealt round-robin: k reads, every array a function of the read index."""
    idx = np.arange(rank, n, world)
    k = len(idx)
    sym = np.zeros(k * cap, dtype=np.uint8)
    for j, i in enumerate(idx):
        sym[j * cap:j * cap + 3] = (i % 200) + 1
    return idx, sym, (idx % 7).astype(np.int32), -idx.astype(np.float64), (idx % 2).astype(np.uint8), ((idx // 2) % 2).astype(np.uint8)


def _worker(rank, world, port, n, q):
    sys.path.insert(0, ROOT)
    from dnastore_amd import shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cap = 16
    idx, sym, olen, ll, st, strand = _shard_results(rank, world, n, cap)
    t = [torch.from_numpy(x) for x in (sym, olen, ll, st)]
    with_strand = shard.gather_results(*t, world, rank, strand=torch.from_numpy(strand))
    without = shard.gather_results(*t, world, rank)
    if rank == 0:
        q.put(([tuple(x.numpy() for x in g) for g in with_strand], [len(g) for g in without]))
    else:
        assert with_strand is None and without is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 7), (3, 10)])          # unequal shards: 4 + 3, 4 + 3 + 3
def test_gather_results_with_strand(world, n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    gathered, plain_sizes = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert plain_sizes == [4] * world                            # without the keyword: tuples of four, as ever
    for r in range(world):
        idx, sym, olen, ll, st, strand = _shard_results(r, world, n, 16)
        assert len(gathered[r]) == 5
        for got, want in zip(gathered[r], (sym, olen, ll, st, strand)):
            assert got.dtype == want.dtype and np.array_equal(got, want)


def test_gather_results_single_process():
    sys.path.insert(0, ROOT)
    from dnastore_amd import shard
    t = [torch.zeros(8, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.uint8)]
    strand = torch.ones(2, dtype=torch.uint8)
    assert len(shard.gather_results(*t, 1, 0)[0]) == 4
    res = shard.gather_results(*t, 1, 0, strand=strand)
    assert len(res) == 1 and len(res[0]) == 5 and res[0][4] is strand
