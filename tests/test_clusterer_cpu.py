"""The persistent clusterer (dnas_clusterer_*, csrc/clusterer_kernels.hip) as far as a machine without a GPU reaches: the exported
symbols, the checks dnas_clusterer_create makes before it touches a device, the command line's usage error, and the handle's
bookkeeping (csrc/host/clusterer.hpp) under AddressSanitizer + UBSan in a program of its own (tools/clusterer_host_check.cpp)."""
import ctypes
import os
import subprocess
import sys

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from test_assign_cpu import NOISY, _fasta  # noqa: E402
from test_cluster_cpu import BIN, ROOT  # noqa: E402

E_INVALID, E_UNSUPPORTED = -1, -9
SYMBOLS = ("dnas_clusterer_create", "dnas_clusterer_add", "dnas_clusterer_reads", "dnas_clusterer_result", "dnas_clusterer_destroy")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_symbols_are_declared_and_exported(da):
    declared = da.lib.declared_symbols()
    L = da.lib.lib()
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name), name
    assert hasattr(da, "Clusterer")


def create(da, params, band=32, k=12, m=32, min_shared=2, floor=0.0, permille=-1, device=0, out=True):
    """-> (status, dnas_last_error, handle or None)."""
    L = da.lib.lib()
    h = ctypes.c_void_p()
    rc = L.dnas_clusterer_create(ctypes.byref(params.c) if params is not None else None, band, k, m, min_shared, floor, permille, device,
                                 ctypes.byref(h) if out else None)
    return rc, L.dnas_last_error().decode(), h


@pytest.mark.parametrize("bad", (dict(m=17), dict(k=0), dict(k=32), dict(min_shared=33), dict(m=16, min_shared=17), dict(min_shared=-1),
                                 dict(permille=-2), dict(permille=1001), dict(band=-2), dict(out=False)),
                         ids=lambda bad: ",".join("%s=%s" % kv for kv in bad.items()))
def test_create_refuses_before_any_device_call(da, bad):
    """DNAS_E_INVALID with a message, whatever the device: -1 would be DNAS_E_UNSUPPORTED and 10 ** 6 names no device, but the
    parameters are looked at first."""
    params = da.MutatorParams.fromFlags(**NOISY)
    L = da.lib.lib()
    for device in (0, -1, 10 ** 6):
        L.dnas_machine_load_json(b"/nonexistent/machine.json", ctypes.byref(ctypes.c_void_p()))   # (leaves another message behind)
        before = L.dnas_last_error().decode()
        rc, msg, h = create(da, params, device=device, **bad)
        assert rc == E_INVALID and msg and msg != before and not h.value, (bad, device, rc, msg)


def test_create_null_params_and_all_devices(da):
    params = da.MutatorParams.fromFlags(**NOISY)
    rc, msg, h = create(da, None)
    assert rc == E_INVALID and msg and not h.value
    rc, msg, h = create(da, params, device=-1)
    assert rc == E_UNSUPPORTED and "device" in msg and not h.value
    with pytest.raises(da.DnasError, match="DNAS_E_UNSUPPORTED"):
        da.Clusterer(params, device=-1)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.Clusterer(params, sketch=17)
    L = da.lib.lib()
    L.dnas_clusterer_destroy(None)                           # allowed
    assert L.dnas_clusterer_reads(None) == 0


def test_cli_usage(tmp_path):
    pool = str(tmp_path / "pool.fa")
    _fasta(pool, ["a", "b"], ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"])
    run = lambda args: subprocess.run([BIN, "-v0"] + args, capture_output=True, timeout=60)
    for args in (["--cluster-add", pool], ["--cluster-add"], ["-V", pool, "--cluster-auto", "--cluster-add", pool],
                 ["--cluster-reads", pool, "--cluster-add"]):
        bad = run(args)
        assert bad.returncode == 1 and bad.stdout == b"" and bad.stderr, args
    assert b"--cluster-add goes with --cluster-reads only" in run(["--cluster-add", pool]).stderr
    assert b"--cluster-add" in run(["--help"]).stdout


def test_bookkeeping_under_sanitizers(tmp_path):
    """The growth arithmetic, the cut into row segments, the prefix over (column, segment) and the band bisection on made-up
    counts, in a stand-alone host program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "clusterer_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "clusterer_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"clusterer host check: ok" in r.stdout, r.stderr.decode()
