"""The bit-vector recurrence on the CPU -- no GPU.

tools/bitvector_host_check.cpp runs the kernels' own text (gatePairWords<W>, gatePairLong, TrimSearch: csrc/cluster_gate.hpp,
csrc/host/trim.hpp) against a full-matrix dynamic program under ASan and UBSan; the test builds and runs it.  The pools of
bitvector_cases.py, which test_gpu_bitvector_pools.py runs through the kernels against the host statements, are held here to
closed forms and to restatements that share nothing with the C++: lev_np for the distances, search_np for the primer search,
itself held to trim_cases.search_py on the shape pool.  Equalities throughout."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
ROOT = os.path.dirname(_HERE)

import bitvector_cases as B  # noqa: E402
import trim_cases as T  # noqa: E402
from test_cluster_gate_cpu import codes, lev_np  # noqa: E402

# what the program prints when every check held: the size of its run
HOST_CHECK_LINE = (b"bit-vector host check: ok (295249 gate cases: 293149 tails, 2100 ladder; 1236477 kernel-text runs, 16518 host pairs, "
                   b"1272 closed forms; 151920 trim searches, 9234 four-in-one loops)")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def test_kernel_text_under_sanitizers(tmp_path):
    """Exhaustive tails behind homopolymer, period-2 and random prefixes on each side of bit 31/32 and of two word boundaries, the
    length ladder with its closed forms, every primer length, the four-in-one column loop: heap blocks of exactly the sequences'
    lengths, the mask table at stride 3 and the long route's slice at stride 2 between canaries."""
    exe = str(tmp_path / "bitvector_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "bitvector_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=900)
    assert r.returncode == 0 and HOST_CHECK_LINE in r.stdout, (r.stdout.decode(), r.stderr.decode()[-4000:])


def test_gate_ladder_on_the_host(da):
    reads, pairs, closed, kinds = B.gate_ladder()
    got = da.editDistances(reads, pairs, host=True)
    assert got.shape == (len(pairs), 2) and got.dtype == np.int32
    assert B.check_closed(got, closed) >= 2 * 175 + 35                    # both distances of the homopolymers, the equal copies
    code = [codes(r) for r in reads]
    for q, (i, j) in enumerate(pairs):
        a, b = sorted((code[i], code[j]), key=len)                       # d is symmetric and d(x, rc y) = d(y, rc x): the short one as rows
        assert (int(got[q][0]), int(got[q][1])) == (lev_np(a, b), lev_np(a, 3 - b[::-1])), q
    # the pool holds what it says: every kind at every length, every word count up to 11 within the first waves
    assert sorted(set(kinds)) == list(range(6)) and {len(reads[min(p, key=lambda x: len(reads[x]))]) for p in pairs} == set(B.LADDER_LENGTHS)
    assert all({B.pattern_words(reads, p) for p in pairs[at:at + 64]} >= {1, 2, 4, 8, 9} for at in range(0, 1024, 64))
    assert {B.pattern_words(reads, p) for p in pairs} == set(range(1, 12))


def test_gate_limit_pool_on_the_host(da):
    from test_cluster_cpu import cluster_models
    reads = B.limit_pool()
    edits = B.limit_edits(reads, lambda a, b: lev_np(codes(a), codes(b)))
    got = da.editDistances(reads, sorted(edits), host=True)
    assert [tuple(int(x) for x in e) for e in got] == [edits[c] for c in sorted(edits)]
    want = B.limit_counts(reads, edits, B.LIMIT_PERMILLE)
    assert want["at"] >= 40 and want["above"] >= 40 and 0 < want["passed"] < want["tested"] == 69 * 68 // 2, want
    res = da.clusterReads(dict(cluster_models(da))["P6"], reads, band=16, min_shared=0, edges=True, max_edit_permille=B.LIMIT_PERMILLE,
                          host=True)
    assert {k: res.gate[k] for k in ("tested", "passed", "word_steps")} == {k: want[k] for k in ("tested", "passed", "word_steps")}
    assert res.gate["long_pairs"] == 0 and res.stats["items"] == 2 * want["passed"]


def test_search_np_is_search_py():
    """The numpy form over many texts against the pure-Python matrix, on the primers and reads of the trim shape pool."""
    primers, reads = T.shape_pool()
    texts = sorted({t for r in reads for v in (r, T.rc(r)) for t in (v, v[::-1])})
    n = 0
    for max_offset in (8, 0, -1):
        for p in sorted({p for F, R in primers for p in (F, R[::-1])}):
            got = B.search_np(p, texts, max_offset)
            assert got == [T.search_py(p, t, max_offset) for t in texts], (p, max_offset)
            n += len(texts)
    assert n == 3 * 12 * len(texts) and len(texts) > 150


@pytest.mark.parametrize("max_offset", (0, 8, -1))
def test_trim_ladder_on_the_host(da, max_offset):
    primers, reads = B.trim_ladder()
    assert sorted(len(F) for F, _ in primers) == sorted(len(R) for _, R in primers) == list(range(1, 65))
    assert len(reads) % 64 != 0 and {0, 1, 31, 32, 33, 63, 64, 65} <= {len(r) for r in reads}
    pairs_won = set()
    with B.searches_of(primers, reads, max_offset):
        for permille, anchors in itertools.product((0, 250, 1000), ("both", "either")):
            got = T.arrays(da.trimReads(primers, reads, max_offset=max_offset, max_edit_permille=permille, anchors=anchors, host=True))
            T.assert_same(got, T.trim_pool_py(primers, reads, max_offset=max_offset, permille=permille, anchors=anchors),
                          (max_offset, permille, anchors))
            pairs_won |= set(got["pair"].tolist())
    assert T.search_py.__name__ == "search_py"                            # the table is gone again
    assert len(pairs_won) > 16
