"""dnas_trim_reads on the GPU (csrc/trim_kernels.hip) against dnas_trim_reads_host: every output array equal, over the shape pool and
the whole parameter grid, whatever the pair chunks and the device count; the planted pool; decode_pool on raw reads."""
import itertools
import os
import random
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import trim_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(_HERE, "golden", "ref_data")


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


@pytest.fixture(scope="module")
def shapes():
    return T.shape_pool()


@pytest.fixture(scope="module")
def planted():
    return T.planted_pool()


def same(da, primers, reads, what="", device=0, **options):
    """The GPU's answer, after it was held to the host's."""
    got = da.trimReads(primers, reads, device=device, **options)
    T.assert_same(T.arrays(got), T.arrays(da.trimReads(primers, reads, host=True, **options)), (what, options))
    assert got.stats["trimmed"] == int((got.status == 0).sum())
    return got


def columns(primers, reads, max_offset):
    window = lambda m, n: n if max_offset < 0 else min(n, m + max_offset)
    return sum(2 * (window(len(F), len(r)) + window(len(R), len(r))) for r in reads for F, R in primers)


@pytest.mark.parametrize("max_offset,permille", list(itertools.product((0, 8, -1), (0, 250, 1000))))
def test_shape_pool_over_the_grid(da, shapes, max_offset, permille):
    primers, reads = shapes
    assert len(reads) % 64 != 0
    many = reads * 5                                                    # a wave's lanes hold every mix of lengths
    assert len(many) > 64 * 5 and len(many) % 64 != 0
    for anchors, min_payload in itertools.product(("both", "either"), (0, 10)):
        options = dict(max_offset=max_offset, max_edit_permille=permille, anchors=anchors, min_payload=min_payload)
        got = same(da, primers, reads, "pool", **options)
        assert got.stats["columns"] == columns(primers, reads, max_offset) and got.stats["devices"] == 1
        assert got.stats["items"] == 2 * got.stats["chunks"]
        same(da, primers, many, "pool x 5", **options)
        for one in (reads[7], reads[-1], ""):
            same(da, primers, [one], "one read", **options)
        none = same(da, primers, [], "no read", **options)
        assert len(none) == 0 and none.stats["items"] == 0
        bare = same(da, [], reads, "no pair", **options)
        assert set(bare.status.tolist()) == {da.lib.TRIM_NO_ANCHOR} and set(bare.pair.tolist()) == {-1}


@pytest.mark.parametrize("chunk", (1, 3))
def test_pair_chunks(da, shapes, planted, monkeypatch, chunk):
    """Seven pairs, and 130 (the planted primers repeated: every pair ties with its copies, across chunks), cut into chunks of 1
    and of 3 pairs: the fold keeps the winner of the (total, k, s) order and the best total of another pair."""
    primers, reads = shapes
    wide = (planted[0] * 17)[:130]
    cases = [(primers, reads * 2, dict(max_offset=8)), (primers, reads, dict(max_offset=-1, anchors="either", min_payload=10)),
             (wide, planted[1], dict(max_offset=8)), (wide, planted[1][:70], dict(max_offset=-1, max_edit_permille=400, anchors="either"))]
    for pr, rd, options in cases:
        whole = same(da, pr, rd, "default chunks", **options)
        monkeypatch.setenv("DNAS_TRIM_PAIR_CHUNK", str(chunk))
        cut = same(da, pr, rd, "chunks of %d" % chunk, **options)
        monkeypatch.delenv("DNAS_TRIM_PAIR_CHUNK")
        T.assert_same(T.arrays(cut), T.arrays(whole))
        assert cut.stats["chunks"] == -(-len(pr) // chunk) and cut.stats["columns"] == whole.stats["columns"]
        assert cut.stats["items"] == cut.stats["chunks"] * -(-len(rd) // 64)
    assert (whole.second[whole.pair >= 0] == whole.total[whole.pair >= 0]).all()      # the copies tie


def test_all_devices(da, shapes, planted, monkeypatch):
    primers, reads = shapes
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    for options in (dict(max_offset=8), dict(max_offset=-1, anchors="either"), dict(max_offset=0, max_edit_permille=1000, min_payload=10)):
        every = same(da, primers, reads * 5, "three workers", device=-1, **options)
        assert every.stats["devices"] == 3 and every.stats["columns"] == columns(primers, reads * 5, options["max_offset"])
        few = same(da, primers, reads[:2], "two reads, three workers", device=-1, **options)
        assert few.stats["devices"] == 3
    same(da, planted[0], planted[1], "planted, three workers", device=-1)


def test_planted_pool(da, planted):
    primers, reads, truth = planted
    got = same(da, primers, reads, "planted", max_offset=8, max_edit_permille=250, anchors="both", min_payload=0)
    T.planted_conditions(reads, truth, T.arrays(got))


def test_invalid_arguments_on_the_device_path(da):
    for kw in (dict(max_edit_permille=1001), dict(max_offset=-2), dict(min_payload=-1), dict(device=-2), dict(device=1 << 20)):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.trimReads([("ACG", "TTG")], ["ACGTACGT"], **kw)
    with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
        da.trimReads([("A" * 65, "TTG")], ["ACGTACGT"])


def test_decode_pool_with_primers(da):
    """Six messages encoded with a shipped machine and wrapped in one primer pair (a second pair is in the call and frames nothing),
    three noisy reads each, every other one reverse-complemented: decode_pool(reads, primers=...) is decode_pool on the
    host-trimmed payloads, its .read counting in the raw reads."""
    rng = random.Random("trim/decode")
    machine = da.Machine.fromFile(os.path.join(DATA, "l4c4.json"))
    primers, _, _ = T.planted_pool()
    F, R = primers[1]
    reads = []
    for m in range(6):
        strand = machine.encodeBytes(bytes(rng.randrange(256) for _ in range(8)))
        for copy in range(3):
            read = T._rand(rng, rng.randint(0, 5)) + T.edited(rng, F, 1) + T.edited(rng, strand, 2) + T.edited(rng, R, 1) + T._rand(rng, rng.randint(0, 5))
            reads.append(T.rc(read) if len(reads) % 2 else read)
    reads.insert(5, T._rand(rng, 90))                                   # a read of no file
    params = da.MutatorParams.fromFlags(sub=.03, dup=.02, del_open=.02, del_ext=.2)
    dec = da.ViterbiDecoder(machine, params, device=0)
    host = da.trimReads(primers[:2], reads, host=True)
    kept = host.kept()
    assert len(kept) == 18 and 5 not in kept and set(host.pair[kept].tolist()) == {1}
    payloads = host.payloads()
    want = dec.decode_pool([payloads[i] for i in kept], band=16)
    got = dec.decode_pool(reads, band=16, primers=primers[:2])
    same_options = dec.decode_pool(reads, band=16, primers=primers[:2], trim_max_offset=8, trim_anchors="both", trim_pair=1, trim_min_margin=0)
    dec.close()
    for out in (got, same_options):
        assert out.kept.tolist() == kept and out.symbols == want.symbols and out.labels == want.labels
        assert out.read.tolist() == [kept[r] if r >= 0 else -1 for r in want.read]
        assert np.array_equal(out.total.view(np.uint64), want.total.view(np.uint64)) and np.array_equal(out.status, want.status)
        assert np.array_equal(out.clusters.cluster, want.clusters.cluster) and out.per_read[0] == want.per_read[0]
        T.assert_same(T.arrays(out.trimmed), T.arrays(host))
    assert want.clusters.n_clusters == 6 and sorted(want.clusters.sizes.tolist()) == [3] * 6
