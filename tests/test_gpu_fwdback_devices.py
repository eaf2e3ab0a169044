"""The forward-backward E-step and the Baum-Welch fit on every GPU of a node (device_id = -1): the alignment pairs dealt
over one handle per device, one host thread per device, the counts and log-likelihoods added on the host in device order.
On a one-GPU box several handles share the card (DNAS_FAKE_DEVICES, read when the handle is made).

The contract (include/dnastore_amd.h, dnas_fb_create): per-pair log-likelihoods bit-identical to one device; counts and the
summed log-likelihood equal to one device up to the order of summation (1e-12 relative); bit-identical from call to call for
a fixed number of devices; with one device, bit-identical to device_id = 0."""
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dnastore_amd", "bin", "dnastore")
ROUTING = ("pairs_onchip", "pairs_streaming", "pairs_narrow", "out_nt")
TESTCOUNT = ["-l6", "--error-sub-prob", "1e-9", "--error-dup-prob", "1e-9", "--error-del-open", "1e-9"]   # reference Makefile:156-159


@pytest.fixture(scope="module")
def da():
    import dnastore_amd
    return dnastore_amd


def _database(O, seed, n_short):
    """Short pairs of mixed lengths for the on-chip kernels and two with long runs of duplications (envelope rows wider than 32
    cells with P = 6: the streaming kernel)."""
    from synth import synthetic_alignment
    rng = random.Random(seed)
    pairs = [O.alignment_pair(synthetic_alignment(rng, rng.choice([1, 7, 33, 100, 256]), sub=.03, dele=.02, dup=.02))
             for _ in range(n_short)]
    pairs.append(O.alignment_pair(synthetic_alignment(random.Random(5), 60, sub=.02, dele=.0, dup=.35)))
    pairs.append(O.alignment_pair(synthetic_alignment(random.Random(6), 90, sub=.02, dele=.0, dup=.8)))
    return pairs


def _empty():
    return dict(ins=np.zeros(0, np.int8), in_off=np.zeros(1, np.int64), outs=np.zeros(0, np.int8), out_off=np.zeros(1, np.int64),
                cm_in=np.zeros(0, np.int32), cm_in_off=np.zeros(1, np.int64), cm_out=np.zeros(0, np.int32),
                cm_out_off=np.zeros(1, np.int64), n=0)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _within_contract(got, want):
    """(counts, ll, per) of a W-device handle against a one-device handle."""
    (c, ll, per), (c1, ll1, per1) = got, want
    assert _same_bits(per, per1)
    assert np.allclose(c, c1, rtol=1e-12, atol=1e-300, equal_nan=True)
    assert ll == ll1 or abs(ll - ll1) <= 1e-12 * abs(ll1), (ll, ll1)


def _all_devices_against_one(da, O, devices):
    pairs = _database(O, 61, 148)
    pk = O.pack_pairs(pairs)
    one = da.ForwardBackward(pk, device=0)
    many = da.ForwardBackward(pk, device=-1)
    assert one.devices == 1 and many.devices == devices
    stats = []
    for length, strict in ((16, False), (6, False), (8, True)):          # P = 8, P = 3, P = 4 with strict guides
        params = da.MutatorParams.fromFlags(length=length)
        want = one.expectedCounts(params, strict=strict)
        got = many.expectedCounts(params, strict=strict)
        st1, st = one.stats(), many.stats()
        _within_contract(got, want)
        oc, oll, oper = O.expected_counts(O.MutatorParams.from_cli(length=length), pairs, strict=strict)
        assert _same_bits(got[2], oper) and np.allclose(got[0], oc, rtol=1e-9, atol=1e-300, equal_nan=True)
        assert [st[k] for k in ROUTING] == [st1[k] for k in ROUTING], (st, st1)
        assert st["pairs_onchip"] + st["pairs_streaming"] == len(pairs)
        stats.append(st)
        again = many.expectedCounts(params, strict=strict)             # the same handle again: the same bits
        assert all(_same_bits(a, b) for a, b in zip(again, got))
    assert stats[0]["pairs_streaming"] >= 1 and stats[0]["pairs_onchip"] >= len(pairs) // 2     # P = 8: both kinds of kernel
    one.close()
    many.close()


def test_three_fake_devices_match_one_device(da, oracle_mod, monkeypatch):
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    _all_devices_against_one(da, oracle_mod, 3)


def test_width_is_read_when_the_handle_is_made(da, oracle_mod, monkeypatch):
    O = oracle_mod
    pairs = _database(O, 62, 30)
    pk = O.pack_pairs(pairs)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    three = da.ForwardBackward(pk, device=-1)
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "2")
    two = da.ForwardBackward(pk, device=-1)
    assert three.devices == 3 and two.devices == 2
    one = da.ForwardBackward(pk, device=0)
    params = da.MutatorParams.fromFlags()
    want = one.expectedCounts(params)
    _within_contract(three.expectedCounts(params), want)
    _within_contract(two.expectedCounts(params), want)
    for fb in (one, two, three):
        fb.close()


def test_one_fake_device_is_device_zero_bit_for_bit(da, oracle_mod, monkeypatch):
    O = oracle_mod
    pk = O.pack_pairs(_database(O, 63, 148))
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "1")
    one = da.ForwardBackward(pk, device=0)
    solo = da.ForwardBackward(pk, device=-1)
    assert solo.devices == 1
    for length, strict in ((12, False), (8, True)):
        params = da.MutatorParams.fromFlags(length=length)
        want, got = one.expectedCounts(params, strict=strict), solo.expectedCounts(params, strict=strict)
        assert all(_same_bits(a, b) for a, b in zip(got, want))
        assert solo.stats()["lse_ops"] == one.stats()["lse_ops"]
    one.close()
    solo.close()
    got = da.expectedCounts(da.MutatorParams.fromFlags(), pk, device=-1)                # the one-call form
    want = da.expectedCounts(da.MutatorParams.fromFlags(), pk, device=0)
    assert all(_same_bits(a, b) for a, b in zip(got, want))


def test_fewer_pairs_than_devices(da, oracle_mod, monkeypatch):
    O = oracle_mod
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    pairs = _database(O, 64, 0)                                          # the two streaming pairs alone
    pk = O.pack_pairs(pairs)
    params = da.MutatorParams.fromFlags()
    fb = da.ForwardBackward(pk, device=-1)
    assert fb.devices == 3
    one = da.ForwardBackward(pk, device=0)
    _within_contract(fb.expectedCounts(params), one.expectedCounts(params))
    assert [fb.stats()[k] for k in ROUTING] == [one.stats()[k] for k in ROUTING]
    one.close()
    fb.load(_empty())
    counts, ll, per = fb.expectedCounts(params)
    assert not counts.any() and ll == 0 and len(per) == 0 and fb.stats()["pairs_onchip"] == fb.stats()["pairs_streaming"] == 0
    fb.close()
    counts, ll, per = da.expectedCounts(params, _empty(), device=-1)
    assert not counts.any() and ll == 0 and len(per) == 0


def test_one_handle_across_changing_databases(da, oracle_mod, monkeypatch):
    """Each sub-handle keeps its shard's routing and count buffers between calls: a new database must replace them all."""
    O = oracle_mod
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    a, b = _database(O, 41, 40), _database(O, 43, 124)
    assert len(b) == 3 * len(a)
    pk_a, pk_b = O.pack_pairs(a), O.pack_pairs(b)
    fb = da.ForwardBackward(pk_a, device=-1)
    results = []

    def step(pk, n, length, strict=False):
        params = da.MutatorParams.fromFlags(length=length)
        got = fb.expectedCounts(params, strict=strict)
        fresh = da.ForwardBackward(pk, device=0)
        want = fresh.expectedCounts(params, strict=strict)
        assert len(got[2]) == n and [fb.stats()[k] for k in ROUTING] == [fresh.stats()[k] for k in ROUTING]
        fresh.close()
        _within_contract(got, want)
        results.append(got)

    step(pk_a, len(a), 16)
    fb.load(pk_b)                                                        # the same model, three times the pairs
    step(pk_b, len(b), 16)
    step(pk_b, len(b), 8, strict=True)
    fb.load(pk_a)                                                        # the first database and model again
    step(pk_a, len(a), 16)
    assert all(_same_bits(x, y) for x, y in zip(results[-1], results[0]))
    fb.close()


def test_errors_match_one_device(da, oracle_mod, monkeypatch):
    O = oracle_mod
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    pairs = _database(O, 65, 60)
    pk = O.pack_pairs(pairs)
    params = da.MutatorParams.fromFlags()
    bad_off = dict(pk); bad_off["cm_out_off"] = pk["cm_out_off"].copy(); bad_off["cm_out_off"][38] += 1     # pair 37: one guide column too many
    bad_base = dict(pk); bad_base["outs"] = pk["outs"].copy(); bad_base["outs"][int(pk["out_off"][45]) + 3] = 7
    for bad, what in ((bad_off, "pair 37: inconsistent offsets"), (bad_base, "bad base")):
        codes = []
        for device in (0, -1):
            fb = da.ForwardBackward(pk, device=device)
            with pytest.raises(da.DnasError, match=what) as e:
                fb.load(bad)
            codes.append(e.value.code)
            counts, ll, _ = fb.expectedCounts(params)                    # the handle is left without a database
            assert not counts.any() and ll == 0
            fb.load(pk)                                                  # ... and takes a good one afterwards
            assert _same_bits(fb.expectedCounts(params)[2], O.expected_counts(O.MutatorParams.from_cli(), pairs)[2])
            fb.close()
            with pytest.raises(da.DnasError, match=what):
                da.expectedCounts(params, bad, device=device)
        assert codes[0] == codes[1], (what, codes)
    assert codes[0] == -6                                                # DNAS_E_BAD_BASE
    for device in (-2, da.lib.lib().dnas_device_count()):
        with pytest.raises(da.DnasError, match="DNAS_E_INVALID"):
            da.ForwardBackward(None, device=device)


def _fit_params(fit):
    return np.array([fit.c.p_del_open, fit.c.p_del_extend, fit.c.p_tan_dup, fit.c.p_transition, fit.c.p_transversion] + fit.pLen)


def test_baum_welch_on_all_devices(da, oracle_mod, ref_data, monkeypatch):
    from synth import synthetic_alignment
    O = oracle_mod
    monkeypatch.setenv("DNAS_FAKE_DEVICES", "3")
    rng = random.Random(3)
    synthetic = O.pack_pairs([O.alignment_pair(synthetic_alignment(rng, 120, sub=.03, dele=.02, dup=.02)) for _ in range(40)])
    for pairs, strict in ((da.StockholmDB(os.path.join(ref_data, "test.stk")), True), (synthetic, False)):
        fit1, it1 = da.baumWelchParams(da.MutatorParams.fromFlags(), pairs, strict=strict, device=0)
        fitw, itw = da.baumWelchParams(da.MutatorParams.fromFlags(), pairs, strict=strict, device=-1)
        assert itw == it1 and fitw.local == fit1.local
        assert np.allclose(_fit_params(fitw), _fit_params(fit1), rtol=1e-10, atol=0)


def _cli(args):
    """The CLI with --device -1 over three handles (DNAS_FAKE_DEVICES=3)."""
    r = subprocess.run([BIN] + args + ["--device", "-1"], capture_output=True, timeout=600, env=dict(os.environ, DNAS_FAKE_DEVICES="3"))
    return r.stdout, r.stderr.decode(errors="replace"), r.returncode


@pytest.mark.parametrize("stk,golden", [("dup.stk", "dup.counts.json"), ("dup.sub.stk", "dup.sub.counts.json"),
                                        ("dup.sub.misaligned.stk", "dup.sub.counts.misaligned.json")])
def test_cli_error_counts_goldens_on_all_devices(ref_data, stk, golden):
    out, err, rc = _cli(["-v0"] + TESTCOUNT + ["--error-counts", os.path.join(ref_data, stk)])
    assert rc == 0 and out == open(os.path.join(ref_data, golden), "rb").read(), err


@pytest.mark.parametrize("stk,golden", [("tiny.stk", "tiny.params.json"), ("test.stk", "test.params.json")])
def test_cli_fit_error_goldens_on_all_devices(ref_data, stk, golden):
    out, err, rc = _cli(["-v0", "--fit-error", os.path.join(ref_data, stk), "--strict-guides"])
    assert rc == 0 and out == open(os.path.join(ref_data, golden), "rb").read(), err


def test_cli_verbose_3_names_the_estep_devices(ref_data):
    out, err, rc = _cli(["-v3"] + TESTCOUNT + ["--error-counts", os.path.join(ref_data, "dup.stk")])
    assert rc == 0 and "E-step devices: 3" in err
    assert out == open(os.path.join(ref_data, "dup.counts.json"), "rb").read()


def test_real_devices_match_one_device(da, oracle_mod, monkeypatch):
    """The first whole-node run: every visible GPU, no fake devices."""
    have = da.lib.lib().dnas_device_count()
    if have < 2:
        pytest.skip("one GPU visible: the real multi-device split needs two or more")
    monkeypatch.delenv("DNAS_FAKE_DEVICES", raising=False)
    _all_devices_against_one(da, oracle_mod, have)
