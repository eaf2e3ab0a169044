"""The row programs no fixture and no fuzz machine compiles (tests/tiera_census.py SHAPED_CASES; tests/test_tiera_census_cpu.py
says which they are and checks the planner's side of them), run through the real HIP path: the model's program is the one the
CPU census predicts, and decoded strings, status, fp64 log-likelihoods and every lattice cell are the oracle's, bit for bit --
local and global, on a ragged batch; three of the cases also in lattice segments (a second compile of every shape), two also
with both strands.  Every comparison is an equality."""
import math

import numpy as np
import pytest

import tiera_census as tc

pytestmark = pytest.mark.gpu

FLAGS = dict(sub=.02, dup=.01, del_open=.02, del_ext=.1)
NO_PATH = 1      # DNAS_READ_NO_PATH
OUT_CAP = 4096   # symbols per read: null edges with an input symbol make a one-base read decode to more than a thousand
CASES = {c.id: c for c in tc.SHAPED_CASES}
_reference = {}  # (case id, global_, read) -> (string, log-likelihood): one oracle decode per read, shared by the tests below


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _setup(monkeypatch, O, case, global_, extra=""):
    """(decoder, oracle, reads) of a shaped case; the decoder is created under the case's thread count and environment, and the
    program it compiled is held to what the CPU census reads off the plan tables."""
    import dnastore_amd as da
    for k in ("DNAS_THREADS", "DNAS_PLAN_PICK", "DNAS_PLAN_ORDER", "DNAS_PLAN_SLACK", "DNAS_PLAN_REMOTE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DNAS_THREADS", str(case.threads))
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    text = tc.shaped_text(case)
    flags = dict(FLAGS, global_=global_)
    dec = da.ViterbiDecoder(da.Machine.fromJSON(text), da.MutatorParams.fromFlags(**flags), options=tc.model_options(case) + extra)
    assert dec.tier.startswith("tier A" if case.members == 1 else "tier C"), dec.tier
    prog = tc.program_of_model(dec)
    assert prog == tc.row_program(dec.flat, case.members), dec.tier
    f = tc.features(prog)
    assert (prog.T, prog.G) == (case.threads, case.members) and all(f[k] == v for k, v in case.features.items()), dec.tier
    assert all(tc.has_shape(prog, s) for s in case.shapes), dec.tier
    orc = O.ViterbiOracle(O.Machine.from_json(text), O.MutatorParams.from_cli(**flags))
    reads = tc.shaped_reads(text)
    assert sorted(len(r) for r in reads)[:2] == [0, 1]
    return dec, orc, reads


def _want(orc, case, global_, read):
    key = (case.id, global_, read)
    if key not in _reference:
        _reference[key] = orc.decode(read)
    return _reference[key]


@pytest.mark.parametrize("global_", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("case", tc.SHAPED_CASES, ids=[c.id for c in tc.SHAPED_CASES])
def test_row_shape_matches_oracle(oracle_mod, monkeypatch, case, global_):
    dec, orc, reads = _setup(monkeypatch, oracle_mod, case, global_)
    out, ll, st = dec.decode(reads, out_cap=OUT_CAP)
    for i, r in enumerate(reads):
        s, oll, olat = orc.decode(r, want_lattice=True)
        _reference[(case.id, global_, r)] = (s, oll)
        assert out[i] == s and bits(ll[i]) == bits(oll), (i, r, out[i], s, ll[i], oll)
        assert st[i] == (NO_PATH if oll == -np.inf else 0), (i, st[i], oll)
        lat = np.ascontiguousarray(dec.lattice(i, len(r)).transpose(0, 2, 1))
        assert lat.shape == olat.shape and not np.isnan(lat).any()
        assert np.array_equal(lat.view(np.uint64), olat.view(np.uint64)), (i, r)
    dec.close()


@pytest.mark.parametrize("global_", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("case_id", tc.SEGMENT_CASES)
def test_row_shape_in_segments_matches_oracle(oracle_mod, monkeypatch, case_id, global_):
    """The bounded-memory decode at the shortest segment the error model allows (D + 2 columns): the DNAS_SEGMENTS=1 compile of a
    program without S rows, of one with a full row of kind 1 and a common non-zero class, and of a cluster's."""
    case = CASES[case_id]
    dec, orc, reads = _setup(monkeypatch, oracle_mod, case, global_, extra=",checkpoint=always,segment=6")
    assert dec.max_dup_len == 4
    out, ll, st = dec.decode(reads, out_cap=OUT_CAP)
    assert dec.stats()["checkpointed_reads"] == len(reads)
    for i, r in enumerate(reads):
        s, oll = _want(orc, case, global_, r)
        assert out[i] == s and bits(ll[i]) == bits(oll), (i, r, out[i], s, ll[i], oll)
        assert st[i] == (NO_PATH if oll == -np.inf else 0), (i, st[i], oll)
    dec.close()


def _revcomp(seq):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seq))


@pytest.mark.parametrize("case_id", tc.STRAND_CASES)
def test_row_shape_both_strands_matches_oracle(oracle_mod, monkeypatch, case_id):
    """strands="both" against two oracle decodes per read: the orientation with the strictly larger log-likelihood wins, ties
    go to the read as written."""
    case = CASES[case_id]
    dec, orc, reads = _setup(monkeypatch, oracle_mod, case, False)
    reads = [r if i % 2 else _revcomp(r) for i, r in enumerate(reads)]
    out, ll, st, strand = dec.decode(reads, out_cap=OUT_CAP, strands="both")
    for i, r in enumerate(reads):
        f, b = _want(orc, case, False, r), _want(orc, case, False, _revcomp(r))
        rev = b[1] > f[1]
        s, oll = b if rev else f
        assert out[i] == s and bits(ll[i]) == bits(oll) and strand[i] == int(rev), (i, r, out[i], s, ll[i], oll, strand[i])
        assert st[i] == (NO_PATH if s == "" and math.isinf(oll) else 0), (i, st[i], oll)
    dec.close()
