"""The forward pair-HMM score's exact reference and case lists -- TEST INFRASTRUCTURE for test_pair_forward_cpu.py and
test_gpu_pair_forward.py.

`exact_forward` sums the weight of every path of the mutator pair HMM from S(0,0) to S(I,O) that stays inside the band of
PairBand (csrc/host/pairalign.hpp), by one pass over the move graph exact_models._moves in 160-bit mpmath: no table, no
log-sum-exp, nothing imported from the library.  `tiny_exact` takes the same sum from exact_models.enumerate_pair, which walks
every path.

The bounds.  Exact mode against these references: 1e-12 relative (at most a few hundred fp64 roundings of under 1.2e-16 each).
Table mode against exact: the table drops at most e^-10 per lse call and never more, its linear interpolation of a convex
function overshoots by under 1e-9; a path visits at most 3 (I + O + 1) nodes, each formed by at most 2 lse calls, so
    exact - 6 (I + O + 1) (e^-10 + 1e-9)  <=  table  <=  exact + 6 (I + O + 1) 1e-9."""
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import exact_models as X  # noqa: E402

NEG = float("-inf")
BASES = "ACGT"
MEDIUM_BANDS = (-1, 8, 0)


def band_predicate(I, O, band):
    """PairBand: cell (ip, op) is inside iff lo <= op - ip <= hi; band < 0: every cell."""
    b = I + O + 1 if band < 0 or band > I + O + 1 else band
    lo, hi = min(0, O - I) - b, max(0, O - I) + b
    return lambda ip, op: lo <= op - ip <= hi


def exact_forward(plain, a, b, band=-1):
    """log of the summed weight of every path inside the band -> float (-inf: none).  plain: an object with the fields of
    oracle.MutatorParams; a, b: base codes."""
    m = X.PairModel(plain)
    a, b = [int(x) for x in a], [int(x) for x in b]
    inside = band_predicate(len(a), len(b), band)
    order = [(ip, op, ln) for ip in range(len(a) + 1) for op in range(len(b) + 1) if inside(ip, op)
             for ln in ["D", "S"] + list(range(min(ip, m.P)))]
    fwd = {n: X.mpf(0) for n in order}
    fwd[(0, 0, "S")] = X.mpf(1)
    for n in order:                                # moves go D -> S -> T_k inside a cell, to a later op of the row, or to a later row
        if fwd[n] != 0:
            for nxt, wt, _ in X._moves(m, n, a, b):
                if nxt in fwd:
                    fwd[nxt] += fwd[n] * wt
    z = fwd[(len(a), len(b), "S")]
    return NEG if z == 0 else float(X.mp.log(z))


def table_bounds(exact, I, O):
    """(lowest, highest) value the table mode may return for a pair whose exact score is `exact`."""
    n = 6 * (I + O + 1)
    return exact - n * (math.exp(-10.) + 1e-9), exact + n * 1e-9


def lib_params(da, plain):
    """oracle.MutatorParams (or a namespace like it) -> the library's MutatorParams, field for field; .plain keeps the source."""
    c = da.lib.MutatorParamsC()
    c.p_del_open, c.p_del_extend, c.p_tan_dup = plain.pDelOpen, plain.pDelExtend, plain.pTanDup
    c.p_transition, c.p_transversion = plain.pTransition, plain.pTransversion
    c.n_len, c.local = len(plain.pLen), int(getattr(plain, "local", True))
    for k, x in enumerate(plain.pLen):
        c.p_len[k] = x
    p = da.MutatorParams(c)
    p.plain = plain
    return p


def _pairs_of(rows):
    out = []
    for r in rows:
        ins, outs, _, _ = X.guide_columns(*r)
        out.append(([int(x) for x in ins], [int(x) for x in outs]))
    return out


def tiny_cases():
    """The 8 loose tiny_models(), 20 pairs each: [(name, plain params, [(a, b)])], a and b lists of base codes."""
    return [(name, params, _pairs_of(rows)) for name, params, strict, rows in X.tiny_models() if not strict]


def medium_cases():
    """Every medium_models() pair: [(name, plain params, [(a, b)])]."""
    return [(name, params, _pairs_of(rows)) for name, params, strict, rows in X.medium_models()]


def boundary_cases():
    """BOUNDARY_ESTEP_BASES x the 14 BOUNDARY_VARIANTS, the base's 20 pairs: [("<base>/<variant>", plain params, [(a, b)])]."""
    return [(name, params, _pairs_of(rows)) for name, params, strict, rows in X.boundary_estep_models()]


_CACHE = {}


def tiny_exact():
    """[(name, plain, pairs, float64[20] of the sum over every enumerated path, [paths walked])], computed once per process."""
    if "tiny" not in _CACHE:
        out = []
        for name, plain, pairs in tiny_cases():
            lls, walked = [], []
            for a, b in pairs:
                ll, _, n = X.enumerate_pair(plain, a, b, None, None, open_envelope=True)
                lls.append(ll)
                walked.append(n)
            out.append((name, plain, pairs, np.array(lls), walked))
        _CACHE["tiny"] = out
    return _CACHE["tiny"]


def medium_exact():
    """[(name, plain, pairs, {band: float64[n] from exact_forward})] over MEDIUM_BANDS, computed once per process."""
    if "medium" not in _CACHE:
        _CACHE["medium"] = [(name, plain, pairs, {band: np.array([exact_forward(plain, a, b, band) for a, b in pairs])
                                                  for band in MEDIUM_BANDS}) for name, plain, pairs in medium_cases()]
    return _CACHE["medium"]


def boundary_exact():
    """[(name, plain, pairs, float64[20] from exact_forward at band -1)], computed once per process."""
    if "boundary" not in _CACHE:
        _CACHE["boundary"] = [(name, plain, pairs, np.array([exact_forward(plain, a, b) for a, b in pairs]))
                              for name, plain, pairs in boundary_cases()]
    return _CACHE["boundary"]


def seqs(pairs):
    """[(a, b)] -> (originals, reads) as int8 arrays, what pairLikelihoods and alignPairs take."""
    return [np.array(a, dtype=np.int8) for a, _ in pairs], [np.array(b, dtype=np.int8) for _, b in pairs]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
