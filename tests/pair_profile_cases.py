"""Exact row profiles of the mutator pair HMM over a band and the case lists -- TEST INFRASTRUCTURE for
test_pair_profiles_cpu.py and test_gpu_pair_profiles.py.

`exact_profile` is the 160-bit mpmath forward and backward pass of pair_counts_cases.exact_counts with each move's posterior filed
by the `ip` of the node it leaves and by the kind of move instead of by count slot: nothing is imported from the library.  Its
rows summed are exact_counts' nNoGap, nDelOpen, nDelExtend and nLen[k], which `hold_to_exact_counts` asserts.

The bounds are those of pair_counts_cases.py: a profile value is a sum of some of the non-negative terms a count sums, so the
factor by which one term can be off bounds it too (exact_rel_bound in exact mode, exp(+-table_log_bound) in table mode)."""
import os
import random
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import exact_models as X  # noqa: E402
import pair_counts_cases as K  # noqa: E402
import pair_forward_cases as C  # noqa: E402

NEG = float("-inf")
MATCH, DEL_OPEN, DEL_EXTEND, DUP = 0, 4, 5, 6                     # planes of a pair's block
SAME, TRANSITION, TRANSVERSION, SUM_DEL_OPEN, SUM_DEL_EXTEND, SUM_DUP = 0, 1, 2, 3, 4, 5      # planes of the aggregate
TINY = np.finfo(np.float64).tiny                                   # the smallest normal double: the GPU tests' atol


def _plane(idx):
    """The profile plane of a move with count indices idx, or None for a move that is not profiled."""
    if X.C_NOGAP in idx:
        return MATCH + (idx[1] - X.C_SUB) % 4
    if X.C_DELOPEN in idx:
        return DEL_OPEN
    if X.C_DELEXT in idx:
        return DEL_EXTEND
    if X.C_TANDUP in idx:
        return DUP + idx[1] - X.C_LEN
    return None


def exact_profile(plain, a, b, band=-1):
    """-> (log-likelihood, float64[6 + P, I + 1]); (-inf, None) when the band holds no path of positive probability."""
    m = X.PairModel(plain)
    a, b = [int(x) for x in a], [int(x) for x in b]
    inside = C.band_predicate(len(a), len(b), band)
    order = [(ip, op, ln) for ip in range(len(a) + 1) for op in range(len(b) + 1) if inside(ip, op)
             for ln in ["D", "S"] + list(range(min(ip, m.P)))]
    fwd = {n: X.mpf(0) for n in order}
    bwd = dict(fwd)
    start, end = (0, 0, "S"), (len(a), len(b), "S")
    edges = {}
    fwd[start] = X.mpf(1)
    for n in order:
        edges[n] = [(nxt, wt, idx) for nxt, wt, idx in X._moves(m, n, a, b) if nxt in fwd and wt != 0]
        if fwd[n] != 0:
            for nxt, wt, _ in edges[n]:
                fwd[nxt] += fwd[n] * wt
    z = fwd[end]
    if z == 0:
        return NEG, None
    bwd[end] = X.mpf(1)
    for n in reversed(order):
        for nxt, wt, _ in edges[n]:
            bwd[n] += wt * bwd[nxt]
    sums = [[X.mpf(0)] * (len(a) + 1) for _ in range(DUP + m.P)]
    for n in order:
        if fwd[n] != 0:
            for nxt, wt, idx in edges[n]:
                j = _plane(idx)
                if j is not None:
                    sums[j][n[0]] += fwd[n] * wt * bwd[nxt]
    return float(X.mp.log(z)), np.array([[float(s / z) for s in row] for row in sums])


def hold_to_exact_counts(profile, counts, P):
    """The rows of an exact profile summed are the exact counts, both rounded from 160 bits once per value."""
    rows = profile.sum(axis=1)
    want = np.concatenate(([counts[X.C_DELOPEN], counts[X.C_DELEXT]], counts[X.C_LEN:X.C_LEN + P]))
    assert np.allclose(rows[DEL_OPEN:], want, rtol=1e-13, atol=1e-300), (rows, want)
    assert abs(rows[:DEL_OPEN].sum() - counts[X.C_NOGAP]) <= 1e-13 * counts[X.C_NOGAP] + 1e-300


_CACHE = {}


def tiny_exact():
    """[(name, plain, pairs, [(ll, profile or None)])] over the whole matrix, computed once per process."""
    if "tiny" not in _CACHE:
        _CACHE["tiny"] = [(name, plain, pairs, [exact_profile(plain, a, b) for a, b in pairs]) for name, plain, pairs in C.tiny_cases()]
    return _CACHE["tiny"]


def medium_exact(bands=C.MEDIUM_BANDS):
    """[(name, plain, pairs, {band: [(ll, profile or None)]})], each band computed once per process."""
    out = []
    for name, plain, pairs in C.medium_cases():
        for band in bands:
            if ("medium", name, band) not in _CACHE:
                _CACHE[("medium", name, band)] = [exact_profile(plain, a, b, band) for a, b in pairs]
        out.append((name, plain, pairs, {band: _CACHE[("medium", name, band)] for band in bands}))
    return out


def boundary_exact():
    """[(name, plain, pairs, [(ll, profile or None)])] at band -1, computed once per process."""
    if "boundary" not in _CACHE:
        _CACHE["boundary"] = [(name, plain, pairs, [exact_profile(plain, a, b) for a, b in pairs]) for name, plain, pairs in C.boundary_cases()]
    return _CACHE["boundary"]


def zero_planes(plain):
    """The planes of moves whose probability is exactly 0 under plain."""
    m = X.PairModel(plain)
    zero = []
    if m.no_gap == 0:
        zero += [MATCH + y for y in range(4)]
    if m.del_open == 0:
        zero.append(DEL_OPEN)
    if m.del_ext == 0:
        zero.append(DEL_EXTEND)
    zero += [DUP + k for k in range(m.P) if m.tan_dup == 0 or m.p_len[k] == 0]
    return sorted(set(zero))


def fold(blocks, originals, status, anchor, n_pos):
    """The aggregate of dnas_pair_profiles restated in numpy from the per-pair blocks: (float64[5 + P, n_pos], int64[n_pos])."""
    P = blocks[0].shape[0] - DUP if blocks else 0
    profile, coverage = np.zeros((SUM_DUP + P, n_pos)), np.zeros(n_pos, dtype=np.int64)
    for blk, a, st in zip(blocks, originals, status):
        if st != K.COUNTS_OK:
            continue
        I = len(a)
        for r in range(I + 1):
            p = I - r if anchor == "end" else r
            if p >= n_pos:
                continue
            coverage[p] += 1
            if r < I:
                x = int(a[r])
                for y in range(4):
                    cls = SAME if y == x else TRANSITION if K._is_transition(x, y) else TRANSVERSION
                    profile[cls, p] += blk[MATCH + y, r]
                profile[SUM_DEL_OPEN, p] += blk[DEL_OPEN, r]
                profile[SUM_DEL_EXTEND, p] += blk[DEL_EXTEND, r]
            profile[SUM_DUP:, p] += blk[DUP:, r]
    return profile, coverage


# ------------------------------------------------------------------------------------------------ shapes of the GPU tests
STRIPE_ROWS = (0, 1, 62, 63, 64, 65, 127, 128, 129)                # I: a profile has I + 1 rows, a stripe 64


def stripe_pairs(seed, longer=True):
    """Originals of every length in STRIPE_ROWS with reads within 8 bases of them, one read of the same length each (the pairs of
    band 0) and O = 0 once; every other read is given reverse-complemented and flagged: (originals, reads, read_strand).
    longer=False, for a model without duplications, under which a read longer than its original has no path: no such read.  (The
    empty original has only the empty read: nothing can be duplicated in front of its end.)"""
    from test_assign_cpu import _rand
    from test_gpu_pair_align import _related
    rng = random.Random(seed)
    ins, outs = [], []
    for I in STRIPE_ROWS:
        a = _rand(rng, I)
        shorter, more = max(0, I - rng.randint(1, 8)), I + rng.randint(1, 8)
        for O in sorted({I, shorter} | ({more} if longer and I else set())):
            ins.append(a)
            outs.append(_related(rng, a, O))
    ins.append(_rand(rng, 5))
    outs.append("")
    strand = [i % 2 for i in range(len(ins))]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    outs = ["".join(comp[c] for c in reversed(b)) if s else b for b, s in zip(outs, strand)]
    return ins, outs, strand
