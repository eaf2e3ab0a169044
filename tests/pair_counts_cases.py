"""Exact posterior move counts of the mutator pair HMM over a band, the derived bounds and the case lists -- TEST INFRASTRUCTURE
for test_pair_counts_cpu.py and test_gpu_pair_counts.py.

`exact_counts` is a forward and a backward pass over the move graph exact_models._moves inside pair_forward_cases.band_predicate
in 160-bit mpmath, as exact_models.exact_fwdback does inside a guide's envelope: no table, no log-sum-exp, nothing imported from
the library.  `tiny_exact` takes the same counts from exact_models.enumerate_pair(open_envelope=True), which walks every path.

The bounds.  A count is a sum of terms exp(F(n) + w + B(n') - Z), all non-negative, so a bound on the factor by which one term
can be off bounds every count and every sum of counts.

Exact mode: F, B and Z are each within 1e-12 relative of their exact values (the bound of pair_forward_cases.py; the backward
pass makes the same kind of sums).  Every one of them is the log of a sum of products of at most 3 (I + O + 1) move weights, so
its magnitude is at most M = 3 (I + O + 1) (wmax + log(P + 3)), wmax the largest finite |log weight| of the model and P + 3 the
most moves that leave a node.  The exponent is then off by at most 3e-12 M, and the sum of at most cells * (4 + 2 P) terms adds
one fp64 rounding each: relative bound expm1(3e-12 M) + terms * 2.3e-16.

Table mode: pair_forward_cases.py bounds F (and Z) by n_F = 6 (I + O + 1) lse calls, each dropping at most a = e^-10 + 1e-9 and
adding at most 1e-9.  A backward value nests, per node of a path, the tree of B_S -- ceil(log2(P + 2)) calls deep -- or the one
call of B_D, or none (B_T), so n_B = 3 (I + O + 1) ceil(log2(P + 2)).  The exponent F + w + B - Z is off by at most
(2 n_F + n_B) a in either direction: every count lies within a factor exp(+-table_log_bound) of exact."""
import math
import os
import random
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import exact_models as X  # noqa: E402
import pair_forward_cases as C  # noqa: E402
import synth  # noqa: E402

NEG = float("-inf")
COUNTS_OK, COUNTS_NO_PATH, COUNTS_TOO_LARGE = 0, 1, 2
LSE_DROP = math.exp(-10.) + 1e-9


def exact_counts(plain, a, b, band=-1):
    """-> (log-likelihood, float64[21 + P] counts); (-inf, None) when the band holds no path of positive probability."""
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
    assert abs(bwd[start] / z - 1) < X.mpf(10) ** -40
    sums = [X.mpf(0)] * (21 + m.P)
    for n in order:
        if fwd[n] != 0:
            for nxt, wt, idx in edges[n]:
                post = fwd[n] * wt * bwd[nxt]
                for i in idx:
                    sums[i] += post
    return float(X.mp.log(z)), np.array([float(s / z) for s in sums])


def _wmax(plain):
    m = X.PairModel(plain)
    ws = [m.del_open, m.tan_dup, m.del_ext, m.no_gap, m.del_end] + [x for row in m.odds for x in row] + list(m.p_len)
    return max([abs(float(X.mp.log(w))) for w in ws if w > 0] + [1.])


def exact_rel_bound(plain, I, O):
    """The relative bound of exact mode on every count (module docstring)."""
    P = len(plain.pLen)
    M = 3 * (I + O + 1) * (_wmax(plain) + math.log(P + 3))
    return math.expm1(3e-12 * M) + (I + 1) * (O + 1) * (4 + 2 * P) * 2.3e-16


def table_log_bound(I, O, P):
    """Every count of table mode lies within a factor exp(+-this) of exact (module docstring)."""
    n_f = 6 * (I + O + 1)
    n_b = 3 * (I + O + 1) * max(1, math.ceil(math.log2(P + 2)))
    return (2 * n_f + n_b) * LSE_DROP


def backward_table_bounds(exact, I, O, P):
    """(lowest, highest) B_S(0,0) of table mode for a pair whose exact log-likelihood is `exact`."""
    n_b = 3 * (I + O + 1) * max(1, math.ceil(math.log2(P + 2)))
    return exact - n_b * LSE_DROP, exact + n_b * 1e-9


_CACHE = {}


def tiny_exact():
    """[(name, plain, pairs, [(ll, counts or None)])] from enumerate_pair over the whole matrix, computed once per process."""
    if "tiny" not in _CACHE:
        out = []
        for name, plain, pairs in C.tiny_cases():
            rows = []
            for a, b in pairs:
                ll, counts, _ = X.enumerate_pair(plain, a, b, None, None, open_envelope=True)
                rows.append((ll, None if ll == NEG else counts))
            out.append((name, plain, pairs, rows))
        _CACHE["tiny"] = out
    return _CACHE["tiny"]


def tiny_passed():
    """The tiny pairs through exact_counts instead of the enumeration (the CPU tests hold the two together; this one costs a
    fraction): [(name, plain, pairs, [(ll, counts or None)])], computed once per process."""
    if "tiny-passed" not in _CACHE:
        _CACHE["tiny-passed"] = [(name, plain, pairs, [exact_counts(plain, a, b) for a, b in pairs]) for name, plain, pairs in C.tiny_cases()]
    return _CACHE["tiny-passed"]


def medium_exact(bands=C.MEDIUM_BANDS):
    """[(name, plain, pairs, {band: [(ll, counts or None)]})] from exact_counts over `bands`, each band computed once per process."""
    out = []
    for name, plain, pairs in C.medium_cases():
        for band in bands:
            if ("medium", name, band) not in _CACHE:
                _CACHE[("medium", name, band)] = [exact_counts(plain, a, b, band) for a, b in pairs]
        out.append((name, plain, pairs, {band: _CACHE[("medium", name, band)] for band in bands}))
    return out


def boundary_exact():
    """[(name, plain, pairs, [(ll, counts or None)])] from exact_counts at band -1, computed once per process."""
    if "boundary" not in _CACHE:
        _CACHE["boundary"] = [(name, plain, pairs, [exact_counts(plain, a, b) for a, b in pairs]) for name, plain, pairs in C.boundary_cases()]
    return _CACHE["boundary"]


def zero_moves(plain):
    """The count slots of moves whose probability is exactly 0 under plain."""
    m = X.PairModel(plain)
    zero = []
    if m.del_open == 0:
        zero.append(X.C_DELOPEN)
    if m.tan_dup == 0:
        zero += [X.C_TANDUP] + [X.C_LEN + k for k in range(m.P)]
    if m.no_gap == 0:
        zero.append(X.C_NOGAP)
    if m.del_ext == 0:
        zero.append(X.C_DELEXT)
    if m.del_end == 0:
        zero.append(X.C_DELEND)
    zero += [X.C_LEN + k for k in range(m.P) if m.p_len[k] == 0]
    return sorted(set(zero))


# ------------------------------------------------------------------------------------------------ the EM, restated in numpy
def _is_transition(x, y):
    return x != y and (x & 1) == (y & 1)


def sub_classes(c):
    """(transitions, transversions, matches) of a MutatorCounts vector."""
    ni = sum(c[5 + 4 * i + j] for i in range(4) for j in range(4) if _is_transition(i, j))
    nv = sum(c[5 + 4 * i + j] for i in range(4) for j in range(4) if i != j and not _is_transition(i, j))
    return ni, nv, c[5] + c[10] + c[15] + c[20]


def m_step(counts):
    """mlParams of counts + the Laplace prior -> dict of the five probabilities (pLen goes back to uniform)."""
    c = np.asarray(counts, dtype=np.float64) + 1.
    ni, nv, nm = sub_classes(c)
    return dict(p_del_open=c[0] / (c[0] + c[1] + c[2]), p_tan_dup=c[1] / (c[0] + c[1] + c[2]), p_del_extend=c[3] / (c[3] + c[4]),
                p_transition=ni / (ni + nv + nm), p_transversion=nv / (ni + nv + nm))


def log_prior(params, n_len):
    """MutatorCounts::logPrior of the Laplace prior (a count of 1 in every slot) at params."""
    lg = math.lgamma
    ni, nv, nm = sub_classes(np.ones(21 + n_len))
    c = params.c

    def dirichlet(p, n):
        al = [x + 1 for x in n]
        return lg(sum(al)) + sum((a - 1) * math.log(q) - lg(a) for a, q in zip(al, p))

    beta = lg(4.) - lg(2.) - lg(2.) + math.log(c.p_del_extend) + math.log(1 - c.p_del_extend)
    return (beta + dirichlet([c.p_del_open, c.p_tan_dup, 1 - c.p_del_open - c.p_tan_dup], [1., 1., 1.])
            + dirichlet([c.p_transition, c.p_transversion, 1 - c.p_transition - c.p_transversion], [ni, nv, nm]))


def params_dict(p):
    return {k: getattr(p.c, k) for k in ("p_del_open", "p_tan_dup", "p_del_extend", "p_transition", "p_transversion")}


EM_BAND = 8


def em_pairs():
    """60 pairs of 20 to 40 bases, the reads drawn with synth.mutate: (originals, reads) as strings."""
    rng = random.Random("pair-counts/em")
    ins, outs = [], []
    for _ in range(60):
        a = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 40)))
        ins.append(a)
        outs.append(synth.mutate(a, rng, sub=.05, dele=.03, dup=.02) or a[:1])
    return ins, outs


def em_start(da):
    """A start with uniform pLen, far enough off the planted rates that the 1e-3 rule lets the loop run four steps."""
    from test_pair_align_cpu import make_params
    return make_params(da, [.25] * 4, pDelOpen=.2, pDelExtend=.6, pTanDup=.2, pTransition=.2, pTransversion=.2)
