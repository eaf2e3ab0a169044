"""Exact references of the two models, written from their generative definitions -- TEST INFRASTRUCTURE.

The C oracle (oracle/*.c) restates the reference's recurrences and the HIP kernels are held to it bit for bit.  This module is
the third pin: it restates neither.  The mutator pair HMM is written down once as a list of moves (`_moves`), from which
`enumerate_pair` walks every path and `exact_fwdback` sums the same paths over the move graph in linear space; the Viterbi
decoder is an explicit graph over (pos, state, lane) solved by Bellman-Ford sweeps (`exact_viterbi`).  All arithmetic is mpmath
at 160 bits: no log-sum-exp table, no band bookkeeping, no topological order of the machine, no worklist.  Nothing here is
imported from dnastore_amd or from the oracle except the independent file readers oracle.oracle.Machine / MutatorParams.

The mutator pair HMM (reference src/mutator.h, src/fwdback.h).  A path starts in S at (ip, op) = (0, 0)
and must end in S at (inLen, outLen).  From S: match/substitute (noGap * 4 p(in, out), one base of each), open a deletion
(pDelOpen, one input base, to D), open a tandem duplication of length k + 1 for k < min(ip, P) (pTanDup * pLen[k], to T_k).
From D: extend (pDelExtend, one input base) or end (1 - pDelExtend, to S).  From T_k: emit one output base scored against input
base in[ip - 1 - k] (4 p), to T_(k-1), or to S from T_0.  noGap = 1 - pDelOpen - pTanDup; p(x, y) = 1 - pTransition -
pTransversion for x == y, pTransition for a transition, pTransversion / 2 for a transversion.  Every (ip, op) a path stands on
must lie in the guide envelope |cm_in[ip] - cm_out[op]| <= maxDistance, maxDistance = P (0 with strict guides).

The Viterbi graph (reference src/viterbi.cpp:6-60 for the input model and the usable-edge rule,
viterbi.cpp:62-176 for what the lattice holds).  Two reference behaviours are not part of the model and are mirrored on purpose,
because the lattice and the decoded string are defined by them:
  * local mode stores max_s S(s, L) in the end state's S cell at L after the fill (viterbi.cpp:171-173); `exact_viterbi` does the
    same after its fixpoint, so that cell is the optimum and feeds nothing;
  * the traceback stops at state 0 whatever the position, and in local mode may stop at any state once pos = 0
    (viterbi.cpp:247, 263-264); the set of tight strings is read with those two stop rules.

Tolerances (the issue's rule: measured oracle-vs-exact gap on the committed case lists, GPU bound = 4x, gradient bound = 2x the
oracle's own deviation).  The E-step gap is the reference's log_sum_exp table (a term is dropped once the difference reaches
10: e^-10 = 4.5e-5 per operation; interpolation adds about 3e-10), which oracle and kernels must both reproduce.  Reproduce with

    python tests/exact_models.py --measure

Measured on tiny_models(), medium_models() and GRADIENT_CASES (oracle built with gcc, x86-64):
                                                                    tiny        medium
    max |oracle ll - exact ll| / max(1, |exact ll|), per pair      3.822e-05   6.833e-05     -> bound 4 x: ESTEP_LL_REL
    max |oracle count - exact count|, per database count           1.299e-04   4.750e-03     -> bound 4 x: ESTEP_COUNT_ABS
    max gradient-identity deviation / sum of the terms             6.803e-04                 -> bound 2 x: GRADIENT_REL
(where no log-sum-exp term is dropped -- the P = 0 and P = 1 tiny models -- the gaps are 7.6e-10 and 7.9e-9; with the table of a
scratch copy of the oracle replaced by log1p(exp(-x)) they are 1e-15 / 2e-14 (tiny), 3.5e-15 / 2e-11 (medium) and 3.1e-7 (gradient):
the table is the whole gap).  The CPU tests hold the oracle, and the GPU tests the library, to the same bounds.
"""
import json
import os
import random
import sys

import mpmath
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

mp = mpmath.mp.clone()
mp.prec = 160
mpf = mp.mpf
NEG_INF = mpf("-inf")

# ---- measured by `python tests/exact_models.py --measure` (see the docstring); the tiny and the medium list each keep their own
#      figure, so that the long pairs' larger gap does not loosen the bound on the tiny ones
MEASURED_LL_REL = {"tiny": 3.822e-05, "medium": 6.833e-05}
MEASURED_COUNT_ABS = {"tiny": 1.299e-04, "medium": 4.750e-03}
MEASURED_GRADIENT_REL = 6.803e-04
ESTEP_LL_REL = {k: 4 * v for k, v in MEASURED_LL_REL.items()}
ESTEP_COUNT_ABS = {k: 4 * v for k, v in MEASURED_COUNT_ABS.items()}
GRADIENT_REL = 2 * MEASURED_GRADIENT_REL
VITERBI_REL = 1e-12             # derived, not measured: <= 3(L+1) + N fp64 roundings along one path
TIGHT = 1e-9
MAX_STRINGS = 64
MAX_PATHS = 60000               # enumerate_pair refuses longer walks: keeps every tiny case well under a second

# MutatorCounts order of dnas_fwdback_estep
C_DELOPEN, C_TANDUP, C_NOGAP, C_DELEXT, C_DELEND, C_SUB, C_LEN = 0, 1, 2, 3, 4, 5, 21
BASES = "ACGT"


# ================================================================================================ the mutator pair HMM
def _is_transition(x, y):
    return x != y and (x & 1) == (y & 1)          # A<->G, C<->T in ACGT order


class PairModel:
    """The move weights of one MutatorParams, as mpf probabilities (odds against the uniform null model for emissions)."""

    def __init__(self, params):
        f = mpf
        self.P = len(params.pLen)
        self.del_open, self.tan_dup, self.del_ext = f(params.pDelOpen), f(params.pTanDup), f(params.pDelExtend)
        self.no_gap = 1 - self.del_open - self.tan_dup
        self.del_end = 1 - self.del_ext
        ti, tv = f(params.pTransition), f(params.pTransversion)
        self.odds = [[4 * ((1 - ti - tv) if x == y else ti if _is_transition(x, y) else tv / 2) for y in range(4)] for x in range(4)]
        self.p_len = [f(x) for x in params.pLen]


def _moves(m, node, ins, outs):
    """Every move out of node = (ip, op, lane) with lane 'S', 'D' or k (T_k): [(next node, weight, count indices)]."""
    ip, op, lane = node
    out = []
    if lane == "S":
        if ip < len(ins) and op < len(outs):
            x, y = ins[ip], outs[op]
            out.append(((ip + 1, op + 1, "S"), m.no_gap * m.odds[x][y], (C_NOGAP, C_SUB + 4 * x + y)))
        if ip < len(ins):
            out.append(((ip + 1, op, "D"), m.del_open, (C_DELOPEN,)))
        for k in range(min(ip, m.P)):
            out.append(((ip, op, k), m.tan_dup * m.p_len[k], (C_TANDUP, C_LEN + k)))
    elif lane == "D":
        if ip < len(ins):
            out.append(((ip + 1, op, "D"), m.del_ext, (C_DELEXT,)))
        out.append(((ip, op, "S"), m.del_end, (C_DELEND,)))
    elif op < len(outs):
        x, y = ins[ip - 1 - lane], outs[op]
        out.append(((ip, op + 1, lane - 1 if lane else "S"), m.odds[x][y], (C_SUB + 4 * x + y,)))
    return out


def _envelope(m, cm_in, cm_out, strict):
    dist = 0 if strict else m.P
    return lambda ip, op: abs(int(cm_in[ip]) - int(cm_out[op])) <= dist


def _result(m, z, sums):
    n = 21 + m.P
    if z == 0:
        return float("-inf"), np.full(n, np.nan), NEG_INF
    return float(mp.log(z)), np.array([float(s / z) for s in sums]), mp.log(z)


def enumerate_pair(params, in_seq, out_seq, cm_in, cm_out, strict=False, open_envelope=False, count_only=False):
    """Depth-first walk over every path of the pair HMM -> (log-likelihood, expected counts float64[21+P], paths walked).
    No legal path: (-inf, NaN counts, paths).  open_envelope: the guide is ignored; count_only: no arithmetic, only the number of
    complete paths (zero-weight ones included)."""
    m = PairModel(params)
    ins, outs = [int(x) for x in in_seq], [int(x) for x in out_seq]
    inside = (lambda ip, op: True) if open_envelope else _envelope(m, cm_in, cm_out, strict)
    end = (len(ins), len(outs), "S")
    sums = [mpf(0)] * (21 + m.P)
    used = [0] * (21 + m.P)
    state = {"z": mpf(0), "paths": 0}

    def walk(node, w):
        if node == end:
            state["paths"] += 1
            if state["paths"] > MAX_PATHS:
                raise OverflowError("more than %d paths" % MAX_PATHS)
            if not count_only:
                state["z"] += w
                for i, c in enumerate(used):
                    if c:
                        sums[i] += c * w
            # (the walk goes on: S at the end cell can still open a duplication, which dies for want of output)
        for nxt, wt, idx in _moves(m, node, ins, outs):
            if not inside(nxt[0], nxt[1]) or (wt == 0 and not count_only):
                continue
            for i in idx:
                used[i] += 1
            walk(nxt, w if count_only else w * wt)
            for i in idx:
                used[i] -= 1

    if inside(0, 0):
        walk((0, 0, "S"), mpf(1))
    if count_only:
        return None, None, state["paths"]
    ll, counts, _ = _result(m, state["z"], sums)
    return ll, counts, state["paths"]


def exact_fwdback(params, in_seq, out_seq, cm_in, cm_out, strict=False):
    """The same sums as enumerate_pair by a forward and a backward pass over the move graph, in linear space (mpf has no
    exponent limit to speak of, so nothing under- or overflows and no log-sum-exp is needed) -> (log-likelihood, counts)."""
    m = PairModel(params)
    ins, outs = [int(x) for x in in_seq], [int(x) for x in out_seq]
    inside = _envelope(m, cm_in, cm_out, strict)
    # moves only ever go D -> S -> T_k inside a cell, to a later op in the same row, or to a later row
    order = [(ip, op, ln) for ip in range(len(ins) + 1) for op in range(len(outs) + 1) if inside(ip, op)
             for ln in ["D", "S"] + list(range(min(ip, m.P)))]
    fwd = {n: mpf(0) for n in order}
    bwd = dict(fwd)
    start, end = (0, 0, "S"), (len(ins), len(outs), "S")
    if start not in fwd or end not in fwd:
        return _result(m, mpf(0), None)[:2]
    edges = {}
    fwd[start] = mpf(1)
    for n in order:
        edges[n] = [(nxt, wt, idx) for nxt, wt, idx in _moves(m, n, ins, outs) if nxt in fwd]
        if fwd[n] != 0:
            for nxt, wt, idx in edges[n]:
                fwd[nxt] += fwd[n] * wt
    bwd[end] = mpf(1)
    for n in reversed(order):
        for nxt, wt, idx in edges[n]:
            bwd[n] += wt * bwd[nxt]
    z = fwd[end]
    sums = [mpf(0)] * (21 + m.P)
    for n in order:
        if fwd[n] != 0:
            for nxt, wt, idx in edges[n]:
                post = fwd[n] * wt * bwd[nxt]
                for i in idx:
                    sums[i] += post
    assert z == 0 or abs(bwd[start] / z - 1) < mpf(10) ** -40
    return _result(m, z, sums)[:2]


def guide_columns(row_in, row_out):
    """Two gapped rows -> (in tokens, out tokens, cm_in, cm_out): cm_x[pos] = matches (columns with a base in both rows) up to and
    including the alignment column of sequence position pos; position 0 stands before the first column."""
    assert len(row_in) == len(row_out)
    gap = "-."
    cm_in, cm_out, matches = [0], [0], 0
    for a, b in zip(row_in, row_out):
        matches += a not in gap and b not in gap
        if a not in gap:
            cm_in.append(matches)
        if b not in gap:
            cm_out.append(matches)
    tok = lambda row: np.array([BASES.index(c.upper()) for c in row if c not in gap], dtype=np.int8)
    return tok(row_in), tok(row_out), np.array(cm_in, dtype=np.int32), np.array(cm_out, dtype=np.int32)


# ================================================================================================ the Viterbi graph
def _log(p):
    p = mpf(p)
    return NEG_INF if p == 0 else mp.log(p)


class ViterbiGraph:
    """The explicit decoding graph of (machine, params): per-layer edge lists over nodes (state, lane), lane 0 = S, 1 = D,
    2 + k = T_k."""

    def __init__(self, machine, params):
        self.n = machine.n
        P = len(params.pLen)
        st = machine.states
        # input model: the symbols a decode can report ('0' '1', control 'A'..'Z', '^' '$'), control ones weighted 4^(-4P)
        alph = sorted({i for s in st for (i, o, d) in s["trans"] if i and (i in "01^$" or "A" <= i <= "Z")})
        wt = {c: (mpf(4) ** (-4 * P) if "A" <= c <= "Z" else mpf(1)) for c in alph}
        norm = sum(wt.values())
        self.sym_logp = {c: mp.log(wt[c] / norm) for c in alph}
        self.D = min(max(len(s["l"]) for s in st), P)
        self.ctx, self.depth = [], []
        for s in st:
            own = [BASES.index(c.upper()) for c in s["l"] if c != "*"]
            self.depth.append(min(self.D, len(own)))
            self.ctx.append(own[::-1])                       # ctx[k] = k bases back from the state's last emitted base
        self.del_open, self.tan_dup, self.del_ext = _log(params.pDelOpen), _log(params.pTanDup), _log(params.pDelExtend)
        self.no_gap = _log(1 - mpf(params.pDelOpen) - mpf(params.pTanDup))
        self.del_end = _log(1 - mpf(params.pDelExtend))
        ti, tv = mpf(params.pTransition), mpf(params.pTransversion)
        self.sub = [[_log(4 * ((1 - ti - tv) if x == y else ti if _is_transition(x, y) else tv / 2)) for y in range(4)] for x in range(4)]
        self.len = [_log(x) for x in params.pLen]
        self.local = params.local
        self.emit, self.null = [], []                         # (src, dest, score, symbol[, base])
        for u, s in enumerate(st):
            for (i, o, d) in s["trans"]:
                if i and i not in self.sym_logp:             # '.', strict symbols: not part of the decoder's input
                    continue
                sc = self.sym_logp[i] if i else mpf(0)
                if o:
                    self.emit.append((u, d, sc, i, BASES.index(o.upper())))
                else:
                    self.null.append((u, d, sc, i))

    def in_layer_edges(self, pos):
        """[(u state, u lane, v state, v lane, weight, symbol)] between nodes of one position."""
        e = []
        for (u, d, sc, sym, b) in self.emit:                 # the edge's base is deleted: the read does not advance
            e.append((u, 0, d, 1, self.del_open + sc, sym))
            e.append((u, 1, d, 1, self.del_ext + sc, sym))
        for (u, d, sc, sym) in self.null:
            e.append((u, 0, d, 0, sc, sym))
            e.append((u, 1, d, 1, sc, sym))
        for v in range(self.n):
            e.append((v, 1, v, 0, self.del_end, ""))
            if pos > 0:
                for k in range(self.depth[v]):
                    e.append((v, 0, v, 2 + k, self.tan_dup + self.len[k], ""))
        return e

    def cross_layer_edges(self, x):
        """Edges from position pos - 1 to pos, where the read has base x."""
        e = []
        for (u, d, sc, sym, b) in self.emit:
            e.append((u, 0, d, 0, self.no_gap + self.sub[b][x] + sc, sym))
        for v in range(self.n):
            for k in range(self.depth[v]):
                e.append((v, 2 + k, v, 1 + k if k else 0, self.sub[self.ctx[v][k]][x], ""))
        return e


def exact_viterbi(machine, params, read):
    """-> (optimum log-likelihood, lattice float64 [L+1][N][D+2] rounded from mpf, set of input-symbol strings along tight paths
    or None when there are more than MAX_STRINGS: "ambiguous").  The position only ever grows along an edge, so the layers are
    solved in order; inside a layer the edges are swept in file order until nothing changes (deletions over emitting cycles make
    the layer's graph cyclic: no order of the states would do)."""
    g = machine if isinstance(machine, ViterbiGraph) else ViterbiGraph(machine, params)
    x = [BASES.index(c.upper()) for c in read]
    L, N, W = len(x), g.n, g.D + 2
    dist = [[[NEG_INF] * W for _ in range(N)] for _ in range(L + 1)]
    for s in (range(N) if g.local else [0]):
        dist[0][s][0] = mpf(0)
    layers = []
    for pos in range(L + 1):
        cross = g.cross_layer_edges(x[pos - 1]) if pos else []
        inner = g.in_layer_edges(pos)
        layers.append((cross, inner))
        cur = dist[pos]
        for (u, ul, v, vl, w, _) in cross:
            c = dist[pos - 1][u][ul] + w
            if c > cur[v][vl]:
                cur[v][vl] = c
        changed, sweeps = True, 0
        while changed:
            changed = False
            sweeps += 1
            assert sweeps <= 2 * N * W + 2, "a positive cycle"
            for (u, ul, v, vl, w, _) in inner:
                c = cur[u][ul] + w
                if c > cur[v][vl]:
                    cur[v][vl] = c
                    changed = True
    ends = range(N) if g.local else [N - 1]
    opt = max(dist[L][s][0] for s in ends)

    # ---- strings along tight paths, read backwards with the traceback's stop rules
    memo = {}
    overflow = [False]

    def tight(a, w, b):
        return a != NEG_INF and abs(a + w - b) <= TIGHT

    def strings(pos, v, vl):
        key = (pos, v, vl)
        if key in memo:
            return memo[key]
        if v == 0:
            memo[key] = {""}
            return memo[key]
        memo[key] = set()                                    # (a tight cycle would need a zero-weight cycle: there is none)
        res = set()
        here = dist[pos][v][vl]
        if g.local and pos == 0 and vl == 0 and here == 0:
            res.add("")
        cross, inner = layers[pos]
        for (edges, ppos) in ((cross, pos - 1), (inner, pos)):
            for (u, ul, v2, vl2, w, sym) in edges:
                if v2 == v and vl2 == vl and tight(dist[ppos][u][ul], w, here):
                    for s in strings(ppos, u, ul):
                        res.add(s + sym)
                        if len(res) > MAX_STRINGS:
                            overflow[0] = True
                            memo[key] = res
                            return res
        memo[key] = res
        return res

    found = set()
    if opt != NEG_INF:
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 20000))
        try:
            for s in ends:
                if abs(dist[L][s][0] - opt) <= TIGHT:
                    found |= strings(L, s, 0)
        finally:
            sys.setrecursionlimit(old)
    else:
        found = {""}                                         # no path: the decode is the empty string (viterbi.cpp:198-201)
    lat = np.array([[[float(c) for c in row] for row in layer] for layer in dist], dtype=np.float64).reshape(L + 1, N, W)
    if g.local:
        lat[L, N - 1, 0] = float(opt)                        # viterbi.cpp:171-173 (see the module docstring)
    return float(opt), lat, (None if overflow[0] or len(found) > MAX_STRINGS else found)


def lattice_close(got, want):
    """Every lane of every cell: -inf in the same places, finite values within VITERBI_REL * max(1, |value|)."""
    if got.shape != want.shape or np.isnan(got).any():
        return False
    inf_g, inf_w = np.isneginf(got), np.isneginf(want)
    if not np.array_equal(inf_g, inf_w) or np.isposinf(got).any():
        return False
    fin = ~inf_w
    return bool(np.all(np.abs(got[fin] - want[fin]) <= VITERBI_REL * np.maximum(1., np.abs(want[fin]))))


def ll_close(got, want, rel=VITERBI_REL):
    if want == float("-inf") or got == float("-inf"):
        return got == want
    return abs(got - want) <= rel * max(1., abs(want))


# ================================================================================================ committed case lists
def _make_params(pLen, **kw):
    from oracle.oracle import MutatorParams
    return MutatorParams(pLen=list(pLen), **kw)


def _plen(P, shape):
    from random_machines import plen_shape
    return [1. / P] * P if shape == "uniform" and P else plen_shape(P, shape)


def _random_guide(rng, a, b, kind):
    """Two gapped rows for sequences a, b.  kind "gaps": no column has both bases; "diag": matches first, the rest gapped at the
    end; "random": columns drawn at random."""
    r1, r2, i, j = [], [], 0, 0
    while i < len(a) or j < len(b):
        both = i < len(a) and j < len(b)
        if kind == "gaps":
            pick = 1 if i < len(a) else 2
        elif kind == "diag":
            pick = 0 if both else 1 if i < len(a) else 2
        else:
            pick = rng.choice([0, 0, 0, 1, 2]) if both else 1 if i < len(a) else 2
        if pick == 0:
            r1.append(a[i]); r2.append(b[j]); i += 1; j += 1
        elif pick == 1:
            r1.append(a[i]); r2.append("-"); i += 1
        else:
            r1.append("-"); r2.append(b[j]); j += 1
    return "".join(r1), "".join(r2)


TINY_P = (0, 1, 2, 3, 5, 6, 8, 9)
TINY_PER_MODEL = 20


def tiny_models():
    """16 models (every P of TINY_P, strict and not) with 20 tiny pairs each: [(name, MutatorParams, strict, rows)], rows =
    [(gapped in, gapped out)].  Probabilities up to 0.5, every pLen shape, in 0..5 and out 0..6 bases, guides from wide open
    (all gaps) to one diagonal."""
    models = []
    for P in TINY_P:
        for strict in (False, True):
            rng = random.Random("tiny/%d/%d" % (P, strict))
            shape = ("uniform", "down", "up", "zero")[(P + strict) % 4]
            ti = rng.uniform(.01, .3)
            params = _make_params(_plen(P, shape), pDelOpen=rng.uniform(.01, .4), pDelExtend=rng.uniform(.01, .5),
                                  pTanDup=rng.uniform(.01, .5), pTransition=ti, pTransversion=rng.uniform(.01, .3))
            rows = []
            for i in range(TINY_PER_MODEL):
                n_in = 0 if i == 0 else rng.choice([1, 2, 3, 3, 4, 4, 5, 5])
                a = "".join(rng.choice(BASES) for _ in range(n_in))
                if i == 1:
                    b = ""
                elif P == 0 and i % 5:                 # no duplications: only an output no longer than the input has a path
                    b = "".join(rng.choice(BASES) if rng.random() < .3 else c for c in a if rng.random() < .8)
                elif rng.random() < .6 and a:          # an output the model explains well: a copy with a repeat or a gap
                    at = rng.randrange(len(a))
                    b = (a[:at + 1] + a[max(0, at - rng.randint(0, 2)):at + 1] + a[at + 1:]) if rng.random() < .6 else a[:at] + a[at + 1:]
                    b = b[:6]
                else:
                    b = "".join(rng.choice(BASES) for _ in range(rng.randint(0, 6)))
                kind = "gaps" if i in (2, 3) else rng.choice(["diag", "diag", "random", "random", "random"])
                rows.append(_random_guide(rng, a, b, kind))
            models.append(("tiny-P%d-%s" % (P, "strict" if strict else "loose"), params, strict, rows))
    return models


def medium_models():
    """Pairs of 20 to 80 bases from synth.synthetic_alignment with realistic guide envelopes, among them a 24-base deletion block
    and long runs of duplications (what test_gpu_fwdback.py steers the E-step's routing with): [(name, params, strict, rows)]."""
    from synth import synthetic_alignment
    out = []
    for name, P, strict, kw in (("medium-P6", 6, False, dict(pDelOpen=.02, pDelExtend=.1, pTanDup=.03, sub=.03)),
                                ("medium-P3-strict", 3, True, dict(pDelOpen=.03, pDelExtend=.2, pTanDup=.02, sub=.05)),
                                ("medium-P9", 9, False, dict(pDelOpen=.01, pDelExtend=.05, pTanDup=.02, sub=.02))):
        rng = random.Random("medium/" + name)
        shape = {6: "uniform", 3: "down", 9: "up"}[P]
        params = _make_params(_plen(P, shape), **kw)
        rows = []
        for n in (20, 33, 47, 64, 80):
            r = synthetic_alignment(rng, n, sub=.03, dele=.03, dup=.03)
            rows.append((r[0][1], r[1][1]))
        src = "".join(rng.choice(BASES) for _ in range(80))
        cut = rng.randrange(10, 40)
        rows.append((src, src[:cut] + "-" * 24 + src[cut + 24:]))             # 24 input bases deleted in a row
        if not strict:                                                        # (strict guides cannot follow a run of copies)
            for seed, n, dup in ((5, 30, .35), (6, 24, .8)):
                r = synthetic_alignment(random.Random(seed), n, sub=.02, dele=.0, dup=dup)
                rows.append((r[0][1], r[1][1]))
        out.append((name, params, strict, rows))
    return out


_CACHE = {}


def exact_database(model, method):
    """(per-pair exact ll float64[n], summed exact counts over the pairs that have a path, paths walked per pair or None).
    method "enumerate" or "fwdback"; cached per process."""
    name, params, strict, rows = model
    key = (name, method)
    if key not in _CACHE:
        per, total, walked = [], np.zeros(21 + len(params.pLen)), []
        for r in rows:
            ins, outs, ci, co = guide_columns(*r)
            if method == "enumerate":
                ll, counts, n = enumerate_pair(params, ins, outs, ci, co, strict)
                walked.append(n)
            else:
                ll, counts = exact_fwdback(params, ins, outs, ci, co, strict)
            per.append(ll)
            if ll != float("-inf"):
                total += counts
        _CACHE[key] = (np.array(per), total, walked or None)
    return _CACHE[key]


def split_database(model, per):
    """A model's rows as two lists of pair tuples: those with a path and those without (the reference's counts are NaN for the
    latter, so they are kept apart)."""
    with_path, without = [], []
    for r, ll in zip(model[3], per):
        (without if ll == float("-inf") else with_path).append(guide_columns(*r))
    return with_path, without


def params_text(params):
    """MutatorParams JSON text with repr() doubles: the library's loader and oracle.MutatorParams.from_json read the same values."""
    return "{\n %s\n}\n" % ",\n ".join([
        '"pDelOpen": %r' % float(params.pDelOpen), '"pDelExtend": %r' % float(params.pDelExtend),
        '"pTanDup": %r' % float(params.pTanDup), '"pTransition": %r' % float(params.pTransition),
        '"pTransversion": %r' % float(params.pTransversion), '"pLen": [ %s ]' % ", ".join(repr(float(x)) for x in params.pLen),
        '"local": %s' % ("true" if params.local else "false")])


# ---- Viterbi cases: (D, seed, states, global, reads)
VITERBI_SHAPES = ((0, 3), (1, 5), (2, 9), (3, 12), (4, 17), (5, 22), (6, 28), (7, 34), (8, 40), (4, 8), (2, 40))
VITERBI_FLAGS = dict(dup=.05, sub=.04, del_open=.04, del_ext=.2)


def viterbi_cases():
    """[(name, machine text, params text, reads)]: random machines of 3 to 40 states at every duplication width 0..8 (wildcard
    contexts at 3, 5, 7), local and global, reads of 0 to 30 bases with noise and planted duplications."""
    from random_machines import params_json, random_read, width_case
    cases = []
    for n, (D, states) in enumerate(VITERBI_SHAPES):
        for global_ in (False, True):
            seed = 300 + 10 * n + global_
            text, pLen = width_case(D, seed, states)
            ptext = params_json(pLen, global_=global_, **VITERBI_FLAGS)
            reads = [""]
            for i, max_len in enumerate((1, 4, 9, 16, 23, 30)):
                r = random_read(seed * 100 + i, text, max_len=max_len, noise=(0., .1, .25)[i % 3], dups=D if i % 2 else 0)
                reads.append(r[:30])
            cases.append(("D%d-N%d-%s" % (D, states, "global" if global_ else "local"), text, ptext, reads))
    return cases


def no_path_case():
    """A global decode that cannot succeed: substitutions are impossible (sub = 0) and the machine never emits a T."""
    from random_machines import params_json, random_read, width_case
    text, pLen = width_case(3, 77, 12)
    j = json.loads(text)
    for st in j["state"]:
        st["l"] = st["l"].replace("T", "A")
        for t in st["trans"]:
            if t.get("out") == "T":
                t["out"] = "A"
    text = json.dumps(j)
    ptext = params_json(pLen, global_=True, **dict(VITERBI_FLAGS, sub=0.))
    r = random_read(7700, text, max_len=12, noise=0.)
    return "no-path-global", text, ptext, [r, r[:len(r) // 2] + "T" + r[len(r) // 2:], "T"]


def exact_viterbi_case(case):
    """[(ll, lattice, strings or None)] for the case's reads; cached per process."""
    from oracle.oracle import Machine, MutatorParams
    name, text, ptext, reads = case
    if ("vit", name) not in _CACHE:
        g = ViterbiGraph(Machine.from_json(text), MutatorParams.from_json(ptext))
        _CACHE[("vit", name)] = [exact_viterbi(g, None, r) for r in reads]
    return _CACHE[("vit", name)]


# ---- boundary variants: probabilities of exactly 0 and 1 (scores of -inf reached through a score, not through an unreachable
#      cell), of 1e-300 (scores near -690: every log-sum-exp difference is beyond the table, anything that leaves log space
#      underflows) and of 1 - 2^-53 (log(1 - p) is the log of the smallest positive gap).  (name, overrides of a base MutatorParams)
BOUNDARY_VARIANTS = (
    ("delOpen0", dict(pDelOpen=0.)),
    ("tanDup0", dict(pTanDup=0.)),
    ("delExt0", dict(pDelExtend=0.)),
    ("delExt1", dict(pDelExtend=1.)),                                   # delEnd = -inf
    ("ti0", dict(pTransition=0.)),
    ("tv0", dict(pTransversion=0.)),
    ("sub0", dict(pTransition=0., pTransversion=0.)),                   # the match score is log 1 - log 1/4
    ("match0", dict(pTransition=.6, pTransversion=.4)),                 # pMatch = 0 (1 - .6 - .4 is 0 in fp64 as well)
    ("noGap0", dict(pDelOpen=.5, pTanDup=.5)),                          # noGap = -inf
    ("gaps0", dict(pDelOpen=0., pTanDup=0.)),
    ("rare", dict(pDelOpen=1e-300, pTanDup=1e-300, pDelExtend=1e-300, pTransition=1e-300, pTransversion=1e-300)),
    ("rareGaps", dict(pDelOpen=1e-300, pTanDup=1e-300)),
    ("subRare", dict(pTransition=1e-300, pTransversion=1e-300)),
    ("delExtNear1", dict(pDelExtend=1 - 2. ** -53)),
)
BOUNDARY_NAMES = tuple(n for n, _ in BOUNDARY_VARIANTS)
BOUNDARY_ESTEP_BASES = ("tiny-P3-loose", "tiny-P2-strict", "tiny-P8-loose", "tiny-P0-loose")
BOUNDARY_VITERBI_MACHINES = ("D0-N3", "D2-N9", "D4-N17", "D8-N40")
BOUNDARY_MAX_READS = 8


def boundary_params(base, name):
    """The base's MutatorParams with the variant's overrides; every other field (pLen and local among them) as the base has it."""
    from oracle.oracle import MutatorParams
    q = MutatorParams(base.pDelOpen, base.pDelExtend, base.pTanDup, base.pTransition, base.pTransversion, list(base.pLen), base.local)
    for field, value in dict(BOUNDARY_VARIANTS)[name].items():
        setattr(q, field, value)
    return q


def boundary_estep_models():
    """BOUNDARY_ESTEP_BASES x the 14 variants, in the shape of tiny_models(): [("<base>/<variant>", params, strict, rows)]."""
    tiny = {m[0]: m for m in tiny_models()}
    return [("%s/%s" % (base, v), boundary_params(tiny[base][1], v), tiny[base][2], tiny[base][3])
            for base in BOUNDARY_ESTEP_BASES for v in BOUNDARY_NAMES]


def boundary_viterbi_cases():
    """BOUNDARY_VITERBI_MACHINES of viterbi_cases(), global and local, x the 14 variants, with the case's first reads (at most
    8): [("<case>/<variant>", machine text, params text, reads)]."""
    from oracle.oracle import MutatorParams
    out = []
    for name, text, ptext, reads in viterbi_cases():
        if name.rsplit("-", 1)[0] in BOUNDARY_VITERBI_MACHINES:
            base = MutatorParams.from_json(ptext)
            for v in BOUNDARY_NAMES:
                out.append(("%s/%s" % (name, v), text, params_text(boundary_params(base, v)), reads[:BOUNDARY_MAX_READS]))
    return out


# ---- gradient identity: pairs of 256 and 1000 bases, out of reach of the exact models
GRADIENT_CASES = ((256, 6, 11), (1000, 6, 12), (256, 3, 13))      # (length, P, seed)


def gradient_case(length, P, seed):
    from synth import synthetic_alignment
    rng = random.Random(seed)
    rows = [synthetic_alignment(rng, length, sub=.03, dele=.02, dup=.02) for _ in range(4)]
    params = _make_params(_plen(P, "down"), pDelOpen=.02, pDelExtend=.15, pTanDup=.03, pTransition=.03, pTransversion=.01)
    return params, [guide_columns(r[0][1], r[1][1]) for r in rows]


def gradient_terms(params, counts):
    """{parameter: (derivative of the log-likelihood by the counts, scale = sum of the absolute terms)}: each probability enters
    the likelihood as p^n (and its complement as (1 - ...)^n'), so d ll / d p = n / p - n' / (1 - ...)."""
    sub = counts[C_SUB:C_SUB + 16].reshape(4, 4)
    n_match = sum(sub[i][i] for i in range(4))
    n_ti = sum(sub[i][j] for i in range(4) for j in range(4) if _is_transition(i, j))
    n_tv = sum(sub[i][j] for i in range(4) for j in range(4) if i != j and not _is_transition(i, j))
    no_gap = 1 - params.pDelOpen - params.pTanDup
    p_match = 1 - params.pTransition - params.pTransversion
    pairs = {"pDelOpen": (counts[C_DELOPEN] / params.pDelOpen, counts[C_NOGAP] / no_gap),
             "pTanDup": (counts[C_TANDUP] / params.pTanDup, counts[C_NOGAP] / no_gap),
             "pDelExtend": (counts[C_DELEXT] / params.pDelExtend, counts[C_DELEND] / (1 - params.pDelExtend)),
             "pTransition": (n_ti / params.pTransition, n_match / p_match),
             "pTransversion": (n_tv / params.pTransversion, n_match / p_match)}
    for k, p in enumerate(params.pLen):
        pairs["pLen[%d]" % k] = (counts[C_LEN + k] / p, 0.)
    return {k: (a - b, a + b) for k, (a, b) in pairs.items()}


def with_parameter(params, name, value):
    from oracle.oracle import MutatorParams
    q = MutatorParams(params.pDelOpen, params.pDelExtend, params.pTanDup, params.pTransition, params.pTransversion,
                      list(params.pLen), params.local)
    if name.startswith("pLen["):
        q.pLen[int(name[5:-1])] = value
    else:
        setattr(q, name, value)
    return q


def parameter_value(params, name):
    return params.pLen[int(name[5:-1])] if name.startswith("pLen[") else getattr(params, name)


def gradient_deviation(O, params, pairs, h=1e-3):
    """max over the free parameters of |central difference of the summed oracle log-likelihood - the counts' derivative| / scale."""
    counts, ll, per = O.expected_counts(params, pairs)
    worst = {}
    for name, (want, scale) in gradient_terms(params, counts).items():
        p = parameter_value(params, name)
        up = O.expected_counts(with_parameter(params, name, p * (1 + h)), pairs)[1]
        dn = O.expected_counts(with_parameter(params, name, p * (1 - h)), pairs)[1]
        worst[name] = abs((up - dn) / (2 * h * p) - want) / scale
    return worst


def measure():
    """The figures of record for the module docstring: oracle against the exact references on the committed case lists."""
    sys.path.insert(0, os.path.dirname(_HERE))
    from oracle import oracle as O
    O.build()
    for kind, models, method in (("tiny", tiny_models(), "enumerate"), ("medium", medium_models(), "fwdback")):
        ll_rel = cnt_abs = 0.
        for model in models:
            per, total, _ = exact_database(model, method)
            with_path, _ = split_database(model, per)
            oc, _, oper = O.expected_counts(model[1], with_path, strict=model[2])
            want = per[per != float("-inf")]
            ll_rel = max(ll_rel, float(np.max(np.abs(oper - want) / np.maximum(1., np.abs(want)))))
            cnt_abs = max(cnt_abs, float(np.max(np.abs(oc - total))))
            print("%-22s ll rel %.3e  count abs %.3e (running maxima)" % (model[0], ll_rel, cnt_abs))
        print("MEASURED_LL_REL[%r] = %.3e\nMEASURED_COUNT_ABS[%r] = %.3e" % (kind, ll_rel, kind, cnt_abs))
    grad = 0.
    for case in GRADIENT_CASES:
        dev = gradient_deviation(O, *gradient_case(*case))
        grad = max(grad, max(dev.values()))
        print(case, "gradient deviation %.3e (%s)" % (max(dev.values()), max(dev, key=dev.get)))
    print("MEASURED_GRADIENT_REL = %.3e" % grad)


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure()
