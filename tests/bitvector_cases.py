"""Structured pools for the bit-vector recurrence (csrc/cluster_gate.hpp: gateBlock) behind the edit-distance gate and the primer
search: what test_bitvector_cpu.py holds the host statements to, and test_gpu_bitvector_pools.py the kernels to the host statements.

Random DNA keeps the carry chains of (Eq & Pv) + Pv a few bits long.  The pools here are homopolymers and repeats of period 2 and
3, whose chains run across bit 31/32 of the add, across the 64-row words and through the partial last word, at every pattern
length around a word boundary; nearly every column of a search in them ties; and the gate's limit is met exactly.  Everything
is integers, every comparison an equality.  The expectations are closed forms and two restatements that share nothing with the
C++: lev_np (test_cluster_gate_cpu.py) and search_np below, a numpy form of trim_cases.search_py over many texts at once."""
import contextlib
import random

import numpy as np

import trim_cases as T

BASES = "ACGT"


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def repeat(unit, n, phase=0):
    """unit repeated from `phase` to n bases."""
    return "".join(unit[(q + phase) % len(unit)] for q in range(n))


def complement(base):
    return BASES[3 - BASES.index(base)]


# ------------------------------------------------------------------------------------------------ the gate's word ladder
LADDER_LENGTHS = (1, 2, 31, 32, 33) + tuple(64 * k + d for k in range(1, 11) for d in (-1, 0, 1))
LADDER_DELTAS = (0, 1, 16, 17, 40)
LADDER_KINDS = ("homopolymers", "homopolymer/period 2", "shifted phase", "tandem duplications", "three substitutions", "unrelated")


def tandem_copy(rng, src, n):
    """src grown to n bases by tandem duplications of 1 to 3 bases."""
    s = list(src)
    while len(s) < n:
        at = rng.randrange(len(s))
        k = min(rng.randint(1, 3), at + 1, n - len(s))
        s[at + 1:at + 1] = s[at + 1 - k:at + 1]
    return "".join(s)


def _ladder_pair(rng, kind, turn, m, n):
    """-> (pattern, text, e0 or None, e1 or None): a pair of the kind, the distances where a closed form gives them."""
    b = BASES[(m + n + turn) & 3]
    other = BASES[BASES.index(b) ^ 1]
    if kind == 0:                                                       # d(A^m, A^n) = n - m, d(A^m, C^n) = n, rc(T^n) = A^n
        text_base, e0, e1 = ((b, n - m, n), (other, n, n), (complement(b), n, n - m))[turn % 3]
        return b * m, text_base * n, e0, e1
    if kind == 1:                                                       # a homopolymer against a period-2 repeat that holds its base
        return (b * m, repeat(b + other, n, m & 1), None, None) if turn % 2 else (repeat(other + b, m), b * n, None, None)
    if kind == 2:                                                       # d((AC)^k, (CA)^k) = 2
        if turn % 2:
            unit = b + other + BASES[BASES.index(b) ^ 2]
            return repeat(unit, m), repeat(unit, n, 1 + (m & 1)), None, None
        return repeat(b + other, m), repeat(b + other, n, 1), 2 if m == n and m % 2 == 0 else None, None
    src = _rand(rng, m)
    if kind == 3:
        return src, tandem_copy(rng, src, n), 0 if m == n else None, None
    if kind == 4:
        s = list(src + _rand(rng, n - m))
        for _ in range(3):
            at = rng.randrange(len(s))
            s[at] = rng.choice([x for x in BASES if x != s[at]])
        return src, "".join(s), None, None
    return src, _rand(rng, n), None, None


def gate_ladder():
    """-> (reads, pairs, closed, kinds): 35 pattern lengths x 5 deltas x 6 kinds = 1050 pairs, shuffled so that a wave of 64 mixes
    every word count, every other pair with the longer read first (the kernels take the shorter read as the pattern);
    closed[q] = (e0 or None, e1 or None), kinds[q] the kind of pair q."""
    rng = random.Random("bitvector/gate-ladder")
    cases, turn = [], 0
    for m in LADDER_LENGTHS:
        for d in LADDER_DELTAS:
            for kind in range(len(LADDER_KINDS)):
                cases.append((kind,) + _ladder_pair(rng, kind, turn, m, m + d))
            turn += 1                                                   # the variants of a kind take turns over (m, d)
    rng.shuffle(cases)
    reads, pairs, closed, kinds = [], [], [], []
    for q, (kind, pat, txt, e0, e1) in enumerate(cases):
        reads += [pat, txt]
        pairs.append((len(reads) - 2, len(reads) - 1) if q % 2 == 0 else (len(reads) - 1, len(reads) - 2))
        closed.append((e0, e1))
        kinds.append(kind)
    assert len(pairs) == 1050 and len(pairs) % 64 != 0
    return reads, pairs, closed, kinds


def pattern_words(reads, pair):
    return (min(len(reads[pair[0]]), len(reads[pair[1]])) + 63) // 64


def check_closed(dist, closed):
    """The closed forms of a ladder against int32[C, 2] -> how many were checked."""
    n = 0
    for q, (e0, e1) in enumerate(closed):
        for got, want in ((dist[q][0], e0), (dist[q][1], e1)):
            if want is not None:
                assert int(got) == want, (q, int(got), want)
                n += 1
    return n


# ------------------------------------------------------------------------------------------------ the gate at its limit
LIMIT_PERMILLE = 100


def limit_pool():
    """-> 69 reads: A^n and T^n for n = 90 .. 110, C^n and G^n for every other n, five random reads of 100 nt, shuffled."""
    rng = random.Random("bitvector/gate-limit")
    reads = [base * n for n in range(90, 111) for base in "AT"] + [base * n for n in range(90, 111, 2) for base in "CG"]
    reads += [_rand(rng, 100) for _ in range(5)]
    rng.shuffle(reads)
    assert len(reads) == 69
    return reads


def is_homopolymer(read):
    return len(set(read)) == 1


def limit_edits(reads, lev):
    """{(i, j): (e0, e1)} for i < j.  d(x^a, r) = max(a, |r|) - min(a, the x's in r): the a bases can be matched to that many of
    r's, the rest of the longer sequence is substituted or indels.  Two reads of more than one base each go to lev."""
    def one(a, b):
        if is_homopolymer(b):
            a, b = b, a
        if is_homopolymer(a):
            return max(len(a), len(b)) - min(len(a), b.count(a[0]))
        return lev(a, b)
    return {(i, j): (one(reads[i], reads[j]), one(reads[i], T.rc(reads[j]))) for i in range(len(reads)) for j in range(i + 1, len(reads))}


def limit_counts(reads, edits, permille):
    """tested, passed, word_steps of the gate, and how many pairs sit at the limit and one above it."""
    limit = lambda i, j: permille * max(len(reads[i]), len(reads[j])) // 1000
    words = lambda i, j: (min(len(reads[i]), len(reads[j])) + 63) // 64
    return dict(tested=len(edits), passed=sum(min(e) <= limit(*c) for c, e in edits.items()),
                word_steps=sum(2 * words(i, j) * max(len(reads[i]), len(reads[j])) for i, j in edits),
                at=sum(min(e) == limit(*c) for c, e in edits.items()), above=sum(min(e) == limit(*c) + 1 for c, e in edits.items()))


# ------------------------------------------------------------------------------------------------ the trim length ladder
def primer_of_kind(rng, kind, m):
    """-> (primer of m bases, the repeat unit a read around it is made of): random, a homopolymer, period 2, period 3, period 2
    with one odd base."""
    b = rng.randrange(4)
    if kind == 0:
        return _rand(rng, m), _rand(rng, 3)
    unit = (BASES[b], BASES[b] + BASES[b ^ 1], BASES[b] + BASES[b ^ 2] + BASES[b ^ 3], BASES[b] + BASES[b ^ 1])[kind - 1]
    p = repeat(unit, m)
    if kind == 4:
        p = p[:m // 2] + BASES[b ^ 2] + p[m // 2 + 1:]
    return p, unit


def trim_ladder():
    """-> (primers, reads): 64 pairs, pair k with an F of k + 1 and an R of 64 - k bases (every length is an F and an R once, the
    two windows of a pair differ everywhere but in the middle), the kinds of primer_of_kind in rotation; 130 reads, shuffled:
    for every fourth pair junk of 0, 8 and 9 bases either side of F . payload . R, the payload of 10 to 40 bases random or of
    F's own repeat unit; for the pairs in between one read; reads of 0, 1, 31 .. 33 and 63 .. 65 bases; two unrelated ones.
    Every other planted read is reverse-complemented."""
    rng = random.Random("bitvector/trim-ladder")
    primers, units = [], []
    for k in range(64):
        F, unit = primer_of_kind(rng, k % 5, k + 1)
        R, _ = primer_of_kind(rng, (k + 2) % 5, 64 - k)
        primers.append((F, R))
        units.append(unit)
    reads = []

    def plant(k, junk, own):
        F, R = primers[k]
        fill = (lambda n: repeat(units[k], n, rng.randrange(3))) if own else (lambda n: _rand(rng, n))
        read = fill(junk) + F + fill(rng.randint(10, 40)) + R + fill(junk)
        reads.append(T.rc(read) if len(reads) % 2 else read)

    for k in range(0, 64, 4):
        for junk in (0, 8, 9):
            plant(k, junk, False)
            plant(k, junk, True)
    for k in range(2, 64, 4):
        plant(k, (0, 8, 9)[k // 4 % 3], k % 8 == 2)
    for n in (0, 1, 31, 32, 33, 63, 64, 65):
        reads += [repeat("AC", n), _rand(rng, n)]
    reads += [_rand(rng, 50), _rand(rng, 80)]
    rng.shuffle(reads)
    assert len(primers) == 64 and len(reads) == 130
    return primers, reads


def trim_columns(primers, reads, max_offset):
    """stats["columns"] of a call, from trimWindow."""
    window = lambda m, n: n if max_offset < 0 else min(n, m + max_offset)
    return sum(2 * (window(len(F), len(r)) + window(len(R), len(r))) for r in reads for F, R in primers)


# ------------------------------------------------------------------------------------------------ search_py over many texts
def search_np(p, texts, max_offset):
    """trim_cases.search_py(p, t, max_offset) for every t of texts -> [(e, c)]: the matrix row by row over all texts at once
    (padded with a base that matches nothing; a column depends on the columns before it alone), the insertions of a row by
    minimum.accumulate."""
    m = len(p)
    w = np.array([len(t) if max_offset < 0 else min(len(t), m + max_offset) for t in texts])
    width = int(w.max()) if len(texts) else 0
    txt = np.full((len(texts), width), 255, dtype=np.uint8)
    for i, t in enumerate(texts):
        txt[i, :w[i]] = np.frombuffer(t[:w[i]].encode(), dtype=np.uint8)
    at = np.arange(width + 1)
    row = np.zeros((len(texts), width + 1), dtype=np.int64)             # D[0][c] = 0
    for r, x in enumerate(p.encode(), 1):
        new = np.empty_like(row)
        new[:, 0] = r
        new[:, 1:] = np.minimum(row[:, :-1] + (txt != x), row[:, 1:] + 1)
        row = np.minimum.accumulate(new - at, axis=1) + at
    out = []
    for i in range(len(texts)):
        last = row[i, :w[i] + 1]
        e = int(last.min())
        out.append((e, int(np.flatnonzero(last == e)[-1])))
    return out


@contextlib.contextmanager
def searches_of(primers, reads, max_offset):
    """Within the block trim_cases.trim_py looks its searches up in a table that search_np filled for these primers and reads."""
    texts = sorted({t for r in reads for v in (r, T.rc(r)) for t in (v, v[::-1])})
    table = {}
    for p in sorted({p for F, R in primers for p in (F, R[::-1])}):
        for t, hit in zip(texts, search_np(p, texts, max_offset)):
            table[p, t] = hit

    def lookup(p, t, offset):
        assert offset == max_offset
        return table[p, t]
    kept = T.search_py
    T.search_py = lookup
    try:
        yield table
    finally:
        T.search_py = kept
