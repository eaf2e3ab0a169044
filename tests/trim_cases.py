"""What the tests of dnas_trim_reads share (test_trim_cpu.py, test_gpu_trim.py): the definition of include/dnastore_amd.h restated
in pure Python over the full matrix of the dynamic program -- it shares nothing with the C++ --, the shape pool, and the planted
pool with its three conditions."""
import functools
import random

import numpy as np

BASES = "ACGT"
FIELDS = ("pair", "strand", "begin", "end", "edits", "second", "status")


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def edited(rng, src, n_edits):
    """A read: the original after up to n_edits substitutions, deletions of 1-2 bases and tandem copies of 1-3 bases."""
    s = list(src)
    for _ in range(n_edits):
        kind = rng.choice("sdt")
        if kind == "s" and s:
            at = rng.randrange(len(s))
            s[at] = rng.choice([b for b in BASES if b != s[at]])
        elif kind == "d" and s:
            at = rng.randrange(len(s))
            del s[at:at + rng.randint(1, 2)]
        elif kind == "t" and s:
            at = rng.randrange(len(s))
            k = rng.randint(1, min(3, at + 1))
            s[at + 1:at + 1] = s[at + 1 - k:at + 1]
    return "".join(s)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def lev(a, b):
    """The Levenshtein distance of two strings (a measure for the planted pool, not part of the definition)."""
    b = np.frombuffer(b.encode(), dtype=np.uint8)
    at = np.arange(len(b) + 1)
    row = at.copy()
    for i, x in enumerate(a.encode(), 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[:-1] + (b != x), row[1:] + 1)
        row = np.minimum.accumulate(new - at) + at
    return int(row[-1])


# ------------------------------------------------------------------------------------------------ the definition, restated
@functools.lru_cache(maxsize=None)
def search_py(p, t, max_offset):
    """search(p, t) = (e, c): the smallest D[m][c] over c = 0 .. w and the largest column that attains it."""
    m = len(p)
    w = len(t) if max_offset < 0 else min(len(t), m + max_offset)
    D = [[0] * (w + 1) for _ in range(m + 1)]
    for r in range(1, m + 1):
        D[r][0] = r
        above, here, x = D[r - 1], D[r], p[r - 1]
        for c in range(1, w + 1):
            here[c] = min(above[c - 1] + (x != t[c - 1]), above[c] + 1, here[c - 1] + 1)
    e = min(D[m])
    return e, max(c for c in range(w + 1) if D[m][c] == e)


def trim_py(primers, read, max_offset=8, permille=250, anchors="both", min_payload=0):
    """One read -> (pair, strand, begin, end, (eF, eR), second, status)."""
    n = len(read)
    accepted, anchored = [], False
    for k, (F, R) in enumerate(primers):
        lim_f, lim_r = permille * len(F) // 1000, permille * len(R) // 1000
        for s in (0, 1):
            v = rc(read) if s else read
            e_f, c_f = search_py(F, v, max_offset)
            e_r, c_r = search_py(R[::-1], v[::-1], max_offset)
            in_f, in_r = e_f <= lim_f, e_r <= lim_r
            if not ((in_f and in_r) if anchors == "both" else (in_f or in_r)):
                continue
            anchored = True
            total = 0
            if in_f:
                total += e_f
            else:
                e_f, c_f, total = -1, 0, total + lim_f + 1
            if in_r:
                total += e_r
            else:
                e_r, c_r, total = -1, 0, total + lim_r + 1
            if c_f + c_r + min_payload <= n:
                accepted.append((total, k, s, e_f, e_r, c_f, c_r))
    if not accepted:
        return -1, 0, 0, 0, (-1, -1), -1, 2 if anchored else 1
    total, k, s, e_f, e_r, c_f, c_r = min(accepted)
    others = [a[0] for a in accepted if a[1] != k]
    begin, end = (c_r, n - c_f) if s else (c_f, n - c_r)
    return k, s, begin, end, (e_f, e_r), min(others) if others else -1, 0


def trim_pool_py(primers, reads, **options):
    """-> the arrays of TrimmedReads, by name."""
    rows = [trim_py(primers, r, **options) for r in reads]
    out = {f: np.array([row[i] for row in rows], dtype=np.int64) for i, f in enumerate(FIELDS)}
    out["edits"] = out["edits"].reshape(len(reads), 2)
    return out


def arrays(trimmed):
    return {f: np.asarray(getattr(trimmed, f), dtype=np.int64) for f in FIELDS}


def assert_same(got, want, what=""):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero((got[f] != want[f]).reshape(len(want["pair"]), -1).any(axis=1))[:8])


def payload_py(read, row):
    """The oriented payload of a read from its outputs (None when it was not trimmed)."""
    k, s, begin, end = row[:4]
    if k < 0:
        return None
    return rc(read[begin:end]) if s else read[begin:end]


# ------------------------------------------------------------------------------------------------ the shape pool
def shape_pool():
    """-> (primers, reads).  Seven pairs: primers of 1, 2, 20, 63 and 64 bases, and of 7, 8, 9, 24 and 25, whose windows at
    max_offset = 8 have 15, 16, 17, 32 and 33 columns (the boundaries of the packed 16-base groups); pair 3 repeats pair 0 (the tie
    goes to the smaller k) and pair 4 has R = rc(F) (the strand tie goes to strand 0).  The short pairs come last, so that the
    long ones win their own exact reads."""
    rng = random.Random("trim/shapes")
    f0 = _rand(rng, 20)
    r0 = f0[-3:] + _rand(rng, 17)                                       # F and R can overlap by 3
    p24 = _rand(rng, 24)
    primers = [(f0, r0), (_rand(rng, 63), _rand(rng, 64)), (_rand(rng, 7), _rand(rng, 8)), (f0, r0), (p24, rc(p24)),
               (_rand(rng, 9), _rand(rng, 25)), ("G", "TC")]
    reads = ["", "A", f0, f0 + r0, f0 + r0[3:]]
    for k in (0, 1, 2, 4, 5):
        F, R = primers[k]
        for junk in (0, 5, 9):                                          # 9 is beyond max_offset = 8: found only with -1
            reads.append(_rand(rng, junk) + F + _rand(rng, 30) + R + _rand(rng, junk))
        reads.append(_rand(rng, 3) + edited(rng, F, 2) + _rand(rng, 30) + edited(rng, R, 2) + _rand(rng, 2))
    reads.append(f0 + f0 + _rand(rng, 30) + r0)                         # F twice, exactly: the later end wins
    reads.append(_rand(rng, 4) + f0 + _rand(rng, 40))                   # no R: accepted under `either` only
    reads.append(_rand(rng, 40) + r0 + _rand(rng, 2))                   # no F
    for n in (63, 64, 65, 130):                                         # read lengths
        reads.append(f0 + _rand(rng, n - 40) + r0)
    for n in (15, 16, 17, 32, 33, 70, 71, 72):                          # windows clipped by n
        F, R = primers[1]
        reads.append((F + R)[:n])
    reads += [rc(r) for r in reads]
    reads += [_rand(rng, 50), _rand(rng, 80)]                           # unrelated
    return primers, reads


# ------------------------------------------------------------------------------------------------ the planted pool
def planted_pool(seed="trim/planted", n_reads=160):
    """-> (primers, reads, truth): 8 pairs of 20-nt primers at least 8 edits apart (from each other, each other's reverse
    complements and their own), read i planted from pair i % 8 with up to 2 edits per primer, 4 in the payload and up to 5 junk
    bases either side, reverse-complemented when (i // 8) % 2.  truth[i] = (k, strand, payload)."""
    rng = random.Random(seed)
    kept = []
    while len(kept) < 16:
        p = _rand(rng, 20)
        if lev(p, rc(p)) >= 8 and all(lev(p, q) >= 8 and lev(p, rc(q)) >= 8 for q in kept):
            kept.append(p)
    primers = [(kept[2 * k], kept[2 * k + 1]) for k in range(8)]
    reads, truth = [], []
    for i in range(n_reads):
        k = i % 8
        F, R = primers[k]
        pay = edited(rng, _rand(rng, rng.randint(100, 120)), 4)
        read = _rand(rng, rng.randint(0, 5))
        read += edited(rng, F, rng.randint(0, 2))
        read += pay
        read += edited(rng, R, rng.randint(0, 2))
        read += _rand(rng, rng.randint(0, 5))
        s = (i // 8) % 2
        reads.append(rc(read) if s else read)
        truth.append((k, s, pay))
    return primers, reads, truth


def planted_conditions(reads, truth, got):
    """The three conditions on a trim of the planted pool with max_offset = 8, 250 permille, both anchors, min_payload = 0; the
    figures are returned after they were asserted."""
    accepted = [i for i in range(len(reads)) if got["status"][i] == 0]
    wrong = [i for i in accepted if (got["pair"][i], got["strand"][i]) != truth[i][:2]]
    dist = [lev(payload_py(reads[i], [int(got[f][i]) for f in FIELDS[:4]]), truth[i][2]) for i in accepted]
    print("planted pool: %d of %d accepted, %d wrong, worst payload distance %d" % (len(accepted), len(reads), len(wrong), max(dist)))
    assert not wrong, wrong
    assert len(accepted) >= 157, len(accepted)
    assert max(dist) <= 6, max(dist)
    return len(accepted), max(dist)
