"""Alignment pairs that sit on the routing thresholds of the forward-backward E-step (test infrastructure, shared by
tests/test_fb_census_cpu.py, which proves on the CPU that each construction hits what it claims, and
tests/test_gpu_fwdback_edges.py, which runs them).

Every pair is written as two gapped rows and goes through oracle.alignment_pair like a pair read from a Stockholm file.
One shape serves all families: n input bases copied to the output, and at one place -- after input base number `at` --
`ins` inserted output bases (tandem copies of the bases before them, which the duplication lanes explain) followed by a block
of `dele` deleted input bases.  The inserted bases widen the envelope rows around them by `ins` cells; the deleted block makes
dele + 1 rows share their bounds, which is what the half-width condition hi(ip) - lo(ip + W) < W is about."""
import random

import fb_census as C
from oracle import oracle as O

BASES = "ACGT"


def gapped_rows(rng, n, at=1, ins=0, dele=0, unit=1, sub=0.0, single_dels=()):
    """n random input bases; after input base number `at` (1 <= at <= n) `ins` output-only columns, then input bases
    at + 1 .. at + dele deleted; the input bases numbered in single_dels deleted one by one; matched bases substituted with
    probability sub (the guide stays what it is)."""
    assert 1 <= at and at + dele <= n
    src = "".join(rng.choice(BASES) for _ in range(n))
    r1, r2 = [], []
    for i in range(1, n + 1):
        c = src[i - 1]
        gone = at < i <= at + dele or i in single_dels
        if not gone and rng.random() < sub:
            c = rng.choice([b for b in BASES if b != c])
        r1.append(src[i - 1]); r2.append("-" if gone else c)
        if i == at and ins:
            u = min(unit, at)
            r = ins % u
            copies = (src[at - r:at] if r else "") + src[at - u:at] * (ins // u)       # whole copies of the last u bases, a shorter one first
            assert len(copies) == ins
            r1.append("-" * ins); r2.append(copies)
    return [("in", "".join(r1)), ("out", "".join(r2))]


def make(rng, n, **kw):
    return O.alignment_pair(gapped_rows(rng, n, **kw))


def place(where, n, dele=0):
    """`at` for the three places a feature is put: at the first match (rows ip < W), in the middle, and so that the wide row is
    the last one / the deleted block ends at ip = I."""
    return {"first": 1, "middle": n // 2, "last": n - dele}[where]


PLACES = ("first", "middle", "last")

# ---- (a) the widest row at 16 | 17 and 32 | 33
WIDTHS = (16, 17, 32, 33)
WIDTH_SETTINGS = (("strict", 6, True), ("P3", 3, False), ("P6", 6, False), ("P8", 8, False))      # name, P, strict guides


def width_k(P, strict, where, width, n=120):
    """How many inserted output bases make `width` the widest envelope row (None: no number does).  Strict guides: a row holds the
    cells of one match count, k + 1 of them; loose guides: those of 2P + 1 match counts, k + 2P + 1."""
    for k in range(0, 40):
        if C.census(make(random.Random(0), n, at=place(where, n), ins=k, unit=P), 0 if strict else P)["width"] == width:
            return k
    return None


def width_database(seed, P, where, k, n_pairs):
    """n_pairs pairs of 113 .. 127 bases with k inserted bases at `where`, every pair of other bases."""
    rng = random.Random("width/%s" % (seed,))
    out = []
    for _ in range(n_pairs):
        n = rng.randint(113, 127)
        out.append(make(rng, n, at=place(where, n), ins=k, unit=P, sub=.03))
    return out


# ---- (b) the half-width conditions at equality: name, P, strict, inserted bases before the block, W
HALF_SETTINGS = (("P6", 6, False, 0, 8), ("P7", 7, False, 0, 8), ("P8", 8, False, 0, 16), ("strict+10", 6, True, 10, 8),
                 ("strict+20/8", 6, True, 20, 8), ("strict+20/16", 6, True, 20, 16), ("P3+14/8", 3, False, 14, 8),
                 ("P3+14/16", 3, False, 14, 16))


def half_place(where, n, d, W):
    """The deleted block behind one of the first full-width rows (ip < W), in the middle, or so that it ends at ip = I."""
    return {"first": 7 if W == 8 else 9, "middle": n // 2, "last": n - d}[where]


def half_pair(rng, n, P, ins, where, d, W, sub=0.0):
    return make(rng, n, at=half_place(where, n, d, W), ins=ins, dele=d, unit=P, sub=sub)


def half_margin(P, strict, ins, W, where, d, n=120):
    return C.census(half_pair(random.Random(0), n, P, ins, where, d, W), 0 if strict else P)["margin%d" % W]


def half_flip(P, strict, ins, W, where):
    """The shortest deleted block with which hi(ip) - lo(ip + W) reaches W somewhere (None: no block of up to 40 bases does)."""
    for d in range(1, 41):
        if half_margin(P, strict, ins, W, where, d) >= W:
            return d
    return None


def half_cases():
    """[dict(id, P, strict, ins, W, where, d, side)], side 0: the half-width condition holds, 1: it does not.  The settings above
    with the block one base short of the flip and at it; and, under strict guides, where a block of W deleted bases makes W + 1
    rows of ins + 1 cells share their bounds (hi(ip) - lo(ip + W) = ins), ins = W - 1 and W.  Without inserted bases the difference
    grows by one per deleted base, and the two sides are W - 1 and W; inserted bases come into a row's reach all at once."""
    out = []
    for name, P, strict, ins, W in HALF_SETTINGS:
        for where in PLACES:
            d = half_flip(P, strict, ins, W, where)
            if d is None:
                continue
            for side in (0, 1):
                out.append(dict(id="%s-%s-d%d" % (name, where, d - 1 + side), P=P, strict=strict, ins=ins, W=W, where=where,
                                d=d - 1 + side, side=side, exact=ins == 0))
    for W in (8, 16):
        for where in PLACES:
            for side in (0, 1):
                out.append(dict(id="strict=%d-%s-ins%d" % (W, where, W - 1 + side), P=6, strict=True, ins=W - 1 + side, W=W,
                                where=where, d=W, side=side, exact=True))
    return out


def half_database(case, n_pairs=3):
    rng = random.Random("half/" + case["id"])
    return [half_pair(rng, rng.randint(113, 127), case["P"], case["ins"], case["where"], case["d"], case["W"], sub=.03)
            for _ in range(n_pairs)]


# ---- (c), (d): one family per on-chip kernel at P = 3 (width 7, 13, 21, 21; the deleted block takes the half-width kernel away),
# and the same at P = 8 for the 32-lane kernel (width 31)
KIND_P = 3
KIND_FAMILY = (dict(ins=0, dele=0), dict(ins=6, dele=6), dict(ins=14, dele=0), dict(ins=14, dele=14))


def kind_pair(rng, kind, n, P=KIND_P, at=None, single_dels=(), sub=.03):
    f = KIND_FAMILY[kind]
    at = at if at is not None else max(1, (n - f["dele"]) // 2)
    return make(rng, n, at=at, ins=f["ins"], dele=f["dele"], unit=P, sub=sub, single_dels=single_dels)


def short_kind_pairs(seed, kind, n_pairs, P=KIND_P):
    """Pairs of about 24 bases of one kind: the feature after base 3 .. 5, 7 .. 10 matched bases behind it."""
    rng = random.Random("short/%s/%d" % (seed, kind))
    f = KIND_FAMILY[kind]
    out = []
    for _ in range(n_pairs):
        at = rng.randint(3, 5)
        n = at + f["dele"] + rng.randint(7, 10) + (10 if not f["dele"] else 0)
        out.append(make(rng, n, at=at, ins=f["ins"], dele=f["dele"], unit=P, sub=.1))
    return out


def persistent_database(kind, cus, P=KIND_P):
    """One pair more than a launch of the kind's kernel holds at once on `cus` compute units: the first wave goes round its
    persistent loop a second time, with one live slot and the others dead."""
    return short_kind_pairs("persistent/%d" % P, kind, cus * C.WAVES_PER_CU * C.PPG[kind] + 1, P)


def lds_databases(kind):
    """[(inLen of the long pair, pairs)]: a pair of the kind's family with inLen = longest - 63, longest and longest + 1, each beside
    two short pairs of the kind (so each is the longest of its list, or streams)."""
    L = C.LONGEST[kind]
    out = []
    for n in (L - 63, L, L + 1):
        rng = random.Random("lds/%d/%d" % (kind, n))
        out.append((n, [kind_pair(rng, kind, n)] + short_kind_pairs("lds%d" % n, kind, 2)))
    return out


def mixed_database():
    """Per on-chip kernel: pair A with the longest input the kernel takes and 150 of its bases deleted one by one (a shorter
    output: fewer wavefront steps) and pair B with an input 64 bases shorter and nothing deleted (more steps), so that in each
    list maxInOnchip and maxSteps come from different pairs.  (steps = I + hi(I) - lo(0) + 1 <= I + O + 1: no 8-base pair that an
    on-chip kernel takes can have the most steps beside these, so the pair with the most steps is the shorter LONG one.)  Beside
    them short pairs that leave dead slots: plain 8-base pairs (the 8-lane list), 8-base pairs with a last row of 20 cells (the
    half-width 16-lane list) and one short pair each for the two full-width lists."""
    rng = random.Random("mixed")
    out = []
    for kind in range(4):
        L = C.LONGEST[kind]
        out.append(kind_pair(rng, kind, L, single_dels=set(range(40, 40 + 150 * 9, 9))))
        out.append(kind_pair(rng, kind, L - 64))
        out.append(make(rng, 8, at=8, ins=16, unit=KIND_P, sub=.1))
        out.append(make(rng, 8, sub=.1))
    out += short_kind_pairs("mixed", 1, 1) + short_kind_pairs("mixed", 3, 1)
    return out


# ---- (e) pairs of 1 .. 4 bases, neighbours never alike
def tiny_pairs(n_pairs, seed="tiny"):
    rng = random.Random(seed)
    out, last = [], None
    while len(out) < n_pairs:
        n = rng.randint(1, 4)
        r = rng.random()
        at = rng.randint(1, n)
        if r < .15 and n >= 2:
            rows = gapped_rows(rng, n, at=min(at, n - 1), dele=1, sub=.2)          # one base deleted (never the only one)
        elif r < .3:
            rows = gapped_rows(rng, n, at=at, ins=rng.randint(1, 2), unit=2, sub=.2)   # a tandem copy of one or two bases
        else:
            rows = gapped_rows(rng, n, sub=.3)
        if rows == last:
            continue
        last = rows
        out.append(O.alignment_pair(rows))
    return out


# ---- (f) the length limit and the pairs without bases
def long_pair(n_in, n_out, seed="long"):
    """A pair with n_in input and n_out output bases, |n_in - n_out| <= 1: the difference is one deleted / one copied base."""
    rng = random.Random("%s/%d/%d" % (seed, n_in, n_out))
    if n_out == n_in - 1:
        return make(rng, n_in, at=n_in // 3, dele=1, sub=.02)
    assert n_out in (n_in, n_in + 1)
    return make(rng, n_in, at=n_in // 3, ins=n_out - n_in, sub=.02)


def all_deleted_pair(n=5):
    return O.alignment_pair([("in", "ACGTA"[:n]), ("out", "-" * n)])


def empty_pair():
    return O.alignment_pair([("in", ""), ("out", "")])
