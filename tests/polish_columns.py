"""Inputs for dnas_cluster_consensus whose columns are planted, and a census of the columns an input holds (test
infrastructure: tests/test_polish_columns_cpu.py checks on the CPU that the pools hold every kind of column the census knows,
tests/test_gpu_polish_columns.py holds the kernels of csrc/polish_kernels.hip to the host statement on them).

The census is the definition of include/dnastore_amd.h as tests/test_polish_cpu.py restates it (consensus_py, vote_and_emit),
counting on the way.  Its kinds, all counted over the rounds a call runs:

  ins             insertion bases emitted (2 N[g][k] > V)
  ins_even_V      ... by an even number of voters
  ins_V_gt_64     ... by more voters than a wave has lanes
  ins_k3          ... as the fourth base of a gap (k = 3)
  ins_gap_I       ... at the gap after the template's last base
  ins_chunk_edge  ... at a gap = 63 or 0 mod 64: the last or the first lane of a chunk of the device's emit
  ins_B_tie       ... where two codes share the maximum of B[g][k][.]
  ins_four_gaps   gaps that emit insertions as the three gaps before them do: neighbouring lanes each add bases to the scan
  long_runs       runs of more than DNAS_POLISH_MAX_INSERT duplication columns at a gap that emits an insertion
  del             template bases dropped (2 D[g] > V)
  del_V_gt_64     ... by more than 64 voters
  del_chunk_edge  ... at a base = 63 or 0 mod 64
  del_tail_only   rounds of a cluster whose new template is a proper prefix of the old: only trailing bases go, so no base the
                  emit writes differs from the old template and the new length alone says that it changed
  tie_2N_eq_V     gaps where the insertion stops at 2 N[g][k] == V
  tie_2D_eq_V     bases kept at 2 D[g] == V
  M_tie_excl      bases whose maximum of M[g][.] is shared and excludes the template's base
  changed_round2  clusters whose template changes in a second round
  changed_round3  ... in a third round
  cross_up        clusters whose template had at most `limit` bases before a round and more after it
  cross_down      ... more than `limit` before and at most `limit` after"""
import collections
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from fb_census import _one  # noqa: E402
from test_assign_cpu import _rand  # noqa: E402
from test_polish_cpu import BASES, MAX_INSERT, consensus_py, revcomp  # noqa: E402

KINDS = ("ins", "ins_even_V", "ins_V_gt_64", "ins_k3", "ins_gap_I", "ins_chunk_edge", "ins_B_tie", "ins_four_gaps", "long_runs", "del", "del_V_gt_64",
         "del_chunk_edge", "del_tail_only", "tie_2N_eq_V", "tie_2D_eq_V", "M_tie_excl", "changed_round2", "changed_round3", "cross_up", "cross_down")

# ---- the constants of the source, read from it: a change there moves the shapes of the tests with it
LDS_POSITIONS = int(_one("polish_kernels.hip", r"^\s*constexpr\s+int\s+kPolishLdsPositions\s*=\s*(\d+)\s*;",
                         "'constexpr int kPolishLdsPositions = <integer>;'"))
ROW_WORDS = int(_one("host/polish.hpp", r"^\s*constexpr\s+int\s+kPolishRow\s*=\s*(\d+)\s*;", "'constexpr int kPolishRow = <integer>;'"))
assert MAX_INSERT == int(_one("../../include/dnastore_amd.h", r"^#define\s+DNAS_POLISH_MAX_INSERT\s+(\d+)\b", "'#define DNAS_POLISH_MAX_INSERT <integer>'"))
LDS_LIMIT_BYTES = 64 * 1024                                   # what a work-group may ask for
LDS_TABLE_BYTES = 4 * (1 + ROW_WORDS * (LDS_POSITIONS + 1))    # the table of a template at the cap: V and a row per position 0 .. I
assert LDS_TABLE_BYTES <= LDS_LIMIT_BYTES, (LDS_POSITIONS, ROW_WORDS)
SMALL_CAP = 64                                                # DNAS_POLISH_LDS_POSITIONS of the mixed-route runs


# ---- planting
def other(base, step=1):
    return BASES[(BASES.index(base) + step) % 4]


def plant(truth, edits):
    """truth after edits, each placed in truth's coordinates: ("t", g, n) a tandem copy of the n bases before gap g, at gap g;
    ("d", p, n) bases p .. p + n - 1 deleted; ("s", p, step) base p substituted; ("h", g, n) n copies of the base before gap g."""
    s = list(truth)
    for kind, at, n in sorted(edits, key=lambda e: -e[1]):
        if kind == "t":
            assert n <= at <= len(truth)
            s[at:at] = truth[at - n:at]
        elif kind == "h":
            assert 1 <= at <= len(truth)
            s[at:at] = truth[at - 1] * n
        elif kind == "d":
            assert at + n <= len(truth)
            del s[at:at + n]
        else:
            s[at] = other(truth[at], n)
    return "".join(s)


def no_repeats(rng, n):
    """n random bases, none equal to the one before it: a planted copy or deletion then has one place it can stand."""
    s = []
    while len(s) < n:
        b = rng.choice(BASES)
        if not s or b != s[-1]:
            s.append(b)
    return "".join(s)


def _cluster(truth, V, edits, template=None):
    """V reads of truth: read i carries every edit (share, edit) with i < share(V)."""
    reads = [plant(truth, [e for share, e in edits if i < share(V)]) for i in range(V)]
    return truth if template is None else template, reads


ALL = lambda V: V
MOST = lambda V: V // 2 + 1
HALF = lambda V: V // 2                                       # a tie where V is even, a minority where it is odd


def planted_pool(da):
    """-> (templates, reads, read_strand): clusters of 0 to 6 and of 65 to 70 reads on templates of 0 to 130 nt.  Tandem copies
    of 1, 2, 4 and 6 bases at gaps 6, 12, 63, 64, 65, 127, 128 and I and deletions of 1-2 bases at 3, 62, 63, 64 and 126, each in
    all, a majority or half of a cluster's reads; the clusters made for one kind of column are named where they are built.
    Every other read is given reverse-complemented."""
    rng = random.Random("polish/planted-columns")
    sets = (((MOST, ("t", 6, 1)), (ALL, ("t", 63, 2)), (HALF, ("t", 127, 1)), (MOST, ("d", 3, 1)), (HALF, ("d", 100, 1)), (ALL, ("t", -1, 4))),
            ((ALL, ("t", 12, 2)), (MOST, ("t", 64, 1)), (MOST, ("t", 128, 6)), (MOST, ("d", 62, 2)), (ALL, ("d", 126, 1)), (HALF, ("t", 40, 2))),
            ((MOST, ("t", 12, 4)), (ALL, ("t", 65, 6)), (MOST, ("t", -1, 1)), (ALL, ("d", 3, 2)), (MOST, ("d", 64, 1)), (HALF, ("d", 30, 1))),
            ((ALL, ("t", 6, 6)), (MOST, ("t", 64, 4)), (ALL, ("t", 127, 2)), (MOST, ("d", 63, 1)), (HALF, ("t", 20, 1)), (MOST, ("t", -1, 2))))
    clusters = []
    for n in (20, 66, 130):
        for V in (2, 3, 4, 5):
            truth = no_repeats(rng, n)
            mine = sets[(V + n // 20) % 4]
            edits = [(share, (k, n if at < 0 else at, m)) for share, (k, at, m) in mine if (n if at < 0 else at) + (m if k == "d" else 0) <= n]
            clusters.append(_cluster(truth, V, edits))
    # a tie in B at an emitted base: all of an even V insert the same copy, half of them with one of its bases substituted by a
    # base that neither neighbour has
    for V, n, g, k, j in ((4, 40, 12, 2, 0), (2, 30, 9, 1, 0), (4, 50, 20, 4, 1), (6, 36, 36, 2, 1), (4, 28, 14, 1, 0)):
        truth = no_repeats(rng, n)
        t, reads = _cluster(truth, V, [(ALL, ("t", g, k))])
        at = g + j                                            # base j of the copy
        for i in range(1, V, 2):
            assert reads[i][at] == truth[g - k + j]
            new = [b for b in BASES if b not in (reads[i][at - 1], reads[i][at], reads[i][at + 1:at + 2])][0]
            reads[i] = reads[i][:at] + new + reads[i][at + 1:]
        clusters.append((t, reads))
    # 2 D > V and 2 N > V with more voters than a wave has lanes: 36 of 70 reads of 20 nt delete a base, 33 of 65 insert one
    clusters.append(_cluster(no_repeats(rng, 20), 70, [(lambda V: 36, ("d", 10, 1))]))
    clusters.append(_cluster(no_repeats(rng, 20), 65, [(lambda V: 33, ("t", 8, 1))]))
    clusters.append(_cluster(no_repeats(rng, 24), 66, [(lambda V: 34, ("d", 5, 2)), (lambda V: 40, ("t", 16, 2))]))
    clusters.append(_cluster(no_repeats(rng, 18), 67, [(lambda V: 34, ("h", 18, 5)), (lambda V: 50, ("d", 0, 1))]))
    # ... and 2 D == V and 2 N == V there: nothing changes
    clusters.append(_cluster(no_repeats(rng, 20), 70, [(HALF, ("d", 10, 1)), (HALF, ("t", 15, 1))]))
    # a template of 2 nt whose reads all carry the copy of both bases twice: a run of 4 at gap I, 2 -> 6 bases
    clusters.append(("AC", ["ACACAC"] * 3))
    clusters.append(("GT", ["GTGTGT"] * 2))
    # four consecutive gaps that each emit insertions, across the edge of a chunk: the lanes 62 .. 65 each add more than one
    # base to the scan.  Copies of one base do it where the model has no longer duplication; a model that has explains them
    # with fewer, longer duplications and substitutions, and takes tandem copies of 2-3 bases (a tail found by search) instead.
    truth = no_repeats(rng, 70)
    clusters.append(_cluster(truth, 3, [(ALL, ("h", g, 2)) for g in (62, 63, 64, 65)]))
    truth = no_repeats(rng, 56) + "TCAGAGCTATGTCA"
    clusters.append(_cluster(truth, 5, [(ALL, ("h", 62, 3)), (ALL, ("t", 63, 2)), (ALL, ("t", 64, 2)), (ALL, ("t", 65, 3))]))
    truth = no_repeats(rng, 70)
    clusters.append(_cluster(truth, 4, [(MOST, ("h", g, 4)) for g in (63, 64, 65, 66)] + [(MOST, ("h", 70, 3))]))
    # deletions at the edges of the chunks
    clusters.append(_cluster(no_repeats(rng, 130), 3, [(ALL, ("d", 0, 1)), (MOST, ("d", 63, 2)), (MOST, ("d", 127, 2))]))
    # twelve copies of one base: a round keeps 4 bases of a run, so the template changes in several rounds -- in three where
    # the model copies one base only, 60 -> 64 -> 68 -> 72 nt, and crosses SMALL_CAP in the second
    for n, V, g in ((60, 3, 30), (30, 4, 30), (64, 2, 64), (24, 5, 7)):
        clusters.append(_cluster(no_repeats(rng, n), V, [(ALL, ("h", g, 12))]))
    # ... and crossing it downwards: 66 -> 63 nt, and 65 -> 60 nt (the template has five bases none of its reads has)
    clusters.append(_cluster(no_repeats(rng, 66), 3, [(ALL, ("d", 20, 2)), (MOST, ("d", 63, 1))]))
    truth = no_repeats(rng, 60)
    clusters.append((plant(truth, [("h", 30, 5)]), [truth] * 3))
    # M ties that exclude the template's base, 2 D == V and 2 N == V with two voters
    truth = no_repeats(rng, 33)
    clusters.append((truth, [plant(truth, [("s", 10, 1), ("d", 20, 1), ("s", 32, 2)]), plant(truth, [("s", 10, 2), ("t", 25, 1), ("s", 32, 3)])]))
    # templates far from their reads (two_round_cluster of test_polish_cpu.py, other seeds and sizes)
    from test_pair_align_cpu import edited
    for n, V in ((60, 5), (100, 4), (129, 3)):
        truth = _rand(rng, n)
        clusters.append((edited(rng, truth, 12)[:130], [edited(rng, truth, 2) for _ in range(V)]))
    # the last one or two bases missing in a majority of the reads and nothing else: the new template is a prefix of the old,
    # on either side of SMALL_CAP
    for n, V, m in ((40, 3, 1), (100, 4, 2), (64, 5, 2), (66, 3, 1)):
        clusters.append(_cluster(no_repeats(rng, n), V, [(MOST, ("d", n - m, m))]))
    # a cluster that is done at once, one without reads, one whose reads are nothing like its template, an empty template
    truth = _rand(rng, 64)
    clusters.append((truth, [truth] * 3))
    clusters.append((_rand(rng, 65), []))
    clusters.append((_rand(rng, 30), [_rand(rng, 34), _rand(rng, 27)]))
    clusters.append(("", ["", "", "A"]))
    templates = [t for t, _ in clusters]
    assert max(len(t) for t in templates) == 130 and min(len(t) for t in templates) == 0
    strands = [[i % 2 for i in range(len(rs))] for _, rs in clusters]
    reads = [[revcomp(r) if s else r for r, s in zip(rs, ss)] for (_, rs), ss in zip(clusters, strands)]
    return templates, reads, strands


def limit_pool(da):
    """-> (templates, reads, read_strand): three clusters at the cap of the LDS route, L = kPolishLdsPositions.
    0: L - 1 nt, 3 reads, two of them with a copy of one base at gap 640: grows to exactly L and stays in LDS.
    1: L nt, 4 reads, all with another last base than the template's, three with a copy of that base after it: the table's last
       two rows decide the output, the template grows past L, its second round has the table in HBM.  (The reads end Y A A, the
       template Y G, Y a pyrimidine: the copy stands at gap L, after the substituted base, where a transition is likelier than a
       transversion -- before it, it would be a copy of Y read as A.)
    2: L + 1 nt, 3 reads, two of them without base 300: the second round has the table in LDS."""
    L = LDS_POSITIONS
    rng = random.Random("polish/limit-columns")
    a, b, c = no_repeats(rng, L - 1), no_repeats(rng, L - 2) + "XA", no_repeats(rng, L + 1)
    b = b.replace("X", "T" if b[L - 3] == "C" else "C")          # ... C A or T A, the template's G for the A: see below
    edge = 64 * ((L - 2) // 64)
    clusters = [_cluster(a, 3, [(MOST, ("h", edge, 1)), (lambda V: 1, ("s", 100, 1))]),
                _cluster(b, 4, [(MOST, ("h", L, 1)), (lambda V: 1, ("s", 200, 1))], template=b[:L - 1] + "G"),
                _cluster(c, 3, [(MOST, ("d", 300, 1)), (lambda V: 1, ("s", 500, 1))])]
    templates = [t for t, _ in clusters]
    assert [len(t) for t in templates] == [L - 1, L, L + 1]
    strands = [[i % 2 for i in range(len(rs))] for _, rs in clusters]
    reads = [[revcomp(r) if s else r for r, s in zip(rs, ss)] for (_, rs), ss in zip(clusters, strands)]
    return templates, reads, strands


# ---- the census
def census(da, params, templates, reads, band, read_strand, rounds, limit=LDS_POSITIONS):
    """-> (what consensus_py returns, Counter of KINDS, per round run the list of (cluster, template length, reads) active)."""
    kinds, trace = collections.Counter({k: 0 for k in KINDS}), []
    want = consensus_py(da, params, templates, reads, band, read_strand, rounds, kinds=kinds, trace=trace, limit=limit)
    assert set(kinds) == set(KINDS)
    return want, kinds, trace


def predicted_stats(trace, cap):
    """What dnas_polish_stats counts on one device with the shipped arena, from a census's active lists; cap: the LDS route's."""
    return dict(rounds=len(trace), batches=len(trace), pairs=sum(n for r in trace for _, _, n in r),
                lds_clusters=sum(1 for r in trace for _, I, _ in r if I <= cap), hbm_clusters=sum(1 for r in trace for _, I, _ in r if I > cap))


_memo = {}


def cached(da, pool, name, params, band, rounds=4, limit=LDS_POSITIONS):
    """pool: planted_pool or limit_pool -> (its inputs, census(...), consensusReads(host=True)), computed once per process."""
    key = (pool.__name__, name, band, rounds, limit)
    if key not in _memo:
        if pool.__name__ not in _memo:
            _memo[pool.__name__] = pool(da)
        templates, reads, strands = _memo[pool.__name__]
        host = da.consensusReads(params, templates, reads, band=band, read_strand=strands, rounds=rounds, host=True)
        _memo[key] = ((templates, reads, strands), census(da, params, templates, reads, band, strands, rounds, limit), host)
    return _memo[key]
