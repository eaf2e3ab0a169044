"""Which fill kernel a machine gets: the row program of a tier-A / tier-C plan, reduced to what viterbi_tiera.hip branches on
(test infrastructure: tests/test_tiera_census_cpu.py pins the programs of every machine the suite decodes on the GPU and checks
that the shaped machines of random_machines.shaped_machine reach the others; tests/test_gpu_row_shapes.py runs those).

The kernel is compiled per machine from the plan's defines (host/plan.cpp): DNAS_T, DNAS_K, DNAS_D, DNAS_SROWS, DNAS_NCLS,
DNAS_G, DNAS_GROWS / DNAS_GSROWS, DNAS_PAIRS and one {nOut, sIdx, kind, cls, full, gOut} tuple per row (DNAS_ROWS).  All of them
are in the plan's key, which the notes of precompile() / precompile_cluster() and ViterbiDecoder.tier carry, e.g.
"T1024K4D4S0C1G1X0x0R{-1,-1,0,-1,0,0},{1,-1,1,0,0,0},...W8"; FlatModel.cluster_plan gives most of them without compiling."""
import collections
import re

import numpy as np

KEY = re.compile(r"T(\d+)K(\d+)D(\d+)S(\d+)C(\d+)G(\d+)X(\d+)x(\d+)R((?:\{-?\d+(?:,-?\d+){5}\},?)+)(?:P(\d+(?:,\d+)*))?(?:W(\d+))?")

Program = collections.namedtuple("Program", "T K D G n_s_rows ncls inbox_rows inbox_s_rows pairs_identity rows")


def parse_key(note):
    """Program of the plan key inside a precompile note or a model's tier note."""
    m = KEY.search(note)
    if not m:
        raise ValueError("no plan key in %r" % note)
    T, K, D, S, C, G, X, x = (int(v) for v in m.groups()[:8])
    rows = tuple(tuple(int(v) for v in r.split(",")) for r in re.findall(r"\{([^}]*)\}", m.group(9)))
    assert len(rows) == K, note
    pairs = tuple(int(v) for v in m.group(10).split(",")) if m.group(10) else tuple(range(K))
    return Program(T, K, D, G, S, C, X, x, pairs == tuple(range(K)), rows)


def row_program(fm, members=1, note=None):
    """Program of the plan FlatModel.cluster_plan(members) describes (members = 1: tier A).  cluster_plan has no word on the
    score classes, the S rows of the inbox and the pairing of the rows: the classes are counted as the planner counts them (0.0
    and every distinct edge score), the other two are read off the tables (the inbox cells of null edges come first and carry an
    S cell in the fold table; a state's lattice slot says which side of which cell pair its row is).  note: a precompile note of
    the same model -- its key must then say the same."""
    pl = fm.cluster_plan(members)
    a = fm.arrays()
    T, K, G = pl["T"], pl["K"], pl["G"]
    scores = {0.0} | set(a["ein_score"].tolist()) | set(a["nin_score"].tolist())
    fold = pl["fold"]
    s_cells = [int(((fold[g] != 0) & ((fold[g] >> 16) != 0xffff)).sum()) for g in range(G)] if G > 1 else [0]
    row = pl["lds_index"].astype(np.int64) // T
    slot = pl["lattice_slot"].astype(np.int64) % (K * T)
    side = (slot // (2 * T)) * 2 + (slot & 1)
    prog = Program(T, K, a["max_dup_len"], G, pl["n_s_rows"], len(scores), pl["n_inbox_rows"], max((c + T - 1) // T for c in s_cells),
                   bool((side == row).all()), tuple(tuple(int(v) for v in r) for r in pl["shapes"]))
    if note is not None:
        assert parse_key(note) == prog, (note, prog)
    return prog


def program_of_model(dec):
    """Program of the kernel a ViterbiDecoder runs (tiers A and C), from its tier note."""
    return parse_key(dec.tier)


def shape_key(row):
    """A row tuple reduced to the classes the kernel distinguishes: ("empty" | "out0" | "out+", "S" | "-", "k0" | "k1" | "k2",
    "c-" | "c0" | "c+", "full" | "holes", "g0" | "g1" | "g2")."""
    n_out, s_idx, kind, cls, full, g_out = (int(v) for v in row)
    return ("empty" if n_out < 0 else "out0" if n_out == 0 else "out+", "S" if s_idx >= 0 else "-", "k%d" % kind,
            "c-" if cls < 0 else "c0" if cls == 0 else "c+", "full" if full else "holes", "g%d" % g_out)


def shape_keys(prog):
    """The distinct row shapes of a program, sorted."""
    return sorted(set(shape_key(r) for r in prog.rows))


def features(prog):
    """The kernel-level features of a program as a dict: what the census tables hold next to the row shapes."""
    empty = [k for k, r in enumerate(prog.rows) if r[0] < 0]
    return dict(T=prog.T, K=prog.K, D=prog.D, G=prog.G, n_s_rows=prog.n_s_rows, ncls=prog.ncls, inbox_rows=prog.inbox_rows,
                fewer_s_inbox_rows=prog.inbox_s_rows < prog.inbox_rows, pairs_identity=prog.pairs_identity, empty_rows=tuple(empty))


def program_key(prog):
    """A program as one line in the spelling of the plan key (pairs: "P=" the identity, "P~" another pairing; the key's
    occupancy suffix W<n> is no property of the rows and is left out)."""
    return "T%dK%dD%dS%dC%dG%dX%dx%dR%s%s" % (prog.T, prog.K, prog.D, prog.n_s_rows, prog.ncls, prog.G, prog.inbox_rows, prog.inbox_s_rows,
                                             ",".join("{%s}" % ",".join(str(v) for v in r) for r in prog.rows), "P=" if prog.pairs_identity else "P~")


def has_shape(prog, pattern):
    """Whether a row of the program matches pattern: a shape key with None where anything goes."""
    return any(all(p is None or p == v for p, v in zip(pattern, shape_key(r))) for r in prog.rows)


# ---- the shaped machines (random_machines.shaped_machine): one row per program the fixtures and the fuzz never compile
ShapedCase = collections.namedtuple("ShapedCase", "id blocks block_len threads members env features shapes")

_E1 = ("E", 1, [""])                       # a plain chain: one emit edge, no input
_E2D = ("E", 2, ["0", "1"])                # two emit edges, data symbols: one non-zero class
_E1D = ("E", 1, ["0", "1"])
_N2D = ("N", 2, ["0", "1"])
_N2M = ("N", 2, ["", "0", "1"], "inside")  # null edges of mixed classes that stay inside their block

SHAPED_CASES = [
    # no null edge anywhere: no S stripe (the SC region of the LDS map is empty), one class (withScore returns early), and the planner
    # leaves the FIRST row empty
    ShapedCase("chain", [_E1] * 4, 700, 1024, 1, {}, dict(n_s_rows=0, ncls=1, empty_rows=(0,)),
               [("out+", "-", "k1", "c0", "holes", "g0")]),
    ShapedCase("chain-c2", [_E1] * 4, 700, 1024, 2, {}, dict(n_s_rows=0, ncls=1),
               [("out+", "-", "k1", "c0", "holes", "g2")]),
    ShapedCase("fan2", [_E2D] * 4, 700, 1024, 1, {}, dict(n_s_rows=0, ncls=2, empty_rows=(0,)),
               [("out+", "-", "k1", "c+", "holes", "g0")]),
    ShapedCase("fan2-512", [_E2D] * 4, 700, 512, 1, {}, dict(n_s_rows=0, ncls=2),
               [("out+", "-", "k1", "c+", "full", "g0"), ("out+", "-", "k1", "c+", "holes", "g0")]),
    ShapedCase("fan2-c2", [_E2D] * 4, 1000, 512, 2, {}, dict(n_s_rows=0, ncls=2, empty_rows=(0,), pairs_identity=False),
               [("out+", "-", "k1", "c+", "full", "g2"), ("out+", "-", "k1", "c+", "full", "g0"), ("out+", "-", "k1", "c+", "holes", "g2")]),
    # three classes (a control symbol has a log-probability of its own), emit rows of mixed classes
    ShapedCase("classes", [("E", 2, ["", "0", "1"]), ("E", 1, ["", "0", "1", "A"]), ("E", 2, ["", "0", "1"]), _E1D], 700, 1024, 1, {},
               dict(n_s_rows=0, ncls=3, empty_rows=(0,)), [("out+", "-", "k1", "c-", "holes", "g0")]),
    # states with null in-edges whose own edges all emit under one class: an S row of kind 1
    ShapedCase("s-emit", [_N2D, _E1D, _N2D, _E1D], 700, 512, 1, {}, dict(ncls=2),
               [("out+", "S", "k1", "c+", "holes", "g0")]),
    # ... cut in three: the proxies' row offers into other members only (gOut 1)
    ShapedCase("s-emit-c3", [_N2D, _E1D, _N2D, _E1D], 700, 512, 3, {}, dict(ncls=2, fewer_s_inbox_rows=False),
               [("out+", "S", "k2", "c0", "holes", "g1"), ("out+", "S", "k0", "c+", "holes", "g2")]),
    ShapedCase("s-null", [("N", 1, ["0", "1"]), ("N", 2, [""]), _E1, ("N", 1, ["", "1"])], 700, 1024, 1, {}, dict(ncls=2, n_s_rows=4),
               [("out+", "S", "k2", "c+", "holes", "g0"), ("out+", "S", "k0", "c0", "holes", "g0")]),
    ShapedCase("s-mixed-c2", [_N2D, _E1D, ("N", 1, ["0", "1"]), _E2D], 700, 1024, 2, {}, dict(ncls=2, fewer_s_inbox_rows=True),
               [("out+", "S", "k0", "c+", "holes", "g2"), ("out+", "S", "k0", "c-", "holes", "g2")]),
    # dead ends: whole rows of states without out-edges stay live (nOut 0)
    ShapedCase("dead-ends", [("E", 2, [""]), ("E", 1, [""], "dead"), ("E", 2, [""]), ("E", 1, [""], "dead"), ("E", 2, [""])], 700, 512, 1, {},
               dict(n_s_rows=0, ncls=1, empty_rows=(7,)), [("out0", "-", "k0", "c-", "full", "g0"), ("out+", "-", "k1", "c0", "full", "g0")]),
    ShapedCase("dead-ends-1024", [("E", 2, [""]), ("E", 1, [""], "dead"), ("E", 2, [""]), ("E", 1, [""], "dead"), ("E", 2, [""])], 700, 1024, 1, {},
               dict(n_s_rows=0, ncls=1), [("out0", "-", "k0", "c-", "holes", "g0")]),
    # null chains of class 0: S rows of kind 2 with holes
    ShapedCase("null-chain", [_E1, ("N", 1, [""], "inside"), _E1, ("N", 1, [""], "inside")], 700, 512, 1, {}, dict(ncls=1),
               [("out+", "S", "k2", "c0", "holes", "g0")]),
    # programs the planner's scoring passes over, forced by DNAS_PLAN_PICK: null rows of mixed classes, and a row reserved for the
    # states that offer into the other member which holds nothing else
    ShapedCase("null-classes-pick", [_E1, _N2M, _E1, _N2M], 700, 512, 1, {"DNAS_PLAN_PICK": "6,3,1,0,0,0"}, dict(ncls=2),
               [("out+", "S", "k2", "c-", "holes", "g0")]),
    ShapedCase("chain-c2-pick", [_E1] * 4, 500, 512, 2, {"DNAS_PLAN_PICK": "3,0,1,0,0,0"}, dict(n_s_rows=0, ncls=1, empty_rows=(3,)),
               [("out+", "-", "k1", "c0", "holes", "g1")]),
]


def shaped_text(case):
    """The machine of a shaped case (seed 1 for all: the blocks make the shape)."""
    from random_machines import shaped_machine
    return shaped_machine(1, case.blocks, case.block_len)


# the cases that also run in segments (checkpoint=always,segment=D+2: DNAS_SEGMENTS=1 is a second compile of every shape) -- one
# without S rows, one with a full row of kind 1 and a common non-zero class, one cluster -- and those that also run both strands
SEGMENT_CASES = ("chain", "fan2-512", "fan2-c2")
STRAND_CASES = ("classes", "s-mixed-c2")


def shaped_reads(text):
    """The batch a shaped case decodes on the GPU: five reads of ragged lengths -- two walks of 20-30 bases and one of 64-70 with
    about one base in ten mutated, one single base, one empty read -- so that the slots of a launch stand in different columns."""
    from random_machines import shaped_read
    return [shaped_read(11, text, 27), shaped_read(12, text, 1, noise=0.), shaped_read(13, text, 70), "", shaped_read(14, text, 24)]


def model_options(case):
    """The options a ViterbiDecoder of a shaped case is created with (next to the case's environment)."""
    return "threads=%d" % case.threads if case.members == 1 else "tier=C,cluster=%d,threads=%d" % (case.members, case.threads)
