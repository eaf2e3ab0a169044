"""Census of the tier-A / tier-C row programs (tests/tiera_census.py), on the CPU.

viterbi_tiera.hip is compiled per machine and branches, with `if constexpr`, on every field of the plan's row tuples and on
DNAS_SROWS, DNAS_NCLS, DNAS_G, DNAS_GROWS / DNAS_GSROWS and DNAS_PAIRS: a machine whose plan has another shape runs another
program, and the suite notices a wrong one only if some test compiles it.  This file

  * pins the program of every machine the GPU tests hold to the oracle (CENSUS: the five fixtures, the fuzz seeds, the width
    cases, as tier A and cut in two and three) and the union of their row shapes (TODAY_G1, TODAY_CLUSTER): a planner change
    that moves a machine to another program shows up as a diff of a literal;
  * checks that each shaped machine (tiera_census.SHAPED_CASES, built by random_machines.shaped_machine) plans to the
    program it is there for, and that together they reach what REQUIRED lists;
  * holds the plan tables of every shaped case to the oracle's lattice through test_tiera_plan_cpu._emulate;
  * JIT-compiles every shaped case at 1024 and 512 threads, as tier A and as a cluster of two.
tests/test_gpu_row_shapes.py runs the shaped cases on the GPU.

What the census of today's machines found: the 23 machines of at most 400 states (fuzz seeds 1, 2, 3, 11, 12 and both sets of
width cases) share ONE program up to D and the class count -- one generic row of 5 entries and an empty one (SMALL) -- because
a work-group has 512 or 1024 threads and a row holds that many states.  No machine of the suite had a program without S rows,
with one class only, or with its FIRST row empty, and none had a row of kind 1 with a common non-zero class, of kind 1 with
mixed classes and holes, of kind 2 with mixed classes, of kind 2 with class 0 and holes, with gOut 1, or a live row without
entries (nOut 0).

(The census is of the machines whose full lattice is held to the oracle; the 12-state machines of test_gpu_exact_models.py are
outside it, and one of them, cut in two, does get a row of kind 1 with a common non-zero class.)

Every one of those is within the planner's reach and a shaped case now has it.  The four that took a search:
  * a live row with nOut 0: dead-end states (no out-edge) in numbers that fill rows; the planner's ascending caps then give them
    rows of their own ("dead-ends", "dead-ends-1024": no forcing needed);
  * kind 2, class 0, with holes: null chains without input at 512 threads ("null-chain"; at 1024 threads the S rows also take
    the emitting states that null edges land on, and are of kind 0);
  * gOut 1 (every entry of the row offers into another member): the row of a cluster's proxies, whose one edge is a null edge
    of class 0 into another member -- "s-emit-c3", a cluster of three at 512 threads, where rows are reserved for the states
    that offer into other members.  With emit edges ("chain-c2-pick") only under DNAS_PLAN_PICK=3,0,1,0,0,0: the candidate
    that keeps the reserved row for the boundary states alone loses to one whose S rows take every state (scores 125 and 109);
    DNAS_PLAN_REMOTE_ROWS=1 at 1024 threads and DNAS_PLAN_ORDER / DNAS_PLAN_SLACK leave that order unchanged;
  * kind 2 with mixed classes: null blocks whose edges draw from "", "0", "1" give it only under DNAS_PLAN_PICK=6,3,1,0,0,0
    ("null-classes-pick"); the planner's own choice puts those states into rows that also hold emitting ones (kind 0).
DNAS_PLAN_PICK forces one of the candidates the planner scores anyway; the kernel it leads to is one the planner can emit."""
import json
import os
import re

import numpy as np
import pytest

import tiera_census as tc
from random_machines import random_machine, shaped_machine, shaped_read, width_case, write_params
from test_tiera_plan_cpu import _emulate

FIXTURES = ("l4c4", "mr2l4c4", "h74l4c4", "s16mr2l4c4", "s16h74l4c4")
FUZZ = [(1, 40, True), (2, 90, False), (3, 150, True), (6, 2300, True), (7, 5000, False), (11, 60, True), (12, 400, False), (13, 2300, True)]
FUZZ_FLAGS = dict(sub=.02, dup=.01, del_open=.02, del_ext=.1)
WIDTH_SEEDS = (50, 70)      # test_tiera_plan_cpu.py and test_gpu_dup_widths.py: width_case(D, seed + D, 150)

# programs at members 1, 2, 3 (tiera_census.program_key; no DNAS_THREADS: tier A plans for 1024 threads, a cluster for 512)
SMALL = ("T1024K2D%(D)dS1C%(C)dG1X0x0R{5,0,0,-1,0,0},{-1,-1,0,-1,0,0}P=",
         "T512K2D%(D)dS1C%(C)dG2X2x1R{5,0,0,-1,0,2},{-1,-1,0,-1,0,0}P=",
         "T512K2D%(D)dS1C%(C)dG3X2x1R{5,0,0,-1,0,2},{-1,-1,0,-1,0,0}P=")
SMALL_FUZZ = (1, 2, 3, 11, 12)
CENSUS = {
    "l4c4": (
        "T1024K2D4S1C3G1X0x0R{5,0,0,-1,0,0},{-1,-1,0,-1,0,0}P=",
        "T512K2D4S1C3G2X2x1R{5,0,0,-1,0,2},{-1,-1,0,-1,0,0}P=",
        "T512K2D4S1C3G3X2x1R{5,0,0,-1,0,2},{-1,-1,0,-1,0,0}P="),
    "mr2l4c4": (
        "T1024K2D4S1C3G1X0x0R{2,0,0,-1,0,0},{5,-1,0,-1,0,0}P=",
        "T512K2D4S1C3G2X2x1R{2,0,0,-1,0,2},{5,-1,0,-1,0,2}P=",
        "T512K2D4S1C3G3X2x1R{5,0,0,-1,0,2},{-1,-1,0,-1,0,0}P="),
    "h74l4c4": (
        "T1024K6D4S2C3G1X0x0R{2,0,0,-1,0,0},{2,1,0,-1,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,0,0},{5,-1,0,-1,0,0}P=",
        "T512K6D4S3C3G2X2x1R{2,0,0,-1,0,0},{1,-1,1,0,1,0},{5,1,0,-1,0,0},{1,-1,1,0,1,0},{5,2,0,-1,0,2},{1,-1,1,0,0,2}P~",
        "T512K4D4S3C3G3X2x1R{2,0,0,-1,0,0},{5,1,0,-1,0,0},{5,2,0,-1,0,2},{5,-1,0,-1,0,2}P~"),
    "s16mr2l4c4": (
        "T1024K10D4S6C2G1X0x0R{1,0,1,0,1,0},{1,1,1,0,0,0},{1,-1,1,0,1,0},{2,2,2,0,1,0},{2,3,0,0,0,0},{1,-1,1,0,1,0},{2,4,0,1,0,0},"
        "{2,5,0,1,0,0},{1,-1,1,-1,1,0},{-1,-1,0,-1,0,0}P=",
        "T512K10D4S6C2G2X2x1R{1,0,1,0,1,0},{1,1,1,0,0,0},{2,2,0,0,0,0},{2,3,0,0,0,0},{2,4,0,1,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},"
        "{2,5,0,-1,0,2},{2,-1,0,-1,0,2},{-1,-1,0,-1,0,0}P~",
        "T512K8D4S6C2G3X2x1R{1,0,1,0,0,0},{2,1,0,0,0,0},{2,2,0,0,0,0},{2,3,0,1,0,0},{2,4,0,0,0,0},{2,5,0,-1,0,2},{2,-1,0,-1,0,2},"
        "{-1,-1,0,-1,0,0}P~"),
    "s16h74l4c4": (
        "T1024K14D4S5C2G1X0x0R{2,0,0,1,0,0},{2,1,0,1,0,0},{2,2,2,1,0,0},{2,3,0,1,1,0},{1,4,1,0,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},"
        "{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,0,0},{2,-1,0,0,0,0},{2,-1,0,0,0,0}P=",
        "T512K16D4S6C2G2X2x1R{2,0,0,1,0,0},{2,1,2,1,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,0,0},{1,-1,1,0,0,0},{2,2,0,1,0,0},"
        "{2,3,0,1,1,0},{2,4,0,0,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{2,5,0,-1,0,2},{2,-1,0,-1,0,2},{2,-1,0,0,0,0},"
        "{-1,-1,0,-1,0,0}P~",
        "T512K10D4S4C2G3X2x1R{2,0,0,1,0,0},{2,1,0,1,0,0},{2,2,0,1,0,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},{1,-1,1,0,1,0},"
        "{2,3,0,-1,0,2},{2,-1,0,-1,0,2},{2,-1,0,0,0,2}P~"),
    "fuzz6": (
        "T1024K4D4S2C3G1X0x0R{5,0,0,-1,0,0},{5,1,0,-1,0,0},{5,-1,0,-1,0,0},{-1,-1,0,-1,0,0}P=",
        "T512K4D4S3C3G2X2x1R{2,0,0,2,0,0},{3,1,0,0,0,0},{5,2,0,-1,0,2},{5,-1,0,-1,0,2}P=",
        "T512K2D4S2C3G3X2x1R{5,0,0,-1,0,2},{5,1,0,-1,0,2}P="),
    "fuzz7": (
        "T1024K6D4S3C3G1X0x0R{2,0,0,-1,0,0},{3,1,0,-1,0,0},{5,2,0,-1,0,0},{2,-1,0,-1,0,0},{3,-1,0,-1,0,0},{-1,-1,0,-1,0,0}P=",
        "T512K6D4S4C3G2X4x1R{2,0,0,-1,0,2},{2,1,0,-1,0,2},{5,2,0,-1,0,2},{5,3,0,-1,0,2},{2,-1,0,-1,0,2},{5,-1,0,-1,0,2}P~",
        "T512K4D4S3C3G3X4x2R{5,0,0,-1,0,2},{5,1,0,-1,0,2},{5,2,0,-1,0,2},{3,-1,0,-1,0,2}P~"),
    "fuzz13": (
        "T1024K4D4S4C3G1X0x0R{5,0,0,1,0,0},{5,1,0,0,0,0},{2,2,0,2,0,0},{5,3,0,-1,0,0}P=",
        "T512K4D4S3C3G2X2x1R{3,0,0,1,0,0},{3,1,0,0,0,0},{5,2,0,-1,0,2},{5,-1,0,-1,0,2}P=",
        "T512K2D4S2C3G3X2x1R{5,0,0,-1,0,2},{5,1,0,-1,0,2}P="),
}

TODAY_G1 = {
    ("empty", "-", "k0", "c-", "holes", "g0"),
    ("out+", "-", "k0", "c-", "holes", "g0"),
    ("out+", "-", "k0", "c0", "holes", "g0"),
    ("out+", "-", "k1", "c-", "full", "g0"),
    ("out+", "-", "k1", "c0", "full", "g0"),
    ("out+", "-", "k1", "c0", "holes", "g0"),
    ("out+", "S", "k0", "c+", "full", "g0"),
    ("out+", "S", "k0", "c+", "holes", "g0"),
    ("out+", "S", "k0", "c-", "holes", "g0"),
    ("out+", "S", "k0", "c0", "holes", "g0"),
    ("out+", "S", "k1", "c0", "full", "g0"),
    ("out+", "S", "k1", "c0", "holes", "g0"),
    ("out+", "S", "k2", "c+", "holes", "g0"),
    ("out+", "S", "k2", "c0", "full", "g0"),
}
TODAY_CLUSTER = {
    ("empty", "-", "k0", "c-", "holes", "g0"),
    ("out+", "-", "k0", "c-", "holes", "g2"),
    ("out+", "-", "k0", "c0", "holes", "g0"),
    ("out+", "-", "k0", "c0", "holes", "g2"),
    ("out+", "-", "k1", "c0", "full", "g0"),
    ("out+", "-", "k1", "c0", "holes", "g0"),
    ("out+", "-", "k1", "c0", "holes", "g2"),
    ("out+", "S", "k0", "c+", "full", "g0"),
    ("out+", "S", "k0", "c+", "holes", "g0"),
    ("out+", "S", "k0", "c-", "holes", "g0"),
    ("out+", "S", "k0", "c-", "holes", "g2"),
    ("out+", "S", "k0", "c0", "holes", "g0"),
    ("out+", "S", "k1", "c0", "full", "g0"),
    ("out+", "S", "k1", "c0", "holes", "g0"),
    ("out+", "S", "k2", "c+", "holes", "g0"),
}

# What the shaped cases must reach between them, by cluster size: kernel features as (name, value), row shapes as patterns
# (None: anything).  The first block is the list the census asked for; the second the shapes that took a search (module docstring).
A = None
REQUIRED = {
    1: [("n_s_rows", 0), ("ncls", 1), ("ncls", 2), ("ncls", 3), ("empty_rows", (0,)),
        ("out+", "-", "k1", "c+", "holes", A), ("out+", "-", "k1", "c+", "full", A), ("out+", "-", "k1", "c-", "holes", A),
        ("out+", "S", "k1", "c+", "holes", A), ("out+", "S", "k2", "c+", A, A),
        ("out0", A, A, A, A, A), ("out+", A, "k2", "c-", A, A), ("out+", A, "k2", "c0", "holes", A)],
    2: [("out+", A, "k1", "c+", "full", "g2"), ("out+", A, "k1", "c0", "holes", "g2"), ("out+", "S", "k0", "c+", "holes", "g2"),
        ("out+", A, A, A, A, "g1")],
    3: [("out+", A, A, A, A, "g1")],
}


def _threads(monkeypatch, threads, env=None):
    """The analysis entry points (cluster_plan, precompile, precompile_cluster) read their thread count from DNAS_THREADS."""
    for k in ("DNAS_THREADS", "DNAS_PLAN_PICK", "DNAS_PLAN_ORDER", "DNAS_PLAN_SLACK", "DNAS_PLAN_REMOTE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if threads:
        monkeypatch.setenv("DNAS_THREADS", str(threads))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _programs(fm):
    return tuple(tc.program_key(tc.row_program(fm, members)) for members in (1, 2, 3))


@pytest.fixture(scope="module")
def today(oracle_mod, ref_data, tmp_path_factory):
    """{machine: its programs at members 1, 2, 3} for every machine of the census, planned once."""
    import dnastore_amd as da
    old = {k: os.environ.pop(k, None) for k in ("DNAS_THREADS", "DNAS_PLAN_PICK", "DNAS_PLAN_ORDER", "DNAS_PLAN_SLACK", "DNAS_PLAN_REMOTE_ROWS")}
    try:
        out = {}
        for name in FIXTURES:
            machine = da.Machine.fromFile(os.path.join(ref_data, name + ".json"))
            for global_ in (False, True):
                out["%s/%s" % (name, "global" if global_ else "local")] = _programs(da.FlatModel(machine, da.MutatorParams.fromFlags(global_=global_)))
        for seed, n, global_ in FUZZ:
            out["fuzz%d" % seed] = _programs(da.FlatModel(da.Machine.fromJSON(random_machine(seed, n)), da.MutatorParams.fromFlags(global_=global_, **FUZZ_FLAGS)))
        tmp = tmp_path_factory.mktemp("census")
        for base in WIDTH_SEEDS:
            for D in range(9):
                text, pLen = width_case(D, base + D, 150)
                dp, _, _ = write_params(tmp, da, oracle_mod, pLen)
                out["width%d/%d" % (D, base + D)] = _programs(da.FlatModel(da.Machine.fromJSON(text), dp))
        return out
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


def test_key_parser():
    note = ("tier C: G=2 K=4 inbox rows 2 exchange edges 0.1 lds=1 entries=4 back=3 "
            "T512K4D4S1C2G2X2x1R{2,0,0,-1,0,2},{1,-1,1,1,1,0},{0,-1,0,-1,0,1},{-1,-1,0,-1,0,0}P0,2,1,3W8; record x")
    p = tc.parse_key(note)
    assert p == tc.Program(512, 4, 4, 2, 1, 2, 2, 1, False, ((2, 0, 0, -1, 0, 2), (1, -1, 1, 1, 1, 0), (0, -1, 0, -1, 0, 1), (-1, -1, 0, -1, 0, 0)))
    assert tc.shape_keys(p) == [("empty", "-", "k0", "c-", "holes", "g0"), ("out+", "-", "k1", "c+", "full", "g0"),
                                ("out+", "S", "k0", "c-", "holes", "g2"), ("out0", "-", "k0", "c-", "holes", "g1")]
    assert tc.features(p) == dict(T=512, K=4, D=4, G=2, n_s_rows=1, ncls=2, inbox_rows=2, fewer_s_inbox_rows=True, pairs_identity=False,
                                  empty_rows=(3,))
    assert tc.parse_key("tier A: T1024K2D0S0C1G1X0x0R{1,-1,1,0,0,0},{-1,-1,0,-1,0,0}W8; x").pairs_identity
    assert tc.parse_key(tc.program_key(p)[:-2]) == p._replace(pairs_identity=True)     # (program_key spells the pairing as a flag)
    with pytest.raises(ValueError):
        tc.parse_key("tier B: more than 8 duplication lanes")


def test_todays_programs_are_pinned(today):
    """The program of every machine of the census, as a literal: the fixtures (local and global plan alike), the fuzz seeds, the
    width cases; and the union of their row shapes."""
    want = {}
    for name in FIXTURES:
        want[name + "/local"] = want[name + "/global"] = CENSUS[name]
    for seed, _, _ in FUZZ:
        want["fuzz%d" % seed] = tuple(k % dict(D=4, C=3) for k in SMALL) if seed in SMALL_FUZZ else CENSUS["fuzz%d" % seed]
    for base in WIDTH_SEEDS:
        for D in range(9):
            want["width%d/%d" % (D, base + D)] = tuple(k % dict(D=D, C=3 if D else 2) for k in SMALL)   # (D 0: a control symbol weighs 4^0)
    assert sorted(today) == sorted(want)
    for name in sorted(want):
        assert today[name] == want[name], name
    progs = [tc.parse_key(k) for ks in today.values() for k in ks]
    assert set(s for p in progs if p.G == 1 for s in tc.shape_keys(p)) == TODAY_G1
    assert set(s for p in progs if p.G > 1 for s in tc.shape_keys(p)) == TODAY_CLUSTER
    # the kernel-level features none of them has (each is the target of a shaped case)
    for p in progs:
        f = tc.features(p)
        assert f["n_s_rows"] > 0 and f["ncls"] in (2, 3) and f["empty_rows"] in ((), (p.K - 1,)), tc.program_key(p)
        assert f["fewer_s_inbox_rows"] == (p.G > 1)


def _case_model(case, global_=True):
    import dnastore_amd as da
    text = tc.shaped_text(case)
    return text, da.FlatModel(da.Machine.fromJSON(text), da.MutatorParams.fromFlags(global_=global_))


def _reaches(prog, item):
    return tc.features(prog)[item[0]] == item[1] if len(item) == 2 else tc.has_shape(prog, item)


@pytest.mark.parametrize("case", tc.SHAPED_CASES, ids=[c.id for c in tc.SHAPED_CASES])
def test_shaped_case_hits_its_targets(case, monkeypatch):
    """The plan of a shaped case has the features and row shapes the case names, at least one of which no machine of the census
    has; local and global plan alike; at most 5000 states."""
    _threads(monkeypatch, case.threads, case.env)
    text, fm = _case_model(case)
    assert fm.arrays()["n_states"] == len(case.blocks) * case.block_len + 1 <= 5001
    prog = tc.row_program(fm, case.members)
    assert (prog.T, prog.G) == (case.threads, case.members)
    f = tc.features(prog)
    for name, value in case.features.items():
        assert f[name] == value, (name, f[name], tc.program_key(prog))
    for pattern in case.shapes:
        assert tc.has_shape(prog, pattern), (pattern, tc.program_key(prog))
    new = [s for s in case.shapes if s not in (TODAY_G1 if case.members == 1 else TODAY_CLUSTER)]
    new += [n for n, v in case.features.items() if (n, v) in (("n_s_rows", 0), ("ncls", 1), ("empty_rows", (0,)), ("fewer_s_inbox_rows", False))]
    # ("s-null": an S row of kind 2 with a common non-zero class is a row s16h74l4c4 has too; here it stands in a program of S rows only)
    assert new or case.id == "s-null", "the case compiles nothing the census machines do not"
    assert tc.row_program(_case_model(case, global_=False)[1], case.members) == prog


def test_shaped_cases_reach_the_required_list(monkeypatch):
    progs = {}
    for case in tc.SHAPED_CASES:
        _threads(monkeypatch, case.threads, case.env)
        progs[case.id] = tc.row_program(_case_model(case)[1], case.members)
    for members, items in REQUIRED.items():
        for item in items:
            hits = [c.id for c in tc.SHAPED_CASES if c.members == members and _reaches(progs[c.id], item)]
            assert hits, (members, item)
    # three of the cases run in segments on the GPU: one without S rows, one with a full row of kind 1 and a common non-zero class,
    # one cluster; two run both strands (tests/test_gpu_row_shapes.py)
    by_id = {c.id: c for c in tc.SHAPED_CASES}
    assert tc.features(progs[tc.SEGMENT_CASES[0]])["n_s_rows"] == 0
    assert tc.has_shape(progs[tc.SEGMENT_CASES[1]], ("out+", A, "k1", "c+", "full", A))
    assert by_id[tc.SEGMENT_CASES[2]].members > 1
    assert len(tc.SEGMENT_CASES) == 3 and len(tc.STRAND_CASES) == 2 and set(tc.STRAND_CASES) <= set(by_id)


def test_shaped_machine_is_valid():
    """shaped_machine keeps random_machine's rules, block by block: the degree and the edge kinds the block names, inputs from
    the block's set, an emit edge into v emits v's last context base, null edges point forward, the last state is the end state,
    and every state that is no dead end sits on a path to the end."""
    blocks = [("E", 2, ["0", "1"]), ("N", 2, ["", "A"], "inside"), ("E", 1, [""], "dead"), ("EN", 3, ["", "0", "1"]), ("N", 1, [""])]
    B = 37
    states = json.loads(shaped_machine(5, blocks, B))["state"]
    n = len(states)
    assert n == len(blocks) * B + 1 and states[-1]["trans"] == [] and [s["n"] for s in states] == list(range(n))
    reach = [False] * n
    reach[-1] = True
    for i in range(n - 2, -1, -1):
        edges, degree, inputs, flags = (blocks[i // B] + ("",))[:4]
        trans = states[i]["trans"]
        if "dead" in flags:
            assert trans == []
            continue
        assert len(trans) == degree
        for d, t in enumerate(trans):
            null = "out" not in t
            assert null == (edges == "N" or (edges == "EN" and d % 2 == 1))
            assert t.get("in", "") in inputs
            assert t["to"] > i if null else t["out"] == states[t["to"]]["l"][-1]
            if "inside" in flags and d > 0 and not (null and i % B == B - 1):
                assert i // B == t["to"] // B
        assert trans[0]["to"] > i and reach[trans[0]["to"]]                 # the spine leads on, past the dead block
        reach[i] = True
    assert sum(reach) == n - B
    assert shaped_machine(5, blocks, B) == shaped_machine(5, blocks, B) != shaped_machine(6, blocks, B)
    for length in (0, 1, 25, 70):
        r = shaped_read(3, shaped_machine(5, blocks, B), length)
        assert set(r) <= set("ACGT") and length - (length + 3) // 4 <= len(r) <= length
    assert shaped_read(3, shaped_machine(5, blocks, B), 40, noise=0.) != shaped_read(4, shaped_machine(5, blocks, B), 40, noise=0.)


@pytest.mark.parametrize("case", tc.SHAPED_CASES, ids=[c.id for c in tc.SHAPED_CASES])
def test_shaped_case_plan_matches_oracle(oracle_mod, case, monkeypatch):
    """The planner's side of every shaped case: its tables, executed by _emulate as tier A and as a cluster of two (and as the
    case's own program where that is another one), give the oracle's S and D lanes bit for bit on one read of at most 10 bases."""
    import dnastore_amd as da
    text, fm = _case_model(case)
    orc = oracle_mod.ViterbiOracle(oracle_mod.Machine.from_json(text), oracle_mod.MutatorParams.from_cli(global_=True))
    read = shaped_read(7, text, 10)
    assert 7 <= len(read) <= 10
    _, _, olat = orc.decode(read, want_lattice=True)
    S_ref, D_ref = np.ascontiguousarray(olat[:, :, 0]).view(np.uint64), np.ascontiguousarray(olat[:, :, 1]).view(np.uint64)
    assert np.isfinite(olat[len(read), :, 0]).any()
    configs = [(case.threads, 1, {}), (case.threads, 2, {})]
    if (case.members, case.env) not in ((1, {}), (2, {})):
        configs.append((case.threads, case.members, case.env))
    for threads, members, env in configs:
        _threads(monkeypatch, threads, env)
        S_lat, D_lat = _emulate(fm, da.tokenize(read), local=False, members=members)
        assert np.array_equal(S_lat.view(np.uint64), S_ref), (threads, members, env)
        assert np.array_equal(D_lat.view(np.uint64), D_ref), (threads, members, env)


@pytest.mark.parametrize("case", tc.SHAPED_CASES, ids=[c.id for c in tc.SHAPED_CASES])
def test_shaped_case_compiles(case, monkeypatch):
    """Every shaped case JIT-compiles (no GPU needed) at 1024 and at 512 threads, as tier A and as a cluster of two, and as the
    program the case is there for; the key in each note is the program row_program reads off the plan tables."""
    _, fm = _case_model(case)
    for threads in (1024, 512):
        _threads(monkeypatch, threads)
        note = fm.precompile()
        assert note.startswith("tier A") and re.search(r"T%dK\d+D4S" % threads, note), note
        tc.row_program(fm, 1, note=note)
        note = fm.precompile_cluster(2)
        assert note.startswith("tier C") and re.search(r"T%dK\d+D4S\d+C\d+G2" % threads, note), note
        tc.row_program(fm, 2, note=note)
    _threads(monkeypatch, case.threads, case.env)
    note = fm.precompile() if case.members == 1 else fm.precompile_cluster(case.members)
    prog = tc.row_program(fm, case.members, note=note)
    for pattern in case.shapes:
        assert tc.has_shape(tc.parse_key(note), pattern) and tc.has_shape(prog, pattern)
