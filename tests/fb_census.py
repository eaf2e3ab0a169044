"""The envelope of an alignment pair and the routing of the forward-backward E-step, restated from their definitions
(test infrastructure: the statement tests/test_gpu_fwdback_edges.py holds fwdback_census_kernel and the routing of
dnas_fb_estep to; tests/test_fb_census_cpu.py checks it and the constructions of tests/fb_edge_pairs.py on the CPU).

A pair is (ins, outs, cm_in, cm_out) as oracle.alignment_pair gives it.  Cell (ip, op), ip = 0..I, op = 0..O, lies in the
envelope iff |cm_out[op] - cm_in[ip]| <= Dm, with Dm = 0 under strict guides and P (the number of duplication lengths)
otherwise.  cm_in and cm_out are non-decreasing, so a row of the envelope is one interval [lo(ip), hi(ip)].

Rows here are never empty: the guide columns of an alignment count its matches, both arrays start at 0 and rise by at most
one per position up to the number of matches, so every value of cm_in occurs in cm_out.  envelope() asserts that."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnastore_amd", "csrc")


def _source(filename):
    with open(os.path.join(CSRC, filename)) as f:
        return f.read()


def _one(filename, pattern, what):
    found = re.findall(pattern, _source(filename), re.M)
    if len(found) != 1:
        raise RuntimeError("%s: expected one %s, found %d" % (filename, what, len(found)))
    return found[0]


def _product(text):
    value = 1
    for factor in text.split("*"):
        value *= int(factor)
    return value


# ---- the constants of the source, read from it: a change there moves the shapes of the tests with it
WAVE = int(_one("fwdback_device.h", r"^\s*constexpr\s+int\s+kFbWave\s*=\s*(\d+)\s*;", "'constexpr int kFbWave = <integer>;'"))
LDS_LIMIT = _product(_one("fwdback_device.h", r"^\s*constexpr\s+size_t\s+kFbOnchipLdsLimit\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;",
                          "'constexpr size_t kFbOnchipLdsLimit = <integer> [* <integer>];'"))
# fbOnchipPairDoubles: <fixed doubles> + ((maxInLen + <pad>) * <arrays> * sizeof(short) + 7) / 8 + <tail>
_PAIR = _one("fwdback_device.h",
             r"fbOnchipPairDoubles\(int W, int maxInLen\)\s*\{\s*return\s+((?:\d+\s*\+\s*)+)\(\(size_t\)\(maxInLen\s*\+\s*(\d+)\)\s*\*\s*(\d+)"
             r"\s*\*\s*sizeof\(short\)\s*\+\s*7\)\s*/\s*8\s*\+\s*(\d+)\s*;", "body of fbOnchipPairDoubles")
PAIR_FIXED = sum(int(x) for x in _PAIR[0].split("+") if x.strip())
PAIR_PAD, PAIR_ARRAYS, PAIR_TAIL = int(_PAIR[1]), int(_PAIR[2]), int(_PAIR[3])
_TABLES = _one("fwdback_runtime.hip", r"constexpr\s+int\s+kFbLanes\[4\]\s*=\s*\{([\d,\s]+)\}\s*,\s*kFbRowCells\[4\]\s*=\s*\{([\d,\s]+)\}\s*;",
               "'constexpr int kFbLanes[4] = {...}, kFbRowCells[4] = {...};'")
LANES = tuple(int(x) for x in _TABLES[0].split(","))          # lanes per pair of the four on-chip kernels (kinds 0..3)
ROW_CELLS = tuple(int(x) for x in _TABLES[1].split(","))      # the widest envelope row each serves
PPG = tuple(WAVE // w for w in LANES)                         # pairs per wave
WAVES_PER_CU = int(_one("fwdback_runtime.hip", r"^#define\s+DNAS_FB_WAVES_PER_CU\s+(\d+)\b", "'#define DNAS_FB_WAVES_PER_CU <integer>'"))
MAX_ONCHIP_P = 8                                              # the general on-chip kernels keep up to 8 duplication lanes
MAX_LEN = 30000                                               # dnas_fb_load_pairs refuses longer sequences


def pair_doubles(max_in_len):
    """fbOnchipPairDoubles: doubles of LDS one pair of an on-chip launch takes."""
    return PAIR_FIXED + ((max_in_len + PAIR_PAD) * PAIR_ARRAYS * 2 + 7) // 8 + PAIR_TAIL


def lds_bytes(kind, max_in_len):
    """Dynamic LDS of an on-chip launch of `kind` whose longest input is max_in_len."""
    return PPG[kind] * pair_doubles(max_in_len) * 8


def _longest(kind):
    n = 0
    while lds_bytes(kind, n + 64) <= LDS_LIMIT:
        n += 64
    return n


LONGEST = tuple(_longest(q) for q in range(4))                # the longest input each on-chip kernel takes
assert LONGEST == (1920, 3968, 3968, 8064), LONGEST           # (a change of fwdback_device.h shows up here)
assert LANES == (8, 16, 16, 32) and ROW_CELLS == (16, 16, 32, 32), (LANES, ROW_CELLS)


# ---- the envelope
def envelope(cm_in, cm_out, Dm):
    """(lo, hi): per row ip the first and the last op with |cm_out[op] - cm_in[ip]| <= Dm."""
    cm_in, cm_out = np.asarray(cm_in, np.int64), np.asarray(cm_out, np.int64)
    assert (np.diff(cm_in) >= 0).all() and (np.diff(cm_out) >= 0).all()
    lo = np.searchsorted(cm_out, cm_in - Dm, side="left")
    hi = np.searchsorted(cm_out, cm_in + Dm, side="right") - 1
    assert (hi >= lo).all(), "an empty envelope row"
    return lo, hi


def envelope_by_definition(cm_in, cm_out, Dm):
    """The same from the predicate alone, cell by cell (small pairs: what test_fb_census_cpu.py checks envelope() with)."""
    lo, hi = [], []
    for a in cm_in:
        ops = [op for op, b in enumerate(cm_out) if abs(int(b) - int(a)) <= Dm]
        assert ops and ops == list(range(ops[0], ops[-1] + 1))
        lo.append(ops[0]); hi.append(ops[-1])
    return np.array(lo), np.array(hi)


def margin(lo, hi, W):
    """max over ip <= I - W of hi(ip) - lo(ip + W): what a wavefront of W lanes needs below W (None without such a row)."""
    if len(lo) <= W:
        return None
    return int((hi[:-W] - lo[W:]).max())


def census(pair, Dm):
    """dict(width, cells, steps, fits8, fits16, margin8, margin16) of one pair."""
    lo, hi = envelope(pair[2], pair[3], Dm)
    m8, m16 = margin(lo, hi, 8), margin(lo, hi, 16)
    return dict(width=int((hi - lo + 1).max()), cells=int((hi - lo + 1).sum()), steps=int(len(lo) - 1 + hi[-1] - lo[0] + 1),
                fits8=m8 is None or m8 < 8, fits16=m16 is None or m16 < 16, margin8=m8, margin16=m16)


# ---- the routing
MODES = (None, "DNAS_FB_NO_NARROW", "DNAS_FB_STREAMING")      # the default routing and the two environment variables that change it


def decide(c, in_len, P, no_narrow=False, streaming=False):
    """(kind, on_chip) from a pair's census: kind 0..3 = the on-chip kernel its envelope asks for (8x16, 16x16, 16x32, 32x32
    lanes x cells), 4 = rows wider than any serves; on_chip: whether the pair runs there.  (Nothing here about the output's
    length: LO[] / HI[] of the on-chip kernels are int16, and dnas_fb_load_pairs has refused every sequence beyond MAX_LEN.)"""
    kind = 1 if c["width"] <= 16 else 3 if c["width"] <= 32 else 4
    if kind < 4 and not no_narrow and (c["fits8"] if kind == 1 else c["fits16"]):
        kind -= 1
    return kind, kind < 4 and P <= MAX_ONCHIP_P and in_len <= LONGEST[kind] and not streaming


def route(pair, P, strict=False, no_narrow=False, streaming=False):
    """(kind, on_chip, census) of one pair."""
    assert len(pair[0]) <= MAX_LEN and len(pair[1]) <= MAX_LEN
    c = census(pair, 0 if strict else P)
    return decide(c, len(pair[0]), P, no_narrow, streaming) + (c,)


def triple(decisions):
    onchip = sum(1 for kind, chip in decisions if chip)
    return onchip, sum(1 for kind, chip in decisions if chip and kind in (0, 2)), len(decisions) - onchip


def predict(pairs, P, strict=False, no_narrow=False, streaming=False):
    """(pairs_onchip, pairs_narrow, pairs_streaming) as dnas_fb_last_stats reports them after an E-step."""
    return triple([route(pair, P, strict, no_narrow, streaming)[:2] for pair in pairs])


def predict_modes(pairs, P, strict=False):
    """{mode: predict(...)} for the three MODES, with one census per pair."""
    cs = [(census(pair, 0 if strict else P), len(pair[0])) for pair in pairs]
    return {mode: triple([decide(c, n, P, mode == "DNAS_FB_NO_NARROW", mode == "DNAS_FB_STREAMING") for c, n in cs]) for mode in MODES}


def lists(pairs, P, strict=False, no_narrow=False, streaming=False):
    """The pair indices of the four on-chip lists and of the streaming list, in database order."""
    out = [[], [], [], [], []]
    for i, pair in enumerate(pairs):
        kind, chip, _ = route(pair, P, strict, no_narrow, streaming)
        out[kind if chip else 4].append(i)
    return out
