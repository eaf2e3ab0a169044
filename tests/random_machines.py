"""Random transducers for fuzzing the tier-A plan and kernel.

random_machine: out-degree up to 5, self loops, high in-degree, mixed emit/null out-edges, short and missing left contexts, three
score classes.  Valid Machine JSON by construction: an emit edge into state v always emits v's last context character
(verifyContexts, trans.cpp:484-496), edges without output only point forward (the decoder's toposort, trans.cpp:604-634), the
last state is the end state.  What these machines do NOT do is reach many of the fill kernel's specialisations: a row of the plan
holds 512 or 1024 states, so every machine of at most about 1000 states plans to one generic row (5 entries, classes mixed) and
an empty one -- of the seeds the tests use only 6, 7 and 13 (2300 and 5000 states) get more rows, all of mixed kind and class
(tests/test_tiera_census_cpu.py pins which machine gets which program).  They fuzz the plan's tables and the generic row.

shaped_machine: the machines for the other specialisations -- blocks of several hundred states that share the out-edge kind,
the out-degree and the input symbols, so that whole rows of the plan share them (tests/tiera_census.py SHAPED_CASES).

The duplication width of a decode is D = min(widest left context, len(pLen)) (viterbi.cpp:63): ctx_width= widens the
contexts so that any D up to 32 can be reached, and write_params() gives both sides one pLen of any length and shape."""
import hashlib
import json
import os
import random


def random_machine(seed, n_states, ctx_width=None, wildcards=False):
    """ctx_width=None: the historical machines (contexts of width 0, 1, 2 or 4; the text of every seed is pinned by
    test_tiera_plan_fuzz_cpu.py).  ctx_width=w: the same edges, but most contexts exactly w wide (state 0's always, so
    the widest is w) and the rest narrower; wildcards=True writes some of the w-wide ones as '*'-prefixed contexts
    ("**TG": the raw width counts towards D, the stripped one is the state's own duplication depth).  The extra draws
    come from a second generator, so the edges are those of random_machine(seed, n_states)."""
    rng = random.Random(seed)
    last = [rng.choice("ACGT") for _ in range(n_states)]
    ctx_len = [rng.choice([0, 1, 2, 4, 4]) for _ in range(n_states)]
    rng2 = random.Random("ctx/%d/%d" % (seed, n_states))
    states = []
    for i in range(n_states):
        l = ""
        if ctx_len[i]:
            l = "".join(rng.choice("ACGT") for _ in range(ctx_len[i] - 1)) + last[i]
        if ctx_width is not None:
            w = ctx_width if i == 0 or rng2.random() < 0.85 else rng2.randrange(0, ctx_width)
            l = "".join(rng2.choice("ACGT") for _ in range(w - 1)) + last[i] if w else ""
            if wildcards and w >= 2 and i > 0 and rng2.random() < 0.3:
                stars = rng2.randrange(1, w)
                l = "*" * stars + l[stars:]
        states.append({"n": i, "id": "s%d" % i, "l": l, "trans": []})
    hub = rng.randrange(1, n_states - 1)                      # a state with many in-edges
    for i in range(n_states - 1):
        trans = states[i]["trans"]
        # a spine edge keeps every state on a path to the end
        if rng.random() < 0.7:
            trans.append({"in": rng.choice(["", "0", "1"]), "out": last[i + 1], "to": i + 1})
        else:
            trans.append({"in": rng.choice(["", "0", "1", "A"]), "out": "", "to": i + 1})
        for _ in range(rng.choice([0, 0, 1, 1, 2, 4])):
            kind = rng.random()
            if kind < 0.55:                                     # emit edge anywhere (back, self, forward)
                to = rng.randrange(0, n_states)
                trans.append({"in": rng.choice(["", "0", "1", "^", "B"]), "out": last[to], "to": to})
            elif kind < 0.85 and i + 1 < n_states:              # null edge, forward only
                to = rng.randrange(i + 1, n_states)
                trans.append({"in": rng.choice(["", "0", "1", "$"]), "out": "", "to": to})
            else:                                               # into the hub
                if hub > i:
                    trans.append({"in": "", "out": "", "to": hub})
                else:
                    trans.append({"in": "1", "out": last[hub], "to": hub})
        for t in trans:
            for k in ("in", "out"):
                if t[k] == "":
                    del t[k]
    return json.dumps({"state": states})


def random_read(seed, machine_json, max_len=40, noise=0.1, dups=0, dup_log=None):
    """Characters emitted along a random walk from state 0 towards the end state, lightly mutated; dups=k: then one tandem
    duplication of every length 1..k is put in (the last j bases copied in place, at a place with j bases before it), each
    appended to dup_log (a list) as (place, j)."""
    rng = random.Random(seed)
    states = json.loads(machine_json)["state"]
    cur, out = 0, []
    for _ in range(4 * max_len):
        trans = states[cur]["trans"]
        if not trans or len(out) >= max_len:
            break
        fwd = [t for t in trans if t["to"] > cur]
        t = rng.choice(fwd if fwd and rng.random() < 0.7 else trans)
        if "out" in t:
            out.append(t["out"])
        cur = t["to"]
    read = []
    for c in out:
        r = rng.random()
        if r < noise / 2:
            continue                                            # deletion
        read.append(rng.choice("ACGT") if r < noise else c)    # substitution
    for j in range(1, dups + 1):
        if len(read) >= j:
            at = rng.randrange(j, len(read) + 1)
            read[at:at] = read[at - j:at]
            if dup_log is not None:
                dup_log.append((at, j))
    return "".join(read) or "A"


def shaped_machine(seed, blocks, block_len, ctx_width=4):
    """A machine of len(blocks) blocks of block_len states each plus the end state, built so that the tier-A planner meets
    whole rows of states with the same out-edges.  A block is (edges, degree, inputs[, flags]):
      edges    "E": every out-edge emits; "N": none does (null edges); "EN": they alternate, emit first
      degree   out-edges per state, every state of the block the same (so that a row of them can be full)
      inputs   the input symbols its edges draw from, one draw per edge: "" adds nothing (score class 0), the data symbols
               "0" / "1" share one log-probability (one more class; "^" and "$" weigh the same), a control symbol (a capital
               letter, "A") has its own (a third).  The probabilities are normalised over the symbols the whole machine uses: a
               machine whose only symbol is "0" has class 0 alone
      flags    "dead": the states have no out-edges at all -- they lie on no path to the end, the one exception to the rules
               below; the spine runs past the block and the edges of other blocks that land in it are what reaches them.
               "inside": the edges other than the spine stay inside the block (forward ones for null edges)
    The first out-edge of a state is the spine: it leads to the next state that is not dead (at last the end state), so that
    every other state sits on a path to the end; the others go to any state (emit: back, self or forward; null: forward only).
    As in random_machine, an emit edge into v emits v's last context base and the last state is the end state."""
    rng = random.Random("shaped/%d" % seed)
    n = len(blocks) * block_len + 1
    spec = [(b[0], b[1], b[2], b[3] if len(b) > 3 else "") for b in blocks]
    assert all(e in ("E", "N", "EN") and d >= 1 and ins and set(f.split()) <= {"dead", "inside"} for e, d, ins, f in spec)
    dead = [("dead" in spec[i // block_len][3].split()) if i < n - 1 else False for i in range(n)]
    last = [rng.choice("ACGT") for _ in range(n)]
    states = [{"n": i, "id": "s%d" % i, "l": "".join(rng.choice("ACGT") for _ in range(ctx_width - 1)) + last[i] if ctx_width else "",
               "trans": []} for i in range(n)]
    for i in range(n - 1):
        if dead[i]:
            continue
        edges, degree, inputs, flags = spec[i // block_len]
        lo, hi = (i // block_len) * block_len, (i // block_len + 1) * block_len          # the own block: [lo, hi)
        spine = next(j for j in range(i + 1, n) if not dead[j])
        for d in range(degree):
            null = edges == "N" or (edges == "EN" and d % 2 == 1)
            if d == 0:
                to = spine
            elif "inside" in flags.split():
                to = rng.randrange(i + 1, hi) if null and i + 1 < hi else spine if null else rng.randrange(lo, hi)
            else:
                to = rng.randrange(i + 1, n) if null else rng.randrange(0, n)
            t = {"to": to}
            sym = rng.choice(list(inputs))
            if sym:
                t["in"] = sym
            if not null:
                t["out"] = last[to]
            states[i]["trans"].append(t)
    return json.dumps({"state": states})


def shaped_read(seed, machine_json, length, noise=0.1):
    """The bases emitted along a walk from state 0 that takes the spine edge seven times in ten, cut after `length` of them (a
    walk that meets a dead end or the end state first starts again from state 0 and the read goes on: any base string is a
    read), then mutated like random_read's: every base dropped with probability noise / 2, substituted with noise / 2."""
    rng = random.Random("read/%d" % seed)
    states = json.loads(machine_json)["state"]
    cur, out = 0, []
    for _ in range(200 * (length + 1) + 4 * len(states)):
        if len(out) >= length:
            break
        trans = states[cur]["trans"]
        if not trans:
            cur = 0
            continue
        t = trans[0] if rng.random() < 0.7 else rng.choice(trans)
        if "out" in t:
            out.append(t["out"])
        cur = t["to"]
    read = []
    for c in out[:length]:
        r = rng.random()
        if r < noise / 2:
            continue
        read.append(rng.choice("ACGT") if r < noise else c)
    return "".join(read)


def params_json(pLen, dup=.05, sub=.02, del_open=.02, del_ext=.1, global_=False, iv=10.):
    """A MutatorParams JSON text (mutator.cpp:6-16's keys) with an explicit pLen; the probabilities are written with repr(),
    so both readers parse the same doubles."""
    return "{\n %s\n}\n" % ",\n ".join([
        '"pDelOpen": %r' % float(del_open), '"pDelExtend": %r' % float(del_ext), '"pTanDup": %r' % float(dup),
        '"pTransition": %r' % (sub * iv / (1 + iv)), '"pTransversion": %r' % (sub / (1 + iv)),
        '"pLen": [ %s ]' % ", ".join(repr(float(x)) for x in pLen), '"local": %s' % ("false" if global_ else "true")])


def plen_shape(P, shape):
    """P duplication-length probabilities: "down" strictly decreasing, "up" strictly increasing, "zero" decreasing with one
    entry 0 (log 0 = -inf: that length can never be a duplication)."""
    if P == 0:
        return []
    w = [float(P - i) for i in range(P)] if shape != "up" else [float(i + 1) for i in range(P)]
    if shape == "zero":
        w[P // 2] = 0.
    tot = sum(w)
    return [x / tot for x in w] if tot else w


def write_params(tmpdir, da, O, pLen, **flags):
    """One params JSON file read by both sides: (library MutatorParams via its JSON loader, oracle MutatorParams, text)."""
    text = params_json(pLen, **flags)
    path = os.path.join(str(tmpdir), "params_%d_%08x.json" % (len(pLen), int(hashlib.md5(text.encode()).hexdigest()[:8], 16)))
    with open(path, "w") as f:
        f.write(text)
    return da.MutatorParams.fromFile(path), O.MutatorParams.from_json(text), text


# D -> (context width, len(pLen), wildcards, pLen shape): D = min(width, len(pLen)) comes from the contexts for some widths and from
# pLen for others (contexts wider than P), '*'-prefixed contexts at some, and all three pLen shapes.  Widths 9..32 are tier B's alone.
WIDTH_CASES = {0: (4, 0, False, "down"), 1: (1, 3, False, "up"), 2: (8, 2, False, "down"), 3: (3, 5, True, "zero"),
               4: (4, 4, False, "up"), 5: (8, 5, True, "down"), 6: (6, 8, False, "up"), 7: (7, 7, True, "zero"),
               8: (8, 12, False, "down"), 9: (9, 9, False, "up"), 12: (12, 16, True, "down"), 16: (20, 16, False, "zero"),
               32: (32, 32, False, "up")}


def width_case(D, seed, n_states, shape=None):
    """(machine text, pLen) whose decode has exactly D duplication lanes (WIDTH_CASES)."""
    width, P, wild, default_shape = WIDTH_CASES[D]
    assert min(width, P) == D
    return random_machine(seed, n_states, ctx_width=width, wildcards=wild), plen_shape(P, shape or default_shape)
