"""Random transducers for fuzzing the tier-A plan and kernel: shapes the fixture machines do not have
(out-degree up to 5, self loops, high in-degree, several score classes, mixed emit/null out-edges, short and
missing left contexts).  Valid Machine JSON by construction: an emit edge into state v always emits v's last
context character (verifyContexts, trans.cpp:484-496), edges without output only point forward (the decoder's
toposort, trans.cpp:604-634), the last state is the end state.

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
