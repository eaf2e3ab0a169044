"""The read sampler of dnas_simulate_reads, restated in Python from its definition (include/dnastore_amd.h, "simulating reads"),
not from the C++: Philox4x32-10, the naming of a draw, the thresholds, the walk over the positions, and an enumeration of the
sampler's outcomes with their probabilities.  Shared by test_simulate_cpu.py and test_gpu_simulate.py."""
import hashlib

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
PER_READ = 0xFFFFFFFF
MAX_DUPS = 16
OP_MATCH, OP_DELETE, OP_DUP = 0, 1, 2


def philox4x32(counter, key):
    """Ten rounds: (c0, c1, c2, c3), (k0, k1) -> (w0, w1, w2, w3)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw_bits(seed, read, position, j):
    w = philox4x32((j >> 1, position, read & MASK, read >> 32), (seed & MASK, seed >> 32))
    x = (w[2] | w[3] << 32) if j & 1 else (w[0] | w[1] << 32)
    return x >> 11


def draw(seed, read, position, j):
    return draw_bits(seed, read, position, j) * 2.0 ** -53


def seed_of(text):
    """The string-derived seeds of the statistical tests: fixed by the name, before any run."""
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")


class Params:
    def __init__(self, pDelOpen, pDelExtend, pTanDup, pTransition, pTransversion, pLen):
        self.pDelOpen, self.pDelExtend, self.pTanDup = pDelOpen, pDelExtend, pTanDup
        self.pTransition, self.pTransversion, self.pLen = pTransition, pTransversion, list(pLen)
        self.local = False


def thresholds(p):
    cum, c = [], 0.0
    for x in p.pLen:
        c = c + x
        cum.append(c)
    sub = (p.pTransition, p.pTransition + p.pTransversion / 2, p.pTransition + p.pTransversion)
    return p.pDelOpen, p.pDelOpen + p.pTanDup, cum, sub


def substitute(sub, x, u):
    others = sorted((x ^ 1, x ^ 3))
    if u < sub[0]:
        return x ^ 2
    if u < sub[1]:
        return others[0]
    if u < sub[2]:
        return others[1]
    return x


def simulate_read(p, strand, seed, read, reverse_prob=0.0):
    """-> (the read as handed out, the op bytes of the read before the reversal, reversed)."""
    t_del, t_dup, cum, sub = thresholds(p)
    P, I = len(p.pLen), len(strand)
    out, ops = [], []
    in_del = False
    for ip in range(I + 1):
        if in_del:
            if ip < I and draw(seed, read, ip, 0) < p.pDelExtend:
                ops.append(OP_DELETE)
                continue
            in_del = False
        j, dups = 1, 0
        n = min(ip, P)
        can_dup = n > 0 and cum[n - 1] > 0
        while True:
            u = draw(seed, read, ip, j)
            j += 1
            if u < t_del and ip < I:
                ops.append(OP_DELETE | 1 << 2)
                in_del = True
                break
            if t_del <= u < t_dup and can_dup and dups < MAX_DUPS:
                v = draw(seed, read, ip, j)
                j += 1
                k = next((k for k in range(n) if v * cum[n - 1] < cum[k]), n - 1)
                for t in range(k, -1, -1):
                    out.append(substitute(sub, strand[ip - 1 - t], draw(seed, read, ip, j)))
                    j += 1
                    ops.append(OP_DUP | ((k + 1) << 2 if t == k else 0))
                dups += 1
                continue
            if ip < I:
                out.append(substitute(sub, strand[ip], draw(seed, read, ip, j)))
                ops.append(OP_MATCH)
            break
    reversed_ = draw(seed, read, PER_READ, 0) < reverse_prob
    if reversed_:
        out = [3 - b for b in reversed(out)]
    return out, ops, reversed_


def enumerate_outcomes(p, strand, max_dups=2, floor=0.0, num=float):
    """The sampler's outcomes as {(ops, read): probability} over every path with at most max_dups duplications per position whose
    probability stays at least `floor` all the way, and the probability of everything else.  Probabilities are formed in `num`
    (float, or mpmath.mpf).  A path is ops (tuple of op bytes) and the read before reversal (tuple of base codes)."""
    P, I = len(p.pLen), len(strand)
    one = num(1)
    d_open, d_ext, t_dup = num(p.pDelOpen), num(p.pDelExtend), num(p.pTanDup)
    ti, tv = num(p.pTransition), num(p.pTransversion)
    p_len = [num(x) for x in p.pLen]

    def subs(x):
        others = sorted((x ^ 1, x ^ 3))
        return [(x ^ 2, ti), (others[0], tv / 2), (others[1], tv / 2), (x, one - ti - tv)]

    outcomes = {}
    kept = [num(0)]

    def emit_copies(bases, prob, ops, read, first_n, done):
        """bases: the source bases still to copy; each through its own substitution."""
        if not bases:
            done(prob, ops, read)
            return
        for y, q in subs(bases[0]):
            if q > 0 and prob * q >= floor:
                emit_copies(bases[1:], prob * q, ops + (OP_DUP | first_n << 2,), read + (y,), 0, done)

    def s_loop(ip, dups, prob, ops, read):
        n = min(ip, P)
        cum = sum(p_len[:n], num(0))
        can_dup = n > 0 and cum > 0
        p_del = d_open if ip < I else num(0)
        p_dup = t_dup if can_dup and dups < MAX_DUPS else num(0)
        if p_del > 0 and prob * p_del >= floor:
            position(ip + 1, True, prob * p_del, ops + (OP_DELETE | 1 << 2,), read)
        if p_dup > 0 and dups < max_dups:
            for k in range(n):
                q = p_len[k] / cum
                if q > 0 and prob * p_dup * q >= floor:
                    emit_copies([strand[ip - 1 - t] for t in range(k, -1, -1)], prob * p_dup * q, ops, read, k + 1,
                                lambda pr, o, r: s_loop(ip, dups + 1, pr, o, r))
        rest = one - p_del - p_dup
        if ip < I:
            for y, q in subs(strand[ip]):
                if q > 0 and prob * rest * q >= floor:
                    position(ip + 1, False, prob * rest * q, ops + (OP_MATCH,), read + (y,))
        elif rest > 0 and prob * rest >= floor:
            outcomes[(ops, read)] = outcomes.get((ops, read), num(0)) + prob * rest
            kept[0] += prob * rest

    def position(ip, in_del, prob, ops, read):
        if in_del and ip < I:
            if d_ext > 0 and prob * d_ext >= floor:
                position(ip + 1, True, prob * d_ext, ops + (OP_DELETE,), read)
            prob = prob * (one - d_ext)
            if not (prob > 0 and prob >= floor):
                return
        s_loop(ip, 0, prob, ops, read)

    position(0, False, one, (), ())
    return outcomes, one - kept[0]


# ---- the cases both test files walk ---------------------------------------------------------------------------------------------

# (pDelOpen, pDelExtend, pTanDup, pTransition, pTransversion)
DEFAULT_SET = (.001, .01, .001, .01 * 10 / 11, .01 / 11)
NOISY_SET = (.15, .3, .1, .1, .1)
PARAM_SETS = {
    "default": DEFAULT_SET,
    "noisy": NOISY_SET,
    "del-open-1": (1., .3, 0., .1, .1),
    "del-extend-1": (.15, 1., .1, .1, .1),
    "dup-.9": (.05, .3, .9, .1, .1),             # the cap of 16 duplications is reached
    "dup-0": (.15, .3, 0., .1, .1),
}
DUP_LENGTHS = (0, 1, 3, 13, 32)
STRAND_LENGTHS = (0, 1, 2, 5, 64, 65, 130)
CHUNK_EDGE_LENGTHS = (63, 64, 65, 127, 128, 129, 191, 192, 300)
REVERSE_PROBS = (0., .5, 1.)


def p_len_of(P, zeros_in_front=False):
    """P duplication-length probabilities that sum to 1: uniform, or with zeros in front."""
    if P == 0:
        return []
    if zeros_in_front and P > 1:
        z = P // 2
        return [0.] * z + [1. / (P - z)] * (P - z)
    return [1. / P] * P


def make_params(da, values, p_len):
    """(the library's MutatorParams, the restatement's Params) of one parameter set."""
    c = da.lib.MutatorParamsC()
    c.p_del_open, c.p_del_extend, c.p_tan_dup, c.p_transition, c.p_transversion = values
    c.n_len, c.local = len(p_len), 0
    for k, x in enumerate(p_len):
        c.p_len[k] = x
    return da.MutatorParams(c), Params(*values, p_len)


def random_strands(lengths, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 4, n).astype(np.int8) for n in lengths]


def assert_same_reads(got, want, what=""):
    """Two SimulatedReads equal byte for byte: reads, ops, reversed flags, offsets (the lengths), status."""
    import numpy as np
    assert len(got) == len(want), what
    assert np.array_equal(got.status, want.status), (what, "status")
    assert np.array_equal(got.reversed, want.reversed), (what, "reversed")
    assert np.array_equal(got.strand, want.strand), (what, "strand")
    assert [len(r) for r in got.reads] == [len(r) for r in want.reads], (what, "offsets")
    assert (got.ops is None) == (want.ops is None), (what, "ops")
    for i in range(len(got)):
        assert np.array_equal(got.reads[i], want.reads[i]), (what, "read", i)
        if got.ops is not None:
            assert np.array_equal(got.ops[i], want.ops[i]), (what, "ops", i)
