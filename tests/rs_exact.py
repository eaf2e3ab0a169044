"""The outer code from its definition, with no library code: GF(2^8) modulo 0x11d with alpha = 2, polynomial evaluation,
is_codeword, encoding by long division, and an exhaustive decoder for k <= 2 that lists all 256^k codewords and applies the
decoding rule of include/dnastore_amd.h literally.  Also the strand frame (CRC-8, polynomial 0x07) and the file stream."""
import numpy as np

RS_OK, RS_CORRECTED, RS_FAILED = 0, 1, 2

EXP = np.zeros(512, dtype=np.uint8)
LOG = np.zeros(256, dtype=np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11d
EXP[255:510] = EXP[:255]
# MUL[a, b] = a b
MUL = np.zeros((256, 256), dtype=np.uint8)
_nz = np.arange(1, 256)
MUL[1:, 1:] = EXP[(LOG[_nz][:, None] + LOG[_nz][None, :]) % 255]


def mul(a, b):
    return int(MUL[a, b])


def poly_eval(word, x):
    """word[0] x^(len-1) + ... + word[-1] at x."""
    y = 0
    for c in word:
        y = mul(y, x) ^ int(c)
    return y


def is_codeword(word, r):
    return all(poly_eval(word, int(EXP[i])) == 0 for i in range(r))


def generator(r):
    """g(x) = prod_{i<r} (x - alpha^i), descending, g[0] = 1."""
    g = [1]
    for i in range(r):
        g = g + [0]
        for j in range(len(g) - 1, 0, -1):
            g[j] ^= mul(g[j - 1], int(EXP[i]))
    return g


def encode(data, r):
    """data (k symbols) -> the n = k + r symbols: data, then the remainder of data x^r modulo g."""
    g = generator(r)
    rem = [int(d) for d in data] + [0] * r
    for i in range(len(data)):
        c = rem[i]
        if c:
            for j in range(1, r + 1):
                rem[i + j] ^= mul(c, g[j])
    return [int(d) for d in data] + rem[len(data):]


def encode_blocks(data, r):
    """The same division for uint8[B, k, L] at once -> uint8[B, k + r, L]."""
    data = np.asarray(data, dtype=np.uint8)
    B, k, L = data.shape
    tail = np.array(generator(r)[1:], dtype=np.uint8)
    rem = np.zeros((B, r, L), dtype=np.uint8)
    for p in range(k):
        fb = data[:, p] ^ rem[:, 0]
        rem = np.concatenate([rem[:, 1:], np.zeros((B, 1, L), dtype=np.uint8)], axis=1) ^ MUL[fb[:, None, :], tail[None, :, None]]
    return np.concatenate([data, rem], axis=1)


def syndromes(blocks, r):
    """uint8[B, n, L] -> uint8[B, r, L]: every column at alpha^0 .. alpha^(r-1); all zero iff the column is a codeword."""
    blocks = np.asarray(blocks, dtype=np.uint8)
    B, n, L = blocks.shape
    at = EXP[:r][None, :, None]
    acc = np.zeros((B, r, L), dtype=np.uint8)
    for p in range(n):
        acc = MUL[acc, at] ^ blocks[:, p][:, None, :]
    return acc


_CODEBOOKS = {}


def codebook(n, k):
    """All 256^k codewords of RS(n, k), uint8[256^k, n] (k <= 2)."""
    assert k <= 2
    if (n, k) not in _CODEBOOKS:
        r = n - k
        rows = [np.array(encode([1 if q == p else 0 for q in range(k)], r), dtype=np.uint8) for p in range(k)]   # the code is linear
        book = np.zeros((256,) * k + (n,), dtype=np.uint8)
        for p in range(k):
            shape = [1] * k + [n]
            shape[p] = 256
            book ^= MUL[np.arange(256)[:, None], rows[p][None, :]].reshape(shape)
        _CODEBOOKS[n, k] = book.reshape(-1, n)
    return _CODEBOOKS[n, k]


def decode_exhaustive(word, present, n, k):
    """The rule, literally -> (output word, status, e)."""
    r = n - k
    word, present = np.asarray(word, dtype=np.uint8), np.asarray(present).astype(bool)
    f = int((~present).sum())
    failed = (np.where(present, word, 0).astype(np.uint8), RS_FAILED, 0)
    if f > r:
        return failed
    book = codebook(n, k)
    e = (book[:, present] != word[present][None, :]).sum(axis=1)
    hit = np.nonzero(2 * e + f <= r)[0]
    if len(hit) == 0:
        return failed
    assert len(hit) == 1, "the codeword within reach is unique"
    return book[hit[0]].copy(), (RS_CORRECTED if e[hit[0]] else RS_OK), int(e[hit[0]])


SMALL_CODES = [(2, 1), (3, 1), (3, 2), (4, 2), (5, 2), (6, 2), (7, 1), (8, 2)]


def small_cases(n, k, rng, cases):
    """Random received words of RS(n, k): a codeword with f in 0 .. r+2 erasures and e in 0 .. r//2+2 errors (as far as n allows),
    the bytes stored at the erased positions 0, 255 or random.  -> words uint8[cases, n], present uint8[cases, n]."""
    r = n - k
    book = codebook(n, k)
    words, present = np.zeros((cases, n), dtype=np.uint8), np.ones((cases, n), dtype=np.uint8)
    for c in range(cases):
        w = book[rng.integers(len(book))].copy()
        f = min(int(rng.integers(0, r + 3)), n)
        e = min(int(rng.integers(0, r // 2 + 3)), n - f)
        pos = rng.permutation(n)
        for p in pos[f:f + e]:
            w[p] ^= rng.integers(1, 256)
        present[c, pos[:f]] = 0
        w[pos[:f]] = (0, 255, rng.integers(0, 256))[c % 3]
        words[c] = w
    return words, present


def crc8(data):
    """Polynomial 0x07, initial value 0, not reflected."""
    crc = 0
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xff if crc & 0x80 else (crc << 1) & 0xff
    return crc


def frame(s, body):
    head = bytes([(s >> 16) & 0xff, (s >> 8) & 0xff, s & 0xff])
    return head + bytes([crc8(head + bytes(body))]) + bytes(body)


def stream_of(data, k, L):
    """-> (the stream: 8 bytes of length little-endian, the file, zeros to B k L; B)."""
    B = -(-(8 + len(data)) // (k * L))
    s = len(data).to_bytes(8, "little") + bytes(data)
    return s + bytes(B * k * L - len(s)), B


def planted_blocks(n, k, L, fs, rng, errors=None):
    """One block per entry of fs: a random codeword per column, f strands erased (their bytes overwritten with noise) and, in
    column j, errors(b, j, f) wrong bytes at present strands (default: floor((r - f) / 2), the capacity).
    -> (clean uint8[B, n, L], received, present uint8[B, n])."""
    r = n - k
    B = len(fs)
    data = rng.integers(0, 256, size=(B, k, L), dtype=np.uint8)
    clean = encode_blocks(data, r)
    received, present = clean.copy(), np.ones((B, n), dtype=np.uint8)
    for b, f in enumerate(fs):
        gone = rng.permutation(n)[:f]
        present[b, gone] = 0
        received[b, gone] = rng.integers(0, 256, size=(len(gone), L), dtype=np.uint8)
        here = np.nonzero(present[b])[0]
        for j in range(L):
            e = (r - f) // 2 if errors is None else errors(b, j, f)
            for p in rng.permutation(here)[:max(e, 0)]:
                received[b, p, j] ^= rng.integers(1, 256)
    return clean, received, present
