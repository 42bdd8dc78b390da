"""Independent model of the engine's random number generation (test
infrastructure only; shares no code with the oracle or the product).

The engine draws every random polynomial from ChaCha20 in counter mode:

  key     eight 32-bit words from the 64-bit seed by splitmix64 (four outputs,
          low word first), see seed_key();
  state   constants | key[8] | counter | 0 | stream_lo | stream_hi, i.e.
          RFC 8439 ChaCha20 with the 32-bit block counter in word 12 and the
          96-bit nonce (0, stream) in words 13..15;
  stream  one fresh stream number per sampled polynomial, counted from 0 at
          every (re)seed.

The three maps from keystream words to coefficients (DESIGN.md section 3,
"Sampling"):

  ternary  coefficient k from block k: r = word0 & 3; 0, 0, +1, -1 for
           r = 0, 1, 2, 3 (density 1/2);
  CBD-21   coefficient k from block k: popcount(word0 & (2^21 - 1)) -
           popcount(word1 & (2^21 - 1)), variance 21/2, |e| <= 21;
  uniform  residue of coefficient k modulo the context's modulus m: block
           k nb + m // 4 with nb = ceil((L + K) / 4), its words
           4 (m % 4) .. 4 (m % 4) + 3 read as a little-endian 128-bit integer,
           reduced modulo q_m.

Stream numbers in the order the API documents:
  he_keypair       s (ternary), a (uniform), e (CBD)
  gen of one evk   per digit j: a_j (uniform), e_j (CBD)
  he_enc_pk        v (ternary), e0 (CBD), e1 (CBD)
  he_enc_sk        a (uniform), e (CBD)
"""
from __future__ import annotations

import numpy as np

MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"
CBD_ETA = 21
CBD_VAR = CBD_ETA / 2.0


def splitmix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def seed_key(seed: int):
    """The eight key words of a 64-bit seed."""
    z = seed & MASK64
    key = []
    for _ in range(4):
        z = (z + 0x9E3779B97F4A7C15) & MASK64
        x = splitmix64(z)
        key += [x & MASK32, x >> 32]
    return key


def _rotl(v, c):
    return ((v << c) & MASK32) | (v >> (32 - c))


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & MASK32
    x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & MASK32
    x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & MASK32
    x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & MASK32
    x[b] = _rotl(x[b] ^ x[c], 7)


ROUND = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
         (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def chacha20_block(key, stream: int, counter: int):
    """The sixteen output words of one block (plain Python integers)."""
    s = list(SIGMA) + [k & MASK32 for k in key] + [counter & MASK32, 0, stream & MASK32, (stream >> 32) & MASK32]
    x = list(s)
    for _ in range(10):
        for q in ROUND:
            _qr(x, *q)
    return [(a + b) & MASK32 for a, b in zip(x, s)]


def chacha20_blocks(key, stream: int, counters) -> np.ndarray:
    """[len(counters)][16] uint32: the blocks of an array of counters (the
    same function as chacha20_block, vectorised over the counter)."""
    counters = np.asarray(counters, dtype=np.uint64)
    m = counters.size
    s = np.empty((16, m), dtype=np.uint32)
    for i, w in enumerate(SIGMA):
        s[i] = w
    for i, w in enumerate(key):
        s[4 + i] = w & MASK32
    s[12] = (counters & np.uint64(MASK32)).astype(np.uint32)
    s[13] = 0
    s[14] = stream & MASK32
    s[15] = (stream >> 32) & MASK32
    x = s.copy()

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    with np.errstate(over="ignore"):
        for _ in range(10):
            for a, b, c, d in ROUND:
                x[a] += x[b]
                x[d] = rotl(x[d] ^ x[a], 16)
                x[c] += x[d]
                x[b] = rotl(x[b] ^ x[c], 12)
                x[a] += x[b]
                x[d] = rotl(x[d] ^ x[a], 8)
                x[c] += x[d]
                x[b] = rotl(x[b] ^ x[c], 7)
        x += s
    return np.ascontiguousarray(x.T)


def block_bytes(words) -> bytes:
    """The 64 keystream bytes of a block (words serialised little-endian)."""
    return b"".join(int(w).to_bytes(4, "little") for w in words)


def key_bytes(key) -> bytes:
    return b"".join(int(w).to_bytes(4, "little") for w in key)


def iv_bytes(stream: int, counter: int) -> bytes:
    """The 16-byte IV of `openssl enc -chacha20` that yields block (stream,
    counter) first: LE32(counter) | LE32(0) | LE64(stream)."""
    return (counter & MASK32).to_bytes(4, "little") + bytes(4) + (stream & MASK64).to_bytes(8, "little")


def _idx(n, idx):
    return np.arange(n, dtype=np.uint64) if idx is None else np.asarray(idx, dtype=np.uint64)


def _popcount(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.uint32)
    out = np.zeros(v.shape, dtype=np.int64)
    for b in range(CBD_ETA):
        out += ((v >> np.uint32(b)) & np.uint32(1)).astype(np.int64)
    return out


def sample_ternary(key, stream, n, idx=None) -> np.ndarray:
    """int64 coefficients (all n, or those at idx) of the ternary polynomial
    of a stream."""
    r = chacha20_blocks(key, stream, _idx(n, idx))[:, 0] & np.uint32(3)
    return np.where(r < 2, 0, np.where(r == 2, 1, -1)).astype(np.int64)


def sample_cbd(key, stream, n, idx=None) -> np.ndarray:
    b = chacha20_blocks(key, stream, _idx(n, idx))
    mask = np.uint32((1 << CBD_ETA) - 1)
    return _popcount(b[:, 0] & mask) - _popcount(b[:, 1] & mask)


def sample_uniform(key, stream, n, m, q, nmod, idx=None) -> np.ndarray:
    """uint64 residues modulo q = modulus number m of a context with nmod
    moduli in all (L + K), for all n coefficients or those at idx."""
    nb = (nmod + 3) // 4
    k = _idx(n, idx)
    b = chacha20_blocks(key, stream, k * np.uint64(nb) + np.uint64(m // 4))
    w = b[:, 4 * (m % 4):4 * (m % 4) + 4]
    out = [(int(a) | int(b_) << 32 | int(c) << 64 | int(d) << 96) % q for a, b_, c, d in w]
    return np.array(out, dtype=np.uint64)


def centred(x, q) -> np.ndarray:
    """Residues in [0, q) as centred int64 (|x| small expected)."""
    x = np.asarray(x, dtype=np.uint64)
    q = np.uint64(q)
    return np.where(x > q // np.uint64(2), -((q - x).astype(np.int64)), x.astype(np.int64))
