"""Constructed residues at the edges of the canonical range (a helper, not a
test): limbs, polynomials, key payloads and matrices that put the words the
kernels' worst-case bound arguments speak of -- 0, 1, q - 1 and the centred
extremes +-(q - 1)/2 -- where uniform samples almost never land.

Everything is canonical (every word below its modulus), so both engines must
accept it through he_import and agree bit for bit.
"""
import numpy as np

#: the limb patterns, in the order mixed() cycles through
NAMES = ("zero", "one", "qm1", "half_lo", "half_hi", "alt_qm1", "alt_half", "rand_half", "rand_edge", "imp0", "impN")

#: key payloads of the crafted-key tests: a limb pattern on every limb of every
#: polynomial, or "digit0" (one on digit 0's two polynomials, zero elsewhere)
KEY_KINDS = ("genuine", "one", "qm1", "half_lo", "rand_half", "digit0")


def pattern(name, q, n, seed=0):
    """One canonical uint64 limb of n words modulo q."""
    q = int(q)
    lo, hi = (q - 1) // 2, (q + 1) // 2  # the centred values +(q-1)/2 and -(q-1)/2
    out = np.zeros(n, dtype=np.uint64)
    if name == "zero":
        pass
    elif name == "one":
        out[:] = 1
    elif name == "qm1":
        out[:] = q - 1
    elif name == "half_lo":
        out[:] = lo
    elif name == "half_hi":
        out[:] = hi
    elif name == "alt_qm1":
        out[0::2] = q - 1
    elif name == "alt_half":
        out[0::2] = lo
        out[1::2] = hi
    elif name == "rand_half":
        pick = np.random.default_rng([seed, 1]).integers(0, 2, n)
        out[:] = np.where(pick == 0, np.uint64(lo), np.uint64(hi))
    elif name == "rand_edge":
        pick = np.random.default_rng([seed, 2]).integers(0, 3, n)
        out[:] = np.array([0, 1, q - 1], dtype=np.uint64)[pick]
    elif name == "imp0":
        out[0] = q - 1
    elif name == "impN":
        out[n - 1] = q - 1
    else:
        raise ValueError(f"unknown pattern {name!r}")
    return out


def poly(names_per_limb, primes, n, seed=0):
    """[len(primes)][n]: limb i holds pattern names_per_limb[i] modulo primes[i]."""
    assert len(names_per_limb) == len(primes)
    return np.stack([pattern(nm, q, n, seed * 131 + i) for i, (nm, q) in enumerate(zip(names_per_limb, primes))])


def mixed(k, primes, n, npolys=1):
    """[npolys][len(primes)][n]: the names cycled over limbs and polynomials
    from offset k, so neighbouring limbs (and polynomials) hold different
    patterns."""
    L = len(primes)
    return np.stack([poly([NAMES[(k + p * (L + 1) + i) % len(NAMES)] for i in range(L)], primes, n, seed=k + 7 * p)
                     for p in range(npolys)])


def pullback(engine, arr, nlimbs):
    """arr ([..][nlimbs][n], limb i modulo the context's modulus i) read as
    coefficient form: its forward NTT by the oracle.  An inverse transform of
    the result -- the one inside ModUp, rescale and ModDown -- returns exactly
    arr, so the words entering the basis conversion are the pattern."""
    out = np.ascontiguousarray(arr, dtype=np.uint64).copy()
    assert out.shape[-2] == nlimbs and out.shape[-1] == engine.n
    engine.lib.poly_ntt_batch(out.ctypes.data, out.size // (nlimbs * engine.n), nlimbs)
    return out


def spec_ct(engine, spec, primes, n, seed=0):
    """A two-polynomial ciphertext payload [2][len(primes)][n] from a spec:
    a pattern name (on every limb of both polynomials), "mixedK", or either
    with the prefix "pb:" (pulled back through the oracle's forward NTT)."""
    pb = spec.startswith("pb:")
    name = spec[3:] if pb else spec
    if name.startswith("mixed"):
        arr = mixed(int(name[5:]), primes, n, npolys=2)
    else:
        arr = np.stack([poly([name] * len(primes), primes, n, seed=seed + 17 * p) for p in range(2)])
    return pullback(engine, arr, len(primes)) if pb else arr


#: key payloads of the batch-kernel tests: KEY_KINDS, the all-zero key (the
#: key switch adds nothing: rot gives (sigma(c0), 0)) and the identity key (rot
#: is the index permutation of both polynomials)
BATCH_KEY_KINDS = ("genuine", "zero", "identity") + KEY_KINDS[1:]


def identity_key(primes, L, K, n, dnum):
    """[2 dnum][L + K][n]: the switching key of the identity.  With digits of
    alpha = ceil(L / dnum) limbs, polynomial 2 j + 1 holds the constant word
    P mod q_m on every limb m of digit j (P the product of the K special
    primes); every other word, and all of the P limbs, is 0.  The key switch of
    d under it sums to (0, P d) exactly, so after the division by P a rotation
    is the pure index permutation of both polynomials, at every level."""
    assert len(primes) == L + K
    alpha = -(-L // dnum)
    P = 1
    for p in primes[L:]:
        P *= int(p)
    out = np.zeros((2 * dnum, L + K, n), dtype=np.uint64)
    for m in range(L):
        out[2 * (m // alpha) + 1, m, :] = P % int(primes[m])
    return out


def key_payload(kind, primes, n, dnum, seed=0, L=None):
    """[2 dnum][len(primes)][n] words for he_import over a generated key
    (primes: all L + K moduli).  None for "genuine" (keep the generated key).
    "identity" needs L (the number of ciphertext moduli among primes)."""
    if kind == "genuine":
        return None
    if kind == "identity":
        return identity_key(primes, L, len(primes) - L, n, dnum)
    if kind == "zero":
        return np.zeros((2 * dnum, len(primes), n), dtype=np.uint64)
    if kind == "digit0":
        names = ["one", "one"] + ["zero"] * (2 * dnum - 2)
    else:
        names = [kind] * (2 * dnum)
    return np.stack([poly([nm] * len(primes), primes, n, seed=seed + 29 * p) for p, nm in enumerate(names)])


def circulant(s, consts):
    """s x s matrix whose diagonal d (entries M[i][(i + d) mod s]) is the
    constant consts[d mod len(consts)].  A constant diagonal encodes to a
    constant polynomial: every NTT-domain word of it is round(c scale) mod q."""
    M = np.zeros((s, s), dtype=np.complex128)
    idx = np.arange(s)
    for d in range(s):
        M[idx, (idx + d) % s] = consts[d % len(consts)]
    return M


def const_diag_matrix(s, c):
    """The dense s x s matrix of the constant c: every diagonal the constant."""
    return circulant(s, [c])


def const_words(X, primes, n):
    """[len(primes)][n]: limb i all X mod q_i -- the NTT form of the constant
    polynomial X (coefficient 0 is X, the others 0)."""
    return np.stack([np.full(n, int(X) % int(q), dtype=np.uint64) for q in primes])


def lift_edges(primes):
    """{name: X} with 0 <= X < Q = prod(primes): the integers at which the
    decoder's centred lift (Garner digits, multiword Horner with carries, the
    2 X > Q comparison, the borrow chain of Q - X, the conversion to double)
    changes path.  Values that fall outside [0, Q) on a short chain are left
    out; names are stable."""
    primes = [int(q) for q in primes]
    nl = len(primes)
    Q = 1
    for q in primes:
        Q *= q
    W = 1 << 64
    lowQ = Q % W
    cand = {
        "0": 0, "1": 1, "Q-1": Q - 1, "(Q-1)/2": (Q - 1) // 2, "(Q+1)/2": (Q + 1) // 2,
        "2^64-1": W - 1, "2^64": W, "Q-2^64": Q - W, "Q-2^128": Q - (1 << 128), "Q-1-2^64": Q - 1 - W,
        "2^128": 1 << 128,
        "lowQ": lowQ,  # a value whose low word equals Q's
        "2^53+1": (1 << 53) + 1, "Q-2^53-1": Q - (1 << 53) - 1,
        "floor(Q/2)-2^64": Q // 2 - W, "ceil(Q/2)+2^64": (Q + 1) // 2 + W,
        "q0": primes[0],
    }
    # Q - X = 2^(64 j) - 1 with X negative: word 0 of Q - X borrows, and words
    # 1 .. j - 1 of X equal Q's, so the borrow passes through equal words
    for j in range(2, nl + 1):
        if 2 * (Q - (1 << 64 * j) + 1) > Q:
            cand[f"Q-2^{64 * j}+1"] = Q - (1 << 64 * j) + 1
    Qk = 1
    for k, q in enumerate(primes):
        Qk *= q
        if k < nl - 1:
            cand[f"q0..q{k}"] = Qk  # Garner digits 0, .., 0, 1
        cand[f"Q{k}-1"] = Qk - 1    # every Garner digit up to k is q_j - 1
    return {name: v for name, v in cand.items() if 0 <= v < Q}


def horner_double(X, primes):
    """The decoder's conversion of the centred lift of X (0 <= X < Q) to a
    double, in Python: negative iff 2 X > Q, the magnitude split into
    len(primes) + 1 little-endian 64-bit words, d = d 2^64 + word from the top
    word down, each step rounded to double."""
    Q = 1
    for q in primes:
        Q *= int(q)
    X = int(X)
    assert 0 <= X < Q
    neg = 2 * X > Q
    mag = Q - X if neg else X
    d = 0.0
    for w in range(len(primes), -1, -1):
        d = d * 18446744073709551616.0 + float((mag >> (64 * w)) & ((1 << 64) - 1))
    return -d if neg else d
