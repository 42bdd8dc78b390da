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


def key_payload(kind, primes, n, dnum, seed=0):
    """[2 dnum][len(primes)][n] words for he_import over a generated key
    (primes: all L + K moduli).  None for "genuine" (keep the generated key)."""
    if kind == "genuine":
        return None
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
