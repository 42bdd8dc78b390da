"""The baby-step giant-step matrix-vector product written with the calls of
include/gpqhe.h (a helper, not a test): the composition include/gpqhe_ext.h
defines he_gemv_bsgs by.  It runs on either engine; the tests run it on the
oracle as the reference for the product's he_gemv_bsgs / he_genrk_bsgs.
"""
import ctypes as C

import numpy as np


def default_g(s):
    """g = 2^ceil(log2(s) / 2)."""
    lg = (s - 1).bit_length()
    return 1 << ((lg + 1) // 2)


def bsgs_rotations(s, g=0):
    """The rotations he_gemv_bsgs(.., g) can need, ascending."""
    g = g or default_g(s)
    return sorted(set(range(1, g)) | set(range(g, s, g)))


def bsgs_keys(e, sk, g=0):
    """rk[slots] with he_genrot(&rk[r], r, sk) for the BSGS rotations, ascending r."""
    rk = e.evks(e.slots)
    for r in bsgs_rotations(e.slots, g):
        e.lib.he_genrot(C.byref(rk[r]), r, C.byref(sk))
    return rk


def diagonals(M, s):
    M = np.asarray(M, dtype=np.complex128).reshape(s, s)
    idx = np.arange(s)
    return {d: M[idx, (idx + d) % s] for d in range(s) if np.any(M[idx, (idx + d) % s] != 0)}


def bsgs_compose(e, M, x, rk, g=0):
    """A new ciphertext y = M x:
         b_i = he_rot(x, i); P_j,i = he_ecd_ex(roll(diag_{jg+i}, jg), s, q_top, lvl);
         u_j = sum_i he_mul_pt(b_i, P_j,i); y = he_rescale(sum_j he_rot(u_j, jg))
    over the non-zero diagonals.  Frees everything else it allocates."""
    s = e.slots
    g = g or default_g(s)
    lvl = x.nlimbs
    q_top = float(e.primes[lvl - 1])
    diag = diagonals(M, s)
    if not diag:
        y = e.ct()
        e.sub(y, x, x)
        e.moddown(y)
        return y
    babies = {}
    for i in sorted({d % g for d in diag}):
        babies[i] = e.ct()
        e.rot(babies[i], x, i, rk)  # (i = 0: a copy)
    pt, t = e.pt(), e.ct()
    y = None
    for j in sorted({d // g for d in diag}):
        u = None
        for i in range(g):
            d = j * g + i
            if d not in diag:
                continue
            e.ecd_ex(pt, np.roll(diag[d], j * g), s, q_top, lvl)
            if u is None:
                u = e.ct()
                e.mul_pt(u, babies[i], pt)
            else:
                e.mul_pt(t, babies[i], pt)
                e.add(u, u, t)
        r = e.ct()
        e.rot(r, u, j * g, rk)
        e.free(u)
        if y is None:
            y = r
        else:
            e.add(y, y, r)
            e.free(r)
    e.rescale(y)
    for b in babies.values():
        e.free(b)
    e.free(pt)
    e.free(t)
    return y
