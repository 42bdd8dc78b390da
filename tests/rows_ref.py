"""he_genrk_rows, he_gemv2_rows_batch and he_hempc_step_rows_batch written with
the calls of include/gpqhe.h (a helper, not a test): the compositions
include/gpqhe_ext_rows_batch.h defines them by, one ciphertext at a time.
They run on either engine; the tests run them on the oracle as the reference
for the product's batch calls.
"""
import ctypes as C

import numpy as np


def pow2(rows):
    """m': the smallest power of two >= rows."""
    return 1 << (rows - 1).bit_length()


def rows_rotations(s, rows):
    """The rotations the row-folded product of `rows` leading rows can need, ascending."""
    mp = pow2(rows)
    fold = []
    r = mp
    while r < s:
        fold.append(r)
        r *= 2
    return sorted(set(range(1, mp)) | set(fold))


def rows_keys(e, sk, rows):
    """rk[slots] with he_genrot(&rk[r], r, sk) for the row-folding rotations, ascending r."""
    rk = e.evks(e.slots)
    for r in rows_rotations(e.slots, rows):
        e.lib.he_genrot(C.byref(rk[r]), r, C.byref(sk))
    return rk


def extended_diagonals(M, s, rows):
    """{i: E_i} over the non-zero ones, E_i[k] = M[k mod m'][(k + i) mod s] where
    k mod m' < rows, else 0.  Reads the leading `rows` rows of M only."""
    top = np.asarray(M, dtype=np.complex128).reshape(-1)[:rows * s].reshape(rows, s)
    mp = pow2(rows)
    k = np.arange(s)
    out = {}
    for i in range(mp):
        E = np.where(k % mp < rows, top[np.minimum(k % mp, rows - 1), (k + i) % s], 0)
        if np.any(E != 0):
            out[i] = E
    return out


def expected_rows(Ma, za, Mb, zb, s, rows):
    """What the composition decodes to: slot k holds (Ma za + Mb zb)[k mod m']
    where k mod m' < rows, and 0 elsewhere."""
    A = np.asarray(Ma, dtype=np.complex128).reshape(-1)[:rows * s].reshape(rows, s)
    B = np.asarray(Mb, dtype=np.complex128).reshape(-1)[:rows * s].reshape(rows, s)
    v = A @ za + B @ zb
    mp = pow2(rows)
    k = np.arange(s)
    return np.where(k % mp < rows, v[np.minimum(k % mp, rows - 1)], 0)


def gemv2_rows_compose(e, Ma, xa, Mb, xb, rk, rows):
    """A new ciphertext y, the leading rows of Ma xa + Mb xb by row folding:
         a_i = he_rot(xa, i); b_i = he_rot(xb, i)   for the non-zero E^A_i / E^B_i;
         u = sum_i he_mul_pt(a_i, he_ecd_ex(E^A_i, s, q_top, lvl))
           + sum_i he_mul_pt(b_i, he_ecd_ex(E^B_i, s, q_top, lvl));
         he_rescale(u);  for r = m', 2m', .. < s: u = he_add(u, he_rot(u, r))
    Frees everything else it allocates."""
    s = e.slots
    assert 1 <= rows <= s
    lvl = xa.nlimbs
    assert xb.nlimbs == lvl
    q_top = float(e.primes[lvl - 1])
    ops = [(extended_diagonals(Ma, s, rows), xa), (extended_diagonals(Mb, s, rows), xb)]
    if not ops[0][0] and not ops[1][0]:
        y = e.ct()
        e.sub(y, xa, xa)
        e.moddown(y)
        return y
    pt, t, b = e.pt(), e.ct(), e.ct()
    u = None
    for ext, x in ops:
        for i in sorted(ext):
            e.rot(b, x, i, rk)  # (i = 0: a copy)
            e.ecd_ex(pt, ext[i], s, q_top, lvl)
            if u is None:
                u = e.ct()
                e.mul_pt(u, b, pt)
            else:
                e.mul_pt(t, b, pt)
                e.add(u, u, t)
    e.rescale(u)
    r = pow2(rows)
    while r < s:
        e.rot(t, u, r, rk)
        e.add(u, u, t)
        r *= 2
    for o in (pt, t, b):
        e.free(o)
    return u


def step_rows_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, rows):
    """A new ciphertext up, ctr_hempc on one loop with the row-folded product:
         xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
         w = gemv2_rows_compose(Ma, xd, Mb, ud); he_neg(w);
         c = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)."""
    xd, ud, c, up = e.ct(), e.ct(), e.ct(), e.ct()
    e.sub(xd, xhat, xr)
    e.sub(ud, uhat, ur)
    w = gemv2_rows_compose(e, Ma, xd, Mb, ud, rk, rows)
    e.neg(w)
    e.copy_ct(c, uhat)
    e.moddown(c)
    e.add(up, c, w)
    for o in (xd, ud, c, w):
        e.free(o)
    return up
