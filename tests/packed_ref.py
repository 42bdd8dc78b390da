"""he_genrk_packed, he_gemv2_packed_batch, he_hempc_step_packed_batch and the
packed ends written with the calls of include/gpqhe.h (a helper, not a test):
the compositions include/gpqhe_ext_packed_batch.h defines them by, one
ciphertext at a time.  They run on either engine; the tests run them on the
oracle as the reference for the product's batch calls.

A context of S slots carries P = S / s loops of s slots; entry k of loop p is
packed slot k P + p.  Matrices are [nmat][rows][s] (leading rows only), nmat 1
(shared) or P (loop p its own); with nmat = 1 a full [s][s] matrix serves, its
rows past `rows` unread.
"""
import ctypes as C

import numpy as np

from tests.rows_ref import pow2


def packed_rotations(S, s, rows):
    """The rotations the packed row-folded product can need, ascending:
    {i P : 1 <= i < m'} U {m' 2^t P < S}."""
    assert S % s == 0 and 1 <= rows <= s
    P, mp = S // s, pow2(rows)
    fold = []
    r = mp
    while r < s:
        fold.append(r * P)
        r *= 2
    return sorted({i * P for i in range(1, mp)} | set(fold))


def packed_keys(e, sk, s, rows):
    """rk[S] with he_genrot(&rk[r], r, sk) for the packed rotations, ascending r."""
    rk = e.evks(e.slots)
    for r in packed_rotations(e.slots, s, rows):
        e.lib.he_genrot(C.byref(rk[r]), r, C.byref(sk))
    return rk


def loop_matrices(M, s, rows, nmat):
    """[nmat][rows][s]: the leading rows every loop reads."""
    return np.asarray(M, dtype=np.complex128).reshape(-1)[:nmat * rows * s].reshape(nmat, rows, s)


def packed_diagonals(M, S, s, rows, nmat=1):
    """{i: E_i} over the non-zero ones, E_i[k P + p] = M_p[k mod m'][(k + i) mod s]
    where k mod m' < rows, else 0 (M_p = M[p mod nmat])."""
    P, mp = S // s, pow2(rows)
    assert nmat in (1, P)
    top = loop_matrices(M, s, rows, nmat)
    j = np.arange(S)
    k, p = j // P, j % P
    out = {}
    for i in range(mp):
        E = np.where(k % mp < rows, top[p % nmat, np.minimum(k % mp, rows - 1), (k + i) % s], 0)
        if np.any(E != 0):
            out[i] = E
    return out


def interleave(z, S):
    """z [P][width] (loop-major) -> the S packed slots: slot k P + p = z[p][k], 0 for k >= width."""
    z = np.asarray(z, dtype=np.complex128)
    P, width = z.shape
    out = np.zeros((S // P, P), dtype=np.complex128)
    out[:width] = z.T
    return out.reshape(S)


def deinterleave(v, P, rows):
    """The S packed slots -> [P][rows]: [p][k] = slot k P + p."""
    v = np.asarray(v)
    return np.ascontiguousarray(v.reshape(-1, P)[:rows].T)


def expected_packed(Ma, za, Mb, zb, s, rows, nmat=1):
    """What the composition decodes to, over the S packed slots: slot k P + p
    holds (Ma_p za_p + Mb_p zb_p)[k mod m'] where k mod m' < rows, 0 elsewhere.
    za, zb: the S packed slots."""
    S = len(za)
    P, mp = S // s, pow2(rows)
    A, B = loop_matrices(Ma, s, rows, nmat), loop_matrices(Mb, s, rows, nmat)
    xa, xb = deinterleave(za, P, s), deinterleave(zb, P, s)   # [P][s]
    out = np.zeros((s, P), dtype=np.complex128)
    k = np.arange(s)
    for p in range(P):
        v = A[p % nmat] @ xa[p] + B[p % nmat] @ xb[p]
        out[:, p] = np.where(k % mp < rows, v[np.minimum(k % mp, rows - 1)], 0)
    return out.reshape(S)


def gemv2_packed_compose(e, Ma, xa, Mb, xb, rk, s, rows, nmat=1):
    """A new ciphertext y, every loop's leading rows of Ma_p xa_p + Mb_p xb_p:
         a_i = he_rot(xa, i P); b_i = he_rot(xb, i P)   for the non-zero E^A_i / E^B_i;
         u = sum_i he_mul_pt(a_i, he_ecd_ex(E^A_i, S, q_top, lvl))
           + sum_i he_mul_pt(b_i, he_ecd_ex(E^B_i, S, q_top, lvl));
         he_rescale(u);  for r = m', 2m', .. < s: u = he_add(u, he_rot(u, r P))
    Frees everything else it allocates."""
    S = e.slots
    assert S % s == 0 and 1 <= rows <= s
    P = S // s
    lvl = xa.nlimbs
    assert xb.nlimbs == lvl
    q_top = float(e.primes[lvl - 1])
    ops = [(packed_diagonals(Ma, S, s, rows, nmat), xa), (packed_diagonals(Mb, S, s, rows, nmat), xb)]
    if not ops[0][0] and not ops[1][0]:
        y = e.ct()
        e.sub(y, xa, xa)
        e.moddown(y)
        return y
    pt, t, b = e.pt(), e.ct(), e.ct()
    u = None
    for ext, x in ops:
        for i in sorted(ext):
            e.rot(b, x, i * P, rk)  # (i = 0: a copy)
            e.ecd_ex(pt, ext[i], S, q_top, lvl)
            if u is None:
                u = e.ct()
                e.mul_pt(u, b, pt)
            else:
                e.mul_pt(t, b, pt)
                e.add(u, u, t)
    e.rescale(u)
    r = pow2(rows)
    while r < s:
        e.rot(t, u, r * P, rk)
        e.add(u, u, t)
        r *= 2
    for o in (pt, t, b):
        e.free(o)
    return u


def step_packed_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, s, rows, nmat=1):
    """A new ciphertext up, ctr_hempc on the P loops of one ciphertext:
         xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
         w = gemv2_packed_compose(Ma, xd, Mb, ud); he_neg(w);
         c = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)."""
    xd, ud, c, up = e.ct(), e.ct(), e.ct(), e.ct()
    e.sub(xd, xhat, xr)
    e.sub(ud, uhat, ur)
    w = gemv2_packed_compose(e, Ma, xd, Mb, ud, rk, s, rows, nmat)
    e.neg(w)
    e.copy_ct(c, uhat)
    e.moddown(c)
    e.add(up, c, w)
    for o in (xd, ud, c, w):
        e.free(o)
    return up
