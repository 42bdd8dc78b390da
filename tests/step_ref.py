"""he_gemv2_bsgs_batch and he_hempc_step_batch written with the calls of
include/gpqhe.h (a helper, not a test): the compositions
include/gpqhe_ext_step_batch.h defines them by, one ciphertext at a time.
They run on either engine; the tests run them on the oracle as the reference
for the product's batch calls.
"""
import numpy as np

from tests.bsgs_ref import default_g, diagonals


def gemv2_compose(e, Ma, xa, Mb, xb, rk, g=0):
    """A new ciphertext y = Ma xa + Mb xb by one baby-step giant-step:
         a_i = he_rot(xa, i); b_i = he_rot(xb, i);
         P_j,i = he_ecd_ex(roll(diag_{jg+i}, jg), s, q_top, lvl) of either matrix;
         u_j = sum_i he_mul_pt(a_i, P^A_j,i) + sum_i he_mul_pt(b_i, P^B_j,i);
         y = he_rescale(sum_j he_rot(u_j, jg))
    over the non-zero diagonals of either matrix.  Frees everything else it
    allocates."""
    s = e.slots
    g = g or default_g(s)
    lvl = xa.nlimbs
    assert xb.nlimbs == lvl
    q_top = float(e.primes[lvl - 1])
    ops = [(diagonals(Ma, s), xa), (diagonals(Mb, s), xb)]
    if not ops[0][0] and not ops[1][0]:
        y = e.ct()
        e.sub(y, xa, xa)
        e.moddown(y)
        return y
    babies = []
    for diag, x in ops:
        bs = {}
        for i in sorted({d % g for d in diag}):
            bs[i] = e.ct()
            e.rot(bs[i], x, i, rk)  # (i = 0: a copy)
        babies.append(bs)
    pt, t = e.pt(), e.ct()
    y = None
    for j in sorted({d // g for diag, _ in ops for d in diag}):
        u = None
        for (diag, _), bs in zip(ops, babies):
            for i in range(g):
                d = j * g + i
                if d not in diag:
                    continue
                e.ecd_ex(pt, np.roll(diag[d], j * g), s, q_top, lvl)
                if u is None:
                    u = e.ct()
                    e.mul_pt(u, bs[i], pt)
                else:
                    e.mul_pt(t, bs[i], pt)
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
    for bs in babies:
        for b in bs.values():
            e.free(b)
    e.free(pt)
    e.free(t)
    return y


def step_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, g=0):
    """A new ciphertext up, ctr_hempc on one loop:
         xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
         w = gemv2_compose(Ma, xd, Mb, ud); he_neg(w);
         c = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)."""
    xd, ud, c, up = e.ct(), e.ct(), e.ct(), e.ct()
    e.sub(xd, xhat, xr)
    e.sub(ud, uhat, ur)
    w = gemv2_compose(e, Ma, xd, Mb, ud, rk, g)
    e.neg(w)
    e.copy_ct(c, uhat)
    e.moddown(c)
    e.add(up, c, w)
    for o in (xd, ud, c, w):
        e.free(o)
    return up
