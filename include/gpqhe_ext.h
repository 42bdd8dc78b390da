/*
 * gpqhe_ext.h - extensions of the GPQHE C ABI that only libgpqhe.so (the
 * MI355X product) exports.  include/gpqhe.h stays the boundary both
 * implementations share; what is declared here has no CPU restatement and is
 * checked against compositions of gpqhe.h calls instead.
 *
 * Pure C99, include-guarded, includes gpqhe.h.
 */
#ifndef GPQHE_EXT_H
#define GPQHE_EXT_H

#include "gpqhe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Baby-step giant-step matrix-vector product.                               */
/*                                                                           */
/* With s = slots, 1 <= g <= s baby steps and G = ceil(s / g) giant steps,  */
/* diag_d[i] = M[i*s + (i+d) mod s] and roll(v, t)[k] = v[(k-t) mod s]:     */
/*   b_i    = he_rot(x, i)                                   0 <= i < g      */
/*   P_j,i  = he_ecd_ex(roll(diag_{jg+i}, jg), s, q_top, lvl)                */
/*   u_j    = sum_i he_mul_pt(b_i, P_j,i)                                    */
/*   y      = he_rescale(sum_j he_rot(u_j, jg))                              */
/* bit for bit, over the non-zero diagonals d = jg + i < s.  It reads the    */
/* g - 1 + G - 1 rotation keys rk[1..g-1] and rk[g], rk[2g], .., not the     */
/* s - 1 keys of he_gemv.  y is one level below x and keeps x's scale.       */
/* ------------------------------------------------------------------------ */

/* y = M x by baby-step giant-step; g = 0: default.  y may be x. */
void he_gemv_bsgs(he_ct_t *y, const gpqhe_complex_t M[], const he_ct_t *x,
                  const he_evk_t rk[], unsigned int g);
/* The keys he_gemv_bsgs(.., g) can need, into rk[slots] (indexed by rotation
 * like he_genrk's): exactly he_genrot(&rk[r], r, sk) for r in
 * {1..g-1} U {g, 2g, .., (G-1)g}, ascending r; every other entry left without
 * payload, rk[0].galois = 1. */
void he_genrk_bsgs(he_evk_t rk[], const poly_mpi_t *sk, unsigned int g);
/* The g that g = 0 selects for the current context. */
unsigned int he_gemv_bsgs_default_g(void);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_H */
