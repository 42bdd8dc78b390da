/*
 * gpqhe_ext_step_batch.h - HECTR's encrypted control step (ctr_hempc) over a
 * batch of ciphertexts in implementation (device) memory: what runs between
 * he_enc_pk_batch and he_dec_dcd_batch.  Part of gpqhe_ext_batch.h, which
 * includes it; like everything there, only libgpqhe.so (the MI355X product)
 * exports these, and they are checked against compositions of gpqhe.h calls.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_STEP_BATCH_H
#define GPQHE_EXT_STEP_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y_c = Ma xa_c + Mb xb_c by one baby-step giant-step over both operands.
 * With s, g, G, diag_d, roll and P as in gpqhe_ext.h (P^A from Ma, P^B from Mb):
 *   a_i = he_rot(xa, i)   b_i = he_rot(xb, i)                        0 <= i < g
 *   u_j = sum_i he_mul_pt(a_i, P^A_j,i) + sum_i he_mul_pt(b_i, P^B_j,i)
 *   y   = he_rescale(sum_j he_rot(u_j, jg))
 * bit for bit, over the non-zero diagonals of either matrix.  Same key subset
 * as he_gemv_bsgs (he_genrk_bsgs(g)); g = 0: he_gemv_bsgs_default_g().
 * xa, xb [count][2][nlimbs][n] -> y [count][2][nlimbs-1][n], device memory.
 * xa and xb may overlap each other; y overlaps neither.  count = 0: no-op.
 * Both matrices zero: y zeroed. */
void he_gemv2_bsgs_batch(uint64_t *y,
                         const gpqhe_complex_t Ma[], const uint64_t *xa,
                         const gpqhe_complex_t Mb[], const uint64_t *xb,
                         size_t count, unsigned int nlimbs,
                         const he_evk_t rk[], unsigned int g);

/* ctr_hempc (reference src/hempc.c:252-266) over count independent loops:
 *   xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
 *   w  = he_gemv2_bsgs(Ma, xd, Mb, ud); he_neg(w);
 *   c  = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)
 * bit for bit.  Four inputs [count][2][nlimbs][n] at one scale ->
 * up [count][2][nlimbs-1][n] at that scale.  Inputs may overlap each other,
 * up overlaps none of them; none is written. */
void he_hempc_step_batch(uint64_t *up,
                         const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                         const uint64_t *xhat, const uint64_t *xr,
                         const uint64_t *uhat, const uint64_t *ur,
                         size_t count, unsigned int nlimbs,
                         const he_evk_t rk[], unsigned int g);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_STEP_BATCH_H */
