/*
 * gpqhe_ext_encgain_batch.h - the packed, row-folded step with encrypted
 * gains.  Every other form of the step takes Ma, Mb in the clear; here the
 * client encrypts the 2 m' extended diagonals of the packed step once, and
 * the cloud multiplies ciphertext by ciphertext: one tensor pass over the
 * 2 m' (rotated input, encrypted diagonal) pairs and ONE relinearisation of
 * their summed quadratic term, in place of 2 m' he_mul_pt.  The cloud sees
 * neither the gains nor which diagonals vanish.  Part of gpqhe_ext_batch.h,
 * which includes it; like everything there, only libgpqhe.so (the MI355X
 * product) exports these, and they are checked against compositions of
 * gpqhe.h calls.
 *
 * Throughout (the notation of gpqhe_ext_packed_batch.h): S = the context's
 * slots; s a power of two dividing S, P = S / s; 1 <= rows <= s, m' the
 * smallest power of two >= rows; lvl = nlimbs, 2 <= lvl <= L, q_top prime
 * lvl - 1.  Entry k of loop p lives at slot k P + p.  Rotation keys: the
 * he_genrk_packed(s, rows) subset; rlk from he_genrlk.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_ENCGAIN_BATCH_H
#define GPQHE_EXT_ENCGAIN_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Client side.  M [nmat][rows][s] (leading rows only), nmat = 1 (all loops
 * share one matrix) or P (loop p its own).  With E_i, 0 <= i < m', the
 * extended diagonals of gpqhe_ext_packed_batch.h,
 *   E_i[k P + p] = M_p[k mod m'][(k + i) mod s]  if (k mod m') < rows, else 0,
 * ALL m' of them, also those that are all zero:
 *   D = he_enc_pk_batch(D, E, m', S, (double)q_top, nlimbs, pk)
 * bit for bit, with the same use of the random streams (3 m' streams).
 * D [m'][2][nlimbs][n], device memory. */
void he_enc_gain_packed_batch(uint64_t *D, const gpqhe_complex_t M[],
                              unsigned int s, unsigned int rows, unsigned int nmat,
                              unsigned int nlimbs, const he_pk_t *pk);

/* Cloud side: loop p of every ciphertext, the leading rows of Ma_p xa_p +
 * Mb_p xb_p, with DA, DB = he_enc_gain_packed_batch of Ma, Mb.  For every
 * ciphertext, bit for bit:
 *   a_i = he_rot(xa, i P),  b_i = he_rot(xb, i P)     0 <= i < m'  (i = 0: the input itself)
 *   over the 2 m' pairs (c, d) = (a_i, DA_i), (b_i, DB_i), per limb m < lvl,
 *   elementwise mod q_m, canonical:
 *     X0 = sum c0 d0    X1 = sum (c0 d1 + c1 d0)    X2 = sum c1 d1
 *   lin  = he_rescale( ct(X0, X1) )                     (level lvl -> lvl - 1)
 *   quad = he_mul_rescale( ct(0, X2), ct(0, 1), rlk )   (1 = the word 1 at every
 *                                                        NTT position of every limb)
 *   u    = he_add(quad, lin)
 *   for r = m', 2m', .. < s:   u = he_add(u, he_rot(u, r P))   (at level lvl - 1)
 *   y = u
 * ct(p0, p1): those words imported as a ciphertext at level lvl (scale
 * sigma q_top for ct(X0, X1) and ct(0, X2), 1 for ct(0, 1), sigma the inputs'
 * scale: all three results carry sigma).  quad is the key switch of X2 under
 * rlk with the ModDown by P q_top.
 * xa, xb [count][2][nlimbs][n] -> y [count][2][nlimbs-1][n]; DA, DB
 * [m'][2][nlimbs][n], shared by all ciphertexts; device memory.  xa and xb may
 * overlap each other; y overlaps no input and no diagonal.  count = 0: no-op. */
void he_gemv2_encgain_packed_batch(uint64_t *y,
                                   const uint64_t *DA, const uint64_t *xa,
                                   const uint64_t *DB, const uint64_t *xb,
                                   size_t count, unsigned int nlimbs, const he_evk_t rk[],
                                   const he_evk_t *rlk, unsigned int s, unsigned int rows);

/* ctr_hempc around it over count ciphertexts of P loops each:
 *   xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
 *   w  = he_gemv2_encgain_packed(DA, xd, DB, ud); he_neg(w);
 *   c  = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)
 * bit for bit.  Only slots k P + p with k < rows of up mean anything to a
 * caller.  Four inputs [count][2][nlimbs][n] at one scale -> up
 * [count][2][nlimbs-1][n] at that scale.  Inputs may overlap each other, up
 * overlaps none of them and no diagonal; none is written. */
void he_hempc_step_encgain_packed_batch(uint64_t *up,
                                        const uint64_t *DA, const uint64_t *DB,
                                        const uint64_t *xhat, const uint64_t *xr,
                                        const uint64_t *uhat, const uint64_t *ur,
                                        size_t count, unsigned int nlimbs, const he_evk_t rk[],
                                        const he_evk_t *rlk, unsigned int s, unsigned int rows);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_ENCGAIN_BATCH_H */
