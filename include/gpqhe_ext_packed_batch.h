/*
 * gpqhe_ext_packed_batch.h - many control loops per ciphertext.  A context of
 * S slots carries P = S / s loops of s slots each: entry k of loop p lives at
 * packed slot k P + p, so he_rot by i P rotates every loop by i at once and one
 * extended diagonal encoded at S slots carries a different matrix row for
 * every loop.  The row-folded step (gpqhe_ext_rows_batch.h) then costs the
 * same 2 (m' - 1) + log2(s / m') key switches and (m' - 1) + log2(s / m')
 * keys for P loops as for one, and per-loop gain matrices come free.  Part of
 * gpqhe_ext_batch.h, which includes it; like everything there, only
 * libgpqhe.so (the MI355X product) exports these, and they are checked
 * against compositions of gpqhe.h calls.
 *
 * Throughout: S = the context's slots; s a power of two, 1 <= s <= S, P = S / s;
 * 1 <= rows <= s, m' the smallest power of two >= rows; lvl = nlimbs, q_top
 * prime lvl - 1.  With s = S (P = 1, nmat = 1) every call is the corresponding
 * rows / io batch call bit for bit.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_PACKED_BATCH_H
#define GPQHE_EXT_PACKED_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* keys the packed row-folded product can need, into rk[S] (indexed by
 * rotation): exactly he_genrot(&rk[r], r, sk) for r in {i P : 1 <= i < m'} U
 * {m' 2^t P < S}, ascending r; every other entry without payload,
 * rk[0].galois = 1. */
void he_genrk_packed(he_evk_t rk[], const poly_mpi_t *sk, unsigned int s, unsigned int rows);

/* Loop p of every ciphertext: the leading rows of Ma_p xa_p + Mb_p xb_p.
 * Ma, Mb: [nmat][rows][s] (leading rows only), nmat = 1 (all loops share one
 * matrix) or P (loop p its own); the matrices are shared by all `count`
 * ciphertexts.  With k = 0..s-1, p = 0..P-1:
 *   E^X_i[k P + p] = M_X,p[k mod m'][(k + i) mod s]  if (k mod m') < rows, else 0   0 <= i < m'
 *   a_i = he_rot(xa, i P)   b_i = he_rot(xb, i P)     only for non-zero E^A_i / E^B_i
 *   u   = sum_i he_mul_pt(a_i, he_ecd_ex(E^A_i, S, q_top, lvl))
 *       + sum_i he_mul_pt(b_i, he_ecd_ex(E^B_i, S, q_top, lvl))
 *   he_rescale(u)
 *   for r = m', 2m', 4m', .. < s:   u = he_add(u, he_rot(u, r P))   (at level lvl - 1)
 *   y = u
 * bit for bit.  Slot k P + p of y holds (Ma_p xa_p + Mb_p xb_p)[k mod m'] where
 * k mod m' < rows and 0 elsewhere.  Keys: the he_genrk_packed(s, rows) subset;
 * only those of rotations actually used are needed.
 * xa, xb [count][2][nlimbs][n] -> y [count][2][nlimbs-1][n], device memory.
 * xa and xb may overlap each other; y overlaps neither.  count = 0: no-op.
 * Both matrices zero in their leading rows: y zeroed. */
void he_gemv2_packed_batch(uint64_t *y,
                           const gpqhe_complex_t Ma[], const uint64_t *xa,
                           const gpqhe_complex_t Mb[], const uint64_t *xb,
                           size_t count, unsigned int nlimbs, const he_evk_t rk[],
                           unsigned int s, unsigned int rows, unsigned int nmat);

/* ctr_hempc around it over count ciphertexts of P loops each:
 *   xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
 *   w  = he_gemv2_packed(Ma, xd, Mb, ud); he_neg(w);
 *   c  = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)
 * bit for bit.  Only slots k P + p with k < rows of up mean anything to a
 * caller.  Four inputs [count][2][nlimbs][n] at one scale -> up
 * [count][2][nlimbs-1][n] at that scale.  Inputs may overlap each other, up
 * overlaps none of them; none is written.  Both matrices zero in their leading
 * rows: up = the lower limbs of uhat. */
void he_hempc_step_packed_batch(uint64_t *up,
                                const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                                const uint64_t *xhat, const uint64_t *xr,
                                const uint64_t *uhat, const uint64_t *ur,
                                size_t count, unsigned int nlimbs, const he_evk_t rk[],
                                unsigned int s, unsigned int rows, unsigned int nmat);

/* z [count][P][width] host memory, loop-major, width <= s; entries k >= width
 * of a loop are 0.  The same words and the same use of the random streams as
 * he_enc_pk_batch(x, Z, count, S, scale, nlimbs, pk) with
 * Z[c][k P + p] = z[c][p][k].  x [count][2][nlimbs][n], device memory. */
void he_enc_pk_packed_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count,
                            unsigned int s, unsigned int width, double scale,
                            unsigned int nlimbs, const he_pk_t *pk);

/* z [count][P][rows] host memory, loop-major: z[c][p][k] = slot k P + p of
 * he_dec + he_dcd_ex(.., S) of ciphertext c, k < rows, the same doubles bit
 * for bit.  y [count][2][nlimbs][n], device memory.  One stream
 * synchronisation per call. */
void he_dec_dcd_packed_batch(gpqhe_complex_t z[], const uint64_t *y, size_t count,
                             unsigned int nlimbs, double scale,
                             unsigned int s, unsigned int rows, const poly_mpi_t *sk);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_PACKED_BATCH_H */
