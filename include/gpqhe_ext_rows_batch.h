/*
 * gpqhe_ext_rows_batch.h - the leading rows of HECTR's encrypted control step
 * by row folding (Halevi-Shoup), over a batch of ciphertexts in implementation
 * (device) memory.  A receding-horizon controller uses only the first nu
 * entries of the step's result; a matrix with `rows` leading rows needs
 * m' = 2^ceil(log2 rows) extended diagonals and log2(slots / m') rotate-and-add
 * steps instead of one rotation per diagonal.  Part of gpqhe_ext_batch.h,
 * which includes it; like everything there, only libgpqhe.so (the MI355X
 * product) exports these, and they are checked against compositions of
 * gpqhe.h calls.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_ROWS_BATCH_H
#define GPQHE_EXT_ROWS_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* keys the row-folded product can need, into rk[slots] (indexed by rotation):
 * exactly he_genrot(&rk[r], r, sk) for r in {1..m'-1} U {m' 2^t < slots},
 * ascending r; every other entry without payload, rk[0].galois = 1. */
void he_genrk_rows(he_evk_t rk[], const poly_mpi_t *sk, unsigned int rows);

/* y_c = the leading rows of Ma xa_c + Mb xb_c.  With s = slots, 1 <= rows <= s,
 * m' the smallest power of two >= rows, k = 0..s-1, lvl = nlimbs and q_top
 * prime lvl - 1:
 *   E^X_i[k] = M_X[k mod m'][(k + i) mod s]  if (k mod m') < rows, else 0   0 <= i < m'
 *   a_i = he_rot(xa, i)   b_i = he_rot(xb, i)        only for non-zero E^A_i / E^B_i
 *   u   = sum_i he_mul_pt(a_i, he_ecd_ex(E^A_i, s, q_top, lvl))
 *       + sum_i he_mul_pt(b_i, he_ecd_ex(E^B_i, s, q_top, lvl))
 *   he_rescale(u)
 *   for r = m', 2m', 4m', .. < s:   u = he_add(u, he_rot(u, r))   (at level lvl - 1)
 *   y = u
 * bit for bit.  Slot k of y holds (Ma xa + Mb xb)[k mod m'] for k mod m' < rows
 * and 0 elsewhere; rows >= `rows` of either matrix are never read.  Keys: the
 * he_genrk_rows(rows) subset; only those of rotations actually used are needed.
 * xa, xb [count][2][nlimbs][n] -> y [count][2][nlimbs-1][n], device memory.
 * xa and xb may overlap each other; y overlaps neither.  count = 0: no-op.
 * Both matrices zero in their leading rows: y zeroed. */
void he_gemv2_rows_batch(uint64_t *y,
                         const gpqhe_complex_t Ma[], const uint64_t *xa,
                         const gpqhe_complex_t Mb[], const uint64_t *xb,
                         size_t count, unsigned int nlimbs,
                         const he_evk_t rk[], unsigned int rows);

/* ctr_hempc (reference src/hempc.c:252-266) over count independent loops, its
 * product by row folding:
 *   xd = he_sub(xhat, xr); ud = he_sub(uhat, ur);
 *   w  = he_gemv2_rows(Ma, xd, Mb, ud); he_neg(w);
 *   c  = he_copy_ct(uhat); he_moddown(c); up = he_add(c, w)
 * bit for bit.  Only the first `rows` slots of up mean anything to a caller.
 * Four inputs [count][2][nlimbs][n] at one scale -> up [count][2][nlimbs-1][n]
 * at that scale.  Inputs may overlap each other, up overlaps none of them;
 * none is written.  Both matrices zero in their leading rows: up = the lower
 * limbs of uhat. */
void he_hempc_step_rows_batch(uint64_t *up,
                              const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                              const uint64_t *xhat, const uint64_t *xr,
                              const uint64_t *uhat, const uint64_t *ur,
                              size_t count, unsigned int nlimbs,
                              const he_evk_t rk[], unsigned int rows);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_ROWS_BATCH_H */
