/*
 * gpqhe_ext_sk_batch.h - the encrypting end for the party that holds the
 * secret key: he_enc_sk over a batch, in the three forms the public-key end
 * has (he_enc_pk_batch, he_enc_pk_packed_batch, he_enc_gain_packed_batch).  A
 * secret-key encryption takes its c1 as the uniform sample it is (already in
 * NTT form) and needs one transform, c0 = NTT(e + m) - c1 s, where a
 * public-key one needs three; its fresh noise is e alone, |e| <= 21 per
 * coefficient.  Part of gpqhe_ext_batch.h, which includes it; like everything
 * there, only libgpqhe.so (the MI355X product) exports these, and they are
 * checked against sequences of gpqhe.h calls.
 *
 * Contract of all three.  Ciphertext i of a call, in order, is bit for bit
 *   he_ecd_ex(&pt, z_i, slots, scale, nlimbs); he_enc_sk(&ct_i, &pt, sk);
 * from the current RNG state, base its next stream:
 *   c1 limb m < nlimbs: the uniform sample of stream base + 2 i -- of
 *     coefficient k the ChaCha block k nb + m / 4, nb = ceil((L + K) / 4) of
 *     the context (not of the level), its words 4 (m % 4) .. 4 (m % 4) + 3 as a
 *     128-bit little-endian integer mod q_m;
 *   e: the CBD-21 sample of stream base + 2 i + 1;
 *   c0 = NTT(e + m) - c1 s, every word canonical.
 * The stream counter advances by 2 count; a single he_enc_pk or he_enc_sk
 * before or after a call sees the streams the sequence of single calls would
 * give it (also at n <= 4096, where single calls are queued).  count = 0: no
 * stream taken, nothing launched.  Argument errors (no secret key at the
 * level, a bad level or slot count, s not dividing the slots, width, rows or
 * nmat out of range, a null pointer with count > 0) end the process with a
 * message before any stream is taken.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_SK_BATCH_H
#define GPQHE_EXT_SK_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* he_enc_pk_batch under the secret key: z [count][slots] (host) ->
 * x [count][2][nlimbs][n] (device).  z is consumed before the call returns. */
void he_enc_sk_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count,
                     unsigned int slots, double scale, unsigned int nlimbs,
                     const poly_mpi_t *sk);

/* he_enc_pk_packed_batch under the secret key: he_enc_sk_batch on the
 * interleaved vectors.  z [count][P][width] loop-major, P = S / s; entry k of
 * loop p at slot k P + p, zero for k >= width; 1 <= width <= s. */
void he_enc_sk_packed_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count,
                            unsigned int s, unsigned int width, double scale,
                            unsigned int nlimbs, const poly_mpi_t *sk);

/* he_enc_gain_packed_batch under the secret key: with E_i, 0 <= i < m', the
 * extended diagonals of M [nmat][rows][s] (gpqhe_ext_encgain_batch.h), ALL m'
 * of them, also those that are all zero,
 *   D = he_enc_sk_batch(D, E, m', S, (double)q_top, nlimbs, sk)
 * bit for bit (2 m' streams).  D [m'][2][nlimbs][n], device memory. */
void he_enc_gain_sk_packed_batch(uint64_t *D, const gpqhe_complex_t M[],
                                 unsigned int s, unsigned int rows, unsigned int nmat,
                                 unsigned int nlimbs, const poly_mpi_t *sk);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_SK_BATCH_H */
