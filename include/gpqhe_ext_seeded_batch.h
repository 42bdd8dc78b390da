/*
 * gpqhe_ext_seeded_batch.h - seeded ("compressed") secret-key batch
 * encryption.  In a secret-key ciphertext c1 is nothing but a uniform sample,
 * so the encrypting party ships c0 alone together with a 40-byte PUBLIC seed,
 * and the machine that computes regenerates c1 from the seed: half the bytes
 * of gpqhe_ext_sk_batch.h's ciphertexts, 8 nlimbs n + 40 / count per
 * ciphertext against 16 nlimbs n.  Part of gpqhe_ext_batch.h, which includes
 * it; like everything there, only libgpqhe.so (the MI355X product) exports
 * these, and they are checked against sequences of gpqhe.h calls.
 *
 * The seed is a ChaCha key and a stream number, both public; the context's own
 * key, which also draws the secrets and the errors, is never shown.
 *
 * SECURITY.  A pair (key, stream) must NEVER serve two ciphertexts under one
 * secret key: both would carry the same a = c1, and the difference of their c0
 * is the difference of their messages (plus two small errors), in the clear.
 * This is why the encrypting calls advance ps->stream themselves; keep one
 * gpqhe_pubseed_t per secret key, pass it to every encrypting call, never
 * rewind it, and draw a fresh key for a fresh counter.
 *
 * Contract of the three encrypting calls.  With (c0', c1') ciphertext i, in
 * order, of
 *   he_ecd_ex(&pt, z_i, slots, scale, nlimbs); he_enc_sk(&ct_i, &pt, sk);
 * from the current RNG state, base its next stream (the contract of
 * gpqhe_ext_sk_batch.h: c1' the uniform sample of private stream base + 2 i, e
 * the CBD-21 sample of base + 2 i + 1):
 *   a_i limb m < nlimbs: the uniform sample under the ChaCha key ps->key and
 *     stream ps->stream + i, by the map of every uniform sample of the engine
 *     -- of coefficient k the block k nb + m / 4, nb = ceil((L + K) / 4) of
 *     the context (not of the level), its words 4 (m % 4) .. 4 (m % 4) + 3 as a
 *     128-bit little-endian integer mod q_m;
 *   c0_i = c0' + (c1' - a_i) s = NTT(e + m) - a_i s, every word canonical.
 * Private stream base + 2 i is skipped: the private counter advances by
 * 2 count, exactly as after he_enc_sk_batch, and a single he_enc_pk or
 * he_enc_sk before or after a call sees the streams it would see around
 * he_enc_sk_batch (also at n <= 4096, where single calls are queued).  On
 * return ps->stream has advanced by count (the gain call: by m').  count = 0:
 * no stream of either kind taken, nothing launched.
 *
 * Argument errors end the process with a message before the first launch and
 * before any stream is taken: those of the gpqhe_ext_sk_batch.h namesakes, a
 * null ps, ps->stream + count wrapping 2^64, and (he_expand_seeded_batch) x
 * overlapping c0.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_SEEDED_BATCH_H
#define GPQHE_EXT_SEEDED_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the public seed, 40 bytes: ciphertext i of a call takes (key, stream + i) */
typedef struct gpqhe_pubseed {
  uint32_t key[8];
  uint64_t stream;
} gpqhe_pubseed_t;

/* he_enc_sk_batch that keeps c1 to itself: z [count][slots] (host) ->
 * c0 [count][nlimbs][n] (device), compact.  z is consumed before the call
 * returns. */
void he_enc_sk_seeded_batch(uint64_t *c0, const gpqhe_complex_t z[], size_t count,
                            unsigned int slots, double scale, unsigned int nlimbs,
                            const poly_mpi_t *sk, gpqhe_pubseed_t *ps);

/* he_enc_sk_packed_batch likewise: z [count][P][width] loop-major, P = S / s;
 * entry k of loop p at slot k P + p, zero for k >= width; 1 <= width <= s. */
void he_enc_sk_seeded_packed_batch(uint64_t *c0, const gpqhe_complex_t z[], size_t count,
                                   unsigned int s, unsigned int width, double scale,
                                   unsigned int nlimbs, const poly_mpi_t *sk,
                                   gpqhe_pubseed_t *ps);

/* he_enc_gain_sk_packed_batch likewise: ALL m' extended diagonals of
 * M [nmat][rows][s], also those that are all zero, at scale q_top:
 * D0 [m'][nlimbs][n], device memory; ps->stream advances by m'. */
void he_enc_gain_sk_seeded_packed_batch(uint64_t *D0, const gpqhe_complex_t M[],
                                        unsigned int s, unsigned int rows, unsigned int nmat,
                                        unsigned int nlimbs, const poly_mpi_t *sk,
                                        gpqhe_pubseed_t *ps);

/* The computing side, which needs no key at all: c0 [count][nlimbs][n] ->
 * x [count][2][nlimbs][n] (both device memory), x[c][0] = c0[c] and x[c][1] the
 * sample a above of stream ps->stream + c.  ps is the value the seed had BEFORE
 * the encrypting call that made c0, and is not written. */
void he_expand_seeded_batch(uint64_t *x, const uint64_t *c0, size_t count,
                            unsigned int nlimbs, const gpqhe_pubseed_t *ps);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_SEEDED_BATCH_H */
