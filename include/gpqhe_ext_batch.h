/*
 * gpqhe_ext_batch.h - batched forms of the extensions in gpqhe_ext.h.  Like
 * them, only libgpqhe.so (the MI355X product) exports what is declared here;
 * it has no CPU restatement and is checked against compositions of gpqhe.h
 * calls.
 *
 * Pure C99, include-guarded, includes gpqhe_ext.h.
 */
#ifndef GPQHE_EXT_BATCH_H
#define GPQHE_EXT_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* he_gemv_bsgs over `count` independent ciphertexts that share M, g and the
 * rotation keys: x [count][2][nlimbs][n] -> y [count][2][nlimbs-1][n] in
 * implementation (device) memory, every y_i holding exactly the residues
 * he_gemv_bsgs(y_i, M, x_i, rk, g) gives.  Reads the same key subset
 * (he_genrk_bsgs).  g = 0: default.  y must not overlap x.  count = 0: no-op. */
void he_gemv_bsgs_batch(uint64_t *y, const gpqhe_complex_t M[], const uint64_t *x,
                        size_t count, unsigned int nlimbs, const he_evk_t rk[],
                        unsigned int g);

#ifdef __cplusplus
}
#endif

/* the two ends of the batch entry points: he_enc_pk_batch, he_dec_dcd_batch */
#include "gpqhe_ext_io_batch.h"
#include "gpqhe_ext_step_batch.h"
#include "gpqhe_ext_rows_batch.h"
/* many control loops per ciphertext: the row-folded step at a slot stride */
#include "gpqhe_ext_packed_batch.h"
/* the packed step with the gains encrypted: ct x ct and one relinearisation */
#include "gpqhe_ext_encgain_batch.h"
/* the encrypting end under the secret key: one transform per ciphertext */
#include "gpqhe_ext_sk_batch.h"
/* ... with c1 shipped as a public seed: half the ciphertext */
#include "gpqhe_ext_seeded_batch.h"

#endif /* GPQHE_EXT_BATCH_H */
