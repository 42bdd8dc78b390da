/*
 * gpqhe_ext_io_batch.h - the two ends of the batch entry points: plaintext
 * vectors into a device array of ciphertexts and such an array back into
 * numbers.  Part of gpqhe_ext_batch.h, which includes it; like everything
 * there, only libgpqhe.so (the MI355X product) exports these, and they are
 * checked against sequences of gpqhe.h calls.
 *
 * Pure C99, include-guarded, includes gpqhe.h.
 */
#ifndef GPQHE_EXT_IO_BATCH_H
#define GPQHE_EXT_IO_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "gpqhe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* he_ecd_ex + he_enc_pk over `count` vectors: z [count][slots] (host) ->
 * x [count][2][nlimbs][n] (device).  x_i holds exactly the residues of
 *   he_ecd_ex(&pt, z_i, slots, scale, nlimbs); he_enc_pk(&ct, &pt, pk);
 * called for i = 0 .. count-1 in that order from the current RNG state.
 * The RNG is left where those calls leave it (3 * count streams taken).
 * z is consumed before the call returns.  count = 0: no-op, no stream taken. */
void he_enc_pk_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count,
                     unsigned int slots, double scale, unsigned int nlimbs,
                     const he_pk_t *pk);

/* he_dec + he_dcd_ex over `count` ciphertexts: y [count][2][nlimbs][n]
 * (device, NTT form, every one at `scale`) -> z [count][slots] (host).
 * The doubles are those of the single calls, bit for bit.
 * One stream synchronisation per call.  y is not written. */
void he_dec_dcd_batch(gpqhe_complex_t z[], const uint64_t *y, size_t count,
                      unsigned int nlimbs, double scale, unsigned int slots,
                      const poly_mpi_t *sk);

#ifdef __cplusplus
}
#endif

#endif /* GPQHE_EXT_IO_BATCH_H */
