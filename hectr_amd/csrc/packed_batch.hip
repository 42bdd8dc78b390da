// packed_batch.hip - gfx950 kernels of he_enc_pk_packed_batch / he_dec_dcd_packed_batch
// (include/gpqhe_ext_packed_batch.h; host side: api.cpp).  A ciphertext of
// S = P s slots carries P loops, entry k of loop p at packed slot k P + p; the
// callers' vectors are loop-major ([P][width] in, [P][rows] out).  Two
// streaming gathers between the two forms over a chunk of ciphertexts, one
// complex value (one 16-byte access) per lane, the strided side on the load,
// the store coalesced, no LDS and no scratch:
//   pack_enc_gather_kernel  v[c][k P + p] = z[c][p][k], 0 for k >= width: the
//                           GPU encoder's input (in front of its first stage)
//   pack_dcd_gather_kernel  out[c][p][k] = z[c][k P + p], k < rows: the decoded
//                           values a caller reads, where the decoder takes
//                           several launches (S > GPQHE_DCD_ONEPASS)
#include "gpqhe_internal.h"

#define TPB 256

typedef double pack_d2 __attribute__((ext_vector_type(2)));

// v [cnt][S] <- z [cnt][P][width]; total = cnt S values.  grid: (total / TPB).
__global__ void __launch_bounds__(TPB) pack_enc_gather_kernel(pack_d2 *v, const pack_d2 *z, size_t total, unsigned logS,
                                                              unsigned logP, unsigned width)
{
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total)
    return;
  const size_t c = t >> logS;
  const unsigned j = (unsigned)(t & (((size_t)1 << logS) - 1));
  const unsigned p = j & ((1u << logP) - 1), k = j >> logP;
  pack_d2 x = {0.0, 0.0};
  if (k < width)
    x = z[((c << logP) + p) * width + k];
  v[t] = x;
}

void k_pack_enc_gather(double *v, const double *z, unsigned S, unsigned P, unsigned width, unsigned cnt)
{
  const size_t total = (size_t)cnt * S, blocks = (total + TPB - 1) / TPB;
  if (!cnt || !S || (S & (S - 1)) || !P || (P & (P - 1)) || P > S || !width || width > S / P || blocks > 0x7fffffffu)
    gpqhe_die("k_pack_enc_gather: %u ciphertexts of %u slots, %u loops of width %u in one chunk", cnt, S, P, width);
  ProfScope ps(KC_PACK_ENC_GATHER, 16.0 * cnt * ((double)P * width + S));  // z read, v written
  hipLaunchKernelGGL(pack_enc_gather_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, (pack_d2 *)v,
                     (const pack_d2 *)z, total, (unsigned)__builtin_ctz(S), (unsigned)__builtin_ctz(P), width);
  HIP_CHECK(hipGetLastError());
}

// out [cnt][P][rows] <- z [cnt][S]; total = cnt P rows values, per = P rows.
// grid: (total / TPB).
__global__ void __launch_bounds__(TPB) pack_dcd_gather_kernel(pack_d2 *out, const pack_d2 *z, size_t total, unsigned per,
                                                              unsigned rows, unsigned logS, unsigned logP)
{
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total)
    return;
  const size_t c = o / per;
  const unsigned r = (unsigned)(o - c * per);
  const unsigned p = r / rows, k = r - p * rows;
  out[o] = z[(c << logS) + ((size_t)k << logP) + p];
}

void k_pack_dcd_gather(double *out, const double *z, unsigned S, unsigned P, unsigned rows, unsigned cnt)
{
  const size_t total = (size_t)cnt * P * rows, blocks = (total + TPB - 1) / TPB;
  if (!cnt || !S || (S & (S - 1)) || !P || (P & (P - 1)) || P > S || !rows || rows > S / P || blocks > 0x7fffffffu)
    gpqhe_die("k_pack_dcd_gather: %u ciphertexts of %u slots, %u loops of %u rows in one chunk", cnt, S, P, rows);
  ProfScope ps(KC_PACK_DCD_GATHER, 16.0 * total * 2);  // the gathered values read and written
  hipLaunchKernelGGL(pack_dcd_gather_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, (pack_d2 *)out,
                     (const pack_d2 *)z, total, P * rows, rows, (unsigned)__builtin_ctz(S), (unsigned)__builtin_ctz(P));
  HIP_CHECK(hipGetLastError());
}
