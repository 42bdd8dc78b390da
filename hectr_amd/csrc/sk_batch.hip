// sk_batch.hip - gfx950 kernels of he_enc_sk_batch and its packed forms
// (include/gpqhe_ext_sk_batch.h; host side: api.cpp).  A chunk of cnt
// ciphertexts x [cnt][2][nl][n] under the secret key:
//   enc_sk_sample_batch_kernel   E [cnt][nl][n] <- e + m lifted to the level's
//                                moduli (coefficient form), and c1 =
//                                x[c][1][m][k] <- the uniform sample, canonical
//   (ntt_polys over E: one transform per ciphertext)
//   enc_sk_combine_batch_kernel  c0 = x[c][0] <- E - c1 s
// No LDS and no scratch.
#include "gpqhe_internal.h"
#include "ntt_device.h"

#define TPB 256

typedef unsigned long long sk_u2 __attribute__((ext_vector_type(2)));

// grid: (n / TPB, cnt, 1 + ceil(nl / 4)); one coefficient k of ciphertext
// c = blockIdx.y per thread.
// z = 0: the noise.  enc_sample_batch_kernel's e0 branch for one polynomial per
// ciphertext: the CBD-21 value of block k of stream `stream + 2 c + 1`, plus
// the plaintext's coefficient where k is a multiple of the gap 2^logT (coef
// [cnt][m2], value j is coefficient j 2^logT), lifted to every limb of E.
// z = 1 + j: limbs 4 j .. 4 j + 3 of c1 from ONE block, k nb + j of stream
// `stream + 2 c` (sample_uniform_kernel's values; it computes the block once
// per limb): words 4 t .. 4 t + 3 as a 128-bit little-endian integer mod
// q_(4 j + t) (chacha_u128_mod).  A grid of depth 1 runs the noise alone (the
// seeded form, seeded_batch.hip: x unread).
__global__ void __launch_bounds__(TPB)
  enc_sk_sample_batch_kernel(uint64_t *x, uint64_t *E, unsigned logn, unsigned nl, unsigned nb, ChachaKey key,
                             uint64_t stream, const int64_t *coef, unsigned logT, unsigned m2, const ModConst *mc,
                             SkQinv qi)
{
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (1u << logn))
    return;
  const size_t c = blockIdx.y, w = (size_t)nl << logn;
  uint32_t b[16];
  if (blockIdx.z == 0) {
    chacha20_block(b, key, stream + 2 * c + 1, k);
    const int v = __popc(b[0] & 0x1FFFFFu) - __popc(b[1] & 0x1FFFFFu);
    const bool addm = !(k & ((1u << logT) - 1));
    const int64_t mco = addm ? coef[c * m2 + (k >> logT)] : 0;
    uint64_t *dst = E + c * w + k;
    for (unsigned l = 0; l < nl; l++) {
      const ModConst &m = mc[l];
      uint64_t r = v >= 0 ? (uint64_t)v : m.q - (uint64_t)(-v);
      if (addm)
        r = add_mod(r, lift_i64(mco, m), m.q);
      dst[(size_t)l << logn] = r;
    }
    return;
  }
  const unsigned j = blockIdx.z - 1;
  chacha20_block(b, key, stream + 2 * c, k * nb + j);
  uint64_t *dst = x + (2 * c + 1) * w + k;
#pragma unroll
  for (unsigned t = 0; t < 4; t++) {
    const unsigned l = 4 * j + t;
    if (l >= nl)  // (workgroup-uniform)
      break;
    dst[(size_t)l << logn] = chacha_u128_mod(b + 4 * t, mc[l], qi.v[l]);
  }
}

void k_enc_sk_sample_batch(uint64_t *x, uint64_t *E, uint64_t stream, const int64_t *coef, unsigned s, unsigned nl,
                           unsigned cnt, bool noise_only)
{
  if (!cnt || cnt > 65535 || !nl || nl > G.L)
    gpqhe_die("k_enc_sk_sample_batch: %u ciphertexts at level %u in one chunk", cnt, nl);
  const unsigned logT = G.logn - 1 - (unsigned)__builtin_ctz(s);
  // both polynomials (noise_only: E alone) written, the compact coefficients read
  ProfScope ps(KC_ENC_SK_SAMPLE_BATCH, 8.0 * G.n * nl * (noise_only ? 1 : 2) * cnt + 16.0 * s * cnt);
  SkQinv qi;
  for (unsigned l = 0; l < GPQHE_MAXMOD; l++)
    qi.v[l] = l < nl ? 1.0 / (double)G.q[l] : 0.0;
  const dim3 grid((G.n + TPB - 1) / TPB, cnt, noise_only ? 1 : 1 + (nl + 3) / 4);
  hipLaunchKernelGGL(enc_sk_sample_batch_kernel, grid, dim3(TPB), 0, G.stream, x, E, G.logn, nl, (G.nmod + 3) / 4,
                     G.key, stream, coef, logT, 2 * s, G.dev.mc, qi);
  HIP_CHECK(hipGetLastError());
}

// c0 = E - c1 s on two adjacent words of limb l0 + blockIdx.y (16-byte
// accesses), the secret-key words held in registers across the IOB_CG
// ciphertexts of group blockIdx.z; a group's operands are all loaded before
// the first store.  Per limb word two words read and one written.
// F64 (q < 2^51): the product f64_mulmod_h of canonical words is an exact
// integer below 1.25 q in magnitude, so e - p is one below 2.25 q < 2^53 and
// f64_canon returns its canonical residue; otherwise the Barrett mul_mod.
// grid: (n / 2 / TPB, limbs of the launch, cnt / IOB_CG).
template <bool F64>
__global__ void __launch_bounds__(TPB)
  enc_sk_combine_batch_kernel(uint64_t *x, const uint64_t *E, const uint64_t *sk, unsigned logn, unsigned nl,
                              unsigned l0, unsigned cnt, const ModConst *mc)
{
  const size_t k = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (k >= ((size_t)1 << logn))
    return;
  const unsigned l = l0 + blockIdx.y;
  const ModConst m = mc[l];
  const size_t o = ((size_t)l << logn) + k, w = (size_t)nl << logn;
  const sk_u2 sv = *(const sk_u2 *)(sk + o);
  const unsigned cb = blockIdx.z * IOB_CG;
  sk_u2 a[IOB_CG], e[IOB_CG];
#pragma unroll
  for (unsigned cc = 0; cc < IOB_CG; cc++)
    if (cb + cc < cnt) {  // (workgroup-uniform)
      a[cc] = *(const sk_u2 *)(x + (2 * (size_t)(cb + cc) + 1) * w + o);
      e[cc] = *(const sk_u2 *)(E + (size_t)(cb + cc) * w + o);
    }
  const double q = (double)m.q, qinv = 1.0 / q;
  const double s0 = f64_from_u52(sv.x), s1 = f64_from_u52(sv.y);  // (F64 only: words below 2^51)
#pragma unroll
  for (unsigned cc = 0; cc < IOB_CG; cc++)
    if (cb + cc < cnt) {
      sk_u2 r;
      if (F64) {
        r.x = f64_canon(f64_from_u52(e[cc].x) - f64_mulmod_h(f64_from_u52(a[cc].x), s0, q, qinv), q, qinv);
        r.y = f64_canon(f64_from_u52(e[cc].y) - f64_mulmod_h(f64_from_u52(a[cc].y), s1, q, qinv), q, qinv);
      } else {
        r.x = sub_mod(e[cc].x, mul_mod(a[cc].x, sv.x, m), m.q);
        r.y = sub_mod(e[cc].y, mul_mod(a[cc].y, sv.y, m), m.q);
      }
      *(sk_u2 *)(x + 2 * (size_t)(cb + cc) * w + o) = r;
    }
}

void k_enc_sk_combine_chunk(uint64_t *x, const uint64_t *E, const uint64_t *sk, unsigned nl, unsigned cnt)
{
  const unsigned groups = (cnt + IOB_CG - 1) / IOB_CG;
  if (!cnt || groups > 65535 || !nl || nl > G.L)
    gpqhe_die("k_enc_sk_combine_chunk: %u ciphertexts at level %u in one chunk", cnt, nl);
  const unsigned bx = (unsigned)((G.n / 2 + TPB - 1) / TPB);
  // limbs in runs of one arithmetic: FP64 below 2^51, Barrett above
  for (unsigned la = 0, lb; la < nl; la = lb) {
    const bool f64 = G.q[la] < F64_QMAX;
    for (lb = la + 1; lb < nl && (G.q[lb] < F64_QMAX) == f64; lb++)
      ;
    ProfScope ps(KC_ENC_SK_COMBINE_BATCH, 8.0 * G.n * (lb - la) * (3.0 * cnt + groups));
    const dim3 grid(bx, lb - la, groups);
    if (f64)
      hipLaunchKernelGGL(enc_sk_combine_batch_kernel<true>, grid, dim3(TPB), 0, G.stream, x, E, sk, G.logn, nl, la, cnt,
                         G.dev.mc);
    else
      hipLaunchKernelGGL(enc_sk_combine_batch_kernel<false>, grid, dim3(TPB), 0, G.stream, x, E, sk, G.logn, nl, la,
                         cnt, G.dev.mc);
    HIP_CHECK(hipGetLastError());
  }
}
