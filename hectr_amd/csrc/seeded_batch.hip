// seeded_batch.hip - gfx950 kernels of he_enc_sk_seeded_batch, its packed
// forms and he_expand_seeded_batch (include/gpqhe_ext_seeded_batch.h; host
// side: api.cpp).  c1 of a secret-key ciphertext is the uniform sample a of a
// PUBLIC ChaCha key and stream, so the client never stores it and the cloud
// regenerates it.  A chunk of cnt ciphertexts, compact c0 [cnt][nl][n]:
//   (enc_sk_sample_batch_kernel's noise branch: c0 <- e + m; ntt_polys over c0)
//   enc_sk_seeded_combine_kernel  c0 <- c0 - a s in place, a from its block
//   seeded_expand_kernel          x [cnt][2][nl][n] <- (c0, a)
// Both compute one ChaCha block per four limbs of a coefficient and reduce its
// quarters with chacha_u128_mod, sk_batch.hip's sample.  No LDS and no scratch.
#include "gpqhe_internal.h"
#include "ntt_device.h"

#define TPB 256

// c0 <- c0 - a s on limbs 4 j .. 4 j + 3 (j = blockIdx.y) of coefficient k, one
// per thread, over the IOB_CG ciphertexts of group blockIdx.z: the thread's (up
// to) four secret-key words stay in registers across them.  Per ciphertext the
// c0 words are loaded first, so their latency hides behind the cipher; a is
// block k nb + j of stream `stream + c` under the public key.  Per limb word
// one word read and one written (+ the key words once a group).
// q < 2^51: the product f64_mulmod_h of canonical words is an exact integer
// below 1.25 q in magnitude, so e - p is one below 2.25 q < 2^53 and f64_canon
// returns its canonical residue (enc_sk_combine_batch_kernel's step);
// otherwise the Barrett mul_mod.  The limbs of one block may be of both kinds
// (workgroup-uniform branches).
// grid: (n / TPB, ceil(nl / 4), ceil(cnt / IOB_CG)).
__global__ void __launch_bounds__(TPB)
  enc_sk_seeded_combine_kernel(uint64_t *c0, const uint64_t *sk, unsigned logn, unsigned nl, unsigned nb,
                               ChachaKey key, uint64_t stream, unsigned cnt, const ModConst *mc, SkQinv qi)
{
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (1u << logn))
    return;
  const unsigned j = blockIdx.y, l0 = 4 * j;
  const size_t w = (size_t)nl << logn;
  uint64_t sv[4];
#pragma unroll
  for (unsigned t = 0; t < 4; t++)
    sv[t] = l0 + t < nl ? sk[((size_t)(l0 + t) << logn) + k] : 0;
  const unsigned cb = blockIdx.z * IOB_CG, ce = min(cb + IOB_CG, cnt);
#pragma unroll 1
  for (unsigned c = cb; c < ce; c++) {
    uint64_t *p = c0 + c * w + ((size_t)l0 << logn) + k;
    uint64_t e[4];
#pragma unroll
    for (unsigned t = 0; t < 4; t++)
      e[t] = l0 + t < nl ? p[(size_t)t << logn] : 0;
    uint32_t b[16];
    chacha20_block(b, key, stream + c, k * nb + j);
#pragma unroll
    for (unsigned t = 0; t < 4; t++) {
      const unsigned l = l0 + t;
      if (l >= nl)  // (workgroup-uniform)
        break;
      const ModConst &m = mc[l];
      const uint64_t a = chacha_u128_mod(b + 4 * t, m, qi.v[l]);
      uint64_t r;
      if (m.q < F64_QMAX) {  // (workgroup-uniform)
        const double q = (double)m.q, qinv = qi.v[l];
        r = f64_canon(f64_from_u52(e[t]) - f64_mulmod_h(f64_from_u52(a), f64_from_u52(sv[t]), q, qinv), q, qinv);
      } else {
        r = sub_mod(e[t], mul_mod(a, sv[t], m), m.q);
      }
      p[(size_t)t << logn] = r;
    }
  }
}

static SkQinv level_qinv(unsigned nl)
{
  SkQinv qi;
  for (unsigned l = 0; l < GPQHE_MAXMOD; l++)
    qi.v[l] = l < nl ? 1.0 / (double)G.q[l] : 0.0;
  return qi;
}

void k_enc_sk_seeded_combine(uint64_t *c0, const uint64_t *sk, const ChachaKey &pub, uint64_t pstream, unsigned nl,
                             unsigned cnt)
{
  const unsigned groups = (cnt + IOB_CG - 1) / IOB_CG;
  if (!cnt || groups > 65535 || !nl || nl > G.L)
    gpqhe_die("k_enc_sk_seeded_combine: %u ciphertexts at level %u in one chunk", cnt, nl);
  // a word read and a word written per limb word, the key words once a group
  ProfScope ps(KC_ENC_SK_SEEDED_COMBINE, 8.0 * G.n * nl * (2.0 * cnt + groups));
  hipLaunchKernelGGL(enc_sk_seeded_combine_kernel, dim3((G.n + TPB - 1) / TPB, (nl + 3) / 4, groups), dim3(TPB), 0,
                     G.stream, c0, sk, G.logn, nl, (G.nmod + 3) / 4, pub, pstream, cnt, G.dev.mc, level_qinv(nl));
  HIP_CHECK(hipGetLastError());
}

// x[c] <- (c0[c], a) on limbs 4 j .. 4 j + 3 (j = blockIdx.z) of coefficient k
// of ciphertext c = blockIdx.y, one per thread: the c0 words loaded, the block
// computed and reduced, up to four words of each polynomial stored.  Per limb
// word one word read and two written.
// grid: (n / TPB, cnt, ceil(nl / 4)).
__global__ void __launch_bounds__(TPB)
  seeded_expand_kernel(uint64_t *x, const uint64_t *c0, unsigned logn, unsigned nl, unsigned nb, ChachaKey key,
                       uint64_t stream, const ModConst *mc, SkQinv qi)
{
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (1u << logn))
    return;
  const unsigned j = blockIdx.z, l0 = 4 * j;
  const size_t c = blockIdx.y, w = (size_t)nl << logn, o = ((size_t)l0 << logn) + k;
  const uint64_t *src = c0 + c * w + o;
  uint64_t *d0 = x + 2 * c * w + o, *d1 = d0 + w;
  uint64_t e[4];
#pragma unroll
  for (unsigned t = 0; t < 4; t++)
    e[t] = l0 + t < nl ? src[(size_t)t << logn] : 0;
  uint32_t b[16];
  chacha20_block(b, key, stream + c, k * nb + j);
#pragma unroll
  for (unsigned t = 0; t < 4; t++) {
    const unsigned l = l0 + t;
    if (l >= nl)  // (workgroup-uniform)
      break;
    d1[(size_t)t << logn] = chacha_u128_mod(b + 4 * t, mc[l], qi.v[l]);
    d0[(size_t)t << logn] = e[t];
  }
}

void k_seeded_expand(uint64_t *x, const uint64_t *c0, const ChachaKey &pub, uint64_t pstream, unsigned nl,
                     unsigned cnt)
{
  if (!cnt || cnt > 65535 || !nl || nl > G.L)
    gpqhe_die("k_seeded_expand: %u ciphertexts at level %u in one chunk", cnt, nl);
  ProfScope ps(KC_SEEDED_EXPAND, 8.0 * G.n * nl * 3.0 * cnt);
  hipLaunchKernelGGL(seeded_expand_kernel, dim3((G.n + TPB - 1) / TPB, cnt, (nl + 3) / 4), dim3(TPB), 0, G.stream, x,
                     c0, G.logn, nl, (G.nmod + 3) / 4, pub, pstream, G.dev.mc, level_qinv(nl));
  HIP_CHECK(hipGetLastError());
}
