// encgain_batch.hip - gfx950 kernels of he_gemv2_encgain_packed_batch /
// he_hempc_step_encgain_packed_batch (include/gpqhe_ext_encgain_batch.h; host
// side: api.cpp).  The gains arrive as ciphertexts, so the sum over the
// 2 m' (rotated input, encrypted diagonal) pairs is a sum of ciphertext tensor
// products; it is formed before anything is relinearised:
//   encgain_tensor_kernel  X0 = sum c0 d0, X1 = sum (c0 d1 + c1 d0),
//                          X2 = sum c1 d1 over the 2 m' pairs of a chunk, and
//                          the (0, X2) ciphertext the relinearisation reads
//   encgain_ones_kernel    the ciphertext (0, 1) of every pair of the chunk
// Canonical residues in and out, two 8-byte words (one 16-byte access) per
// lane, no LDS and no scratch.
#include "gpqhe_internal.h"
#include "ntt_device.h"

#define TPB 256

typedef unsigned long long eg_u2 __attribute__((ext_vector_type(2)));

// (hi : lo) mod q, any 128-bit value (reduce64 takes any 64-bit word)
__device__ __forceinline__ uint64_t eg_red128(unsigned __int128 v, const ModConst &m)
{
  const uint64_t hi = reduce64((uint64_t)(v >> 64), m), lo = reduce64((uint64_t)v, m);
  return add_mod(mul_mod(hi, m.r64, m), lo, m.q);
}

// Lazy sums of one word of one ciphertext.
// F64 (q < 2^51): signed doubles holding exact integers.  A product
// f64_mulmod_h of canonical words is below 1.25 q in magnitude and a reduced
// sum at most q / 2, so with a reduction per term x1 peaks at 3 q and x0, x2
// at 1.75 q, all below 2^53.
// Integer (q < 2^61): 128-bit sums, reduced to one word every 16 terms: x1
// holds at most 32 products and one residue, 32 (2^61 - 1)^2 + 2^61 < 2^128.
template <bool F64> struct EgAcc;

template <> struct EgAcc<true> {
  double x0 = 0, x1 = 0, x2 = 0;
  __device__ __forceinline__ void term(uint64_t c0, uint64_t c1, uint64_t d0, uint64_t d1, unsigned, const ModConst &,
                                       double q, double qinv)
  {
    const double a0 = f64_from_u52(c0), a1 = f64_from_u52(c1), b0 = f64_from_u52(d0), b1 = f64_from_u52(d1);
    x0 = f64_red(x0 + f64_mulmod_h(a0, b0, q, qinv), q, qinv);
    x1 = f64_red(x1 + f64_mulmod_h(a0, b1, q, qinv) + f64_mulmod_h(a1, b0, q, qinv), q, qinv);
    x2 = f64_red(x2 + f64_mulmod_h(a1, b1, q, qinv), q, qinv);
  }
  __device__ __forceinline__ void out(uint64_t &r0, uint64_t &r1, uint64_t &r2, const ModConst &, double q,
                                      double qinv) const
  {
    r0 = f64_canon(x0, q, qinv);
    r1 = f64_canon(x1, q, qinv);
    r2 = f64_canon(x2, q, qinv);
  }
};

template <> struct EgAcc<false> {
  unsigned __int128 x0 = 0, x1 = 0, x2 = 0;
  __device__ __forceinline__ void term(uint64_t c0, uint64_t c1, uint64_t d0, uint64_t d1, unsigned t,
                                       const ModConst &m, double, double)
  {
    x0 += (unsigned __int128)c0 * d0;
    x1 += (unsigned __int128)c0 * d1;
    x1 += (unsigned __int128)c1 * d0;
    x2 += (unsigned __int128)c1 * d1;
    if ((t & 15) == 15) {  // (wave-uniform)
      x0 = eg_red128(x0, m);
      x1 = eg_red128(x1, m);
      x2 = eg_red128(x2, m);
    }
  }
  __device__ __forceinline__ void out(uint64_t &r0, uint64_t &r1, uint64_t &r2, const ModConst &m, double,
                                      double) const
  {
    r0 = eg_red128(x0, m);
    r1 = eg_red128(x1, m);
    r2 = eg_red128(x2, m);
  }
};

// Term t < 2 mp of ciphertext c: the pair (rot(xa, t P), DA_t) for t < mp, else
// (rot(xb, (t - mp) P), DB_(t - mp)).  Rotation 0 is xa / xb itself ([cnt][2][lvl][n]),
// rotation i >= 1 slot i - 1 of Ra / Rb ([mp - 1][cnt][2][lvl][n]); DA, DB
// [mp][2][lvl][n].  X01 [cnt][2][lvl][n] <- (X0, X1), Q [cnt][2][lvl][n] <- (0, X2).
// A workgroup holds a term's diagonal words in registers across CG
// ciphertexts.  grid: (n / 2 / TPB, limbs of the launch, cnt / CG); limb
// l0 + blockIdx.y.
template <bool F64, int CG>
__global__ void __launch_bounds__(TPB)
  encgain_tensor_kernel(uint64_t *X01, uint64_t *Q, const uint64_t *xa, const uint64_t *xb, const uint64_t *Ra,
                        const uint64_t *Rb, const uint64_t *DA, const uint64_t *DB, unsigned mp, unsigned cnt,
                        unsigned lvl, unsigned l0, unsigned logn, const ModConst *mc)
{
  const size_t k = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (k >= ((size_t)1 << logn))
    return;
  const unsigned l = l0 + blockIdx.y;
  const ModConst m = mc[l];
  const double q = (double)m.q, qinv = 1.0 / q;
  const size_t pw = (size_t)lvl << logn, cw = 2 * pw, sw = (size_t)cnt * cw;
  const size_t o = ((size_t)l << logn) + k;
  const unsigned cb = blockIdx.z * CG;
  EgAcc<F64> acc[CG][2];
  for (unsigned t = 0; t < 2 * mp; t++) {
    const bool second = t >= mp;
    const unsigned i = second ? t - mp : t;
    const uint64_t *d = (second ? DB : DA) + (size_t)i * cw + o;
    const uint64_t *x = i ? (second ? Rb : Ra) + (size_t)(i - 1) * sw : (second ? xb : xa);
    const eg_u2 d0 = *(const eg_u2 *)d, d1 = *(const eg_u2 *)(d + pw);
#pragma unroll
    for (int cc = 0; cc < CG; cc++) {
      if (cb + cc >= cnt)  // (workgroup-uniform)
        break;
      const uint64_t *xc = x + (size_t)(cb + cc) * cw + o;
      const eg_u2 c0 = *(const eg_u2 *)xc, c1 = *(const eg_u2 *)(xc + pw);
      acc[cc][0].term(c0.x, c1.x, d0.x, d1.x, t, m, q, qinv);
      acc[cc][1].term(c0.y, c1.y, d0.y, d1.y, t, m, q, qinv);
    }
  }
#pragma unroll
  for (int cc = 0; cc < CG; cc++) {
    if (cb + cc >= cnt)
      break;
    uint64_t r0[2], r1[2], r2[2];
    acc[cc][0].out(r0[0], r1[0], r2[0], m, q, qinv);
    acc[cc][1].out(r0[1], r1[1], r2[1], m, q, qinv);
    const size_t oc = (size_t)(cb + cc) * cw + o;
    *(eg_u2 *)(X01 + oc) = eg_u2{r0[0], r0[1]};
    *(eg_u2 *)(X01 + oc + pw) = eg_u2{r1[0], r1[1]};
    *(eg_u2 *)(Q + oc) = eg_u2{0, 0};
    *(eg_u2 *)(Q + oc + pw) = eg_u2{r2[0], r2[1]};
  }
}

constexpr int EG_CG_F64 = 4, EG_CG_INT = 2;

void k_encgain_tensor(uint64_t *X01, uint64_t *Q, const uint64_t *xa, const uint64_t *xb, const uint64_t *Ra,
                      const uint64_t *Rb, const uint64_t *DA, const uint64_t *DB, unsigned mp, unsigned lvl,
                      unsigned cnt)
{
  if (!cnt || !mp || !lvl || cnt > 65535 * EG_CG_INT)
    gpqhe_die("k_encgain_tensor: %u ciphertexts, %u diagonals at level %u in one chunk", cnt, mp, lvl);
  const unsigned bx = (unsigned)((G.n / 2 + TPB - 1) / TPB);
  // limbs in runs of one arithmetic: FP64 below 2^51, 128-bit integer sums above
  for (unsigned la = 0, lb; la < lvl; la = lb) {
    const bool f64 = G.q[la] < F64_QMAX;
    for (lb = la + 1; lb < lvl && (G.q[lb] < F64_QMAX) == f64; lb++)
      ;
    const unsigned cg = f64 ? EG_CG_F64 : EG_CG_INT, groups = (cnt + cg - 1) / cg;
    // per limb: both words of 2 mp inputs per ciphertext and of 2 mp diagonals
    // per group read, four words per ciphertext written
    ProfScope ps(KC_ENCGAIN_TENSOR, 8.0 * G.n * (lb - la) * ((4.0 * mp + 4.0) * cnt + 4.0 * mp * groups));
    const dim3 grid(bx, lb - la, groups);
    if (f64)
      hipLaunchKernelGGL((encgain_tensor_kernel<true, EG_CG_F64>), grid, dim3(TPB), 0, G.stream, X01, Q, xa, xb, Ra, Rb,
                         DA, DB, mp, cnt, lvl, la, G.logn, G.dev.mc);
    else
      hipLaunchKernelGGL((encgain_tensor_kernel<false, EG_CG_INT>), grid, dim3(TPB), 0, G.stream, X01, Q, xa, xb, Ra,
                         Rb, DA, DB, mp, cnt, lvl, la, G.logn, G.dev.mc);
    HIP_CHECK(hipGetLastError());
  }
}

// one [cnt][2][lvl][n] <- (0, 1) per ciphertext: polynomial p of the chunk is
// all p mod 2.  total = cnt 2 lvl n words.  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) encgain_ones_kernel(uint64_t *one, size_t total, unsigned lvl, unsigned logn)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const unsigned long long v = ((w >> logn) / lvl) & 1;
  *(eg_u2 *)(one + w) = eg_u2{v, v};
}

void k_encgain_ones(uint64_t *one, unsigned lvl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * lvl << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || !lvl || blocks > 0x7fffffffu)
    gpqhe_die("k_encgain_ones: %u ciphertexts at level %u in one chunk", cnt, lvl);
  ProfScope ps(KC_ENCGAIN_ONES, 8.0 * total);
  hipLaunchKernelGGL(encgain_ones_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, one, total, lvl, G.logn);
  HIP_CHECK(hipGetLastError());
}
