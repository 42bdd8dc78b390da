// step_batch.hip - gfx950 kernels of he_hempc_step_batch
// (include/gpqhe_ext_step_batch.h; host side: api.cpp).  Two streaming
// kernels over a chunk of ciphertexts, canonical residues in and out, two
// 8-byte words (one 16-byte access) per lane, no LDS and no scratch:
//   step_diff_batch_kernel  xd = xhat - xr and ud = uhat - ur in one launch
//   step_tail_batch_kernel  up = uhat (its lower limbs) - w, w already in up
#include "gpqhe_internal.h"

#define TPB 256

typedef unsigned long long step_u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ step_u2 step_sub2(step_u2 a, step_u2 b, uint64_t q)
{
  return step_u2{sub_mod(a.x, b.x, q), sub_mod(a.y, b.y, q)};
}

// xd = xhat - xr, ud = uhat - ur, all six [cnt][2][lvl][n], total = cnt 2 lvl n
// words; a word pair never straddles a limb (n is even).  The inputs may be
// one another; an output is none of them.  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) step_diff_batch_kernel(uint64_t *xd, uint64_t *ud, const uint64_t *xhat,
                                                              const uint64_t *xr, const uint64_t *uhat,
                                                              const uint64_t *ur, size_t total, unsigned lvl,
                                                              unsigned logn, const ModConst *mc)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const uint64_t q = mc[(unsigned)((w >> logn) % lvl)].q;
  const step_u2 a = *(const step_u2 *)(xhat + w), b = *(const step_u2 *)(xr + w);
  const step_u2 c = *(const step_u2 *)(uhat + w), d = *(const step_u2 *)(ur + w);
  *(step_u2 *)(xd + w) = step_sub2(a, b, q);
  *(step_u2 *)(ud + w) = step_sub2(c, d, q);
}

void k_step_diff_batch(uint64_t *xd, uint64_t *ud, const uint64_t *xhat, const uint64_t *xr, const uint64_t *uhat,
                       const uint64_t *ur, unsigned lvl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * lvl << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || blocks > 0x7fffffffu)
    gpqhe_die("k_step_diff_batch: %u ciphertexts in one chunk", cnt);
  ProfScope ps(KC_STEP_DIFF_BATCH, 8.0 * total * 6);  // four reads and two writes per word
  hipLaunchKernelGGL(step_diff_batch_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, xd, ud, xhat, xr, uhat, ur,
                     total, lvl, G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// up [cnt][2][lvl-1][n] <- uhat [cnt][2][lvl][n] (limbs below lvl - 1) - up:
// he_add(he_moddown(copy of uhat), he_neg(w)) with w what the rescale left in
// up, sub_mod being the canonical result of add(c, neg(w)).  total = cnt 2
// (lvl - 1) n words of up; polynomial p = w / ((lvl - 1) n) of the chunk starts
// p lvl n words into uhat.  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) step_tail_batch_kernel(uint64_t *up, const uint64_t *uhat, size_t total,
                                                              unsigned lvl, unsigned logn, const ModConst *mc)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const size_t row = w >> logn;  // (polynomial, limb) of up
  const size_t p = row / (lvl - 1);
  const unsigned l = (unsigned)(row - p * (lvl - 1));
  const uint64_t q = mc[l].q;
  const step_u2 c = *(const step_u2 *)(uhat + (((p * lvl + l) << logn) | (w & (((size_t)1 << logn) - 1))));
  const step_u2 v = *(const step_u2 *)(up + w);
  *(step_u2 *)(up + w) = step_sub2(c, v, q);
}

void k_step_tail_batch(uint64_t *up, const uint64_t *uhat, unsigned lvl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * (lvl - 1) << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || lvl < 2 || blocks > 0x7fffffffu)
    gpqhe_die("k_step_tail_batch: %u ciphertexts at level %u in one chunk", cnt, lvl);
  ProfScope ps(KC_STEP_TAIL_BATCH, 8.0 * total * 3);  // uhat's lower limbs and w read, up written
  hipLaunchKernelGGL(step_tail_batch_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, up, uhat, total, lvl,
                     G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}
