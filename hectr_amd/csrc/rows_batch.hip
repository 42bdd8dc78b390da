// rows_batch.hip - gfx950 kernels of he_gemv2_rows_batch / he_hempc_step_rows_batch
// (include/gpqhe_ext_rows_batch.h; host side: api.cpp).  The fold of the
// row-folded product, u += rot(u, r) over a chunk of ciphertexts at level
// lvl - 1, with the rotation R already in a workspace.  Two streaming kernels,
// canonical residues in and out, two 8-byte words (one 16-byte access) per
// lane, no LDS and no scratch:
//   rows_fold_add_batch_kernel   y = y + R
//   rows_fold_tail_batch_kernel  up = uhat (its lower limbs) - (y + R): the
//                                last fold step of a step call and its tail
#include "gpqhe_internal.h"

#define TPB 256

typedef unsigned long long rows_u2 __attribute__((ext_vector_type(2)));

// y [cnt][2][nl][n] += R (same layout), total = cnt 2 nl n words; a word pair
// never straddles a limb (n is even).  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) rows_fold_add_batch_kernel(uint64_t *y, const uint64_t *R, size_t total,
                                                                  unsigned nl, unsigned logn, const ModConst *mc)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const uint64_t q = mc[(unsigned)((w >> logn) % nl)].q;
  const rows_u2 a = *(const rows_u2 *)(y + w), b = *(const rows_u2 *)(R + w);
  *(rows_u2 *)(y + w) = rows_u2{add_mod(a.x, b.x, q), add_mod(a.y, b.y, q)};
}

void k_rows_fold_add_batch(uint64_t *y, const uint64_t *R, unsigned nl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * nl << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || !nl || blocks > 0x7fffffffu)
    gpqhe_die("k_rows_fold_add_batch: %u ciphertexts at level %u in one chunk", cnt, nl);
  ProfScope ps(KC_ROWS_FOLD_ADD_BATCH, 8.0 * total * 3);  // y and R read, y written
  hipLaunchKernelGGL(rows_fold_add_batch_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, y, R, total, nl,
                     G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// up [cnt][2][lvl-1][n] <- uhat [cnt][2][lvl][n] (limbs below lvl - 1) - (up + R):
// the last u = he_add(u, he_rot(u, r)) and he_add(he_moddown(copy of uhat),
// he_neg(u)) in one pass, sub_mod being the canonical result of add(c, neg(u)).
// total = cnt 2 (lvl - 1) n words of up and of R; polynomial p = w / ((lvl - 1) n)
// of the chunk starts p lvl n words into uhat.  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) rows_fold_tail_batch_kernel(uint64_t *up, const uint64_t *R,
                                                                   const uint64_t *uhat, size_t total, unsigned lvl,
                                                                   unsigned logn, const ModConst *mc)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const size_t row = w >> logn;  // (polynomial, limb) of up
  const size_t p = row / (lvl - 1);
  const unsigned l = (unsigned)(row - p * (lvl - 1));
  const uint64_t q = mc[l].q;
  const rows_u2 c = *(const rows_u2 *)(uhat + (((p * lvl + l) << logn) | (w & (((size_t)1 << logn) - 1))));
  const rows_u2 v = *(const rows_u2 *)(up + w), r = *(const rows_u2 *)(R + w);
  *(rows_u2 *)(up + w) = rows_u2{sub_mod(c.x, add_mod(v.x, r.x, q), q), sub_mod(c.y, add_mod(v.y, r.y, q), q)};
}

void k_rows_fold_tail_batch(uint64_t *up, const uint64_t *R, const uint64_t *uhat, unsigned lvl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * (lvl - 1) << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || lvl < 2 || blocks > 0x7fffffffu)
    gpqhe_die("k_rows_fold_tail_batch: %u ciphertexts at level %u in one chunk", cnt, lvl);
  ProfScope ps(KC_ROWS_FOLD_TAIL_BATCH, 8.0 * total * 4);  // uhat's lower limbs, up and R read, up written
  hipLaunchKernelGGL(rows_fold_tail_batch_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, up, R, uhat, total,
                     lvl, G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}
