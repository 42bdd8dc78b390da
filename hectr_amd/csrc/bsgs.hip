// bsgs.hip - gfx950 kernels of he_gemv_bsgs (include/gpqhe_ext.h; host side:
// api.cpp).  Three elementwise kernels over (limb, coefficient), canonical
// residues in and out, integer arithmetic that is right for every modulus
// below 2^61:
//   bsgs_ks_kernel     the key-switch inner products of a list of rotations
//   bsgs_inner_kernel  the plaintext inner sums u_j = sum_i P_j,i b_i
//   bsgs_sum_kernel    the sum of the rotated giant steps
// and the two of he_gemv_bsgs_batch (include/gpqhe_ext_batch.h) over a chunk
// of ciphertexts in slot-major buffers:
//   bsgs_inner_batch_kernel  the inner sums, a P word shared by a ciphertext tile
//   bsgs_sum_batch_kernel    the sum of the rotated giant steps of every ciphertext
#include "gpqhe_internal.h"

#define TPB 256

__device__ __forceinline__ unsigned bsgs_brev(unsigned x, unsigned bits)
{
  return __brev(x) >> (32 - bits);
}

// NTT-domain index map of the automorphism X -> X^g (kernels.hip auto_index)
__device__ __forceinline__ unsigned bsgs_auto_index(unsigned k, uint64_t g, unsigned logn)
{
  const uint64_t mask = (2ull << logn) - 1;
  const uint64_t e = ((2ull * bsgs_brev(k, logn) + 1) * g) & mask;
  return bsgs_brev((unsigned)(e >> 1), logn);
}

// Job r of a launch: acc0 / acc1 (over basis_qp(lvl), acc1 nm limbs after
// acc0) <- sum_j D_j[perm k] evk_j[k], plus [P] c0[perm k] into acc0 on the q
// limbs; perm the index map of Galois element g.  The arithmetic of
// ks_inner_kernel without a plaintext, one job per grid z.
// grid: (n / TPB, nm, jobs).
__global__ void __launch_bounds__(TPB) bsgs_ks_kernel(const BsgsKsJob *jobs, unsigned logn, unsigned lvl, unsigned L,
                                                      unsigned nm, unsigned nmod, unsigned ndig, const ModConst *mc)
{
  const size_t n = (size_t)1 << logn;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const BsgsKsJob job = jobs[blockIdx.z];
  const unsigned t = blockIdx.y;
  const unsigned m = t < lvl ? t : L + (t - lvl);
  const ModConst mm = mc[m];
  const size_t tl = (size_t)t << logn;
  const size_t src = bsgs_auto_index((unsigned)k, job.g, logn);
  uint64_t s0 = 0, s1 = 0;
  for (unsigned j = 0; j < ndig; j++) {
    const uint64_t dv = job.D[(((size_t)j * nm) << logn) + tl + src];
    s0 = add_mod(s0, mul_mod(dv, job.evk[(((size_t)(2 * j) * nmod + m) << logn) + k], mm), mm.q);
    s1 = add_mod(s1, mul_mod(dv, job.evk[(((size_t)(2 * j + 1) * nmod + m) << logn) + k], mm), mm.q);
  }
  if (t < lvl)
    s0 = add_mod(s0, mul_shoup(job.c0[tl + src], mm.pmod, mm.pmodp, mm.q), mm.q);
  job.acc[tl + k] = s0;
  job.acc[((size_t)nm << logn) + tl + k] = s1;
}

void k_bsgs_ks(const BsgsKsJob *jobs_dev, unsigned njobs, unsigned lvl, double bytes)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  if (!njobs || njobs > 65535)
    gpqhe_die("k_bsgs_ks: %u jobs", njobs);
  ProfScope ps(KC_BSGS_KS, bytes);
  hipLaunchKernelGGL(bsgs_ks_kernel, dim3((G.n + TPB - 1) / TPB, nm, njobs), dim3(TPB), 0, G.stream, jobs_dev, G.logn,
                     lvl, G.L, nm, G.nmod, ndig, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// (hi : lo) mod q for hi < 2^62: what a sum of 16 products of residues below
// 2^61 fits.
__device__ __forceinline__ uint64_t bsgs_red128(unsigned __int128 v, const ModConst &m)
{
  const uint64_t hi = reduce64((uint64_t)(v >> 64), m), lo = reduce64((uint64_t)v, m);
  return add_mod(mul_mod(hi, m.r64, m), lo, m.q);
}

typedef unsigned long long bsgs_u2 __attribute__((ext_vector_type(2)));

// u_j[p][l][k] = sum_i P[tab[j][i]][l][k] b_i[p][l][k] mod q_l for every
// giant step j of the launch: tab [nj][gs] names the encoded diagonal of
// (giant step j, baby slot i), -1 where M has none.  A thread owns one
// coefficient of one limb; the baby words of up to BSGS_TILE slots stay in its
// registers over the j loop, both polynomials, so every P word is read once
// and every b word once per tile.  Sums are 128-bit with one reduction per
// output.  With more than BSGS_TILE baby slots the later tiles add to what
// the first one wrote (the same thread's own words).  One 8-byte word per
// lane: the form with two (16-byte loads) holds 192 registers against 104 and
// measured 1.6x slower (profiles/bsgs_ab_words.txt).
// grid: (n / TPB, lvl).
#define BSGS_TILE 16
__global__ void __launch_bounds__(TPB) bsgs_inner_kernel(uint64_t *U, const uint64_t *B, const uint64_t *P,
                                                         const int *tab, unsigned nj, unsigned gs, unsigned lvl,
                                                         unsigned logn, const ModConst *mc)
{
  const size_t n = (size_t)1 << logn;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const unsigned l = blockIdx.y;
  const ModConst m = mc[l];
  const size_t pw = (size_t)lvl << logn;  // words of one polynomial
  const size_t lo = ((size_t)l << logn) + k;
  for (unsigned i0 = 0; i0 < gs; i0 += BSGS_TILE) {
    uint64_t b0[BSGS_TILE], b1[BSGS_TILE];
#pragma unroll
    for (int ii = 0; ii < BSGS_TILE; ii++) {
      b0[ii] = b1[ii] = 0;
      if (i0 + ii < gs) {
        const uint64_t *b = B + (size_t)(i0 + ii) * 2 * pw + lo;
        b0[ii] = b[0];
        b1[ii] = b[pw];
      }
    }
    for (unsigned j = 0; j < nj; j++) {
      const int *tj = tab + (size_t)j * gs + i0;
      unsigned __int128 a0 = 0, a1 = 0;
      bool any = false;
#pragma unroll
      for (int h = 0; h < BSGS_TILE; h += 8) {
        uint64_t w[8];
        int e[8];
#pragma unroll
        for (int ii = 0; ii < 8; ii++) {
          e[ii] = i0 + h + ii < gs ? tj[h + ii] : -1;  // (wave-uniform)
          w[ii] = 0;
          if (e[ii] >= 0)
            w[ii] = P[(size_t)e[ii] * pw + lo];
        }
#pragma unroll
        for (int ii = 0; ii < 8; ii++)
          if (e[ii] >= 0) {
            any = true;
            a0 += (unsigned __int128)w[ii] * b0[h + ii];
            a1 += (unsigned __int128)w[ii] * b1[h + ii];
          }
      }
      if (i0 && !any)
        continue;
      uint64_t *u = U + (size_t)j * 2 * pw + lo;
      uint64_t r0 = bsgs_red128(a0, m), r1 = bsgs_red128(a1, m);
      if (i0) {
        r0 = add_mod(r0, u[0], m.q);
        r1 = add_mod(r1, u[pw], m.q);
      }
      u[0] = r0;
      u[pw] = r1;
    }
  }
}

void k_bsgs_inner(uint64_t *U, const uint64_t *B, const uint64_t *P, const int *tab_dev, unsigned nj, unsigned gs,
                  unsigned ndiag, unsigned lvl)
{
  if (!nj || !gs)
    gpqhe_die("k_bsgs_inner: %u giant steps, %u baby slots", nj, gs);
  const unsigned tiles = (gs + BSGS_TILE - 1) / BSGS_TILE;
  // every P word once; the baby words once per tile; u written once (and
  // re-read and re-written by each later tile)
  ProfScope ps(KC_BSGS_INNER, 8.0 * G.n * lvl * ((double)ndiag + 2.0 * gs + 2.0 * nj * (2 * tiles - 1)));
  hipLaunchKernelGGL(bsgs_inner_kernel, dim3((G.n + TPB - 1) / TPB, lvl), dim3(TPB), 0, G.stream, U, B, P, tab_dev, nj,
                     gs, lvl, G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// out [2][lvl][n] = base (null: 0) + sum over t < cnt of R[t] ([2][lvl][n]
// each, r_stride words apart).  out may be base.  grid: (2 lvl n / 2 / TPB).
__global__ void __launch_bounds__(TPB) bsgs_sum_kernel(uint64_t *out, const uint64_t *base, const uint64_t *R,
                                                       unsigned cnt, size_t r_stride, unsigned lvl, unsigned logn,
                                                       const ModConst *mc)
{
  const size_t total = (size_t)2 * lvl << logn;
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const uint64_t q = mc[(unsigned)(w >> logn) % lvl].q;
  bsgs_u2 s{0, 0};
  if (base)
    s = *(const bsgs_u2 *)(base + w);
  for (unsigned t = 0; t < cnt; t++) {
    const bsgs_u2 r = *(const bsgs_u2 *)(R + t * r_stride + w);
    s = bsgs_u2{add_mod(s.x, r.x, q), add_mod(s.y, r.y, q)};
  }
  *(bsgs_u2 *)(out + w) = s;
}

void k_bsgs_sum(uint64_t *out, const uint64_t *base, const uint64_t *R, unsigned cnt, size_t r_stride, unsigned lvl)
{
  const size_t total = (size_t)2 * lvl << G.logn;
  ProfScope ps(KC_BSGS_SUM, 8.0 * total * (cnt + (base ? 2 : 1)));
  hipLaunchKernelGGL(bsgs_sum_kernel, dim3((unsigned)((total / 2 + TPB - 1) / TPB)), dim3(TPB), 0, G.stream, out, base,
                     R, cnt, r_stride, lvl, G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// The inner sums of a chunk of cnt ciphertexts: B [gs][cnt][2][lvl][n] ->
// U [nj][cnt][2][lvl][n], u_{c,j} = sum_i P[tab[j][i]] b_{c,i} as above.  A
// thread owns one (limb, coefficient) of a tile of CB ciphertexts (grid z):
// the baby words of TB slots of those CB ciphertexts stay in its registers
// over the j loop, and every P word it loads serves all CB of them, so P moves
// once per tile and not once per ciphertext.  Words per ciphertext and (limb,
// coefficient): ndiag / CB + 2 gs + 2 nj (2 ceil(gs / TB) - 1).  The last
// tile of a chunk may be partial: its missing ciphertexts load nothing and
// store nothing (wave-uniform).  128-bit sums, one reduction per output, later
// baby tiles add to what the same thread wrote.
// grid: (n / TPB, lvl, ceil(cnt / CB)).
template <int TB, int CB>
__global__ void __launch_bounds__(TPB) bsgs_inner_batch_kernel(uint64_t *U, const uint64_t *B, const uint64_t *P,
                                                               const int *tab, unsigned nj, unsigned gs, unsigned lvl,
                                                               unsigned logn, unsigned cnt, const ModConst *mc)
{
  const size_t n = (size_t)1 << logn;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const unsigned l = blockIdx.y, c0 = blockIdx.z * CB;
  const ModConst m = mc[l];
  const size_t pw = (size_t)lvl << logn;  // words of one polynomial
  const size_t sw = (size_t)cnt * 2 * pw;  // words of one slot (baby or giant) of the chunk
  const size_t lo = (size_t)c0 * 2 * pw + ((size_t)l << logn) + k;
  for (unsigned i0 = 0; i0 < gs; i0 += TB) {
    uint64_t b0[CB][TB], b1[CB][TB];
#pragma unroll
    for (int cc = 0; cc < CB; cc++)
#pragma unroll
      for (int ii = 0; ii < TB; ii++) {
        b0[cc][ii] = b1[cc][ii] = 0;
        if (i0 + ii < gs && c0 + cc < cnt) {
          const uint64_t *b = B + (size_t)(i0 + ii) * sw + (size_t)cc * 2 * pw + lo;
          b0[cc][ii] = b[0];
          b1[cc][ii] = b[pw];
        }
      }
    for (unsigned j = 0; j < nj; j++) {
      const int *tj = tab + (size_t)j * gs + i0;
      unsigned __int128 a0[CB], a1[CB];
#pragma unroll
      for (int cc = 0; cc < CB; cc++)
        a0[cc] = a1[cc] = 0;
      bool any = false;
#pragma unroll
      for (int h = 0; h < TB; h += 8) {
        uint64_t w[8];
        int e[8];
#pragma unroll
        for (int ii = 0; ii < 8; ii++) {
          e[ii] = i0 + h + ii < gs ? tj[h + ii] : -1;  // (wave-uniform)
          w[ii] = 0;
          if (e[ii] >= 0)
            w[ii] = P[(size_t)e[ii] * pw + ((size_t)l << logn) + k];
        }
#pragma unroll
        for (int ii = 0; ii < 8; ii++)
          if (e[ii] >= 0) {
            any = true;
#pragma unroll
            for (int cc = 0; cc < CB; cc++) {
              a0[cc] += (unsigned __int128)w[ii] * b0[cc][h + ii];
              a1[cc] += (unsigned __int128)w[ii] * b1[cc][h + ii];
            }
          }
      }
      if (i0 && !any)
        continue;
#pragma unroll
      for (int cc = 0; cc < CB; cc++) {
        if (c0 + cc >= cnt)
          continue;
        uint64_t *u = U + (size_t)j * sw + (size_t)cc * 2 * pw + lo;
        uint64_t r0 = bsgs_red128(a0[cc], m), r1 = bsgs_red128(a1[cc], m);
        if (i0) {
          r0 = add_mod(r0, u[0], m.q);
          r1 = add_mod(r1, u[pw], m.q);
        }
        u[0] = r0;
        u[pw] = r1;
      }
    }
  }
}

// The tile form.  CB = 2; TB = 8 (the single kernel's 32 baby words: 116
// VGPRs, 4 waves / SIMD) up to 8 baby slots, where a wider tile is half empty,
// and TB = 16 (182 VGPRs, 2 waves / SIMD) above: same box, 16 ciphertexts at
// N = 2^16, L = 8, the kernel alone took 901 against 1217 us at 8 baby slots,
// 3659 against 3463 us at 16 and 15546 against 14658 us at 32
// (profiles/bsgs_batch_time.json).  GPQHE_BSGS_INNER_TB = 8 or 16 (read per
// call) forces one form for such A/Bs.
#define BSGS_BATCH_CB 2
void k_bsgs_inner_batch(uint64_t *U, const uint64_t *B, const uint64_t *P, const int *tab_dev, unsigned nj, unsigned gs,
                        unsigned ndiag, unsigned lvl, unsigned cnt)
{
  if (!nj || !gs || !cnt)
    gpqhe_die("k_bsgs_inner_batch: %u giant steps, %u baby slots, %u ciphertexts", nj, gs, cnt);
  const unsigned ctiles = (cnt + BSGS_BATCH_CB - 1) / BSGS_BATCH_CB;
  if (ctiles > 65535)
    gpqhe_die("k_bsgs_inner_batch: %u ciphertexts in one chunk", cnt);
  const char *e = getenv("GPQHE_BSGS_INNER_TB");
  const unsigned forced = e ? (unsigned)atoi(e) : 0;
  const unsigned tb = forced == 8 || forced == 16 ? forced : gs > 8 ? 16 : 8, tiles = (gs + tb - 1) / tb;
  // every P word once per ciphertext tile; per ciphertext the baby words once
  // per baby tile, u written once (and re-read and re-written by each later tile)
  ProfScope ps(KC_BSGS_INNER_BATCH,
               8.0 * G.n * lvl * ((double)ndiag * ctiles + (double)cnt * (2.0 * gs + 2.0 * nj * (2 * tiles - 1))));
  const dim3 grid((G.n + TPB - 1) / TPB, lvl, ctiles);
  if (tb == 16)
    hipLaunchKernelGGL((bsgs_inner_batch_kernel<16, BSGS_BATCH_CB>), grid, dim3(TPB), 0, G.stream, U, B, P, tab_dev, nj,
                       gs, lvl, G.logn, cnt, G.dev.mc);
  else
    hipLaunchKernelGGL((bsgs_inner_batch_kernel<8, BSGS_BATCH_CB>), grid, dim3(TPB), 0, G.stream, U, B, P, tab_dev, nj,
                       gs, lvl, G.logn, cnt, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}

// out [cnt][2][lvl][n] = base (null: 0) + sum over t < nt of R[t] ([cnt][2][lvl][n]
// each, r_stride words apart): bsgs_sum_kernel over a whole chunk, total =
// cnt 2 lvl n words.  out may be base.  grid: (total / 2 / TPB).
__global__ void __launch_bounds__(TPB) bsgs_sum_batch_kernel(uint64_t *out, const uint64_t *base, const uint64_t *R,
                                                             unsigned nt, size_t r_stride, size_t total, unsigned lvl,
                                                             unsigned logn, const ModConst *mc)
{
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (w >= total)
    return;
  const uint64_t q = mc[(unsigned)((w >> logn) % lvl)].q;
  bsgs_u2 s{0, 0};
  if (base)
    s = *(const bsgs_u2 *)(base + w);
  for (unsigned t = 0; t < nt; t++) {
    const bsgs_u2 r = *(const bsgs_u2 *)(R + t * r_stride + w);
    s = bsgs_u2{add_mod(s.x, r.x, q), add_mod(s.y, r.y, q)};
  }
  *(bsgs_u2 *)(out + w) = s;
}

void k_bsgs_sum_batch(uint64_t *out, const uint64_t *base, const uint64_t *R, unsigned nt, size_t r_stride,
                      unsigned lvl, unsigned cnt)
{
  const size_t total = (size_t)cnt * 2 * lvl << G.logn, blocks = (total / 2 + TPB - 1) / TPB;
  if (!cnt || blocks > 0x7fffffffu)
    gpqhe_die("k_bsgs_sum_batch: %u ciphertexts in one chunk", cnt);
  ProfScope ps(KC_BSGS_SUM_BATCH, 8.0 * total * (nt + (base ? 2 : 1)));
  hipLaunchKernelGGL(bsgs_sum_batch_kernel, dim3((unsigned)blocks), dim3(TPB), 0, G.stream, out, base, R, nt, r_stride,
                     total, lvl, G.logn, G.dev.mc);
  HIP_CHECK(hipGetLastError());
}
