// api.cpp - the he_* / hectx_* C ABI of libgpqhe.so (include/gpqhe.h) on
// MI355X.  Host C++ orchestrating the gfx950 kernels of kernels.hip on one
// HIP stream; every object payload lives in HBM.  Call-site contract:
// reference src/ctr.c:445-618 and src/hempc.c:216-274 (see gpqhe.h).
#include "gpqhe_internal.h"
#include "../../include/gpqhe_ext.h"
#include "../../include/gpqhe_ext_batch.h"  // (and gpqhe_ext_io_batch.h, gpqhe_ext_step_batch.h, gpqhe_ext_rows_batch.h, gpqhe_ext_packed_batch.h, ..)

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <iterator>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>

Context G;

// ===========================================================================
// Device memory pool: exact-size free lists, stream-ordered reuse.
// ===========================================================================
static std::map<size_t, std::vector<void *>> g_free;
static std::unordered_map<void *, size_t> g_size;

static size_t pool_round(size_t b)
{
  return (b + 4095) & ~(size_t)4095;
}

static void flush_ew();
static void fold_cache_trim();
static unsigned env_u(const char *name, unsigned dflt);
void gemv_cache_clear();
static void plan_caches_clear();

void *pool_alloc(size_t bytes)
{
  const size_t b = pool_round(bytes ? bytes : 1);
  auto it = g_free.find(b);
  if (it != g_free.end() && !it->second.empty()) {
    void *p = it->second.back();
    it->second.pop_back();
    return p;
  }
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, b);
  if (e != hipSuccess) {
    // give cached blocks back and retry once (queued elementwise ops may
    // still name a free-listed block: they run first); folded key sets no
    // running call reads go back too
    flush_ew();
    HIP_CHECK(hipStreamSynchronize(G.stream));
    fold_cache_trim();
    for (auto &kv : g_free)
      for (void *q : kv.second) {
        (void)hipFree(q);
        g_size.erase(q);
      }
    g_free.clear();
    HIP_CHECK(hipMalloc(&p, b));
  }
  g_size[p] = b;
  return p;
}

void pool_free(void *p)
{
  if (!p)
    return;
  auto it = g_size.find(p);
  if (it == g_size.end())
    return;  // payload of an object that outlived a previous context (already released)
  g_free[it->second].push_back(p);
}

void pool_release_all()
{
  // g_size holds every block ever allocated (free-listed or still owned by a
  // caller object that outlives the context); free each exactly once
  for (auto &kv : g_size)
    HIP_CHECK(hipFree(kv.first));
  g_size.clear();
  g_free.clear();
}

// RAII workspace
struct Ws {
  uint64_t *p;
  explicit Ws(size_t words) : p(words ? (uint64_t *)pool_alloc(words * 8) : nullptr) {}
  ~Ws() { pool_free(p); }
  Ws(const Ws &) = delete;
  Ws &operator=(const Ws &) = delete;
};

// Folded gemv / rotation keys (see the fold caches below).
static uint64_t g_key_gen = 1;
struct FoldEntry {  // a matrix of he_gemv
  std::vector<double> M;
  unsigned s, lvl;
  uint64_t gen;
  const he_evk_t *rk;
  std::vector<unsigned> d;  // rotation of each folded diagonal
  double *K;
  size_t bytes;
};
struct RotFold {  // one rotation key
  const he_evk_t *rk;
  uint64_t gen;
  unsigned lvl, rot;
  double *K;
  size_t bytes;
};
// While a call reads a folded set of either kind, an out-of-memory retry
// inside it keeps that set (fold_cache_trim).
static const double *g_fold_inuse = nullptr;
struct FoldUse {
  explicit FoldUse(const double *K) { g_fold_inuse = K; }
  ~FoldUse() { g_fold_inuse = nullptr; }
};

static void fold_cache_clear();
static bool gemv_fold_fits(const double *Md, unsigned lvl, const he_evk_t rk[]);
static bool gemv_win_on(unsigned lvl);
static const FoldEntry &gemv_fold(const double *Md, unsigned lvl, const he_evk_t rk[]);
static const RotFold &rotkey_fold(unsigned r, unsigned lvl, const he_evk_t rk[]);

// he_gemv's encoded diagonals, cached by content (the caller recomputes the
// same gain matrices every control step: reference src/hempc.c:232-238), and
// the whole matrices already seen (HECTR passes the same two every step): the
// non-zero diagonals' rotations and cached encodings, so a repeat he_gemv
// costs one compare of the matrix instead of s diagonal keys.
// gemv_cache_clear frees every block and bumps gen.  Only gemv_now's encodes
// clear, after he_gemv ran the queued gemvs; whatever else keeps a pointer
// into the cache across calls (GemvMat, SgRec) keeps the generation it was
// built under with it, and is dropped where the two differ.
struct GemvMat {
  unsigned s, lvl;
  uint64_t dgen;
  std::vector<double> M;
  std::vector<GemvDiags> dgs;  // evk filled per call from its rk
  std::vector<unsigned> rot;   // the rotation of each diagonal, in dgs order
};
struct DiagCache {
  std::unordered_map<std::string, uint64_t *> pt;
  std::vector<void *> blocks;  // what the entries live in (one entry or a batch)
  size_t bytes = 0;
  std::vector<GemvMat> mats;
  uint64_t gen = 1;
};
static DiagCache g_dc;

// The cache is cleared when it would grow past this (GPQHE_DIAG_MIB, 2 GiB).
static size_t diag_cache_cap()
{
  static const size_t cap = (size_t)env_u("GPQHE_DIAG_MIB", 2048) << 20;
  return cap;
}

// Pinned staging ring for small host->device uploads (encode).
struct Stage {
  void *host = nullptr;
  hipEvent_t ev = nullptr;
  size_t bytes = 0;
};
static Stage g_stage[8];
static unsigned g_stage_next = 0;

// The next slot, free again (its last reader has run), holding a copy of src.
static Stage &stage_fill(const void *src, size_t bytes)
{
  Stage &s = g_stage[g_stage_next++ % 8];
  if (s.ev)
    HIP_CHECK(hipEventSynchronize(s.ev));
  else
    HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  if (s.bytes < bytes) {
    if (s.host)
      HIP_CHECK(hipHostFree(s.host));
    HIP_CHECK(hipHostMalloc(&s.host, bytes, hipHostMallocDefault));
    s.bytes = bytes;
  }
  memcpy(s.host, src, bytes);
  return s;
}

static void upload(void *dst, const void *src, size_t bytes)
{
  Stage &s = stage_fill(src, bytes);
  HIP_CHECK(hipMemcpyAsync(dst, s.host, bytes, hipMemcpyHostToDevice, G.stream));
  HIP_CHECK(hipEventRecord(s.ev, G.stream));
}

// Zero-copy form for a few KB that one launch reads: the kernel reads the
// pinned slot over PCIe (no copy launch); stage_done() after that launch.
static Stage &stage_map(const void *src, size_t bytes, const void **dev)
{
  Stage &s = stage_fill(src, bytes);
  void *d = nullptr;
  HIP_CHECK(hipHostGetDevicePointer(&d, s.host, 0));
  *dev = d;
  return s;
}

static void stage_done(Stage &s) { HIP_CHECK(hipEventRecord(s.ev, G.stream)); }

static void *g_zpin = nullptr;  // pinned decode output (he_dcd_ex)
static size_t g_zpin_bytes = 0;

// he_mul_rescale_batch's second sub-chunk stream and its fork / join events
// (created on first use, released by hectx_exit: no HIP object of the engine
// is left for the runtime's or a profiler's exit handlers)
struct SecondStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, d2 = nullptr, join = nullptr;
};
static SecondStream g_s2;
static hipEvent_t g_dcd_ev = nullptr;  // end of the small-N decode (spec_launch)

static void stage_release()
{
  if (g_zpin)
    (void)hipHostFree(g_zpin);
  g_zpin = nullptr;
  g_zpin_bytes = 0;
  for (Stage &s : g_stage) {
    if (s.ev) {
      (void)hipEventSynchronize(s.ev);
      (void)hipEventDestroy(s.ev);
    }
    if (s.host)
      (void)hipHostFree(s.host);
    s = Stage{};
  }
}

// ===========================================================================
// Deferred encode + public-key encryption (the small-N latency path).
//
// HECTR encodes and encrypts its five state vectors back to back every control
// step (src/ctr.c:466-475), then frees the plaintexts.  Each he_ecd (host FFT,
// upload, lift + NTT) and he_enc_pk (sample v, e0, e1, NTT, combine) is queued
// instead of launched, and the queue runs as one batch -- one upload, one
// lift + NTT, one sampling, one NTT and one combine launch for all of them --
// when anything else touches the engine (every other entry point flushes
// first).  The RNG streams are taken at call time, so the results are the
// ones of the sequential calls bit for bit.
// ===========================================================================
struct PendEcd {
  uint64_t *dst;
  unsigned lvl, slots;
  size_t coff;  // its 2 slots coefficient values at g_pcoef + coff (hm_encode_slots)
};
struct PendEnc {
  uint64_t *c0, *c1;
  const uint64_t *m, *pk0, *pk1;
  unsigned lvl;
  uint64_t stream;
  int ecd;  // m is queued encode ecd (its coefficients join e0: EncCoef), else -1
};
static std::vector<PendEcd> g_pecd;
static std::vector<int64_t> g_pcoef;  // 2 slots coefficient values per pending encode
static std::vector<PendEnc> g_penc;

// Speculative encryption noise.  HECTR encrypts its K = 5 states every control
// step on consecutive RNG streams (src/ctr.c:471-475).  When a step ends in the
// small-N he_dcd, the noise of the next K encryptions -- streams G.counter ..
// G.counter + 3K - 1, sampled and transformed exactly as flush_pending would --
// is launched behind the decode (the host waits for the decode only), so it
// runs while the caller works on the host.  A later flush whose encryptions
// take exactly those streams at that level uses it, and its combine
// evaluates the plaintexts from their coefficients (k_enc_combine_m): the step
// starts with the combine instead of sampling and transforms.
struct SpecNoise {
  uint64_t *buf = nullptr;  // [3k][lvl][n], NTT form (pool block, kept)
  size_t words = 0;
  uint64_t base = 0;  // first stream
  unsigned k = 0, lvl = 0;
  bool valid = false;
};
static SpecNoise g_spec;
static unsigned g_spec_next_k = 0, g_spec_next_lvl = 0;  // the last flush's encryptions (one run)
static uint64_t g_step_base = 0;                          // their first stream

// Speculative ModUp.  The c1 of a fresh encryption, v pk1 + e1, does not
// depend on the plaintext, and HECTR's he_gemv inputs are differences of two
// fresh encryptions (src/hempc.c:253-259).  The queued small-N calls record
// how each c1 poly was made (C1Prov: an encryption's stream, or the he_sub of
// two of them); when a step's gemv inputs were such differences, the next
// step's he_dcd also forms the same differences from the speculative noise
// and runs their ModUp, and a he_gemv whose input c1 has exactly that
// provenance (same streams, public key and level) takes the precomputed
// digits.  Any other write clears the record (check_ctx, non-queued writers),
// so a match always names the same values.
struct C1Prov {
  uint64_t sa, sb;  // streams: the encryption's (sb unused), or a - b
  const uint64_t *pk1;
  unsigned lvl;
  bool sub;
  bool c0 = false;  // the record of an encryption's c0 poly (SpecGemv), not c1
};
static std::unordered_map<const uint64_t *, C1Prov> g_prov;
struct SpecPat {
  unsigned oa, ob;  // encryption offsets within the step's run
};
static std::vector<SpecPat> g_spec_pats_next;  // the last step's gemv inputs
static const uint64_t *g_spec_pk1_next = nullptr;
struct SpecModup {
  uint64_t *D = nullptr;  // [np][ndig][nm][n]
  size_t dwords = 0;
  uint64_t *Y = nullptr;  // [np][lvl][n] the split ModUp's hand-off (ModupHalves)
  size_t ywords = 0;
  std::vector<SpecPat> pats;
  uint64_t base = 0;
  const uint64_t *pk1 = nullptr;
  unsigned lvl = 0;
  bool valid = false;
};
static SpecModup g_smu;
// spec_attach's ModUp, launched behind the decode (spec_modup_launch)
struct SpecModupNext {
  C1Diffs cd{};
  unsigned np = 0, lvl = 0;
  size_t d_stride = 0;
  const uint64_t *pk1 = nullptr;
  bool pending = false;
};
static SpecModupNext g_smu_next;

// Speculative gemv (GPQHE_SPEC_GEMV).  Once the step's encryptions have run
// (spec_flush_early), the last step's gemvs -- the same encryption slots, the
// same matrices and keys, HECTR's he_gemv of xhat - xr and uhat - ur, src/
// hempc.c:253-259 -- run at once on this step's ciphertexts: the inner
// products on the speculated ModUp digits with the differences formed in the
// kernel, and the ModDown, into SpecGemv::Y.  That device work then overlaps
// the caller's host work up to its he_gemv calls (the horizon matrices,
// src/hempc.c:225-240) instead of running between them and the decode.  A
// he_gemv whose input is the queued difference of exactly those polys, still
// holding those encryptions (C1Prov records of c0 and c1, dropped by any
// write), with the same matrix, keys and key generation, queues a copy of its
// Y instead; anything else takes the normal path.
struct SgRec {  // a step's gemv, recorded for the next step's speculation
  SpecPat pat;
  std::vector<double> M;
  GemvDiags dg;  // its one launch's diagonals (evk filled)
  const he_evk_t *rk;
  uint64_t gen, dgen;  // g_key_gen and g_dc.gen when dg was filled
};
static std::vector<SgRec> g_sg_next;  // this step's gemvs (in g_spec_pats_next order)
struct SpecGemv {
  // pattern i's result, in a block shaped as a ciphertext object's (2 polys
  // of G.L limbs): a taking he_gemv swaps it with its output object's block
  uint64_t *Y[GemvJobs::MAX] = {};
  unsigned np = 0, lvl = 0;
  const uint64_t *x[GemvJobs::MAX][4];  // a0, b0, a1, b1 per pattern
  uint64_t sa[GemvJobs::MAX], sb[GemvJobs::MAX];
  SgRec rec[GemvJobs::MAX];
  bool used[GemvJobs::MAX];
  bool valid = false;
};
static SpecGemv g_sg;
static unsigned g_sg_taken = 0;  // gpqhe_spec_gemv_taken

extern "C" unsigned gpqhe_spec_gemv_taken(void)
{
  return g_sg_taken;
}

// Speculative decode of the small-N step (SpecDcd; GPQHE_SPEC_DCD=0 turns it
// off).  A step's tail -- the queued elementwise program (HECTR's he_add,
// he_neg, he_copy_ct, he_add, he_dec: src/hempc.c:261-266, src/ctr.c:486) and
// the decode -- waits on the caller: it is issued at he_dcd, after the
// caller's own host work.  Its operands are this step's speculated gemv
// results, its encryptions, its own temporaries and the secret key, so the
// last step's program, recorded by the roles of its operands (SdPat), is
// replayed on this step's objects right after the speculated gemvs (temporaries
// in scratch, the decode into pinned memory), where it runs in the caller's
// shadow.  he_dcd takes the replay's values when this step's program has the
// same pattern, reading the same blocks (the gemv results still in the blocks
// the speculation wrote, the encryptions still holding their streams:
// C1Prov), and the real program then runs without being waited for.  When the
// replay is still running at he_dcd on two consecutive steps (the caller
// outruns the device: the replay only adds work to the step's chain) it stops.
enum : uint8_t { SR_OUT = 0, SR_Y = 1, SR_ENC = 2 };
struct SdRole {
  uint8_t kind = 0, idx = 0, poly = 0;
  bool operator==(const SdRole &o) const { return kind == o.kind && idx == o.idx && poly == o.poly; }
};
struct SdPat {
  unsigned count = 0, nl = 0, slots = 0, sid = 0;  // sid: the out id holding the decoded plaintext
  double scale = 0;
  const uint64_t *sk = nullptr;
  uint32_t kind[EwProg::MAX] = {}, lvl[EwProg::MAX] = {};
  SdRole out[EwProg::MAX], a[EwProg::MAX], b[EwProg::MAX];
  bool same(const SdPat &o) const
  {
    if (count != o.count || nl != o.nl || slots != o.slots || sid != o.sid || scale != o.scale || sk != o.sk)
      return false;
    for (unsigned j = 0; j < count; j++)
      if (kind[j] != o.kind[j] || lvl[j] != o.lvl[j] || !(out[j] == o.out[j]) || !(a[j] == o.a[j]) ||
          !(b[j] == o.b[j]))
        return false;
    return true;
  }
};
struct SdCtx {  // a step's role blocks (spec_gemv_launch)
  const uint64_t *y[GemvJobs::MAX] = {};
  unsigned ny = 0, ylvl = 0;
  const uint64_t *e[GPQHE_MAXGRP][2] = {};
  uint64_t es[GPQHE_MAXGRP] = {};
  unsigned ne = 0, elvl = 0;
  bool valid = false;
};
struct SpecDcd {
  SdPat pat;  // the pattern replayed this step
  uint64_t *scratch = nullptr, *cws = nullptr;
  size_t swords = 0, cwords = 0;
  void *z = nullptr;  // pinned decoded values
  size_t zbytes = 0;
  hipEvent_t ev = nullptr;
  bool valid = false;
};
static SdCtx g_sd_ctx;    // this step's roles
static SdPat g_sd_next;   // this step's pattern, replayed by the next step
static bool g_sd_next_ok = false;
static SpecDcd g_sd;
static unsigned g_sd_taken = 0, g_sd_late = 0;
static bool g_sd_off = false;

extern "C" unsigned gpqhe_spec_dcd_taken(void)
{
  return g_sd_taken;
}

// The roles of program p's operands and of the decoded plaintext ptd under the
// step roles c; false when some operand has none (or could alias one).
static bool sd_pattern(const EwProg &p, const uint64_t *ptd, unsigned nl, unsigned slots, double scale,
                       const SdCtx &c, SdPat &r)
{
  if (!c.valid || !p.count || nl < 1 || nl > 2)
    return false;
  const size_t n = G.n, ypw = (size_t)G.L << G.logn;
  r = SdPat{};
  r.count = p.count;
  r.nl = nl;
  r.slots = slots;
  r.scale = scale;
  auto ov = [&](const uint64_t *x, unsigned lx, const uint64_t *y, unsigned ly) {
    return x < y + (size_t)ly * n && y < x + (size_t)lx * n;
  };
  unsigned oid[EwProg::MAX];
  // operand x read over lv limbs before op j: the latest earlier writer of
  // exactly x (with at least those limbs), else a role block
  auto read = [&](unsigned j, const uint64_t *x, unsigned lv, SdRole &role) {
    for (int k = (int)j - 1; k >= 0; k--) {
      const EwOp &w = p.op[k];
      if (w.out == x) {
        if (w.lvl < lv)
          return false;
        role = SdRole{SR_OUT, (uint8_t)oid[k], 0};
        return true;
      }
      if (ov(w.out, w.lvl, x, lv))
        return false;
    }
    for (unsigned i = 0; i < c.ny; i++)
      for (unsigned q = 0; q < 2; q++)
        if (x == c.y[i] + q * ypw) {
          if (lv > c.ylvl)
            return false;
          role = SdRole{SR_Y, (uint8_t)i, (uint8_t)q};
          return true;
        }
    for (unsigned o = 0; o < c.ne; o++)
      for (unsigned q = 0; q < 2; q++)
        if (x == c.e[o][q]) {
          if (lv > c.elvl)
            return false;
          role = SdRole{SR_ENC, (uint8_t)o, (uint8_t)q};
          return true;
        }
    return false;
  };
  for (unsigned j = 0; j < p.count; j++) {
    const EwOp &o = p.op[j];
    r.kind[j] = o.kind;
    r.lvl[j] = o.lvl;
    oid[j] = j;
    for (unsigned k = 0; k < j; k++) {
      if (p.op[k].out == o.out) {
        oid[j] = oid[k];
        break;
      }
      if (ov(p.op[k].out, p.op[k].lvl, o.out, o.lvl))
        return false;
    }
    r.out[j] = SdRole{SR_OUT, (uint8_t)oid[j], 0};
    if (!read(j, o.a, o.lvl, r.a[j]))
      return false;
    if ((o.kind == EW_ADD || o.kind == EW_SUB || o.kind == EW_DEC) && !read(j, o.b, o.lvl, r.b[j]))
      return false;
    if (o.kind == EW_DEC) {  // the key: one block, never an output
      if (r.sk && r.sk != o.s)
        return false;
      r.sk = o.s;
      for (unsigned k = 0; k < p.count; k++)
        if (ov(p.op[k].out, p.op[k].lvl, o.s, o.lvl))
          return false;
    }
  }
  SdRole pr;
  if (!read(p.count, ptd, nl, pr) || pr.kind != SR_OUT)
    return false;
  r.sid = pr.idx;
  return true;
}

// Every encryption role of r still holds its stream (C1Prov: any write since
// dropped it).
static bool sd_enc_fresh(const SdPat &r, const SdCtx &c)
{
  auto ok = [&](const SdRole &q) {
    if (q.kind != SR_ENC)
      return true;
    auto it = g_prov.find(c.e[q.idx][q.poly]);
    return it != g_prov.end() && !it->second.sub && it->second.c0 == (q.poly == 0) && it->second.sa == c.es[q.idx] &&
           it->second.lvl == c.elvl;
  };
  for (unsigned j = 0; j < r.count; j++)
    if (!ok(r.a[j]) || !ok(r.b[j]))
      return false;
  return true;
}

// The last step's pattern on this step's roles (g_sd_ctx): the program with
// its temporaries in scratch, then the decode into pinned memory.
static void sd_replay(const SdPat &r)
{
  const size_t blk = (size_t)G.L << G.logn, ypw = blk;
  unsigned nid = 0;
  for (unsigned j = 0; j < r.count; j++)
    nid = std::max(nid, (unsigned)r.out[j].idx + 1);
  const SdCtx &c = g_sd_ctx;
  auto ptr = [&](const SdRole &q) -> const uint64_t * {
    if (q.kind == SR_OUT)
      return q.idx < nid ? g_sd.scratch + q.idx * blk : nullptr;
    if (q.kind == SR_Y)
      return q.idx < c.ny ? c.y[q.idx] + q.poly * ypw : nullptr;
    return q.idx < c.ne ? c.e[q.idx][q.poly] : nullptr;
  };
  if (g_sd.swords < nid * blk) {
    pool_free(g_sd.scratch);  // stream-ordered: its last reader was launched before
    g_sd.scratch = (uint64_t *)pool_alloc(nid * blk * 8);
    g_sd.swords = nid * blk;
  }
  if (g_sd.cwords < ((size_t)r.nl << G.logn)) {
    pool_free(g_sd.cws);
    g_sd.cws = (uint64_t *)pool_alloc(((size_t)r.nl << G.logn) * 8);
    g_sd.cwords = (size_t)r.nl << G.logn;
  }
  EwProg p{};
  p.count = r.count;
  for (unsigned j = 0; j < r.count; j++) {
    const bool hb = r.kind[j] == EW_ADD || r.kind[j] == EW_SUB || r.kind[j] == EW_DEC;
    const uint64_t *a = ptr(r.a[j]), *b = hb ? ptr(r.b[j]) : nullptr;
    if (!a || (hb && !b) || r.out[j].idx >= nid)
      return;
    p.op[j] = EwOp{g_sd.scratch + r.out[j].idx * blk, a, b, r.kind[j] == EW_DEC ? r.sk : nullptr, r.kind[j], r.lvl[j]};
  }
  const size_t zb = (size_t)r.slots * 16;
  if (g_sd.zbytes < zb) {
    if (g_sd.ev)
      HIP_CHECK(hipEventSynchronize(g_sd.ev));  // (an earlier replay may still write it)
    if (g_sd.z)
      HIP_CHECK(hipHostFree(g_sd.z));
    HIP_CHECK(hipHostMalloc(&g_sd.z, zb, hipHostMallocDefault));
    g_sd.zbytes = zb;
  }
  void *zd = nullptr;
  HIP_CHECK(hipHostGetDevicePointer(&zd, g_sd.z, 0));
  if (!g_sd.ev)
    HIP_CHECK(hipEventCreateWithFlags(&g_sd.ev, hipEventDisableTiming));
  k_ew_decode(p, (double *)zd, g_sd.scratch + r.sid * blk, r.nl, r.slots, r.scale, g_sd.cws);
  HIP_CHECK(hipEventRecord(g_sd.ev, G.stream));
  g_sd.pat = r;
  g_sd.valid = true;
}

static bool sd_on()
{
  static const bool on = env_u("GPQHE_SPEC_DCD", 1) != 0;
  return on && !g_sd_off;
}

static void prov_forget(const void *obj_data, size_t pstride_words)
{
  if (g_prov.empty() || !obj_data)
    return;
  g_prov.erase((const uint64_t *)obj_data);
  g_prov.erase((const uint64_t *)obj_data + pstride_words);
}

// he_gemv is queued the same way (at most two, run as one batch: the two
// independent products of every control step of the caller, reference
// src/hempc.c:255-262).  At any time only one of the two queues is non-empty:
// he_gemv runs the encode/encrypt queue before queueing, and a deferred
// encode / encryption runs the gemv queue first.
struct PendGemv {
  uint64_t *y;
  size_t ypstride;
  const uint64_t *x0, *x1;
  const void *xdata;
  unsigned lvl;
  std::vector<GemvDiags> dgs;  // launches of up to GemvDiags::MAX diagonals; empty: all-zero matrix
  const uint64_t *dspec = nullptr;  // x1's ModUp digits, precomputed (SpecModup), or null
  // x = a - b is a queued he_sub (ew_lazy_sub): its polys a0 - b0, a1 - b1,
  // formed where the inner products read them; null otherwise
  const uint64_t *la0 = nullptr, *lb0 = nullptr, *la1 = nullptr, *lb1 = nullptr;
};
static std::vector<PendGemv> g_pgemv;

// The elementwise calls of a control step (he_sub x2 before the gemvs; he_add,
// he_neg, he_copy_ct, he_add after them, src/hempc.c:253-266; he_dec,
// src/ctr.c:486) are queued too and run as one ew_prog_kernel launch per run
// (kernels.hip).  The queue keeps call order element by element, so a freed
// object's block may be handed out again while queued ops still name it:
// every writer outside this queue flushes it first.  The three queues are
// never non-empty at once.
static EwProg g_pew{};

static void flush_pending();
static void flush_gemvs();
static bool g_spec_early = false;  // the next step's speculation rides on this step's gemv / ModDown (spec_attach)

static void flush_ew()
{
  if (!g_pew.count)
    return;
  const EwProg p = g_pew;
  g_pew.count = 0;
  k_ew_prog(p);
}

static void check_ctx()
{
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  // a non-queued entry point: it may write any object (C1Prov)
  g_prov.clear();
  g_smu.valid = false;
  g_smu_next.pending = false;
  g_sd.valid = false;
  flush_ew();
  if (!g_pgemv.empty())
    flush_gemvs();
  if (!g_pecd.empty() || !g_penc.empty())
    flush_pending();
}

static inline he_ct_t *OB(void *o) { return (he_ct_t *)o; }
static inline const he_ct_t *OB(const void *o) { return (const he_ct_t *)o; }

static inline uint64_t *limb(const void *vo, unsigned p, unsigned l)
{
  const he_ct_t *o = OB(vo);
  return o->data + (((size_t)p * o->cap + l) << G.logn);
}

static inline size_t pstride(const void *vo)
{
  return (size_t)OB(vo)->cap << G.logn;
}

static LimbSet limbset(uint64_t *base, const unsigned *mods, unsigned per, unsigned groups, size_t stride)
{
  LimbSet s{};
  s.base = base;
  s.per = per;
  s.count = per * groups;
  s.stride = stride;
  for (unsigned i = 0; i < per; i++)
    s.mods[i] = (uint8_t)mods[i];
  return s;
}

static LimbSet qlimbs(uint64_t *base, unsigned lvl, unsigned groups, size_t stride)
{
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned i = 0; i < lvl; i++)
    mods[i] = i;
  return limbset(base, mods, lvl, groups, stride);
}

static unsigned basis_qp(unsigned lvl, unsigned *mods)
{
  for (unsigned t = 0; t < lvl; t++)
    mods[t] = t;
  for (unsigned k = 0; k < G.K; k++)
    mods[lvl + k] = G.L + k;
  return lvl + G.K;
}

static void obj_alloc(void *vo, unsigned npoly, unsigned cap)
{
  // no flush of the queued work: a fresh block cannot alias a live object
  // that queued work refers to (objects are flushed before they are freed)
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  he_ct_t *o = OB(vo);
  memset(o, 0, sizeof(*o));
  o->npoly = npoly;
  o->cap = cap;
  const size_t bytes = ((size_t)npoly * cap << G.logn) * 8;
  // No zero fill: a fresh object has nlimbs = 0, and every read of an object
  // is bounded by its nlimbs, so its payload is written before it is read.
  o->data = (uint64_t *)pool_alloc(bytes);
  prov_forget(o->data, (size_t)cap << G.logn);
}

// Freeing the target of a queued encode that no other queued work reads
// (HECTR frees its five plaintexts right after encrypting them, src/ctr.c:
// 476-480; the queued encryptions take the coefficients, not the payload):
// the encode is dropped instead of flushing the queue.  True if so.
static bool drop_dead_encode(const uint64_t *data)
{
  if (!data || !g_pgemv.empty() || g_pew.count)
    return false;
  bool target = false;
  for (const PendEcd &e : g_pecd)
    target |= e.dst == data;
  if (!target)
    return false;
  for (const PendEnc &e : g_penc)
    if (e.c0 == data || e.c1 == data || e.pk0 == data || e.pk1 == data || (e.m == data && e.ecd < 0))
      return false;
  for (PendEcd &e : g_pecd)
    if (e.dst == data)
      e.dst = nullptr;
  return true;
}

// Every queued encode dropped (its plaintext freed) and the queued
// encryptions are exactly the speculated ones (SpecNoise): they run now --
// only the combine, from the speculative noise and the plaintexts'
// coefficients -- so it overlaps the caller's host work up to its next call
// that needs them (HECTR's horizon matrices in ctr_hempc, src/hempc.c:225-240)
// instead of starting at that call.  GPQHE_SPEC_EARLY=0: at that call.
static void spec_gemv_launch(const std::vector<PendEnc> &enc, const std::vector<SgRec> &recs);

static void spec_flush_early()
{
  static const bool on = env_u("GPQHE_SPEC_EARLY", 1) != 0;
  if (!on || !g_spec.valid || g_penc.empty() || g_penc.size() != g_spec.k || !g_pgemv.empty() || g_pew.count ||
      g_penc[0].stream != g_spec.base || g_penc[0].lvl != g_spec.lvl)
    return;
  for (const PendEcd &e : g_pecd)
    if (e.dst)
      return;
  const std::vector<PendEnc> enc = g_penc;
  const std::vector<SgRec> recs = g_sg_next;  // the last step's gemvs (flush_pending starts a new record)
  flush_pending();
  spec_gemv_launch(enc, recs);
}

static void obj_free(void *vo)
{
  // a queued encode / encryption / gemv may still use the payload (queued
  // elementwise ops keep their order with any later user of the block)
  bool dropped = false;
  if (G.init && (!g_pgemv.empty() || !g_pecd.empty() || !g_penc.empty())) {
    dropped = drop_dead_encode(OB(vo)->data);
    if (!dropped)
      check_ctx();
  }
  he_ct_t *o = OB(vo);
  if (o->data && G.init) {
    prov_forget(o->data, (size_t)o->cap << G.logn);
    const uint64_t *lo = o->data, *hi = o->data + ((size_t)o->npoly * o->cap << G.logn);
    if (g_smu.pk1 >= lo && g_smu.pk1 < hi)
      g_smu.valid = false;  // the speculative ModUp's public key
    if (g_smu_next.pk1 >= lo && g_smu_next.pk1 < hi)
      g_smu_next.pending = false;  // (its pending launch reads it)
    if (g_spec_pk1_next >= lo && g_spec_pk1_next < hi)
      g_spec_pats_next.clear();
    if (g_pew.count) {
      // queued elementwise ops writing this block while no queued op reads it:
      // their results can never be read, so they are dropped (HECTR's xdiff
      // and udiff, src/hempc.c:269-270, once he_gemv read their operands)
      auto in = [&](const uint64_t *p) { return p && p >= lo && p < hi; };
      bool read = false;
      for (unsigned j = 0; j < g_pew.count; j++)
        read |= in(g_pew.op[j].a) || in(g_pew.op[j].b) || in(g_pew.op[j].s);
      if (!read) {
        unsigned w = 0;
        for (unsigned j = 0; j < g_pew.count; j++)
          if (!in(g_pew.op[j].out))
            g_pew.op[w++] = g_pew.op[j];
        g_pew.count = w;
      }
    }
    pool_free(o->data);
  }
  memset(o, 0, sizeof(*o));
  if (dropped)
    spec_flush_early();
}

static uint64_t next_stream()
{
  return G.counter++;
}

static void sample_small_ntt(uint64_t *dst, const unsigned *mods, unsigned nm, int cbd)
{
  LimbSet s = limbset(dst, mods, nm, 1, (size_t)nm << G.logn);
  k_sample_small(s, next_stream(), cbd);
  k_ntt(s, false);
}

static void sample_uniform(uint64_t *dst, const unsigned *mods, unsigned nm)
{
  LimbSet s = limbset(dst, mods, nm, 1, (size_t)nm << G.logn);
  k_sample_uniform(s, next_stream());
}

// ===========================================================================
// MPI
// ===========================================================================
struct gpqhe_mpi {
  unsigned nwords;
  uint64_t w[64];
};

extern "C" MPI gpqhe_mpi_set_ui(MPI w, unsigned long u)
{
  if (!w)
    w = (MPI)calloc(1, sizeof(*w));
  memset(w->w, 0, sizeof(w->w));
  w->w[0] = u;
  w->nwords = 1;
  return w;
}

extern "C" void gpqhe_mpi_lshift(MPI x, MPI a, unsigned int n)
{
  uint64_t src[64], dst[64];
  memcpy(src, a->w, sizeof(src));
  memset(dst, 0, sizeof(dst));
  const unsigned ws = n / 64, bs = n % 64;
  for (int i = 63; i >= 0; i--) {
    const int s = i - (int)ws;
    if (s < 0)
      continue;
    uint64_t v = src[s] << bs;
    if (bs && s > 0)
      v |= src[s - 1] >> (64 - bs);
    dst[i] = v;
  }
  memcpy(x->w, dst, sizeof(dst));
  x->nwords = 64;
}

extern "C" void gpqhe_mpi_release(MPI a)
{
  free(a);
}

extern "C" unsigned gpqhe_mpi_get_nbits(MPI a)
{
  for (int i = 63; i >= 0; i--)
    if (a->w[i])
      return (unsigned)(i * 64 + 64 - __builtin_clzll(a->w[i]));
  return 0;
}

// ===========================================================================
// Context
// ===========================================================================
static void set_seed_words(uint64_t seed)
{
  uint64_t z = seed;
  for (int i = 0; i < 4; i++) {
    z += 0x9E3779B97F4A7C15ull;
    const uint64_t x = splitmix64_mix(z);
    G.key.k[2 * i] = (uint32_t)x;
    G.key.k[2 * i + 1] = (uint32_t)(x >> 32);
  }
  G.counter = 0;
  g_spec.valid = false;  // noise of the old key
  g_smu.valid = false;
  g_smu_next.pending = false;
}

extern "C" void gpqhe_set_seed(uint64_t seed)
{
  if (G.init)
    check_ctx();  // queued encryptions sample with the current key
  set_seed_words(seed);
}

static uint64_t default_seed()
{
  const char *e = getenv("GPQHE_SEED");
  if (e && *e)
    return strtoull(e, nullptr, 0);
  uint64_t s = 0;
  FILE *f = fopen("/dev/urandom", "rb");
  if (!f || fread(&s, sizeof(s), 1, f) != 1)
    gpqhe_die("cannot read /dev/urandom");
  fclose(f);
  return s;
}

extern "C" void hectx_init_params(const gpqhe_params_t *p)
{
  if (G.init)
    hectx_exit();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    gpqhe_die("no HIP device visible: libgpqhe.so runs on MI355X only (no CPU fallback)");
  if (p->logn < 4 || p->logn > 17)
    gpqhe_die("logn %u out of range [4, 17]", p->logn);
  if (p->nlimbs < 1 || p->nspecial < 1 || p->nlimbs + p->nspecial > GPQHE_MAXMOD)
    gpqhe_die("bad limb counts L=%u K=%u", p->nlimbs, p->nspecial);
  if (p->q0_bits > 61 || p->qi_bits > 61 || p->p_bits > 61 || p->q0_bits < 32 || p->qi_bits < 32 ||
      p->p_bits < 32)
    gpqhe_die("prime sizes must be within [32, 61] bits");
  Context &C = G;
  C.logn = p->logn;
  C.n = 1u << p->logn;
  C.L = p->nlimbs;
  C.K = p->nspecial;
  C.nmod = C.L + C.K;
  C.dnum = p->dnum ? p->dnum : p->nlimbs;
  if (C.dnum > C.L)
    C.dnum = C.L;
  C.alpha = (C.L + C.dnum - 1) / C.dnum;
  C.dnum = (C.L + C.alpha - 1) / C.alpha;
  C.slots = p->slots ? p->slots : C.n / 2;
  if ((C.slots & (C.slots - 1)) || C.slots > C.n / 2)
    gpqhe_die("slots %u must be a power of two <= n/2", C.slots);
  C.delta = p->delta;
  const uint64_t two_n = 2ull * C.n;
  unsigned used = 0;
  C.q[used] = hm_pick_prime(p->q0_bits, two_n, C.q, used);
  used++;
  for (unsigned i = 1; i < C.L; i++, used++)
    C.q[used] = hm_pick_prime(p->qi_bits, two_n, C.q, used);
  for (unsigned i = 0; i < C.K; i++, used++)
    C.q[used] = hm_pick_prime(p->p_bits, two_n, C.q, used);
  for (unsigned m = 0; m < C.nmod; m++) {
    hm_modconst(C.mc[m], C.q[m]);
    C.psi[m] = hm_find_psi(C.q[m], C.n);
    C.mc[m].ninv = hm_inv_mod(C.n, C.q[m]);
    C.mc[m].ninvp = (uint64_t)(((unsigned __int128)C.mc[m].ninv << 64) / C.q[m]);
    uint64_t pm = 1;
    for (unsigned k = 0; k < C.K; k++)
      pm = hm_mul_mod(pm, C.q[C.L + k] % C.q[m], C.q[m]);
    C.mc[m].pmod = pm;
    C.mc[m].pmodp = (uint64_t)(((unsigned __int128)pm << 64) / C.q[m]);
  }
  HIP_CHECK(hipGetDevice(&C.device));
  (void)hipGetLastError();  // start from a clean error state
  if (!C.own_stream)
    HIP_CHECK(hipStreamCreateWithFlags(&C.own_stream, hipStreamNonBlocking));
  if (!C.stream)
    C.stream = C.own_stream;
  tables_upload();
  set_seed_words(p->seed ? p->seed : default_seed());
  C.init = true;
  tables_prewarm();
}

static unsigned env_u(const char *name, unsigned dflt)
{
  const char *e = getenv(name);
  return (e && *e) ? (unsigned)strtoul(e, nullptr, 0) : dflt;
}

// GPQHE_HOSTPROF=1: host time spent inside each entry point the small-N
// control step uses (outermost calls only) and between calls (the caller's
// own work), printed to stderr by hectx_exit.  Measurement aid only.
struct HostProfEntry {
  double us = 0;
  unsigned long calls = 0;
};
static std::map<std::string, HostProfEntry> g_hp;
static double g_hp_outside = 0, g_hp_last = -1;
// GPQHE_HOSTPROF=2 also keeps every outermost call (name, start, end) and
// prints one steady-state control step's calls relative to the end of the
// decode before it (the caller's host timeline between two decodes)
struct HpEvent {
  const char *name;
  double t0, t1;
};
static std::vector<HpEvent> g_hp_ev;
static int g_hp_depth = 0;
static double hp_now()
{
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static bool hp_on()
{
  static const bool on = env_u("GPQHE_HOSTPROF", 0) != 0;
  return on;
}
struct HpScope {
  const char *name;
  double t0 = 0;
  bool top = false;
  explicit HpScope(const char *nm) : name(nm)
  {
    if (!hp_on())
      return;
    top = g_hp_depth++ == 0;
    if (top) {
      t0 = hp_now();
      if (g_hp_last >= 0)
        g_hp_outside += t0 - g_hp_last;
    }
  }
  ~HpScope()
  {
    if (!hp_on())
      return;
    g_hp_depth--;
    if (top) {
      g_hp_last = hp_now();
      HostProfEntry &e = g_hp[name];
      e.us += g_hp_last - t0;
      e.calls++;
      static const bool ev = env_u("GPQHE_HOSTPROF", 0) >= 2;
      if (ev && g_hp_ev.size() < 100000)
        g_hp_ev.push_back(HpEvent{name, t0, g_hp_last});
    }
  }
};
#define HPROF(nm) HpScope hp_scope_(nm)

static void hp_report()
{
  if (!hp_on() || g_hp.empty())
    return;
  double in = 0;
  for (auto &kv : g_hp)
    in += kv.second.us;
  fprintf(stderr, "[gpqhe hostprof] inside the library %.1f us, outside (caller) %.1f us\n", in, g_hp_outside);
  for (auto &kv : g_hp)
    fprintf(stderr, "[gpqhe hostprof] %-12s %8lu calls %10.1f us %8.2f us/call\n", kv.first.c_str(), kv.second.calls,
            kv.second.us, kv.second.us / (double)kv.second.calls);
  // the calls after the (ndcd/2)-th decode up to and including the next one
  std::vector<size_t> dcd;
  for (size_t i = 0; i < g_hp_ev.size(); i++)
    if (!strcmp(g_hp_ev[i].name, "dcd"))
      dcd.push_back(i);
  if (dcd.size() >= 4) {
    const size_t a = dcd[dcd.size() / 2], b = dcd[dcd.size() / 2 + 1];
    const double t = g_hp_ev[a].t1;
    fprintf(stderr, "[gpqhe hostprof] one step, us after the decode before it returned: start end name\n");
    for (size_t i = a + 1; i <= b; i++)
      fprintf(stderr, "[gpqhe hostprof] %8.1f %8.1f %s\n", g_hp_ev[i].t0 - t, g_hp_ev[i].t1 - t, g_hp_ev[i].name);
  }
  g_hp_ev.clear();
  g_hp.clear();
  g_hp_outside = 0;
  g_hp_last = -1;
}

extern "C" void hectx_init(unsigned int logn, MPI q, unsigned int slots, uint64_t Delta)
{
  gpqhe_params_t p;
  memset(&p, 0, sizeof(p));
  const unsigned logq = gpqhe_mpi_get_nbits(q) - 1;
  const unsigned logd = 63 - (unsigned)__builtin_clzll(Delta);
  p.logn = env_u("GPQHE_LOGN", logn);
  p.slots = slots;
  p.delta = (double)Delta;
  p.qi_bits = logd;
  p.nspecial = 1;
  p.p_bits = 60;
  unsigned L = env_u("GPQHE_NLIMBS", 0);
  if (L) {
    p.nlimbs = L;
    p.q0_bits = 60;
  } else {
    L = 2;
    while (logq > (L - 1) * logd + 61)
      L++;
    p.nlimbs = L;
    p.q0_bits = logq - (L - 1) * logd;
  }
  p.dnum = env_u("GPQHE_DNUM", p.nlimbs);
  p.seed = 0;
  hectx_init_params(&p);
}

extern "C" void hectx_exit(void)
{
  if (!G.init)
    return;
  hp_report();
  check_ctx();
  HIP_CHECK(hipStreamSynchronize(G.stream));
  // every HIP object the engine created goes here, after its last use: the
  // second sub-chunk stream and its events, the decode event, the profiling
  // events and (below, with the pool) the context's own stream
  if (g_s2.s) {
    HIP_CHECK(hipStreamSynchronize(g_s2.s));
    HIP_CHECK(hipEventDestroy(g_s2.fork));
    HIP_CHECK(hipEventDestroy(g_s2.d2));
    HIP_CHECK(hipEventDestroy(g_s2.join));
    HIP_CHECK(hipStreamDestroy(g_s2.s));
    g_s2 = SecondStream{};
  }
  if (g_dcd_ev) {
    HIP_CHECK(hipEventDestroy(g_dcd_ev));
    g_dcd_ev = nullptr;
  }
  if (g_sd.ev)
    HIP_CHECK(hipEventDestroy(g_sd.ev));
  if (g_sd.z)
    HIP_CHECK(hipHostFree(g_sd.z));
  g_sd = SpecDcd{};  // (its scratch blocks go with the pool)
  g_sd_ctx = SdCtx{};
  g_sd_next_ok = false;
  g_sd_taken = g_sd_late = 0;
  g_sd_off = false;
  k_prof_release();
  gemv_cache_clear();
  plan_caches_clear();
  fold_cache_clear();
  g_key_gen++;
  tables_free();
  g_spec = SpecNoise{};  // its blocks go with the pool
  g_spec_next_k = 0;
  g_smu = SpecModup{};
  g_smu_next = SpecModupNext{};
  g_sa = SpecAttach{};
  g_sg = SpecGemv{};
  g_sg_next.clear();
  g_sg_taken = 0;
  g_prov.clear();
  g_spec_pats_next.clear();
  g_spec_pk1_next = nullptr;
  pool_release_all();
  stage_release();
  if (G.own_stream) {
    HIP_CHECK(hipStreamDestroy(G.own_stream));
    if (G.stream == G.own_stream)
      G.stream = nullptr;  // (a caller's stream from gpqhe_set_stream stays set)
    G.own_stream = nullptr;
  }
  G.init = false;
}

extern "C" void hectx_info(gpqhe_info_t *info)
{
  check_ctx();
  memset(info, 0, sizeof(*info));
  info->logn = G.logn;
  info->n = G.n;
  info->nlimbs = G.L;
  info->nspecial = G.K;
  info->dnum = G.dnum;
  info->alpha = G.alpha;
  info->slots = G.slots;
  info->delta = G.delta;
  for (unsigned m = 0; m < G.nmod; m++) {
    info->primes[m] = G.q[m];
    info->psi[m] = G.psi[m];
  }
}

extern "C" void gpqhe_set_stream(void *stream)
{
  if (G.init)
    check_ctx();
  if (G.stream)
    HIP_CHECK(hipStreamSynchronize(G.stream));
  G.stream = stream ? (hipStream_t)stream : G.own_stream;
}

extern "C" void gpqhe_sync(void)
{
  if (G.init)
    check_ctx();
  if (G.stream)
    HIP_CHECK(hipStreamSynchronize(G.stream));
}

// ===========================================================================
// Objects
// ===========================================================================
extern "C" void he_alloc_pk(he_pk_t *pk) { obj_alloc(pk, 2, G.L); }
extern "C" void he_free_pk(he_pk_t *pk) { obj_free(pk); }
extern "C" void he_alloc_sk(poly_mpi_t *sk) { obj_alloc(sk, 1, G.nmod); }
extern "C" void he_free_sk(poly_mpi_t *sk) { obj_free(sk); }
extern "C" void he_alloc_ct(he_ct_t *ct)
{
  HPROF("alloc_ct");
  obj_alloc(ct, 2, G.L);
}
extern "C" void he_free_ct(he_ct_t *ct)
{
  HPROF("free_ct");
  obj_free(ct);
}
extern "C" void he_alloc_pt(he_pt_t *pt)
{
  HPROF("alloc_pt");
  obj_alloc(pt, 1, G.nmod);
}
extern "C" void he_free_pt(he_pt_t *pt)
{
  HPROF("free_pt");
  obj_free(pt);
}

extern "C" void he_alloc_evk(he_evk_t *evk)
{
  check_ctx();
  memset(evk, 0, sizeof(*evk));
}

// Montgomery-form shadow of a key (x 2^64 mod q), kept in `reserved`, used by
// the fused key-switch inner product.  Exported/imported keys stay canonical.
static void evk_make_mont(he_evk_t *evk)
{
  const size_t words = ((size_t)evk->npoly * evk->cap) << G.logn;
  uint64_t *m = (uint64_t *)(uintptr_t)evk->reserved;
  if (!m)
    m = (uint64_t *)pool_alloc(words * 8);
  k_to_mont(m, evk->data, evk->npoly * evk->cap);
  evk->reserved = (uint64_t)(uintptr_t)m;
}

extern "C" void he_free_evk(he_evk_t *evk)
{
  g_key_gen++;
  if (evk->reserved && G.init)
    pool_free((void *)(uintptr_t)evk->reserved);
  obj_free(evk);
}

extern "C" size_t he_export(const void *vo, uint64_t *host)
{
  check_ctx();
  const he_ct_t *o = OB(vo);
  const size_t n = G.n;
  HIP_CHECK(hipStreamSynchronize(G.stream));
  size_t w = 0;
  for (unsigned p = 0; p < o->npoly; p++) {
    HIP_CHECK(hipMemcpy(host + w, limb(o, p, 0), (size_t)o->nlimbs * n * 8, hipMemcpyDeviceToHost));
    w += (size_t)o->nlimbs * n;
  }
  return w;
}

extern "C" void he_import(void *vo, const uint64_t *host, unsigned int nlimbs, double scale, uint32_t flags)
{
  check_ctx();
  he_ct_t *o = OB(vo);
  if (!o->data) {
    const uint32_t g = o->galois, dn = o->dnum;
    if (!dn || dn != G.dnum)
      gpqhe_die("he_import into an unallocated object (evk needs dnum=%u)", G.dnum);
    obj_alloc(o, 2 * dn, G.nmod);
    o->galois = g;
    o->dnum = dn;
  }
  if (nlimbs > o->cap)
    gpqhe_die("he_import: %u limbs > capacity %u", nlimbs, o->cap);
  HIP_CHECK(hipStreamSynchronize(G.stream));
  size_t w = 0;
  for (unsigned p = 0; p < o->npoly; p++) {
    HIP_CHECK(hipMemcpy(limb(o, p, 0), host + w, (size_t)nlimbs * G.n * 8, hipMemcpyHostToDevice));
    w += (size_t)nlimbs * G.n;
  }
  o->nlimbs = nlimbs;
  o->scale = scale;
  o->flags = flags;
  if (o->dnum && o->npoly == 2 * o->dnum && o->cap == G.nmod) {
    g_key_gen++;
    evk_make_mont((he_evk_t *)o);  // key objects keep their Montgomery shadow in sync
  }
}

extern "C" void he_evk_meta(const he_evk_t *evk, uint32_t *galois, uint32_t *dnum)
{
  *galois = evk->galois;
  *dnum = evk->dnum;
}

// ===========================================================================
// Keys
// ===========================================================================
extern "C" void he_keypair(he_pk_t *pk, poly_mpi_t *sk)
{
  check_ctx();
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned m = 0; m < G.nmod; m++)
    mods[m] = m;
  sample_small_ntt(sk->data, mods, G.nmod, 0);  // s: ternary over all moduli
  sk->nlimbs = G.nmod;
  sample_uniform(limb(pk, 1, 0), mods, G.L);     // a
  Ws e((size_t)G.L << G.logn);
  sample_small_ntt(e.p, mods, G.L, 1);           // e
  k_enc_sk_combine(limb(pk, 0, 0), limb(pk, 1, 0), e.p, sk->data, nullptr, G.L);  // -a s + e
  pk->nlimbs = G.L;
}

static void gen_evk(he_evk_t *evk, const uint64_t *sprime, const poly_mpi_t *sk, uint32_t galois)
{
  g_key_gen++;
  if (evk->data)
    he_free_evk(evk);
  obj_alloc(evk, 2 * G.dnum, G.nmod);
  evk->nlimbs = G.nmod;
  evk->galois = galois;
  evk->dnum = G.dnum;
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned m = 0; m < G.nmod; m++)
    mods[m] = m;
  Ws e((size_t)G.nmod << G.logn);
  for (unsigned j = 0; j < G.dnum; j++) {
    sample_uniform(limb(evk, 2 * j + 1, 0), mods, G.nmod);
    sample_small_ntt(e.p, mods, G.nmod, 1);
    const unsigned lo = j * G.alpha, hi = std::min(lo + G.alpha, G.L);
    k_evk_combine(limb(evk, 2 * j, 0), limb(evk, 2 * j + 1, 0), e.p, sk->data, sprime, lo, hi);
  }
  evk_make_mont(evk);
}

static uint64_t galois_of_rot(unsigned r)
{
  return hm_pow_mod(5, r, 2ull * G.n);
}

static void gen_rot_key(he_evk_t *evk, uint64_t g, const poly_mpi_t *sk)
{
  Ws sp((size_t)G.nmod << G.logn);
  k_automorph(sp.p, sk->data, G.nmod, g);
  gen_evk(evk, sp.p, sk, (uint32_t)g);
}

// rk[r] <- the key of every rotation r in [1, slots) that `want` selects, in
// ascending r (the keys' stream numbers follow that order); the others freed.
template <class Want>
static void gen_rot_keys(he_evk_t rk[], const poly_mpi_t *sk, Want want)
{
  if (rk[0].data)
    obj_free(&rk[0]);
  rk[0].galois = 1;
  for (unsigned r = 1; r < G.slots; r++) {
    if (want(r))
      gen_rot_key(&rk[r], galois_of_rot(r), sk);
    else if (rk[r].data)
      he_free_evk(&rk[r]);
  }
}

extern "C" void he_genrk(he_evk_t rk[], const poly_mpi_t *sk)
{
  check_ctx();
  gen_rot_keys(rk, sk, [](unsigned) { return true; });
}

extern "C" void he_genrot(he_evk_t *evk, unsigned int rot, const poly_mpi_t *sk)
{
  check_ctx();
  gen_rot_key(evk, galois_of_rot(rot), sk);
}

extern "C" void he_genrlk(he_evk_t *rlk, const poly_mpi_t *sk)
{
  check_ctx();
  Ws s2((size_t)G.nmod << G.logn);
  k_square(s2.p, sk->data, G.nmod);
  gen_evk(rlk, s2.p, sk, 1);
}

// ===========================================================================
// Encoding / encryption
// ===========================================================================
// Encode z at `scale` into `dst` limbs for moduli mods[0..nm) (NTT domain).
// Slot counts from which the special FFT runs on the GPU (GPQHE_GPU_ECD_MIN;
// below it the host FFT plus one upload has the lower latency, e.g. HECTR's
// 16-32 slots).
static unsigned gpu_ecd_min()
{
  static const unsigned m = env_u("GPQHE_GPU_ECD_MIN", 2048);
  return m;
}

// Deferral applies to host-FFT encodes at n <= 2^12 (the whole-limb NTT
// lifts in-kernel) into q limbs 0..lvl-1.
static bool defer_ok(unsigned s)
{
  static const bool on = env_u("GPQHE_DEFER", 1) != 0;
  return on && G.logn <= 12 && G.logn >= 10 && s < gpu_ecd_min();
}

static void flush_pending()
{
  std::vector<PendEcd> ecd;
  std::vector<PendEnc> enc;
  std::vector<int64_t> vals;
  ecd.swap(g_pecd);
  enc.swap(g_penc);
  if (!ecd.empty() || !enc.empty())
    g_sd.valid = false;  // (its outputs may take blocks the replayed tail read: SpecDcd)
  vals.swap(g_pcoef);
  const size_t n = G.n;
  // an encoding of s slots is zero off the stride n / 2s: the launches take
  // one row of the coefficients on the widest stride every queued encode
  // shares (value j = coefficient j 2^clog)
  unsigned clog = G.logn;
  for (const PendEcd &e : ecd)
    clog = std::min(clog, (unsigned)__builtin_ctz(G.n / (2 * e.slots)));
  const size_t row = n >> clog;
  std::vector<int64_t> coef(ecd.size() * row);
  for (size_t i = 0; i < ecd.size(); i++) {
    const size_t step = (n / (2 * ecd[i].slots)) >> clog;
    for (size_t t = 0; t < 2 * (size_t)ecd[i].slots; t++)
      coef[i * row + t * step] = vals[ecd[i].coff + t];
  }
  // a device-readable copy of the rows, made when a launch needs more values
  // than travel in its arguments: up to 64 KB the kernels read pinned host
  // memory, more is uploaded
  const size_t cbytes = ecd.size() * row * 8;
  Ws up(0);
  Stage *st = nullptr;
  const int64_t *dcoef = nullptr;
  auto dev_coef = [&]() {
    if (!dcoef) {
      if (cbytes <= 65536) {
        const void *dmap = nullptr;
        st = &stage_map(coef.data(), cbytes, &dmap);
        dcoef = (const int64_t *)dmap;
      } else {
        up.p = (uint64_t *)pool_alloc(cbytes);
        upload(up.p, coef.data(), cbytes);
        dcoef = (const int64_t *)up.p;
      }
    }
    return dcoef;
  };
  // the encodes whose plaintext still lives (dropped ones: drop_dead_encode)
  for (size_t i0 = 0; i0 < ecd.size();) {
    if (!ecd[i0].dst) {
      i0++;
      continue;
    }
    // one launch per run of live encodes at equal levels (at most GPQHE_MAXGRP)
    size_t i1 = i0 + 1;
    while (i1 < ecd.size() && i1 - i0 < GPQHE_MAXGRP && ecd[i1].dst && ecd[i1].lvl == ecd[i0].lvl)
      i1++;
    unsigned mods[GPQHE_MAXMOD];
    for (unsigned l = 0; l < ecd[i0].lvl; l++)
      mods[l] = l;
    LimbSet ls = limbset(nullptr, mods, ecd[i0].lvl, (unsigned)(i1 - i0), 0);
    ls.ngp = (uint32_t)(i1 - i0);
    for (size_t i = i0; i < i1; i++) {
      ls.gp[i - i0] = ecd[i].dst;
      g_prov.erase(ecd[i].dst);
    }
    // up to CoefArg::MAX values (HECTR's step: 5 x 32) in the kernel arguments
    if ((i1 - i0) * row <= CoefArg::MAX)
      k_lift_ntt_arg(ls, coef.data() + i0 * row, clog);
    else
      k_lift_ntt(ls, dev_coef() + i0 * row, clog);
    i0 = i1;
  }
  for (size_t i0 = 0; i0 < enc.size();) {
    // a run of encryptions at one level with consecutive RNG streams and the
    // same public key
    size_t i1 = i0 + 1;
    while (i1 < enc.size() && i1 - i0 < GPQHE_MAXGRP && enc[i1].lvl == enc[i0].lvl &&
           enc[i1].stream == enc[i0].stream + 3 * (i1 - i0) && enc[i1].pk0 == enc[i0].pk0)
      i1++;
    const unsigned k = (unsigned)(i1 - i0), lvl = enc[i0].lvl;
    const size_t w = (size_t)lvl << G.logn;
    unsigned mods[GPQHE_MAXMOD];
    for (unsigned l = 0; l < lvl; l++)
      mods[l] = l;
    EncBatch b{};
    for (unsigned e = 0; e < k; e++) {
      b.c0[e] = enc[i0 + e].c0;
      b.c1[e] = enc[i0 + e].c1;
      b.m[e] = enc[i0 + e].ecd >= 0 ? nullptr : enc[i0 + e].m;
    }
    if (i0 == 0 && i1 == enc.size()) {
      g_spec_next_k = k;
      g_spec_next_lvl = lvl;
      g_step_base = enc[i0].stream;
    } else {
      g_spec_next_k = 0;
    }
    if (i0 == 0) {
      g_spec_pats_next.clear();  // a new step: its gemv inputs are recorded afresh
      g_sg_next.clear();
      g_sd_ctx.valid = false;
      g_sd.valid = false;
    }
    for (unsigned e = 0; e < k; e++) {
      g_prov[enc[i0 + e].c1] = C1Prov{enc[i0 + e].stream, 0, enc[i0 + e].pk1, lvl, false};
      g_prov[enc[i0 + e].c0] = C1Prov{enc[i0 + e].stream, 0, enc[i0 + e].pk1, lvl, false, true};
    }
    // the speculative noise of exactly these streams: only the combine runs,
    // with the queued plaintexts evaluated from their coefficients
    const uint64_t off = (enc[i0].stream - g_spec.base) / 3;
    unsigned mrows = 0;
    for (unsigned e = 0; e < k; e++)
      mrows += enc[i0 + e].ecd >= 0;
    if (g_spec.valid && lvl == g_spec.lvl && enc[i0].stream >= g_spec.base &&
        (enc[i0].stream - g_spec.base) % 3 == 0 && off + k <= g_spec.k && row >= 4 && row <= EncM::MAXROW &&
        (size_t)mrows * lvl * row <= EncM::MAX) {
      EncM em{};
      em.row = (uint32_t)row;
      em.clog = clog;
      unsigned r = 0;
      for (unsigned e = 0; e < k; e++) {
        em.row_of[e] = -1;
        const int ei = enc[i0 + e].ecd;
        if (ei < 0)
          continue;
        for (unsigned l = 0; l < lvl; l++) {
          const uint64_t q = G.q[l];
          for (size_t j = 0; j < row; j++) {
            const int64_t c = coef[(size_t)ei * row + j];
            const uint64_t a = c >= 0 ? (uint64_t)c % q : (q - (uint64_t)(-(c + 1)) % q - 1) % q;
            em.v[((size_t)r * lvl + l) * row + j] = a;
          }
        }
        em.row_of[e] = (int32_t)r++;
      }
      k_enc_combine_m(b, em, k, g_spec.buf + off * 3 * w, enc[i0].pk0, enc[i0].pk1, lvl);
      i0 = i1;
      continue;
    }
    // plaintexts that are queued encodes join e0 as coefficients (EncCoef):
    // the combine then reads no NTT-form plaintext
    EncCoef ec{};
    ec.clog = clog;
    ec.row = (uint32_t)row;
    unsigned nrows = 0;
    for (unsigned e = 0; e < k; e++)
      ec.row_of[e] = enc[i0 + e].ecd;
    for (unsigned e = 0; e < k; e++)
      nrows += enc[i0 + e].ecd >= 0;
    if (nrows * row <= EncCoef::MAX) {
      unsigned r = 0;
      for (unsigned e = 0; e < k; e++)
        if (enc[i0 + e].ecd >= 0) {
          memcpy(ec.v + r * row, coef.data() + (size_t)enc[i0 + e].ecd * row, row * 8);
          ec.row_of[e] = (int32_t)r++;
        }
    } else {
      ec.p = dev_coef();
    }
    Ws vee(3 * k * w);
    LimbSet s = limbset(vee.p, mods, lvl, 3 * k, w);
    k_sample_enc(s, enc[i0].stream, 3 * k, nrows ? &ec : nullptr);
    k_ntt(s, false);
    k_enc_combine_batch(b, k, vee.p, enc[i0].pk0, enc[i0].pk1, lvl);
    i0 = i1;
  }
  if (st)
    stage_done(*st);
}

static void encode_limbs(uint64_t *dst, const double *z, unsigned s, double scale, const unsigned *mods,
                         unsigned nm)
{
  Ws dcoef(G.n);
  if (s >= gpu_ecd_min()) {
    Ws work(2 * (size_t)s + 2);
    upload(work.p, z, (size_t)s * 16);
    k_encode_coeffs((int64_t *)dcoef.p, (double *)work.p, s, scale);
  } else {
    std::vector<int64_t> coef(G.n);
    hm_encode_coeffs(coef.data(), z, s, G.n, scale);
    upload(dcoef.p, coef.data(), (size_t)G.n * 8);
  }
  LimbSet ls = limbset(dst, mods, nm, 1, (size_t)nm << G.logn);
  k_lift_ntt(ls, (const int64_t *)dcoef.p);
}

extern "C" void he_ecd_ex(he_pt_t *pt, const gpqhe_complex_t z[], unsigned int slots, double scale,
                          unsigned int nlimbs)
{
  HPROF("ecd");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  if (!defer_ok(slots))
    check_ctx();
  if (nlimbs < 1 || nlimbs > G.L)
    gpqhe_die("he_ecd_ex: bad level %u", nlimbs);
  if (defer_ok(slots)) {
    // queued (flush_pending); a plaintext a queued encryption still reads, or
    // a queued encode target, is flushed first
    flush_ew();
    if (!g_pgemv.empty())
      flush_gemvs();
    bool busy = false;
    for (const PendEnc &e : g_penc)
      busy |= e.m == pt->data || e.c0 == pt->data;
    for (const PendEcd &e : g_pecd)
      busy |= e.dst == pt->data;
    if (busy)
      flush_pending();
    if (slots > G.n / 2)
      gpqhe_die("bad slot count %u", slots);
    const size_t at = g_pcoef.size();
    g_pcoef.resize(at + 2 * (size_t)slots);
    hm_encode_slots(g_pcoef.data() + at, (const double *)z, slots, scale);
    g_pecd.push_back({pt->data, nlimbs, slots, at});
  } else {
    unsigned mods[GPQHE_MAXMOD];
    for (unsigned i = 0; i < nlimbs; i++)
      mods[i] = i;
    encode_limbs(pt->data, (const double *)z, slots, scale, mods, nlimbs);
  }
  pt->nlimbs = nlimbs;
  pt->scale = scale;
  pt->flags = 0;
}

extern "C" void he_ecd(he_pt_t *pt, const gpqhe_complex_t z[])
{
  he_ecd_ex(pt, z, G.slots, G.delta, G.L);
}

static void *zpin(size_t bytes)
{
  if (g_zpin_bytes < bytes) {
    if (g_zpin)
      HIP_CHECK(hipHostFree(g_zpin));
    HIP_CHECK(hipHostMalloc(&g_zpin, bytes, hipHostMallocDefault));
    g_zpin_bytes = bytes;
  }
  void *dz = nullptr;
  HIP_CHECK(hipHostGetDevicePointer(&dz, g_zpin, 0));
  return dz;
}

// After the small-N decode (he_dcd_ex): record the decode's end, then launch
// the next step's encryption noise (SpecNoise) if the last flush had one run
// of encryptions.  True if launched (the caller then waits on g_dcd_ev).
static bool spec_launch()
{
  static const bool on = env_u("GPQHE_SPEC", 1) != 0;
  const unsigned k = g_spec_next_k, lvl = g_spec_next_lvl;
  g_smu_next.pending = false;  // superseded
  if (!on || !k || !lvl || k > GPQHE_MAXGRP || !defer_ok(0))
    return false;
  if (!g_dcd_ev)
    HIP_CHECK(hipEventCreateWithFlags(&g_dcd_ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(g_dcd_ev, G.stream));
  const size_t w = (size_t)lvl << G.logn, words = 3 * (size_t)k * w;
  if (g_spec.words != words) {
    pool_free(g_spec.buf);  // stream-ordered: its last reader was launched before
    g_spec.buf = (uint64_t *)pool_alloc(words * 8);
    g_spec.words = words;
  }
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned l = 0; l < lvl; l++)
    mods[l] = l;
  LimbSet s = limbset(g_spec.buf, mods, lvl, 3 * k, w);
  k_sample_enc(s, G.counter, 3 * k);
  k_ntt(s, false);
  g_spec.base = G.counter;
  g_spec.k = k;
  g_spec.lvl = lvl;
  g_spec.valid = true;
  // the gemv inputs of the last step, made from the same encryption slots of
  // this noise: their c1 differences and ModUp (SpecModup)
  g_smu.valid = false;
  const std::vector<SpecPat> &pats = g_spec_pats_next;
  bool ok = !pats.empty() && g_spec_pk1_next && lvl >= 2;
  for (const SpecPat &p : pats)
    ok &= p.oa < k && p.ob < k;
  if (ok) {
    const unsigned np = (unsigned)pats.size(), nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
    const size_t dw = (size_t)np * ndig * nm << G.logn;
    if (g_smu.dwords != dw) {
      pool_free(g_smu.D);
      g_smu.D = (uint64_t *)pool_alloc(dw * 8);
      g_smu.dwords = dw;
    }
    C1Diffs cd{};
    for (unsigned i = 0; i < np; i++) {
      cd.va[i] = g_spec.buf + (size_t)3 * pats[i].oa * w;
      cd.vb[i] = g_spec.buf + (size_t)3 * pats[i].ob * w;
    }
    k_modup_ntt_diffs(g_smu.D, cd, np, (size_t)ndig * nm << G.logn, g_spec_pk1_next, lvl);
    g_smu.pats = pats;
    g_smu.base = g_spec.base;
    g_smu.pk1 = g_spec_pk1_next;
    g_smu.lvl = lvl;
    g_smu.valid = true;
  }
  return true;
}

// flush_gemvs of a small-N step: the next step's speculation (the same noise
// and ModUp spec_launch runs after the decode) is carried by this step's
// gemv_inner and ModDown launches as extra workgroups (SpecAttach), where it
// uses the CUs those few-workgroup kernels leave idle.  Only when the three
// launches take it: the gemvs in one inner-product launch (one), the noise
// sampling fits its z slice, and the ModDown of P q_top drops K + 1 >= 2
// limbs (the two-launch form).  The buffers are free: this step's combine and
// inner products, which read the current speculation, run before in stream
// order.  (A second stream for this work measured 3x slower)
static bool spec_attach(bool one, unsigned glvl, const std::vector<SpecPat> &pats = g_spec_pats_next,
                        const uint64_t *pk1 = g_spec_pk1_next)
{
  static const bool on = env_u("GPQHE_SPEC", 1) != 0 && env_u("GPQHE_SPEC_ATTACH", 1) != 0;
  const unsigned k = g_spec_next_k, lvl = g_spec_next_lvl;
  if (!on || !one || !k || !lvl || k > GPQHE_MAXGRP || !defer_ok(0) || G.logn < 10 || G.logn > 12 || G.K < 1)
    return false;
  if ((size_t)3 * k * (G.n / 512) > (size_t)(G.n / 64) * (glvl + G.K))
    return false;
  const size_t w = (size_t)lvl << G.logn, words = 3 * (size_t)k * w;
  if (g_spec.words != words) {
    pool_free(g_spec.buf);  // stream-ordered: its last reader was launched before
    g_spec.buf = (uint64_t *)pool_alloc(words * 8);
    g_spec.words = words;
  }
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned l = 0; l < lvl; l++)
    mods[l] = l;
  g_sa = SpecAttach{};
  g_smu_next.pending = false;
  g_sa.noise = limbset(g_spec.buf, mods, lvl, 3 * k, w);
  g_sa.stream = G.counter;
  g_sa.npoly = 3 * k;
  g_sa.sample = g_sa.ntt = true;
  g_spec.base = G.counter;
  g_spec.k = k;
  g_spec.lvl = lvl;
  g_spec.valid = true;
  g_smu.valid = false;
  bool ok = !pats.empty() && pk1 && lvl >= 2;
  for (const SpecPat &p : pats)
    ok &= p.oa < k && p.ob < k;
  if (ok) {
    const unsigned np = (unsigned)pats.size(), nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
    const size_t dw = (size_t)np * ndig * nm << G.logn;
    if (g_smu.dwords != dw) {
      pool_free(g_smu.D);  // stream-ordered: its last reader was launched before
      g_smu.D = (uint64_t *)pool_alloc(dw * 8);
      g_smu.dwords = dw;
    }
    // the ModUp itself runs behind this step's decode (he_dcd_ex), in the
    // device time the caller's host work leaves idle: attached to the
    // ModDown it lengthened the chain the decode waits on (13.9 -> 21.5 us)
    for (unsigned i = 0; i < np; i++) {
      g_smu_next.cd.va[i] = g_spec.buf + (size_t)3 * pats[i].oa * w;
      g_smu_next.cd.vb[i] = g_spec.buf + (size_t)3 * pats[i].ob * w;
    }
    g_smu_next.np = np;
    g_smu_next.d_stride = (size_t)ndig * nm << G.logn;
    g_smu_next.pk1 = pk1;
    g_smu_next.lvl = lvl;
    g_smu_next.pending = true;
    // its first half (the differences' inverse transforms) rides on this
    // step's ModDown (k_moddown: the launch after the noise transforms), so
    // only the second half runs behind the decode (GPQHE_SPEC_MODUP_SPLIT=0:
    // the whole ModUp there)
    static const bool split = env_u("GPQHE_SPEC_MODUP_SPLIT", 1) != 0;
    if (split) {
      const size_t yw = (size_t)np * lvl << G.logn;
      if (g_smu.ywords != yw) {
        pool_free(g_smu.Y);  // stream-ordered: its last reader was launched before
        g_smu.Y = (uint64_t *)pool_alloc(yw * 8);
        g_smu.ywords = yw;
      }
      g_sa.mh.cd = g_smu_next.cd;
      g_sa.mh.pk1 = pk1;
      g_sa.mh.D = g_smu.D;
      g_sa.mh.Y = g_smu.Y;
      g_sa.mh.d_stride = g_smu_next.d_stride;
      g_sa.mh.np = np;
      g_sa.mh.lvl = lvl;
      g_sa.modup_inv = true;
    }
    const std::vector<SpecPat> keep = pats;  // (pats may be g_smu.pats itself)
    g_smu.pats = keep;
    g_smu.base = g_spec.base;
    g_smu.pk1 = pk1;
    g_smu.lvl = lvl;
  }
  return true;
}

// The ModUp spec_attach left pending, behind the decode: true if launched.
static bool spec_modup_launch()
{
  if (!g_smu_next.pending)
    return false;
  g_smu_next.pending = false;
  if (g_sa.modup_inv_done) {  // its first half ran in this step's ModDown
    g_sa.modup_inv_done = false;
    k_modup_fwd_diffs(g_sa.mh);
  } else {
    k_modup_ntt_diffs(g_smu.D, g_smu_next.cd, g_smu_next.np, g_smu_next.d_stride, g_smu_next.pk1, g_smu_next.lvl);
  }
  g_smu.valid = true;
  return true;
}

// k gemvs, each one launch's worth of diagonals: the inner products of all in
// one launch, and one ModDown of their accumulators (acc, one after another)
// into y0 (and y1).
static void gemv_run_jobs(const GemvJobs &jobs, unsigned k, unsigned lvl, uint64_t *acc, size_t ypstride, uint64_t *y0,
                          uint64_t *y1)
{
  k_gemv_inner_jobs(jobs, k, lvl);
  k_moddown(y0, ypstride, acc, (size_t)(lvl + G.K) * G.n, 2 * k, lvl, 1, k == 1 ? nullptr : y1);
  // spec_attach predicts which launches take the attached work; should a
  // launch's own eligibility test (kernels.hip: gemv_inner's z slice, the
  // ModDown's dropped limbs) ever disagree, the work runs here in its own
  // launches, same streams and buffers, so the speculation stays valid
  if (g_sa.sample) {
    g_sa.sample = false;
    k_sample_enc(g_sa.noise, g_sa.stream, g_sa.npoly);
  }
  if (g_sa.ntt) {
    g_sa.ntt = false;
    k_ntt(g_sa.noise, false);
  }
}

// The last step's gemvs on this step's encryptions (SpecGemv), right after
// their combine: one inner-product launch for both (differences formed in the
// kernel, the speculated ModUp digits), one ModDown with two outputs, and the
// next step's speculation attached to them as flush_gemvs would (spec_attach,
// the patterns predicted to repeat).  Only when every recorded gemv ran one
// launch of diagonals and the ModUp digits speculated for this step are there.
static void spec_gemv_launch(const std::vector<PendEnc> &enc, const std::vector<SgRec> &recs)
{
  static const bool on = env_u("GPQHE_SPEC_GEMV", 1) != 0;
  g_sg.valid = false;
  const unsigned np = (unsigned)recs.size(), lvl = enc.empty() ? 0 : enc[0].lvl;
  if (!on || !np || np > GemvJobs::MAX || !g_smu.valid || g_smu.lvl != lvl || g_smu.base != enc[0].stream ||
      g_smu.pats.size() != np || lvl < 2)
    return;
  for (unsigned i = 0; i < np; i++) {
    const SgRec &r = recs[i];
    if (r.pat.oa != g_smu.pats[i].oa || r.pat.ob != g_smu.pats[i].ob || r.pat.oa >= enc.size() ||
        r.pat.ob >= enc.size() || r.gen != g_key_gen || r.dgen != g_dc.gen || !r.dg.count)
      return;  // (dgen: the diagonal cache was cleared since, r.dg.pt points into freed blocks)
  }
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n, dstride = (size_t)ndig * nm * n, ypw = (size_t)G.L * n;
  for (unsigned i = 0; i < np; i++)
    if (!g_sg.Y[i])  // (stream-ordered: a block swapped in last step was last read before this launch)
      g_sg.Y[i] = (uint64_t *)pool_alloc(2 * ypw * 8);
  Ws acc((size_t)np * 2 * nm * n);
  GemvJobs jobs;
  for (unsigned i = 0; i < np; i++) {
    const PendEnc &a = enc[recs[i].pat.oa], &b = enc[recs[i].pat.ob];
    jobs.j[i] = GemvJob{acc.p + (size_t)i * 2 * nm * n, g_smu.D + i * dstride, a.c0, a.c1, recs[i].dg, 0};
    jobs.j[i].y0 = b.c0;
    jobs.j[i].y1 = b.c1;
    g_sg.x[i][0] = a.c0;
    g_sg.x[i][1] = b.c0;
    g_sg.x[i][2] = a.c1;
    g_sg.x[i][3] = b.c1;
    g_sg.sa[i] = a.stream;
    g_sg.sb[i] = b.stream;
    g_sg.rec[i] = recs[i];
    g_sg.used[i] = false;
  }
  // the next step's noise in these launches' idle CUs, its ModUp behind the
  // decode, for the same patterns (the digits these jobs read are overwritten
  // only by that ModUp, after the decode in stream order)
  if (!g_spec_early && spec_attach(true, lvl, std::vector<SpecPat>(g_smu.pats), g_smu.pk1))
    g_spec_early = true;
  gemv_run_jobs(jobs, np, lvl, acc.p, ypw, g_sg.Y[0], g_sg.Y[1]);
  g_sg.np = np;
  g_sg.lvl = lvl;
  g_sg.valid = true;
  // this step's role blocks, and the last step's tail replayed on them (SpecDcd)
  g_sd_ctx = SdCtx{};
  for (unsigned i = 0; i < np; i++)
    g_sd_ctx.y[i] = g_sg.Y[i];
  g_sd_ctx.ny = np;
  g_sd_ctx.ylvl = lvl - 1;
  for (unsigned o = 0; o < enc.size() && o < GPQHE_MAXGRP; o++) {
    g_sd_ctx.e[o][0] = enc[o].c0;
    g_sd_ctx.e[o][1] = enc[o].c1;
    g_sd_ctx.es[o] = enc[o].stream;
    g_sd_ctx.ne = o + 1;
  }
  g_sd_ctx.elvl = lvl;
  g_sd_ctx.valid = true;
  g_sd.valid = false;
  if (g_sd_next_ok && sd_on())
    sd_replay(g_sd_next);
}

extern "C" void he_dcd_ex(gpqhe_complex_t z[], const he_pt_t *pt, unsigned int slots)
{
  HPROF("dcd");
  const size_t zb = (size_t)slots * 16;
  if (G.init && defer_ok(0) && slots && !(slots & (slots - 1)) && slots <= GPQHE_DCD_ONEPASS &&
      slots <= G.n / 2 && !(pt->flags & GPQHE_F_COEFF) && pt->nlimbs >= 1 && pt->nlimbs <= 2) {
    // the small-N step's tail: the queued elementwise program (he_add, he_neg,
    // he_copy_ct, he_add, he_dec), then the inverse transform and the decoder
    // in one more launch (k_ew_decode)
    // this step's tail pattern (replayed next step), and the replay of the
    // last step's (SpecDcd) when this step's is the same
    SdPat cur;
    const bool quiet = g_pgemv.empty() && g_pecd.empty() && g_penc.empty();
    g_sd_next_ok = quiet && sd_pattern(g_pew, pt->data, pt->nlimbs, slots, pt->scale, g_sd_ctx, cur);
    if (g_sd_next_ok)
      g_sd_next = cur;
    if (g_sd.valid && g_sd_next_ok && g_spec_early && cur.same(g_sd.pat) && sd_enc_fresh(cur, g_sd_ctx)) {
      g_sd.valid = false;
      flush_ew();  // the real program: its objects, not waited for
      g_spec_early = false;
      if (g_smu_next.pending)
        spec_modup_launch();
      const hipError_t q = hipEventQuery(g_sd.ev);
      (void)hipGetLastError();  // (not ready is no error)
      if (q != hipSuccess) {
        // the device behind the caller: the replay only lengthens the chain
        // (GPQHE_SPEC_DCD=2 keeps it on: tests)
        if (++g_sd_late >= 2 && env_u("GPQHE_SPEC_DCD", 1) != 2)
          g_sd_off = true;
      } else {
        g_sd_late = 0;
      }
      HIP_CHECK(hipEventSynchronize(g_sd.ev));
      memcpy(z, g_sd.z, zb);
      g_sd_taken++;
      return;
    }
    g_sd.valid = false;
    if (!g_pgemv.empty())
      flush_gemvs();
    if (!g_pecd.empty() || !g_penc.empty())
      flush_pending();
    // workspace and pinned buffer first: the pool's out-of-memory path flushes
    // the elementwise queue, which must still hold the program then (its ops
    // may name freed blocks the flush would otherwise release under it)
    Ws c((size_t)pt->nlimbs << G.logn);
    double *zd = (double *)zpin(zb);
    const EwProg p = g_pew;
    g_pew.count = 0;
    k_ew_decode(p, zd, pt->data, pt->nlimbs, slots, pt->scale, c.p);
    const bool early = g_spec_early;
    g_spec_early = false;
    bool spec = false;
    if (early && g_smu_next.pending) {
      if (!g_dcd_ev)
        HIP_CHECK(hipEventCreateWithFlags(&g_dcd_ev, hipEventDisableTiming));
      HIP_CHECK(hipEventRecord(g_dcd_ev, G.stream));
      spec = spec_modup_launch();
    } else if (!early) {
      spec = spec_launch();
    }
    if (spec) {
      HIP_CHECK(hipEventSynchronize(g_dcd_ev));  // the decode, not the noise behind it
    } else {
      HIP_CHECK(hipStreamSynchronize(G.stream));
    }
    memcpy(z, g_zpin, zb);
    return;
  }
  check_ctx();
  const unsigned nl = pt->nlimbs;
  const size_t words = (size_t)nl << G.logn;
  Ws c(words);
  const uint64_t *src = pt->data;
  if (!(pt->flags & GPQHE_F_COEFF)) {
    // out-of-place inverse transform (the plaintext stays in NTT form)
    k_ntt_ex(qlimbs(pt->data, nl, 1, words), qlimbs(c.p, nl, 1, words), true, nullptr);
    src = c.p;
  }
  // CRT lift + FFT on the GPU (k_decode); only the s values cross PCIe,
  // written by the kernel straight into pinned host memory when one launch
  // does it (no copy launch)
  if (slots <= GPQHE_DCD_ONEPASS) {
    k_decode((double *)zpin(zb), src, nl, slots, pt->scale);
    HIP_CHECK(hipStreamSynchronize(G.stream));
    memcpy(z, g_zpin, zb);
    return;
  }
  Ws zd(2 * (size_t)slots);
  k_decode((double *)zd.p, src, nl, slots, pt->scale);
  HIP_CHECK(hipMemcpyAsync(z, zd.p, zb, hipMemcpyDeviceToHost, G.stream));
  HIP_CHECK(hipStreamSynchronize(G.stream));
}

extern "C" void he_dcd(gpqhe_complex_t z[], const he_pt_t *pt)
{
  he_dcd_ex(z, pt, G.slots);
}

extern "C" void he_enc_pk(he_ct_t *ct, const he_pt_t *pt, const he_pk_t *pk)
{
  HPROF("enc_pk");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  const unsigned lvl = pt->nlimbs;
  if (defer_ok(0)) {
    // queued (flush_pending): streams taken now, in call order
    flush_ew();
    if (!g_pgemv.empty())
      flush_gemvs();
    bool busy = false;
    for (const PendEnc &e : g_penc)
      busy |= e.m == ct->data || e.c0 == ct->data;
    for (const PendEcd &e : g_pecd)
      busy |= e.dst == ct->data;
    if (busy)
      flush_pending();
    const uint64_t stream = next_stream();
    next_stream();
    next_stream();
    // a plaintext that is itself a queued encode (at this level) joins e0 as
    // coefficients (EncCoef)
    int ei = -1;
    for (size_t i = 0; i < g_pecd.size(); i++)
      if (g_pecd[i].dst == pt->data && g_pecd[i].lvl == lvl)
        ei = (int)i;
    g_penc.push_back({limb(ct, 0, 0), limb(ct, 1, 0), pt->data, limb(pk, 0, 0), limb(pk, 1, 0), lvl, stream, ei});
    ct->nlimbs = lvl;
    ct->scale = pt->scale;
    ct->flags = 0;
    return;
  }
  check_ctx();
  const size_t w = (size_t)lvl << G.logn;
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned i = 0; i < lvl; i++)
    mods[i] = i;
  // v (ternary), e0, e1 (CBD) on consecutive streams, sampled and NTT'd in
  // one launch each (the values of three sample_small_ntt calls in order)
  Ws vee(3 * w);
  LimbSet s = limbset(vee.p, mods, lvl, 3, w);
  const uint64_t stream = next_stream();
  next_stream();
  next_stream();
  k_sample_enc(s, stream, 3);
  k_ntt(s, false);
  k_enc_combine(limb(ct, 0, 0), limb(ct, 1, 0), vee.p, vee.p + w, vee.p + 2 * w, limb(pk, 0, 0), limb(pk, 1, 0),
                pt->data, lvl);
  ct->nlimbs = lvl;
  ct->scale = pt->scale;
  ct->flags = 0;
}

extern "C" void he_enc_sk(he_ct_t *ct, const he_pt_t *pt, const poly_mpi_t *sk)
{
  check_ctx();
  const unsigned lvl = pt->nlimbs;
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned i = 0; i < lvl; i++)
    mods[i] = i;
  sample_uniform(limb(ct, 1, 0), mods, lvl);
  Ws e((size_t)lvl << G.logn);
  sample_small_ntt(e.p, mods, lvl, 1);
  k_enc_sk_combine(limb(ct, 0, 0), limb(ct, 1, 0), e.p, sk->data, pt->data, lvl);
  ct->nlimbs = lvl;
  ct->scale = pt->scale;
  ct->flags = 0;
}

// Queue elementwise ops (defer_ok(0): n <= 2^12); false: run them now.
static bool ew_defer(unsigned nops)
{
  if (!defer_ok(0))
    return false;
  if (!g_pgemv.empty())
    flush_gemvs();
  if (!g_pecd.empty() || !g_penc.empty())
    flush_pending();
  if (g_pew.count + nops > EwProg::MAX)
    flush_ew();
  return true;
}

static void ew_push(uint32_t kind, uint64_t *out, const uint64_t *a, const uint64_t *b, const uint64_t *sk,
                    unsigned lvl)
{
  g_pew.op[g_pew.count++] = EwOp{out, a, b, sk, kind, lvl};
  // out's provenance after this op (C1Prov): the difference of two fresh
  // encryptions at their full level with one public key, or none
  C1Prov d{};
  bool known = false;
  if (kind == EW_SUB && !g_prov.empty()) {
    auto ia = g_prov.find(a), ib = g_prov.find(b);
    if (ia != g_prov.end() && ib != g_prov.end() && !ia->second.sub && !ib->second.sub && !ia->second.c0 &&
        !ib->second.c0 && ia->second.pk1 == ib->second.pk1 && ia->second.lvl == lvl && ib->second.lvl == lvl) {
      d = C1Prov{ia->second.sa, ib->second.sa, ia->second.pk1, lvl, true};
      known = true;
    }
  }
  if (known)
    g_prov[out] = d;
  else if (!g_prov.empty())
    g_prov.erase(out);
}

extern "C" void he_dec(he_pt_t *pt, const he_ct_t *ct, const poly_mpi_t *sk)
{
  HPROF("dec");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  if (ew_defer(1)) {
    ew_push(EW_DEC, pt->data, limb(ct, 0, 0), limb(ct, 1, 0), sk->data, ct->nlimbs);
    pt->nlimbs = ct->nlimbs;
    pt->scale = ct->scale;
    pt->flags = 0;
    return;
  }
  check_ctx();
  k_dec(pt->data, limb(ct, 0, 0), limb(ct, 1, 0), sk->data, ct->nlimbs);
  pt->nlimbs = ct->nlimbs;
  pt->scale = ct->scale;
  pt->flags = 0;
}

// ===========================================================================
// Evaluation
// ===========================================================================
static void check_scales(double a, double b, const char *op)
{
  if (fabs(a / b - 1.0) > 1e-9)
    gpqhe_die("%s: scale mismatch (%g vs %g)", op, a, b);
}

static void addsub(he_ct_t *out, const he_ct_t *a, const he_ct_t *b, int op)
{
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  check_scales(a->scale, b->scale, op ? "he_sub" : "he_add");
  const unsigned lvl = std::min(a->nlimbs, b->nlimbs);
  const double scale = a->scale;
  if (ew_defer(2)) {
    for (unsigned p = 0; p < 2; p++)
      ew_push(op ? EW_SUB : EW_ADD, limb(out, p, 0), limb(a, p, 0), limb(b, p, 0), nullptr, lvl);
  } else {
    check_ctx();
    k_binop(out->data, a->data, b->data, 2, lvl, pstride(out), pstride(a), pstride(b), op);
  }
  out->nlimbs = lvl;
  out->scale = scale;
  out->flags = 0;
}

extern "C" void he_add(he_ct_t *out, const he_ct_t *a, const he_ct_t *b)
{
  HPROF("add");
  addsub(out, a, b, 0);
}
extern "C" void he_sub(he_ct_t *out, const he_ct_t *a, const he_ct_t *b)
{
  HPROF("sub");
  addsub(out, a, b, 1);
}

extern "C" void he_neg(he_ct_t *ct)
{
  HPROF("neg");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  if (ew_defer(2)) {
    for (unsigned p = 0; p < 2; p++)
      ew_push(EW_NEG, limb(ct, p, 0), limb(ct, p, 0), nullptr, nullptr, ct->nlimbs);
    return;
  }
  check_ctx();
  k_neg(ct->data, 2, ct->nlimbs, pstride(ct));
}

extern "C" void he_copy_ct(he_ct_t *dst, const he_ct_t *src)
{
  HPROF("copy_ct");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  if (dst == src)
    return;
  if (ew_defer(2)) {
    for (unsigned p = 0; p < 2; p++)
      ew_push(EW_COPY, limb(dst, p, 0), limb(src, p, 0), nullptr, nullptr, src->nlimbs);
  } else {
    check_ctx();
    const size_t bytes = ((size_t)src->nlimbs << G.logn) * 8;
    for (unsigned p = 0; p < 2; p++)
      HIP_CHECK(hipMemcpyAsync(limb(dst, p, 0), limb(src, p, 0), bytes, hipMemcpyDeviceToDevice, G.stream));
  }
  dst->nlimbs = src->nlimbs;
  dst->scale = src->scale;
  dst->flags = src->flags;
}

extern "C" void he_moddown(he_ct_t *ct)
{
  HPROF("moddown");
  // bookkeeping only (queued work captured its levels): no flush
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  if (ct->nlimbs < 2)
    gpqhe_die("he_moddown: ciphertext at the lowest level");
  ct->nlimbs--;
}

extern "C" void he_add_pt(he_ct_t *out, const he_ct_t *a, const he_pt_t *pt)
{
  check_ctx();
  check_scales(a->scale, pt->scale, "he_add_pt");
  const unsigned lvl = std::min(a->nlimbs, pt->nlimbs);
  const double scale = a->scale;
  if (out != a) {
    he_copy_ct(out, a);
    flush_ew();  // the copy may have been queued
  }
  k_add_pt(out->data, out->data, pt->data, lvl, pstride(out));
  out->nlimbs = lvl;
  out->scale = scale;
  out->flags = 0;
}

extern "C" void he_mul_pt(he_ct_t *out, const he_ct_t *a, const he_pt_t *pt)
{
  check_ctx();
  const unsigned lvl = std::min(a->nlimbs, pt->nlimbs);
  const double scale = a->scale * pt->scale;
  if (pstride(out) != pstride(a))
    gpqhe_die("he_mul_pt: layout mismatch");
  k_mul_pt(out->data, a->data, pt->data, lvl, pstride(a));
  out->nlimbs = lvl;
  out->scale = scale;
  out->flags = 0;
}

// Tensor + relinearize [+ rescale] for `count` ciphertext pairs.
//   a, b: ciphertext i at a + i*in_stride, c1 at + in_pstride;
//   out:  polynomial p (= 2 i + {0,1}) at out + p*out_pstride.
// out may overlap a or b (he_mul(c, c, b)): every input read precedes the
// final ModDown kernel, the only writer of out, on one stream.
static void mul_chunk(uint64_t *out, size_t out_pstride, const uint64_t *a, const uint64_t *b, size_t in_stride,
                      size_t in_pstride, unsigned count, unsigned lvl, const he_evk_t *rlk, bool rescale)
{
  if (!rlk->data || rlk->dnum != G.dnum)
    gpqhe_die("relinearization key missing or built for another dnum");
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n;
  if (k_mul_split_ok(lvl) && rlk->reserved) {
    // split key switch: the kept slots' epilogue writes out while other pairs'
    // inputs may still be unread, so out must not overlap the inputs -- except
    // he_mul(c, c, b) on one pair, where every output word replaces the input
    // word read by the same thread
    const uint64_t *evkm = (const uint64_t *)(uintptr_t)rlk->reserved;
    const unsigned keep = rescale ? lvl - 1 : lvl;
    auto span = [](const uint64_t *p, size_t hi) { return std::make_pair((uintptr_t)p, (uintptr_t)(p + hi)); };
    const auto o = span(out, (2 * (size_t)count - 1) * out_pstride + (size_t)keep * n);
    const auto ia = span(a, (count - 1) * in_stride + in_pstride + (size_t)lvl * n);
    const auto ib = span(b, (count - 1) * in_stride + in_pstride + (size_t)lvl * n);
    auto overlap = [&](std::pair<uintptr_t, uintptr_t> x) { return o.first < x.second && x.first < o.second; };
    const bool same_layout = count == 1 && out_pstride == in_pstride && (out == a || out == b);
    if ((overlap(ia) || overlap(ib)) && !(same_layout && (!overlap(ia) || out == a) && (!overlap(ib) || out == b))) {
      const size_t words = (2 * (size_t)count - 1) * out_pstride + (size_t)keep * n;
      Ws tmp(words);
      k_mul_relin_split(tmp.p, out_pstride, a, b, in_stride, in_pstride, evkm, count, lvl, rescale);
      HIP_CHECK(hipMemcpyAsync(out, tmp.p, words * 8, hipMemcpyDeviceToDevice, G.stream));
      return;
    }
    k_mul_relin_split(out, out_pstride, a, b, in_stride, in_pstride, evkm, count, lvl, rescale);
    return;
  }
  const size_t d2_stride = lvl * n, D_stride = (size_t)ndig * nm * n, acc_stride = 2 * nm * n;
  Ws d2(count * d2_stride), D(count * D_stride), acc(count * acc_stride);
  if (k_ks_fused_ok() && rlk->reserved) {
    // fused path (2^13 <= n <= 2^17): d0/d1 are formed by the key switch from
    // a and b (no tensor buffer); the ModDown runs on the dropped limbs'
    // inverse row passes
    Ws y(count * d2_stride);
    const unsigned keep = rescale ? lvl - 1 : lvl;
    const uint64_t *evkm = (const uint64_t *)(uintptr_t)rlk->reserved;
    k_mul_keyswitch_fused(acc.p, d2.p, y.p, D.p, a, b, in_stride, in_pstride, evkm, count, lvl, keep);
    k_moddown_fused(out, out_pstride, acc.p, nm * n, 2 * count, lvl, rescale ? 1 : 0);
    return;
  }
  // generic path (n <= 2^12: HECTR's own ring): materialized tensor, ModUp,
  // NTT, inner product, ModDown as separate launches
  const size_t d01_stride = 2 * lvl * n;
  Ws d01(count * d01_stride);
  k_tensor(d01.p, d2.p, a, b, lvl, in_stride, in_pstride, count, d01_stride);
  k_ntt(qlimbs(d2.p, lvl, count, d2_stride), true);
  k_modup(D.p, d2.p, count, d2_stride, D_stride, lvl);
  unsigned mods[GPQHE_MAXMOD];
  basis_qp(lvl, mods);
  k_ntt(limbset(D.p, mods, nm, count * ndig, nm * n), false);
  k_ks_inner(acc.p, D.p, count, D_stride, acc_stride, rlk->data, lvl, 1, d01.p, d01.p + lvl * n, d01_stride,
             nullptr, false);
  k_moddown(out, out_pstride, acc.p, nm * n, 2 * count, lvl, rescale ? 1 : 0);
}

static void mul_core(he_ct_t *out, const he_ct_t *a, const he_ct_t *b, const he_evk_t *rlk, bool rescale)
{
  check_ctx();
  const unsigned lvl = std::min(a->nlimbs, b->nlimbs);
  if (rescale && lvl < 2)
    gpqhe_die("he_mul_rescale: no level left to rescale");
  if (pstride(a) != pstride(b))
    gpqhe_die("he_mul: layout mismatch");
  const double scale = a->scale * b->scale;
  mul_chunk(out->data, pstride(out), a->data, b->data, 0, pstride(a), 1, lvl, rlk, rescale);
  out->nlimbs = rescale ? lvl - 1 : lvl;
  out->scale = rescale ? scale / (double)G.q[lvl - 1] : scale;
  out->flags = 0;
}

extern "C" void he_mul(he_ct_t *out, const he_ct_t *a, const he_ct_t *b, const he_evk_t *rlk)
{
  mul_core(out, a, b, rlk, false);
}

extern "C" void he_mul_rescale(he_ct_t *out, const he_ct_t *a, const he_ct_t *b, const he_evk_t *rlk)
{
  mul_core(out, a, b, rlk, true);
}

extern "C" void he_rescale(he_ct_t *ct)
{
  check_ctx();
  const unsigned lvl = ct->nlimbs;
  if (lvl < 2)
    gpqhe_die("he_rescale: ciphertext at the lowest level");
  k_moddown(ct->data, pstride(ct), ct->data, pstride(ct), 2, lvl, 2);
  ct->scale /= (double)G.q[lvl - 1];
  ct->nlimbs = lvl - 1;
}

static const he_evk_t *find_rot_key(const he_evk_t rk[], unsigned r, uint64_t g)
{
  const he_evk_t *k = &rk[r];
  if (!k->data || k->galois != (uint32_t)g)
    gpqhe_die("rotation key for r=%u (galois %llu) missing", r, (unsigned long long)g);
  if (k->dnum != G.dnum)
    gpqhe_die("rotation key built for dnum=%u, context dnum=%u", k->dnum, G.dnum);
  return k;
}

// c1 of x -> coefficient domain -> ModUp digits (NTT domain) in D.
static void hoist_modup(uint64_t *D, const he_ct_t *x, unsigned lvl)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  XPtrs x1{};
  x1.p[0] = limb(x, 1, 0);
  k_modup_ntt(D, x1, 1, (size_t)ndig * nm * G.n, lvl);
}

extern "C" void he_rot(he_ct_t *out, const he_ct_t *in, unsigned int rot, const he_evk_t rk[])
{
  check_ctx();
  rot %= G.slots;
  if (!rot) {
    he_copy_ct(out, in);
    return;
  }
  const unsigned lvl = in->nlimbs, nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n;
  const uint64_t g = galois_of_rot(rot);
  const he_evk_t *k = find_rot_key(rk, rot, g);
  if (gemv_win_on(lvl)) {  // (reads every input word before the ModDown writes out: in place is fine)
    const RotFold &f = rotkey_fold(rot, lvl, rk);
    FoldUse use(f.K);
    const double scale = in->scale;
    k_gemv_batch_ex(out->data, 0, pstride(out), in->data, 0, pstride(in), 1, lvl, f.K, &f.rot, 1, 0);
    out->nlimbs = lvl;
    out->scale = scale;
    out->flags = 0;
    return;
  }
  Ws D((size_t)ndig * nm * n), acc(2 * nm * n);
  hoist_modup(D.p, in, lvl);
  k_ks_inner(acc.p, D.p, 1, 0, 0, k->data, lvl, g, limb(in, 0, 0), nullptr, 0, nullptr, false);
  const double scale = in->scale;
  k_moddown(out->data, pstride(out), acc.p, nm * n, 2, lvl, 0);
  out->nlimbs = lvl;
  out->scale = scale;
  out->flags = 0;
}

// ---------------------------------------------------------------------------
// he_gemv: diagonal method, hoisted ModUp, diagonals encoded at scale q_top
// over the QP basis, one ModDown-and-rescale by P q_top at the end.
// Encoded diagonals are cached by content (DiagCache).
// ---------------------------------------------------------------------------
// y = M x, x at level lvl: y's metadata (x's scale read first: y may be x).
static void gemv_set_meta(he_ct_t *y, const he_ct_t *x, unsigned lvl)
{
  const double scale = x->scale;
  y->nlimbs = lvl - 1;
  y->scale = scale;
  y->flags = 0;
}

static int spec_record_pattern(const C1Prov &c, unsigned lvl);

// A he_gemv of SpecGemv pattern i: y <- Y_i, the result speculated at this
// step's encryptions, as a swap of blocks or two queued copies, and the
// pattern recorded for the next step as gemv_queued does (before anything
// flushes the queued differences it matches).  False: the normal path.
static bool spec_gemv_take(he_ct_t *y, const double *Md, const he_ct_t *x, const he_evk_t rk[])
{
  if (!g_sg.valid || !g_pecd.empty() || !g_penc.empty() || x->nlimbs != g_sg.lvl || !g_pgemv.empty() || !defer_ok(0))
    return false;
  const unsigned lvl = g_sg.lvl, s = G.slots;
  // x = a - b: the last queued op writing each of its polys is a he_sub
  const uint64_t *lz[4] = {};
  const uint64_t *xp[2] = {limb(x, 0, 0), limb(x, 1, 0)};
  for (unsigned j = 0; j < g_pew.count; j++)
    for (unsigned p = 0; p < 2; p++)
      if (g_pew.op[j].out == xp[p]) {
        const EwOp &o = g_pew.op[j];
        const bool sub = o.kind == EW_SUB && o.lvl >= lvl;
        lz[2 * p] = sub ? o.a : nullptr;
        lz[2 * p + 1] = sub ? o.b : nullptr;
      }
  if (!lz[0] || !lz[2])
    return false;
  // y must not be an operand of the queued ops (the copies run in the queue's
  // order, and a later op reading y would read the copy)
  const uint64_t *ylo = y->data, *yhi = y->data + 2 * pstride(y);
  auto hits = [&](const uint64_t *q, unsigned l) { return q && q < yhi && q + ((size_t)l << G.logn) > ylo; };
  for (unsigned j = 0; j < g_pew.count; j++) {
    const EwOp &o = g_pew.op[j];
    if (hits(o.a, o.lvl) || hits(o.b, o.lvl) || hits(o.s, o.lvl))
      return false;
  }
  auto fresh = [&](const uint64_t *p, uint64_t stream, bool c0) {
    auto it = g_prov.find(p);
    return it != g_prov.end() && !it->second.sub && it->second.c0 == c0 && it->second.sa == stream &&
           it->second.lvl == lvl;
  };
  for (unsigned i = 0; i < g_sg.np; i++) {
    const SgRec &r = g_sg.rec[i];
    if (g_sg.used[i] || lz[0] != g_sg.x[i][0] || lz[1] != g_sg.x[i][1] || lz[2] != g_sg.x[i][2] ||
        lz[3] != g_sg.x[i][3] || r.rk != rk || r.gen != g_key_gen || r.M.size() != 2 * (size_t)s * s ||
        memcmp(r.M.data(), Md, r.M.size() * 8) || !fresh(lz[0], g_sg.sa[i], true) ||
        !fresh(lz[1], g_sg.sb[i], true) || !fresh(lz[2], g_sg.sa[i], false) || !fresh(lz[3], g_sg.sb[i], false))
      continue;
    const size_t ypw = (size_t)G.L << G.logn;
    if (!ew_defer(2))
      return false;
    g_sg.used[i] = true;
    g_sg_taken++;
    prov_forget(y->data, pstride(y));
    if (y->npoly == 2 && y->cap == G.L && y->data) {
      // an object of the engine's own ciphertext shape: its block and Y_i's
      // trade places (no copy; the old block is the next step's Y_i -- no
      // queued op can name it: a queued op writing y would have to come
      // after this call, and the next speculation starts with empty queues)
      std::swap(y->data, g_sg.Y[i]);
    } else {
      for (unsigned p = 0; p < 2; p++)
        ew_push(EW_COPY, limb(y, p, 0), g_sg.Y[i] + p * ypw, nullptr, nullptr, lvl - 1);
    }
    auto pv = g_prov.find(limb(x, 1, 0));
    const int pat =
        pv != g_prov.end() && pv->second.sub && pv->second.lvl == lvl ? spec_record_pattern(pv->second, lvl) : -1;
    // Y_i was computed from the cached diagonals in stream order, before any
    // block a later clear of the cache freed could be written again, so it
    // is good to take whatever happened to the cache since.  Its record goes
    // on to the next step only while r.dg still points into the cache.
    if (pat >= 0 && (size_t)pat == g_sg_next.size() && r.dgen == g_dc.gen)
      g_sg_next.push_back({g_spec_pats_next[pat], r.M, r.dg, rk, g_key_gen, g_dc.gen});
    gemv_set_meta(y, x, lvl);
    return true;
  }
  return false;
}

// The pattern of a gemv input c whose c1 is the difference of two of this
// step's encryptions (C1Prov), recorded for the next step's speculation:
// its index in g_spec_pats_next, or -1.
static int spec_record_pattern(const C1Prov &c, unsigned lvl)
{
  const uint64_t span = 3 * (uint64_t)g_spec_next_k;
  if (g_spec_next_k && lvl == g_spec_next_lvl && c.sa >= g_step_base && c.sb >= g_step_base &&
      c.sa < g_step_base + span && c.sb < g_step_base + span && (c.sa - g_step_base) % 3 == 0 &&
      (c.sb - g_step_base) % 3 == 0 && g_spec_pats_next.size() < XPtrs::MAX &&
      (g_spec_pats_next.empty() || g_spec_pk1_next == c.pk1)) {
    g_spec_pk1_next = c.pk1;
    g_spec_pats_next.push_back({(unsigned)((c.sa - g_step_base) / 3), (unsigned)((c.sb - g_step_base) / 3)});
    return (int)g_spec_pats_next.size() - 1;
  }
  return -1;
}

// ... and the gemv itself (SgRec), when it is one launch of diagonals
static void spec_record_gemv(int pat, const double *Md, const PendGemv &pg, const he_evk_t rk[])
{
  if (pat < 0 || pg.dgs.size() != 1 || (size_t)pat != g_sg_next.size())
    return;
  const size_t mwords = 2 * (size_t)G.slots * G.slots;
  g_sg_next.push_back(
      {g_spec_pats_next[pat], std::vector<double>(Md, Md + mwords), pg.dgs[0], rk, g_key_gen, g_dc.gen});
}

void gemv_cache_clear()
{
  for (void *b : g_dc.blocks)
    pool_free(b);
  g_dc = DiagCache{{}, {}, 0, {}, g_dc.gen + 1};  // (what older generations recorded never matches again)
}

static std::string diag_key(const double *diag, unsigned s, unsigned lvl)
{
  std::string key((const char *)diag, (size_t)s * 16);
  key.append((const char *)&lvl, sizeof(lvl));
  return key;
}

// Would encoding count more diagonals at this level overflow the cache (and
// so clear it)?  he_gemv runs what refers to the cache before that happens.
static bool diag_cache_full(unsigned lvl, unsigned count = 1)
{
  const size_t bytes = ((size_t)(lvl + G.K) << G.logn) * 8;
  return g_dc.bytes + count * bytes > diag_cache_cap();
}

static const uint64_t *diag_pt(const double *diag, unsigned s, unsigned lvl)
{
  const std::string key = diag_key(diag, s, lvl);
  auto it = g_dc.pt.find(key);
  if (it != g_dc.pt.end())
    return it->second;
  unsigned mods[GPQHE_MAXMOD];
  const unsigned nm = basis_qp(lvl, mods);
  const size_t bytes = ((size_t)nm << G.logn) * 8;
  if (diag_cache_full(lvl))
    gemv_cache_clear();
  uint64_t *p = (uint64_t *)pool_alloc(bytes);
  g_dc.blocks.push_back(p);
  encode_limbs(p, diag, s, (double)G.q[lvl - 1], mods, nm);
  g_dc.pt[key] = p;
  g_dc.bytes += bytes;
  return p;
}

// The non-zero diagonals of M in increasing d: f(d, diag), diag the s complex
// values of diagonal d (row i's is in column i + d, cyclically).
template <class F> static void for_each_diagonal(const double *Md, F &&f)
{
  const unsigned s = G.slots;
  std::vector<double> diag(2 * (size_t)s);
  for (unsigned d = 0; d < s; d++) {
    bool nz = false;
    for (unsigned i = 0; i < s; i++) {
      const size_t src = (size_t)i * s + (i + d) % s;
      diag[2 * i] = Md[2 * src];
      diag[2 * i + 1] = Md[2 * src + 1];
      nz |= diag[2 * i] != 0.0 || diag[2 * i + 1] != 0.0;
    }
    if (nz)
      f(d, diag.data());
  }
}

// Diagonal d, encoded at pt, joins the launch being filled; a launch that is
// full (GemvDiags::MAX) goes to full(dg) and the next one starts.
template <class F>
static void diags_append(GemvDiags &dg, unsigned d, const uint64_t *pt, const he_evk_t rk[], F &&full)
{
  const uint64_t g = d == 0 ? 1 : galois_of_rot(d);
  dg.evk[dg.count] = d == 0 ? nullptr : find_rot_key(rk, d, g)->data;
  dg.pt[dg.count] = pt;
  dg.g[dg.count] = g;
  if (++dg.count == GemvDiags::MAX) {
    full(dg);
    dg.count = 0;
  }
}

// x = a - b, both polys written by queued he_sub ops that nothing else in the
// queue touches (HECTR's xhat - xr and uhat - ur, src/hempc.c:253-256: the
// queue then holds exactly those four ops)?  Then he_gemv leaves them queued
// -- they run with the step's later elementwise ops -- and the inner products
// form the difference where they read x (gemv_inner_kernel), which saves the
// step a launch.  src: a0, b0, a1, b1.
static bool ew_lazy_sub(const he_ct_t *y, const he_ct_t *x, const uint64_t *src[4])
{
  static const bool on = env_u("GPQHE_DEFER_SUB", 1);
  if (!g_pew.count || !on)
    return false;
  const uint64_t *o0 = limb(x, 0, 0), *o1 = limb(x, 1, 0);
  const EwOp *m0 = nullptr, *m1 = nullptr;
  for (unsigned j = 0; j < g_pew.count; j++) {
    const EwOp &o = g_pew.op[j];
    if (o.kind != EW_SUB || o.lvl < x->nlimbs)
      return false;
    for (unsigned i = 0; i < g_pew.count; i++)  // no op reads what a queued op writes
      if (g_pew.op[i].a == o.out || g_pew.op[i].b == o.out)
        return false;
    if (o.out == o0) {
      if (m0)
        return false;
      m0 = &o;
    } else if (o.out == o1) {
      if (m1)
        return false;
      m1 = &o;
    }
  }
  if (!m0 || !m1)
    return false;
  // the gemv then runs before these ops (flush_gemvs precedes the queued
  // program): its output must not be an operand or output of any of them
  // (in-place he_gemv, or y = an operand of a sub), nor of the pending gemvs'
  // formed differences
  const uint64_t *ylo = y->data, *yhi = y->data + 2 * pstride(y);
  auto hits = [&](const uint64_t *p, unsigned lvl) { return p && p < yhi && p + ((size_t)lvl << G.logn) > ylo; };
  for (unsigned j = 0; j < g_pew.count; j++) {
    const EwOp &o = g_pew.op[j];
    if (hits(o.out, o.lvl) || hits(o.a, o.lvl) || hits(o.b, o.lvl) || hits(o.s, o.lvl))
      return false;
  }
  src[0] = m0->a;
  src[1] = m0->b;
  src[2] = m1->a;
  src[3] = m1->b;
  return true;
}

// Runs the queued gemvs: ModUp of every input in one pass (k_modup_ntt: one
// fused launch at n <= 2^12), the inner products per gemv, and one ModDown
// for each pair of outputs.  The arithmetic per
// ciphertext is that of the unbatched sequence, so the results are too.
static void flush_gemvs()
{
  std::vector<PendGemv> q;
  q.swap(g_pgemv);
  if (q.empty())
    return;
  g_sd.valid = false;  // (its outputs may take blocks the replayed tail read: SpecDcd)
  const unsigned k = (unsigned)q.size(), lvl = q[0].lvl;
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n;
  // ModUp of the inputs without precomputed digits (SpecModup), in one pass
  const size_t dstride = (size_t)ndig * nm * n;
  unsigned miss = 0;
  for (unsigned i = 0; i < k; i++)
    miss += !q[i].dspec;
  Ws D((size_t)miss * dstride), acc((size_t)k * 2 * nm * n);
  std::vector<const uint64_t *> Dp(k);
  XPtrs x1{};
  for (unsigned i = 0, m = 0; i < k; i++) {
    if (q[i].dspec) {
      Dp[i] = q[i].dspec;
    } else {
      x1.p[m] = q[i].x1;
      Dp[i] = D.p + m++ * dstride;
    }
    prov_forget(q[i].y, q[i].ypstride);
  }
  if (miss)
    k_modup_ntt(D.p, x1, miss, dstride, lvl);
  // every gemv with one launch's worth of diagonals: all in one launch
  bool one = k <= GemvJobs::MAX;
  for (unsigned i = 0; i < k; i++)
    one &= q[i].dgs.size() == 1;
  if (one) {
    if (!g_spec_early && spec_attach(true, lvl))
      g_spec_early = true;
    GemvJobs jobs;
    for (unsigned i = 0; i < k; i++) {
      jobs.j[i] = GemvJob{acc.p + (size_t)i * 2 * nm * n, Dp[i], q[i].x0, q[i].x1, q[i].dgs[0], 0};
      if (q[i].lb0) {  // the queued difference, formed in the kernel
        jobs.j[i].x0 = q[i].la0;
        jobs.j[i].x1 = q[i].la1;
        jobs.j[i].y0 = q[i].lb0;
        jobs.j[i].y1 = q[i].lb1;
      }
    }
    gemv_run_jobs(jobs, k, lvl, acc.p, q[0].ypstride, q[0].y, q[k - 1].y);
    return;
  }
  for (unsigned i = 0; i < k; i++)
    if (q[i].lb0)
      flush_ew();  // the queued differences, materialised first
  for (unsigned i = 0; i < k; i++) {
    uint64_t *a = acc.p + (size_t)i * 2 * nm * n;
    bool started = false;
    for (const GemvDiags &dg : q[i].dgs) {
      k_gemv_inner(a, Dp[i], q[i].x0, q[i].x1, lvl, dg, started);
      started = true;
    }
    if (!started)  // all-zero matrix
      HIP_CHECK(hipMemsetAsync(a, 0, 2 * nm * n * 8, G.stream));
  }
  // (nothing is attached to these launches: spec_attach runs only above)
  k_moddown(q[0].y, q[0].ypstride, acc.p, nm * n, 2 * k, lvl, 1, k == 1 ? nullptr : q[1].y);
}

// Unqueued he_gemv for matrices whose diagonals may overflow the cache: a
// launch that refers to cached diagonals runs before the cache is cleared.
static void gemv_now(he_ct_t *y, const double *Md, const he_ct_t *x, const he_evk_t rk[], unsigned lvl)
{
  prov_forget(y->data, pstride(y));
  const unsigned s = G.slots, nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n;
  Ws D((size_t)ndig * nm * n), acc(2 * nm * n);
  hoist_modup(D.p, x, lvl);
  GemvDiags dg{};
  bool started = false;
  auto launch = [&](const GemvDiags &l) {
    k_gemv_inner(acc.p, D.p, limb(x, 0, 0), limb(x, 1, 0), lvl, l, started);
    started = true;
  };
  for_each_diagonal(Md, [&](unsigned d, const double *diag) {
    if (diag_cache_full(lvl) && dg.count) {  // the cache may be cleared below: launch what refers to it first
      launch(dg);
      dg.count = 0;
    }
    diags_append(dg, d, diag_pt(diag, s, lvl), rk, launch);
  });
  if (dg.count)
    launch(dg);
  if (!started)  // all-zero matrix
    HIP_CHECK(hipMemsetAsync(acc.p, 0, 2 * nm * n * 8, G.stream));
  k_moddown(y->data, pstride(y), acc.p, nm * n, 2, lvl, 1);
  gemv_set_meta(y, x, lvl);
}

// n >= 2^13: the windowed batch path on one ciphertext, unqueued.  It takes
// no part in the small-N step's queues and speculation (check_ctx drops
// any pending speculative ModUp): those serve HECTR's own ring (n <= 2^12),
// where a step is a handful of small launches; at 2^13 and above a gemv is
// tens of microseconds of device work on its own.  (In place, y == x, is
// fine: every input word is read before the ModDown writes y.)
static bool gemv_folded(he_ct_t *y, const double *Md, const he_ct_t *x, const he_evk_t rk[], unsigned lvl, bool lazy)
{
  if (!gemv_win_on(lvl) || !gemv_fold_fits(Md, lvl, rk))
    return false;
  if (lazy)
    flush_ew();
  check_ctx();
  prov_forget(y->data, pstride(y));
  const FoldEntry &f = gemv_fold(Md, lvl, rk);
  FoldUse use(f.K);
  k_gemv_batch_ex(y->data, 0, pstride(y), x->data, 0, pstride(x), 1, lvl, f.K, f.d.data(), (unsigned)f.d.size(), 1);
  gemv_set_meta(y, x, lvl);
  return true;
}

// A matrix not among g_dc.mats: its non-zero diagonals, their encodings looked
// up or made, in as few launches as possible (GemvDiags::MAX each, evk from
// rk), kept for the next he_gemv of the same matrix.
static const GemvMat &gemv_mat_new(const double *Md, unsigned lvl, const he_evk_t rk[])
{
  const unsigned s = G.slots;
  // diagonals not cached yet (host-FFT sizes) are encoded together after the
  // walk: one upload and one lift + NTT launch for all of them
  const bool batch_enc = s < gpu_ecd_min();
  const size_t n = G.n, per = (size_t)(lvl + G.K) << G.logn;
  std::vector<std::string> keys;  // of every non-zero diagonal
  std::vector<size_t> fresh;      // the ones to encode (indices in keys)
  std::vector<int64_t> newcoef;
  std::vector<unsigned> rots;
  for_each_diagonal(Md, [&](unsigned d, const double *diag) {
    keys.push_back(diag_key(diag, s, lvl));
    rots.push_back(d);
    if (g_dc.pt.count(keys.back()))
      return;
    if (!batch_enc) {
      diag_pt(diag, s, lvl);
      return;
    }
    g_dc.pt[keys.back()] = nullptr;  // (a repeat of this diagonal finds it; set below)
    newcoef.resize((fresh.size() + 1) * n);
    hm_encode_coeffs(newcoef.data() + fresh.size() * n, diag, s, n, (double)G.q[lvl - 1]);
    fresh.push_back(keys.size() - 1);
  });
  if (!fresh.empty()) {
    const unsigned cnt = (unsigned)fresh.size();
    uint64_t *slab = (uint64_t *)pool_alloc((size_t)cnt * per * 8);
    g_dc.blocks.push_back(slab);
    Ws dcoef(newcoef.size());
    upload(dcoef.p, newcoef.data(), newcoef.size() * 8);
    unsigned mods[GPQHE_MAXMOD];
    const unsigned nm = basis_qp(lvl, mods);
    k_lift_ntt(limbset(slab, mods, nm, cnt, per), (const int64_t *)dcoef.p);
    for (unsigned i = 0; i < cnt; i++)
      g_dc.pt[keys[fresh[i]]] = slab + (size_t)i * per;
    g_dc.bytes += (size_t)cnt * per * 8;
  }
  GemvMat gm{s, lvl, g_dc.gen, std::vector<double>(Md, Md + 2 * (size_t)s * s), {}, rots};
  GemvDiags dg{};
  auto push = [&](const GemvDiags &l) { gm.dgs.push_back(l); };
  for (size_t r = 0; r < rots.size(); r++)
    diags_append(dg, rots[r], g_dc.pt[keys[r]], rk, push);
  if (dg.count)
    push(dg);
  if (g_dc.mats.size() >= 8)
    g_dc.mats.erase(g_dc.mats.begin());
  g_dc.mats.push_back(std::move(gm));
  return g_dc.mats.back();
}

// The queued path: behind the pending gemv when the two are independent, at
// one level, with one output layout (the caller saw that no diagonal encode
// can clear the cache the pending one refers to).  lz: x's queued difference
// (ew_lazy_sub), or null.
static void gemv_queued(he_ct_t *y, const double *Md, const he_ct_t *x, const he_evk_t rk[], unsigned lvl,
                        const uint64_t *const *lz)
{
  static const bool defer = env_u("GPQHE_DEFER", 1) && env_u("GPQHE_DEFER_GEMV", 1);
  const unsigned s = G.slots;
  if (!g_pgemv.empty()) {
    const PendGemv &p = g_pgemv.back();
    if (g_pgemv.size() >= 2 || p.lvl != lvl || p.ypstride != pstride(y) || x->data == (void *)p.y ||
        (const void *)y->data == p.xdata || y->data == p.y)
      flush_gemvs();
  }
  PendGemv pg{y->data, pstride(y), limb(x, 0, 0), limb(x, 1, 0), x->data, lvl, {}};
  prov_forget(y->data, pstride(y));
  int pat = -1;  // the pattern recorded for the next step's speculation
  // x's c1: the difference of two fresh encryptions of this step?  Then its
  // ModUp may be precomputed (SpecModup), and the pattern is kept for the
  // next step's speculation.
  auto pv = g_prov.find(pg.x1);
  if (pv != g_prov.end() && pv->second.sub && pv->second.lvl == lvl) {
    const C1Prov &c = pv->second;
    if (g_smu.valid && g_smu.lvl == lvl && g_smu.pk1 == c.pk1)
      for (size_t i = 0; i < g_smu.pats.size(); i++)
        if (g_smu.base + 3 * (uint64_t)g_smu.pats[i].oa == c.sa && g_smu.base + 3 * (uint64_t)g_smu.pats[i].ob == c.sb) {
          const unsigned nmx = lvl + G.K, ndx = (lvl + G.alpha - 1) / G.alpha;
          pg.dspec = g_smu.D + i * ((size_t)ndx * nmx << G.logn);
          break;
        }
    pat = spec_record_pattern(c, lvl);
  }
  if (lz && pg.dspec) {
    pg.la0 = lz[0];
    pg.lb0 = lz[1];
    pg.la1 = lz[2];
    pg.lb1 = lz[3];
  } else if (lz) {
    flush_ew();  // the ModUp reads x1 itself
  }
  const GemvMat *gm = nullptr;
  for (const GemvMat &m : g_dc.mats)
    if (m.s == s && m.lvl == lvl && m.dgen == g_dc.gen && !memcmp(m.M.data(), Md, m.M.size() * 8)) {
      gm = &m;
      break;
    }
  if (gm) {
    size_t r = 0;
    pg.dgs = gm->dgs;
    for (GemvDiags &dg : pg.dgs)
      for (unsigned e = 0; e < dg.count; e++, r++)
        dg.evk[e] = gm->rot[r] ? find_rot_key(rk, gm->rot[r], dg.g[e])->data : nullptr;
  } else {
    pg.dgs = gemv_mat_new(Md, lvl, rk).dgs;
  }
  spec_record_gemv(pat, Md, pg, rk);
  g_pgemv.push_back(std::move(pg));
  if (!defer)
    flush_gemvs();
  gemv_set_meta(y, x, lvl);
}

extern "C" void he_gemv(he_ct_t *y, const gpqhe_complex_t M[], const he_ct_t *x, const he_evk_t rk[])
{
  HPROF("gemv");
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  const double *Md = (const double *)M;
  if (spec_gemv_take(y, Md, x, rk))
    return;
  // x may be a queued difference: left queued when the inner products can
  // form it (ew_lazy_sub, only with x's ModUp digits precomputed), else run now
  const uint64_t *lz[4];
  const bool lazy = ew_lazy_sub(y, x, lz);
  if (!lazy)
    flush_ew();
  if (!g_pecd.empty() || !g_penc.empty())
    flush_pending();  // x may be a queued encryption
  const unsigned lvl = x->nlimbs;
  if (lvl < 2)
    gpqhe_die("he_gemv: input at the lowest level");
  if (gemv_folded(y, Md, x, rk, lvl, lazy))
    return;
  if (diag_cache_full(lvl, G.slots)) {
    // the diagonal cache may be cleared inside this call: unqueued form
    flush_gemvs();
    flush_ew();
    gemv_now(y, Md, x, rk, lvl);
    return;
  }
  gemv_queued(y, Md, x, rk, lvl, lazy ? lz : nullptr);
}

// ===========================================================================
// he_gemv_bsgs (include/gpqhe_ext.h): the baby-step giant-step form of the
// diagonal method.  With g baby steps and G = ceil(s / g) giant steps,
//   b_i   = rot(x, i)                                  (hoisted: one ModUp)
//   u_j   = sum_i P_j,i b_i,  P_j,i = ecd(roll(diag_{jg+i}, jg)) over the q limbs
//   y     = rescale(sum_j rot(u_j, jg))
// every step the exact arithmetic of he_rot / he_mul_pt / he_add / he_rescale,
// so the residues are those of that composition.  Kernels: bsgs.hip.
// Non-queued: it takes no part in the small-N step's queues and speculation,
// and he_gemv takes none of this code.
//
// The encoded diagonals live in a plan cache (PlanCache), keyed by a header of
// integers and the bytes of the matrices, least recently used first out,
// bounded by diag_cache_cap().  There are three instances, each bounded on its
// own, so what one kind of call finds does not depend on calls of another:
//   g_bsgs   (s, lvl, g), M                    he_gemv_bsgs, he_gemv_bsgs_batch
//   g_bsgs2  (s, lvl, g), the ordered (Ma, Mb) he_gemv2_bsgs_batch, he_hempc_step_batch
//   g_rows   (s, lvl, rows, sl, nmat), the leading rows of (Ma, Mb)
//                                              the row-folded and packed forms
// An entry owns its device blocks; nothing outside this section keeps a pointer
// into one across calls, and a call holds its entry only until it returns
// (nothing inside a call evicts).
// ===========================================================================
// One operand's host lists.
struct BsgsOp {
  std::vector<unsigned> ds;     // the non-zero diagonals, ascending: pts order
  std::vector<unsigned> baby;   // the baby rotations they use, ascending: slot order of B
  std::vector<unsigned> giant;  // the giant steps they use, ascending: row order of tab
  std::vector<int> tab;         // [giant][baby] -> index into the operand's diagonals, -1: none
};

// The plan of y = Ma xa (+ Mb xb): operand b is empty for the single product.
struct BsgsPlan {
  std::vector<unsigned> hdr;    // the key: the header and the matrices it was made
  std::vector<double> Ma, Mb;   // from (compared in place on a lookup)
  BsgsOp a, b;
  std::vector<unsigned> giant;  // the union of their giant steps, ascending: row order of tab and U
  std::vector<int> tab;         // [giant][baby slots of a | baby slots of b] -> index into pts, -1: none
  uint64_t *pts = nullptr;      // [a.ds.size() + b.ds.size()][lvl][n]: a's diagonals, then b's
  int *tab_dev = nullptr;
  size_t bytes = 0;
  unsigned ndiag() const { return (unsigned)(a.ds.size() + b.ds.size()); }
};

// What keeps a plan that is not in the cache alive for one call.
struct PlanHold {
  BsgsPlan tmp;
  std::unique_ptr<Ws> pts, tab;
};

struct PlanCache {
  std::list<BsgsPlan> plans;  // most recently used first (a list: a running call's entry stays where it is)
  size_t bytes = 0;

  void clear()
  {
    for (BsgsPlan &p : plans) {
      pool_free(p.pts);
      pool_free(p.tab_dev);
    }
    plans.clear();
    bytes = 0;
  }

  // The plan of (hdr, Ma, Mb) at level lvl, mwords doubles per matrix (Mb null:
  // one matrix): cached, or (a set larger than the cache, or no diagonal at
  // all) in the holder.  plan(p) fills p.a and p.b on the host, encode(p, pts)
  // writes their diagonals' limbs.  One compare of the matrices per call; every
  // eviction happens here, before the call's first launch.
  template <class Plan, class Encode>
  const BsgsPlan *get(PlanHold &h, const std::vector<unsigned> &hdr, unsigned lvl, const double *Ma, const double *Mb,
                      size_t mwords, Plan plan, Encode encode)
  {
    for (auto it = plans.begin(); it != plans.end(); ++it)
      if (it->hdr == hdr && !memcmp(it->Ma.data(), Ma, mwords * 8) && (!Mb || !memcmp(it->Mb.data(), Mb, mwords * 8))) {
        plans.splice(plans.begin(), plans, it);
        return &plans.front();
      }
    BsgsPlan &tmp = h.tmp;
    plan(tmp);
    const BsgsOp &a = tmp.a, &b = tmp.b;
    if (!tmp.ndiag())
      return &tmp;  // no diagonal: no blocks
    std::set_union(a.giant.begin(), a.giant.end(), b.giant.begin(), b.giant.end(), std::back_inserter(tmp.giant));
    const size_t na = a.baby.size(), nb = b.baby.size(), gs = na + nb;
    tmp.tab.assign(tmp.giant.size() * gs, -1);
    for (size_t r = 0, ja = 0, jb = 0; r < tmp.giant.size(); r++) {
      if (ja < a.giant.size() && a.giant[ja] == tmp.giant[r]) {
        for (size_t i = 0; i < na; i++)
          tmp.tab[r * gs + i] = a.tab[ja * na + i];
        ja++;
      }
      if (jb < b.giant.size() && b.giant[jb] == tmp.giant[r]) {
        for (size_t i = 0; i < nb; i++)
          if (b.tab[jb * nb + i] >= 0)
            tmp.tab[r * gs + na + i] = (int)a.ds.size() + b.tab[jb * nb + i];
        jb++;
      }
    }
    const size_t pw = (size_t)lvl * G.n, tabw = (tmp.tab.size() * sizeof(int) + 7) / 8;
    tmp.bytes = tmp.ndiag() * pw * 8;
    if (tmp.bytes > diag_cache_cap()) {
      h.pts.reset(new Ws(tmp.ndiag() * pw));
      h.tab.reset(new Ws(tabw));
      tmp.pts = h.pts->p;
      tmp.tab_dev = (int *)h.tab->p;
    } else {
      while (!plans.empty() && bytes + tmp.bytes > diag_cache_cap()) {
        pool_free(plans.back().pts);
        pool_free(plans.back().tab_dev);
        bytes -= plans.back().bytes;
        plans.pop_back();
      }
      tmp.pts = (uint64_t *)pool_alloc(tmp.bytes);
      tmp.tab_dev = (int *)pool_alloc(tabw * 8);
    }
    encode(tmp, tmp.pts);
    upload(tmp.tab_dev, tmp.tab.data(), tmp.tab.size() * sizeof(int));
    if (h.pts)
      return &tmp;
    tmp.hdr = hdr;  // the owned copies: made on a miss only
    tmp.Ma.assign(Ma, Ma + mwords);
    if (Mb)
      tmp.Mb.assign(Mb, Mb + mwords);
    bytes += tmp.bytes;
    plans.push_front(std::move(tmp));
    return &plans.front();
  }
};
static PlanCache g_bsgs, g_bsgs2, g_rows;

static void plan_caches_clear()
{
  for (PlanCache *c : {&g_bsgs, &g_bsgs2, &g_rows})
    c->clear();
}

static unsigned bsgs_default_g()
{
  unsigned lg = 0;
  while ((1u << lg) < G.slots)
    lg++;
  return 1u << ((lg + 1) / 2);
}

// Which diagonals, baby rotations and giant steps M uses (host only).
static void bsgs_plan(BsgsOp &p, const double *Md, unsigned g)
{
  const unsigned s = G.slots, ng = (s + g - 1) / g;
  std::vector<char> ub(g, 0), uj(ng, 0);
  for_each_diagonal(Md, [&](unsigned d, const double *) {
    p.ds.push_back(d);
    ub[d % g] = 1;
    uj[d / g] = 1;
  });
  std::vector<int> bslot(g, -1), jrow(ng, -1);
  for (unsigned i = 0; i < g; i++)
    if (ub[i]) {
      bslot[i] = (int)p.baby.size();
      p.baby.push_back(i);
    }
  for (unsigned j = 0; j < ng; j++)
    if (uj[j]) {
      jrow[j] = (int)p.giant.size();
      p.giant.push_back(j);
    }
  p.tab.assign(p.giant.size() * p.baby.size(), -1);
  for (size_t e = 0; e < p.ds.size(); e++)
    p.tab[(size_t)jrow[p.ds[e] / g] * p.baby.size() + bslot[p.ds[e] % g]] = (int)e;
}

// pts <- P_j,i of every non-zero diagonal d = j g + i, in p.ds order.
static void bsgs_encode(const BsgsOp &p, const double *Md, unsigned lvl, unsigned g, uint64_t *pts)
{
  const unsigned s = G.slots;
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned l = 0; l < lvl; l++)
    mods[l] = l;
  std::vector<double> v(2 * (size_t)s);
  for (size_t e = 0; e < p.ds.size(); e++) {
    const unsigned d = p.ds[e], sh = d / g * g;
    for (unsigned k = 0; k < s; k++) {  // roll(diag_d, j g)[k] = diag_d[k - j g]
      const unsigned i = (k + s - sh) % s;
      const size_t src = (size_t)i * s + (i + d) % s;
      v[2 * k] = Md[2 * src];
      v[2 * k + 1] = Md[2 * src + 1];
    }
    encode_limbs(pts + e * ((size_t)lvl << G.logn), v.data(), s, (double)G.q[lvl - 1], mods, lvl);
  }
}

static void bsgs_ks_launch(const std::vector<BsgsKsJob> &jobs, unsigned lvl, bool shared_d)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t bytes = jobs.size() * sizeof(BsgsKsJob);
  Ws jd((bytes + 7) / 8);
  upload(jd.p, jobs.data(), bytes);
  // per job: the key, c0, both accumulators; the digits once per job or per launch
  const double cnt = (double)jobs.size();
  k_bsgs_ks((const BsgsKsJob *)jd.p, (unsigned)jobs.size(), lvl,
            8.0 * G.n * (cnt * (2.0 * ndig * nm + lvl + 2.0 * nm) + (shared_d ? 1.0 : cnt) * ndig * nm));
}

extern "C" unsigned int he_gemv_bsgs_default_g(void)
{
  if (!G.init)
    gpqhe_die("context not initialised (hectx_init)");
  return bsgs_default_g();
}

extern "C" void he_genrk_bsgs(he_evk_t rk[], const poly_mpi_t *sk, unsigned int g)
{
  check_ctx();
  const unsigned s = G.slots;
  if (!g)
    g = bsgs_default_g();
  if (g > s)
    gpqhe_die("he_genrk_bsgs: g = %u > slots = %u", g, s);
  gen_rot_keys(rk, sk, [g](unsigned r) { return r < g || r % g == 0; });
}

// ---------------------------------------------------------------------------
// The stages of a BSGS product, shared by he_gemv_bsgs and the batch products
// (include/gpqhe_ext_batch.h).  A stage writes its slots (baby slots, rotated
// giant steps) `stride` words apart: 2 lvl n for the single call's packed
// buffers, cnt 2 lvl n for a chunk's slot-major ones.
// ---------------------------------------------------------------------------
// The plan of one matrix: (M, lvl, g) in g_bsgs.
static const BsgsPlan *bsgs_plan_get(PlanHold &h, const double *Md, unsigned lvl, unsigned g)
{
  const unsigned s = G.slots;
  return g_bsgs.get(
    h, {s, lvl, g}, lvl, Md, nullptr, 2 * (size_t)s * s, [&](BsgsPlan &p) { bsgs_plan(p.a, Md, g); },
    [&](const BsgsPlan &p, uint64_t *pts) { bsgs_encode(p.a, Md, lvl, g, pts); });
}

// Every rotation a plan uses and its key (found before anything is launched).
struct BsgsKeys {
  unsigned nbs = 0, nj = 0;      // baby slots, giant steps
  unsigned has0 = 0, nbr = 0;    // slot 0 is x itself; rotated baby slots
  unsigned hasj0 = 0, njr = 0;   // giant step 0 is not rotated; rotated giant steps
  std::vector<unsigned> brot, grot;
  std::vector<const he_evk_t *> bkey, gkey;
  std::vector<uint64_t> bgal, ggal;
};

// The keys of the baby rotations `baby` and of the giant steps `giant` (step j
// is the rotation j g); either list may be empty.
static BsgsKeys bsgs_find_keys(const std::vector<unsigned> &baby, const std::vector<unsigned> &giant, unsigned g,
                               const he_evk_t rk[])
{
  BsgsKeys k;
  k.nbs = (unsigned)baby.size();
  k.nj = (unsigned)giant.size();
  k.has0 = k.nbs && baby[0] == 0;
  k.nbr = k.nbs - k.has0;
  k.hasj0 = k.nj && giant[0] == 0;
  k.njr = k.nj - k.hasj0;
  k.brot.resize(k.nbr);
  k.bkey.resize(k.nbr);
  k.bgal.resize(k.nbr);
  k.grot.resize(k.njr);
  k.gkey.resize(k.njr);
  k.ggal.resize(k.njr);
  for (unsigned r = 0; r < k.nbr; r++) {
    k.brot[r] = baby[k.has0 + r];
    k.bgal[r] = galois_of_rot(k.brot[r]);
    k.bkey[r] = find_rot_key(rk, k.brot[r], k.bgal[r]);
  }
  for (unsigned r = 0; r < k.njr; r++) {
    k.grot[r] = giant[k.hasj0 + r] * g;
    k.ggal[r] = galois_of_rot(k.grot[r]);
    k.gkey[r] = find_rot_key(rk, k.grot[r], k.ggal[r]);
  }
  return k;
}

// ModDown by P of cnt rotations' accumulators into slots `stride` words
// apart: one launch where the slots are packed, else one per rotation.
static void bsgs_down(uint64_t *out, size_t stride, uint64_t *acc, unsigned cnt, unsigned lvl)
{
  const unsigned nm = lvl + G.K;
  const size_t n = G.n, pw = (size_t)lvl * n, accw = 2 * (size_t)nm * n;
  if (stride == 2 * pw || cnt == 1) {
    k_moddown(out, pw, acc, (size_t)nm * n, 2 * cnt, lvl, 0);
    return;
  }
  for (unsigned t = 0; t < cnt; t++)
    k_moddown(out + t * stride, pw, acc + t * accw, (size_t)nm * n, 2, lvl, 0);
}

// Baby stage of one ciphertext: slot i of B <- rot(x, baby[i]), slot 0 x
// itself where diagonals use it.  One hoisted ModUp, rotations in chunks whose
// accumulators fit the budget.
static void bsgs_baby(uint64_t *B, size_t stride, const he_ct_t *x, const BsgsKeys &k, unsigned lvl, size_t budget)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n, pw = (size_t)lvl * n, accw = 2 * (size_t)nm * n, dw = (size_t)ndig * nm * n;
  if (k.has0 && B != x->data)  // (he_hempc_step_batch forms x in slot 0)
    for (unsigned p = 0; p < 2; p++)
      HIP_CHECK(hipMemcpyAsync(B + p * pw, limb(x, p, 0), pw * 8, hipMemcpyDeviceToDevice, G.stream));
  if (!k.nbr)
    return;
  const unsigned cb = (unsigned)std::min<size_t>(k.nbr, std::max<size_t>(1, budget / accw));
  Ws D(dw), acc((size_t)cb * accw);
  hoist_modup(D.p, x, lvl);
  for (unsigned r0 = 0; r0 < k.nbr; r0 += cb) {
    const unsigned cnt = std::min(cb, k.nbr - r0);
    std::vector<BsgsKsJob> jobs(cnt);
    for (unsigned t = 0; t < cnt; t++)
      jobs[t] = BsgsKsJob{D.p, limb(x, 0, 0), k.bkey[r0 + t]->data, acc.p + t * accw, k.bgal[r0 + t]};
    bsgs_ks_launch(jobs, lvl, true);
    bsgs_down(B + (size_t)(k.has0 + r0) * stride, stride, acc.p, cnt, lvl);
  }
}

// Words of key-switch workspace one giant step holds (its ModUp digits and
// accumulators), and how many fit the budget next to `extra` words each.
static unsigned bsgs_giant_chunk(const BsgsKeys &k, unsigned lvl, size_t budget, size_t extra)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n, accw = 2 * (size_t)nm * n, dw = (size_t)ndig * nm * n;
  return (unsigned)std::min<size_t>(k.njr, std::max<size_t>(1, budget / (dw + accw + extra)));
}

// Giant stage of one ciphertext, rotated giant steps [r0, r0 + cnt): u of step
// r at U + (hasj0 + r) u_stride, its rotation by giant[r] g into R + (r - r0)
// r_stride.  Dg [cnt][ndig][nm][n] and acc [cnt][2][nm][n] are workspace.
static void bsgs_giant(uint64_t *R, size_t r_stride, const uint64_t *U, size_t u_stride, const BsgsKeys &k,
                       unsigned r0, unsigned cnt, unsigned lvl, uint64_t *Dg, uint64_t *acc)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n, pw = (size_t)lvl * n, accw = 2 * (size_t)nm * n, dw = (size_t)ndig * nm * n;
  const uint64_t *u = U + (size_t)(k.hasj0 + r0) * u_stride;
  for (unsigned b0 = 0; b0 < cnt; b0 += XPtrs::MAX) {
    const unsigned c = std::min(XPtrs::MAX, cnt - b0);
    XPtrs x1{};
    for (unsigned t = 0; t < c; t++)
      x1.p[t] = u + (size_t)(b0 + t) * u_stride + pw;
    k_modup_ntt(Dg + b0 * dw, x1, c, dw, lvl);
  }
  std::vector<BsgsKsJob> jobs(cnt);
  for (unsigned t = 0; t < cnt; t++)
    jobs[t] = BsgsKsJob{Dg + t * dw, u + (size_t)t * u_stride, k.gkey[r0 + t]->data, acc + t * accw, k.ggal[r0 + t]};
  bsgs_ks_launch(jobs, lvl, false);
  bsgs_down(R, r_stride, acc, cnt, lvl);
}

static size_t bsgs_budget()
{
  return ((size_t)env_u("GPQHE_WS_MIB", 8192) << 20) / 8;  // words per key-switch workspace
}

extern "C" void he_gemv_bsgs(he_ct_t *y, const gpqhe_complex_t M[], const he_ct_t *x, const he_evk_t rk[],
                             unsigned int g)
{
  HPROF("gemv_bsgs");
  check_ctx();  // x may be a queued difference or encryption
  const unsigned s = G.slots, lvl = x->nlimbs;
  if (!g)
    g = bsgs_default_g();
  if (g > s)
    gpqhe_die("he_gemv_bsgs: g = %u > slots = %u", g, s);
  if (lvl < 2)
    gpqhe_die("he_gemv_bsgs: input at the lowest level");
  const size_t n = G.n, pw = (size_t)lvl * n;
  const size_t budget = bsgs_budget();

  PlanHold hold;
  const BsgsPlan *plan = bsgs_plan_get(hold, (const double *)M, lvl, g);
  prov_forget(y->data, pstride(y));
  if (plan->a.ds.empty()) {  // all-zero matrix
    for (unsigned p = 0; p < 2; p++)
      HIP_CHECK(hipMemsetAsync(limb(y, p, 0), 0, (size_t)(lvl - 1) * n * 8, G.stream));
    gemv_set_meta(y, x, lvl);
    return;
  }
  const BsgsKeys k = bsgs_find_keys(plan->a.baby, plan->a.giant, g, rk);

  // baby steps: B [nbs][2][lvl][n]
  Ws B((size_t)k.nbs * 2 * pw);
  bsgs_baby(B.p, 2 * pw, x, k, lvl, budget);

  // the plaintext inner sums: U [nj][2][lvl][n]
  Ws U((size_t)k.nj * 2 * pw);
  k_bsgs_inner(U.p, B.p, plan->pts, plan->tab_dev, k.nj, k.nbs, (unsigned)plan->a.ds.size(), lvl);

  // giant steps: each u_j (j >= 1) rotated by j g through its own ModDown,
  // then summed (with u_0) over the q limbs; chunks of cg giant steps
  uint64_t *S = U.p;
  Ws Sw(k.njr ? 2 * pw : 0);
  if (k.njr) {
    const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
    const unsigned cg = bsgs_giant_chunk(k, lvl, budget, 2 * pw);
    Ws Dg((size_t)cg * ndig * nm * n), acc((size_t)cg * 2 * nm * n), R((size_t)cg * 2 * pw);
    const uint64_t *base = k.hasj0 ? U.p : nullptr;
    for (unsigned r0 = 0; r0 < k.njr; r0 += cg) {
      const unsigned cnt = std::min(cg, k.njr - r0);
      bsgs_giant(R.p, 2 * pw, U.p, 2 * pw, k, r0, cnt, lvl, Dg.p, acc.p);
      k_bsgs_sum(Sw.p, base, R.p, cnt, 2 * pw, lvl);
      base = Sw.p;
    }
    S = Sw.p;
  }
  // rescale by q_top into y (every read of x is already on the stream: y may be x)
  k_moddown(y->data, pstride(y), S, pw, 2, lvl, 2);
  gemv_set_meta(y, x, lvl);
}

// ===========================================================================
// Batched entry points
// ===========================================================================
static unsigned g_mul_streams = 2;  // he_mul_rescale_batch: sub-chunks on their own streams (1 or 2)

extern "C" void gpqhe_set_streams(unsigned int n)
{
  if (n != 1 && n != 2)
    gpqhe_die("gpqhe_set_streams: 1 or 2, not %u", n);
  g_mul_streams = n;
}

extern "C" void he_mul_rescale_batch(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t count,
                                     unsigned int nlimbs, const he_evk_t *rlk)
{
  check_ctx();
  const unsigned lvl = nlimbs;
  if (lvl < 2 || lvl > G.L)
    gpqhe_die("he_mul_rescale_batch: bad level %u", lvl);
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n;
  // workspace limbs per pair: the split key switch holds y, T1, the dropped
  // slots and conv; the streaming one d2, y, T1 and both accumulators
  const size_t per_ct = (k_mul_split_ok(lvl) ? (size_t)(lvl + ndig * nm + 2 * (G.K + 1) + 2 * lvl)
                                              : (size_t)(2 * lvl + 2 * lvl + ndig * nm + 2 * nm + 2 * lvl)) * n * 8;
  // workspace per chunk (GPQHE_WS_MIB, default 8 GiB: 292 pairs at N=2^16,
  // L=8, dnum=2 on the split key switch, so the bench's 256 pairs run as one
  // chunk: 39.7k vs 38.4k ct-mult/s for two chunks of 128, same box).  Bigger
  // chunks fill the GPU better and amortize the key tiles over more pairs;
  // 288 GB of HBM leave room.
  static const size_t budget = (size_t)env_u("GPQHE_WS_MIB", 8192) << 20;
  size_t chunk = std::max<size_t>(1, budget / per_ct);
  chunk = std::min<size_t>(chunk, 65535 / (ndig * nm));
  if (const char *e = getenv("GPQHE_CHUNK"))  // test hook: force several chunks on a small batch
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, strtoul(e, nullptr, 0)));
  // equal chunks: a short last chunk runs at a fraction of the GPU's width
  const size_t nchunks = (count + chunk - 1) / chunk;
  if (nchunks)
    chunk = (count + nchunks - 1) / nchunks;
  const size_t in_stride = 2 * lvl * n, out_stride = 2 * (size_t)(lvl - 1) * n;
  // Two sub-chunks on two streams, the second started once the first's
  // d2_rows has run, so one's VALU-bound column kernels overlap the other's
  // HBM-bound kernels on the same CUs (same box: 42.1k -> 42.7k ct-mult/s,
  // 60-bit 32.3k -> 32.7k, config 5 7.87k -> 7.98k; three or four streams
  // and four or more sub-chunks were slower).  Only without aliasing: a
  // sub-chunk's output must not overlap the other's inputs.
  const unsigned nsub = g_mul_streams;
  const uint64_t *oend = out + count * out_stride, *aend = a + count * in_stride, *bend = b + count * in_stride;
  const bool alias = (out < aend && a < oend) || (out < bend && b < oend);
  const bool split2 = count >= 2 && nchunks == 1 && !alias && k_mul_split_ok(lvl) && rlk->reserved &&
                      rlk->dnum == G.dnum;
  const uint64_t *evkm = (const uint64_t *)(uintptr_t)rlk->reserved;
  // (K pipelined sub-chunks with the HBM-bound stages on one stream and the
  // VALU-bound ones on the other, with or without a CU mask on the second:
  // DESIGN 5b, profiles/r5_ab_pipe.txt and r5_ab_cumask.txt, code at 7e2495a)
  if (split2 && nsub == 2 && !g_s2.s) {
    HIP_CHECK(hipStreamCreateWithFlags(&g_s2.s, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&g_s2.fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&g_s2.d2, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&g_s2.join, hipEventDisableTiming));
  }
  hipStream_t s2 = g_s2.s;
  hipEvent_t ev_fork = g_s2.fork, ev_d2 = g_s2.d2, ev_join = g_s2.join;
  if (nsub == 2 && split2) {
    const unsigned c1 = (unsigned)(count / 2), c2 = (unsigned)(count - c1);
    // both workspaces come from the engine stream's pool before the fork and
    // go back to it after the join
    Ws w1(k_mul_split_ws_words(c1, lvl, true)), w2(k_mul_split_ws_words(c2, lvl, true));
    HIP_CHECK(hipEventRecord(ev_fork, G.stream));
    HIP_CHECK(hipStreamWaitEvent(s2, ev_fork, 0));
    // the second sub-chunk starts once the first's d2_rows has run (where it
    // starts -- at once, after d2_rows or after ks_cols -- was within +-1 %
    // on two boxes, profiles/r4_ab_split_shift.txt)
    k_mul_relin_split(out, (lvl - 1) * n, a, b, in_stride, lvl * n, evkm, c1, lvl, true, w1.p, 0, 1);
    HIP_CHECK(hipEventRecord(ev_d2, G.stream));
    k_mul_relin_split(out, (lvl - 1) * n, a, b, in_stride, lvl * n, evkm, c1, lvl, true, w1.p, 1, 5);
    HIP_CHECK(hipStreamWaitEvent(s2, ev_d2, 0));
    const hipStream_t eng = G.stream;
    G.stream = s2;
    k_mul_relin_split(out + c1 * out_stride, (lvl - 1) * n, a + c1 * in_stride, b + c1 * in_stride, in_stride,
                      lvl * n, evkm, c2, lvl, true, w2.p);
    G.stream = eng;
    HIP_CHECK(hipEventRecord(ev_join, s2));
    HIP_CHECK(hipStreamWaitEvent(G.stream, ev_join, 0));
    return;
  }
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const unsigned cnt = (unsigned)std::min(chunk, count - c0);
    mul_chunk(out + c0 * out_stride, (lvl - 1) * n, a + c0 * in_stride, b + c0 * in_stride, in_stride, lvl * n, cnt,
              lvl, rlk, true);
  }
}

// ---------------------------------------------------------------------------
// he_gemv / he_rot on the windowed path (gemv_win.hip) for n >= 2^13.  The
// rotation keys are folded with their diagonals once and cached: HECTR passes
// the same gain matrices every control step (src/hempc.c:232-238), the bench
// the same matrix every step.  A change of a key (generation, import, free)
// bumps g_key_gen: entries of an older generation never match again and are
// released at the next insert (or when the pool runs out of memory).
// A matrix whose folded set would exceed the cap (GPQHE_FOLD_MIB, 16 GiB:
// (2 ndig nm + lvl) n words per non-zero diagonal, ~30 GB for a dense
// 1024-slot matrix at N=2^16, L=8) takes the per-ciphertext path, whose
// diagonal cache is bounded and streams.
// ---------------------------------------------------------------------------
static size_t fold_cap()
{
  static const size_t cap = (size_t)env_u("GPQHE_FOLD_MIB", 16384) << 20;
  return cap;
}

// Two lists.  g_folds: the matrices of he_gemv, newest first, at most eight
// entries and fold_cap() bytes (a 16-slot gemv at N=2^16, L=8 folds to 480
// MB).  g_rfolds: single rotation keys, one entry per (key array, key
// generation, level, rotation), most recently used first, at most fold_cap()
// bytes -- every windowed rotation looks its key up here (rotkey_fold): he_rot,
// he_rot_batch and the BSGS, rows, packed and encrypted-gain products, whose
// 30 rotations a call would turn eight entries over.  Each list has
// fold_cap() to itself.  Entries of an older key generation never match and
// leave at the list's next insert; a caller holds an entry only while the
// launches that read it are issued (FoldUse).
// (lists: a caller's reference to its entry survives the eviction of others)
static std::list<FoldEntry> g_folds;
static std::list<RotFold> g_rfolds;

// Releases the entries drop() names; the bytes of those that stay.
template <class List, class Drop> static size_t fold_drop(List &l, Drop drop)
{
  size_t kept = 0;
  for (auto it = l.begin(); it != l.end();)
    if (drop(*it)) {
      pool_free(it->K);
      it = l.erase(it);
    } else {
      kept += it->bytes;
      ++it;
    }
  return kept;
}

// Room for an entry of `bytes` in a list of at most max_entries: the entries
// folded with keys that changed since go, then the list's last ones (the
// oldest of g_folds, the least recently used of g_rfolds).
template <class List> static void fold_make_room(List &l, size_t bytes, size_t max_entries)
{
  size_t total = bytes + fold_drop(l, [](const auto &f) { return f.gen != g_key_gen; });
  while (!l.empty() && (l.size() >= max_entries || total > fold_cap())) {
    total -= l.back().bytes;
    pool_free(l.back().K);
    l.pop_back();
  }
}

static void fold_cache_clear()
{
  fold_drop(g_folds, [](const FoldEntry &) { return true; });
  fold_drop(g_rfolds, [](const RotFold &) { return true; });
}

// out of memory: every set no running call reads goes back to the pool
static void fold_cache_trim()
{
  fold_drop(g_folds, [](const FoldEntry &f) { return f.K != g_fold_inuse; });
  fold_drop(g_rfolds, [](const RotFold &f) { return f.K != g_fold_inuse; });
}

static bool gemv_win_on(unsigned lvl)
{
  static const bool on = env_u("GPQHE_GEMV_WIN", 1) != 0;
  return on && k_gemv_win_ok(lvl);
}

static const FoldEntry *fold_find(const double *Md, unsigned lvl, const he_evk_t rk[])
{
  const unsigned s = G.slots;
  const size_t mwords = 2 * (size_t)s * s;
  for (const FoldEntry &f : g_folds)
    if (f.s == s && f.lvl == lvl && f.gen == g_key_gen && f.rk == rk &&
        !memcmp(f.M.data(), Md, mwords * 8))
      return &f;
  return nullptr;
}

// Would M's folded set (plus the encoded diagonals it is folded from) fit the
// cap?  Cached sets always do.
static bool gemv_fold_fits(const double *Md, unsigned lvl, const he_evk_t rk[])
{
  if (fold_find(Md, lvl, rk))
    return true;
  size_t E = 0;
  for_each_diagonal(Md, [&](unsigned, const double *) { E++; });
  const size_t pts = E * (((size_t)lvl + G.K) << G.logn) * 8;
  return k_gemv_fold_words((unsigned)E, lvl) * 8 + pts <= fold_cap();
}

// The non-zero diagonals of M, encoded at scale q_{lvl-1} over basis_qp(lvl),
// folded with their rotation keys (the caller checked gemv_fold_fits).
static const FoldEntry &gemv_fold(const double *Md, unsigned lvl, const he_evk_t rk[])
{
  if (const FoldEntry *f = fold_find(Md, lvl, rk))
    return *f;
  const unsigned s = G.slots;
  const size_t mwords = 2 * (size_t)s * s;
  std::vector<double> diags;
  std::vector<unsigned> ds;
  for_each_diagonal(Md, [&](unsigned d, const double *diag) {
    ds.push_back(d);
    diags.insert(diags.end(), diag, diag + 2 * (size_t)s);
  });
  const unsigned E = (unsigned)ds.size();
  unsigned mods[GPQHE_MAXMOD];
  const unsigned nm = basis_qp(lvl, mods);
  const size_t per = (size_t)nm << G.logn;
  Ws pts((size_t)E * per);
  std::vector<GemvDiagIn> dg(E);
  for (unsigned e = 0; e < E; e++) {
    encode_limbs(pts.p + e * per, diags.data() + 2 * (size_t)s * e, s, (double)G.q[lvl - 1], mods, nm);
    dg[e].d = ds[e];
    dg[e].pt = pts.p + e * per;
    dg[e].evk = ds[e] ? find_rot_key(rk, ds[e], galois_of_rot(ds[e]))->data : nullptr;
  }
  FoldEntry f{std::vector<double>(Md, Md + mwords), s, lvl, g_key_gen, rk, ds, nullptr,
              k_gemv_fold_words(E, lvl) * 8};
  f.K = E ? k_gemv_fold(dg.data(), E, lvl) : nullptr;
  fold_make_room(g_folds, f.bytes, 8);  // (f.bytes is within the cap: gemv_fold_fits)
  g_folds.push_front(std::move(f));
  return g_folds.front();
}

// The key of rotation r folded for level lvl.
static const RotFold &rotkey_fold(unsigned r, unsigned lvl, const he_evk_t rk[])
{
  const he_evk_t *k = find_rot_key(rk, r, galois_of_rot(r));
  for (auto it = g_rfolds.begin(); it != g_rfolds.end(); ++it)
    if (it->rot == r && it->lvl == lvl && it->gen == g_key_gen && it->rk == rk) {
      g_rfolds.splice(g_rfolds.begin(), g_rfolds, it);
      return g_rfolds.front();
    }
  const size_t bytes = k_gemv_fold_words(1, lvl) * 8;
  fold_make_room(g_rfolds, bytes, SIZE_MAX);
  const GemvDiagIn dg{r, nullptr, k->data};
  double *K = k_gemv_fold(&dg, 1, lvl);  // (an out-of-memory retry inside may empty the list)
  g_rfolds.push_front(RotFold{rk, g_key_gen, lvl, r, K, bytes});
  return g_rfolds.front();
}

static bool gemv_batch_fast(uint64_t *y, const double *Md, const uint64_t *x, size_t count, unsigned lvl,
                            const he_evk_t rk[])
{
  if (!gemv_win_on(lvl) || !gemv_fold_fits(Md, lvl, rk))
    return false;
  const FoldEntry &f = gemv_fold(Md, lvl, rk);
  FoldUse use(f.K);
  k_gemv_batch(y, x, count, lvl, f.K, f.d.data(), (unsigned)f.d.size(), 1);
  return true;
}

static bool rot_batch_fast(uint64_t *out, const uint64_t *x, size_t count, unsigned lvl, unsigned r,
                           const he_evk_t rk[])
{
  if (!gemv_win_on(lvl))
    return false;
  const RotFold &f = rotkey_fold(r, lvl, rk);
  FoldUse use(f.K);
  k_gemv_batch(out, x, count, lvl, f.K, &f.rot, 1, 0);
  return true;
}

// A ciphertext of a batch as an object view (no payload of its own).
static he_ct_t ct_view(const uint64_t *base, unsigned nlimbs)
{
  he_ct_t c{};
  c.data = (uint64_t *)base;
  c.nlimbs = c.cap = nlimbs;
  c.npoly = 2;
  c.scale = 1.0;
  return c;
}

extern "C" void he_gemv_batch(uint64_t *y, const gpqhe_complex_t M[], const uint64_t *x, size_t count,
                              unsigned int nlimbs, const he_evk_t rk[])
{
  check_ctx();
  const unsigned lvl = nlimbs;
  if (lvl < 2 || lvl > G.L)
    gpqhe_die("he_gemv_batch: bad level %u", lvl);
  const size_t n = G.n, in_words = 2 * (size_t)lvl * n, out_words = 2 * (size_t)(lvl - 1) * n;
  if (count && y < x + count * in_words && x < y + count * out_words)
    gpqhe_die("he_gemv_batch: output overlaps the input");
  if (gemv_batch_fast(y, (const double *)M, x, count, lvl, rk))
    return;
  // one ciphertext at a time on the per-call path (its diagonals cached
  // after the first)
  for (size_t i = 0; i < count; i++) {
    he_ct_t cx = ct_view(x + i * in_words, lvl), cy = ct_view(y + i * out_words, lvl - 1);
    gemv_now(&cy, (const double *)M, &cx, rk, lvl);
  }
}

extern "C" void he_rot_batch(uint64_t *out, const uint64_t *x, size_t count, unsigned int nlimbs, unsigned int rot,
                             const he_evk_t rk[])
{
  check_ctx();
  const unsigned lvl = nlimbs;
  if (lvl < 1 || lvl > G.L)
    gpqhe_die("he_rot_batch: bad level %u", lvl);
  const size_t words = 2 * (size_t)lvl * G.n;
  if (count && out < x + count * words && x < out + count * words)
    gpqhe_die("he_rot_batch: output overlaps the input");
  if (rot % G.slots && rot_batch_fast(out, x, count, lvl, rot % G.slots, rk))
    return;
  for (size_t i = 0; i < count; i++) {
    he_ct_t cx = ct_view(x + i * words, lvl), co = ct_view(out + i * words, lvl);
    he_rot(&co, &cx, rot, rk);
  }
}

// ---------------------------------------------------------------------------
// The batch products over BSGS plans: he_gemv_bsgs_batch here, the pair, the
// step and the row-folded and packed forms below.  One plan lookup per call;
// the ciphertexts in chunks that fit GPQHE_WS_MIB; inside a chunk the buffers
// are slot-major -- B [baby slot][ct][2][lvl][n], U [giant step][ct][2][lvl][n]
// and the rotated giant steps R likewise -- so a rotation of the whole chunk is
// one contiguous batch for the windowed path (win_rot_chunk), and the inner
// sums share every encoded diagonal word among a tile of ciphertexts
// (bsgs_inner_batch_kernel).  Where the windowed path is off, the single
// call's hoisted stages run per ciphertext into the same buffers.  Every step
// gives the residues of he_gemv_bsgs's.
// ---------------------------------------------------------------------------
// The four inputs of a step (null: the operands are given).
struct StepIn {
  const uint64_t *xhat, *xr, *uhat, *ur;
};

// The windowed rotation of whole slot-major chunks: out + t sw <- rot(x + t
// x_stride, rot[t]) for t < nrot, each one k_gemv_batch with the rotation's
// fold (as he_rot_batch).
static void win_rot_chunk(uint64_t *out, const uint64_t *x, size_t x_stride, const unsigned *rot, unsigned nrot,
                          unsigned cnt, unsigned lvl, const he_evk_t rk[])
{
  const size_t sw = (size_t)cnt * 2 * lvl * G.n;
  for (unsigned t = 0; t < nrot; t++) {
    const RotFold &f = rotkey_fold(rot[t], lvl, rk);
    FoldUse use(f.K);
    k_gemv_batch(out + t * sw, x + t * x_stride, cnt, lvl, f.K, &f.rot, 1, 0);
  }
}

// Baby stage of one operand over a chunk: slot i of B ([k.nbs][cnt][2][lvl][n])
// <- rot(x, baby[i]); x may already be slot 0.
static void bsgs_baby_chunk(uint64_t *B, const uint64_t *x, unsigned cnt, unsigned lvl, const BsgsKeys &k,
                            const he_evk_t rk[], size_t budget)
{
  const size_t cw = 2 * (size_t)lvl * G.n, sw = (size_t)cnt * cw;
  if (!k.nbs)
    return;
  if (gemv_win_on(lvl)) {
    if (k.has0 && B != x)
      HIP_CHECK(hipMemcpyAsync(B, x, sw * 8, hipMemcpyDeviceToDevice, G.stream));
    win_rot_chunk(B + (size_t)k.has0 * sw, x, 0, k.brot.data(), k.nbr, cnt, lvl, rk);
    return;
  }
  for (unsigned c = 0; c < cnt; c++) {
    const he_ct_t cx = ct_view(x + c * cw, lvl);
    bsgs_baby(B + c * cw, sw, &cx, k, lvl, budget);
  }
}

// The end of a chunk of the row-folded forms: the fold steps at level lvl - 1
// -- y (cnt ciphertexts) rotated into R, then accumulated -- and the step's
// tail y = uhat - y: the last fold step's kernel, or k_step_tail_batch where
// there is no fold.
static void fold_tail_chunk(uint64_t *y, uint64_t *R, const StepIn *st, const std::vector<unsigned> &fold,
                            unsigned cnt, unsigned lvl, const he_evk_t rk[])
{
  const size_t ow = 2 * (size_t)(lvl - 1) * G.n;
  for (size_t t = 0; t < fold.size(); t++) {
    if (gemv_win_on(lvl - 1)) {
      win_rot_chunk(R, y, 0, &fold[t], 1, cnt, lvl - 1, rk);
    } else {
      for (unsigned c = 0; c < cnt; c++) {
        he_ct_t cx = ct_view(y + c * ow, lvl - 1), co = ct_view(R + c * ow, lvl - 1);
        he_rot(&co, &cx, fold[t], rk);
      }
    }
    if (st && t + 1 == fold.size())
      k_rows_fold_tail_batch(y, R, st->uhat, lvl, cnt);
    else
      k_rows_fold_add_batch(y, R, lvl - 1, cnt);
  }
  if (st && fold.empty())
    k_step_tail_batch(y, st->uhat, lvl, cnt);
}

// The entry check of every batch product: the context, the level, and y
// (count ciphertexts at level lvl - 1) apart from every input (at level lvl).
static void batch_check(const char *who, const uint64_t *y, const uint64_t *xa, const uint64_t *xb, const StepIn *st,
                        size_t count, unsigned lvl)
{
  check_ctx();
  if (lvl < 2 || lvl > G.L)
    gpqhe_die("%s: bad level %u", who, lvl);
  const size_t in_words = 2 * (size_t)lvl * G.n, out_words = 2 * (size_t)(lvl - 1) * G.n;
  const uint64_t *ins[4] = {st ? st->xhat : xa, st ? st->xr : xb, st ? st->uhat : nullptr, st ? st->ur : nullptr};
  for (const uint64_t *x : ins)
    if (x && y < x + count * in_words && x < y + count * out_words)
      gpqhe_die("%s: output overlaps %s input", who, ins[1] ? "an" : "the");
}

// Ciphertexts per chunk: as many as GPQHE_WS_MIB holds at per_ct_words each,
// at most cap, in equal chunks (a short last one runs at a fraction of the
// GPU's width).  hook: the test variable that forces several chunks on a small
// batch.  The two hooks differ, and are kept as they are: GPQHE_BSGS_CHUNK is
// the chunk as given, GPQHE_CHUNK (the I/O calls') is equalised like any other.
static size_t batch_chunk_size(size_t count, size_t per_ct_words, size_t cap, const char *hook)
{
  size_t chunk = std::min(std::max<size_t>(1, bsgs_budget() / per_ct_words), std::max<size_t>(1, cap));
  if (const char *e = getenv(hook)) {
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, strtoul(e, nullptr, 0)));
    if (!strcmp(hook, "GPQHE_BSGS_CHUNK"))
      return chunk;
  }
  const size_t nchunks = (count + chunk - 1) / chunk;
  return (count + nchunks - 1) / nchunks;
}

// The chunk loop of a batch product at level lvl: run(y, xa, xb, st, cnt) on
// each chunk's part of y and of the operands (st null) or of the step's inputs.
template <class Run>
static void batch_chunks(uint64_t *y, const uint64_t *xa, const uint64_t *xb, const StepIn *st, size_t count,
                         unsigned lvl, size_t chunk, Run run)
{
  const size_t in_words = 2 * (size_t)lvl * G.n, out_words = 2 * (size_t)(lvl - 1) * G.n;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const unsigned cnt = (unsigned)std::min(chunk, count - c0);
    const size_t o = c0 * in_words;
    const StepIn sc = st ? StepIn{st->xhat + o, st->xr + o, st->uhat + o, st->ur + o} : StepIn{};
    run(y + c0 * out_words, st ? nullptr : xa + o, st || !xb ? nullptr : xb + o, st ? &sc : nullptr, cnt);
  }
}

// One chunk of cnt ciphertexts, y = Ma xa + Mb xb: ka / kb the baby rotations
// of each operand (kb empty: the single product), kg the giant steps of the
// union, fold the rotate-and-add steps at level lvl - 1 behind the rescale.
// st: form xa = xhat - xr and xb = uhat - ur first (into slot 0 of the
// operand's baby slots where its plan uses the unrotated slot, else into a
// workspace) and finish with y = uhat - y (fold_tail_chunk).
static void bsgs_chunk(uint64_t *y, const uint64_t *xa, const uint64_t *xb, const StepIn *st, unsigned cnt,
                       unsigned lvl, const BsgsPlan &plan, const BsgsKeys &ka, const BsgsKeys &kb, const BsgsKeys &kg,
                       const std::vector<unsigned> &fold, const he_evk_t rk[], size_t budget)
{
  const unsigned nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t n = G.n, pw = (size_t)lvl * n, cw = 2 * pw, sw = (size_t)cnt * cw;  // words: ciphertext, slot
  const unsigned nbs = ka.nbs + kb.nbs;
  // (the rotated giant steps, then the fold's rotated copy, take the baby
  // slots' place: the inner sums are the last to read those)
  Ws B((size_t)std::max(nbs, kg.njr) * sw), U((size_t)kg.nj * sw);
  uint64_t *Ba = B.p, *Bb = B.p + (size_t)ka.nbs * sw, *R = B.p;

  Ws Xd(st && !ka.has0 ? sw : 0), Ud(st && !kb.has0 ? sw : 0);
  if (st) {
    uint64_t *xd = ka.has0 ? Ba : Xd.p, *ud = kb.has0 ? Bb : Ud.p;
    k_step_diff_batch(xd, ud, st->xhat, st->xr, st->uhat, st->ur, lvl, cnt);
    xa = xd;
    xb = ud;
  }

  // baby steps of each operand, then the inner sums over all of their slots
  bsgs_baby_chunk(Ba, xa, cnt, lvl, ka, rk, budget);
  bsgs_baby_chunk(Bb, xb, cnt, lvl, kb, rk, budget);
  k_bsgs_inner_batch(U.p, B.p, plan.pts, plan.tab_dev, kg.nj, nbs, plan.ndiag(), lvl, cnt);

  // giant steps of the union: u_j of the whole chunk rotated by j g into R
  if (gemv_win_on(lvl)) {
    win_rot_chunk(R, U.p + (size_t)kg.hasj0 * sw, sw, kg.grot.data(), kg.njr, cnt, lvl, rk);
  } else if (kg.njr) {
    const unsigned cg = bsgs_giant_chunk(kg, lvl, budget, 0);
    Ws Dg((size_t)cg * ndig * nm * n), acc((size_t)cg * 2 * nm * n);
    for (unsigned c = 0; c < cnt; c++)
      for (unsigned r0 = 0; r0 < kg.njr; r0 += cg)
        bsgs_giant(R + (size_t)r0 * sw + c * cw, sw, U.p + c * cw, sw, kg, r0, std::min(cg, kg.njr - r0), lvl, Dg.p,
                   acc.p);
  }

  // sum over the giant steps (u_0 is not rotated) and rescale by q_top into y
  uint64_t *S = U.p;
  Ws Sw(kg.njr ? sw : 0);
  if (kg.njr) {
    k_bsgs_sum_batch(Sw.p, kg.hasj0 ? U.p : nullptr, R, kg.njr, sw, lvl, cnt);
    S = Sw.p;
  }
  k_moddown(y, (size_t)(lvl - 1) * n, S, pw, 2 * cnt, lvl, 2);

  fold_tail_chunk(y, R, st, fold, cnt, lvl, rk);
}

// What an entry point's own argument checks leave for the run: the rotation
// of giant step 1 and the fold steps.
struct BatchKind {
  unsigned g;
  std::vector<unsigned> fold;
};

// The run of every entry point: check() makes the entry point's own argument
// checks (after batch_check's), get(hold) looks its plan up.  Plan, then keys,
// then the first launch.
template <class Check, class Get>
static void bsgs_run(const char *who, uint64_t *y, const uint64_t *xa, const uint64_t *xb, const StepIn *st,
                     size_t count, unsigned lvl, const he_evk_t rk[], Check check, Get get)
{
  batch_check(who, y, xa, xb, st, count, lvl);
  const BatchKind kind = check();
  const size_t pw = (size_t)lvl * G.n, in_words = 2 * pw, out_words = 2 * (size_t)(lvl - 1) * G.n;
  if (!count)
    return;

  PlanHold hold;
  const BsgsPlan *plan = get(hold);
  if (plan->giant.empty()) {  // no diagonal: y = 0, up = the lower limbs of uhat
    HIP_CHECK(hipMemsetAsync(y, 0, count * out_words * 8, G.stream));
    for (size_t c0 = 0; st && c0 < count; c0 += 16384) {
      const unsigned cnt = (unsigned)std::min<size_t>(16384, count - c0);
      k_step_tail_batch(y + c0 * out_words, st->uhat + c0 * in_words, lvl, cnt);
    }
    return;
  }
  // every key is found before anything is launched
  const BsgsKeys ka = bsgs_find_keys(plan->a.baby, {}, kind.g, rk), kb = bsgs_find_keys(plan->b.baby, {}, kind.g, rk);
  const BsgsKeys kg = bsgs_find_keys({}, plan->giant, kind.g, rk);
  for (unsigned r : kind.fold)
    find_rot_key(rk, r, galois_of_rot(r));

  // a ciphertext's share of a chunk, in words of one ciphertext (2 lvl n):
  //   max(nbs_a + nbs_b, njr)  the baby slots of the operands, later the rotated giant steps
  //                            (and the fold's rotated copy, which is smaller)
  //   + nj                     the giant steps of the union
  //   + 1                      their sum, where a giant step is rotated
  //   + 1 per operand of a step whose difference has no slot 0 to live in;
  // on the windowed path k_gemv_batch's workspace besides (the generic stages'
  // workspaces do not grow with the chunk)
  const size_t slots_ct =
    std::max(ka.nbs + kb.nbs, kg.njr) + kg.nj + (kg.njr ? 1 : 0) + (st ? !ka.has0 + !kb.has0 : 0);
  const size_t per_ct = slots_ct * 2 * pw + (gemv_win_on(lvl) ? k_gemv_batch_ws_words(lvl) : 0);
  batch_chunks(y, xa, xb, st, count, lvl, batch_chunk_size(count, per_ct, 16384, "GPQHE_BSGS_CHUNK"),
               [&](uint64_t *yc, const uint64_t *xac, const uint64_t *xbc, const StepIn *sc, unsigned cnt) {
                 bsgs_chunk(yc, xac, xbc, sc, cnt, lvl, *plan, ka, kb, kg, kind.fold, rk, bsgs_budget());
               });
}

// g = 0: the default; g > slots: an error (the check() of the forms with giant steps)
static BatchKind bsgs_check_g(const char *who, unsigned &g)
{
  if (!g)
    g = bsgs_default_g();
  if (g > G.slots)
    gpqhe_die("%s: g = %u > slots = %u", who, g, G.slots);
  return BatchKind{g, {}};
}

// he_gemv_bsgs_batch (include/gpqhe_ext_batch.h): he_gemv_bsgs over count
// ciphertexts that share M, g and the keys.
extern "C" void he_gemv_bsgs_batch(uint64_t *y, const gpqhe_complex_t M[], const uint64_t *x, size_t count,
                                   unsigned int nlimbs, const he_evk_t rk[], unsigned int g)
{
  HPROF("gemv_bsgs_batch");
  bsgs_run(
    "he_gemv_bsgs_batch", y, x, nullptr, nullptr, count, nlimbs, rk,
    [&] { return bsgs_check_g("he_gemv_bsgs_batch", g); },
    [&](PlanHold &h) { return bsgs_plan_get(h, (const double *)M, nlimbs, g); });
}

// ---------------------------------------------------------------------------
// he_gemv2_bsgs_batch / he_hempc_step_batch (include/gpqhe_ext_step_batch.h):
// y = Ma xa + Mb xb by one BSGS over both operands, and ctr_hempc around it.
// The two products are summed before the giant rotations, so the inner sums
// run over the concatenated baby slots of both operands and every giant step
// of the union is rotated once: 2 (g - 1) + (G - 1) key switches and one
// rescale per ciphertext.  The step adds step_diff_batch_kernel in front and
// step_tail_batch_kernel behind (step_batch.hip).
// ---------------------------------------------------------------------------
// The pair plan: (Ma, Mb, lvl, g), the ordered pair, in g_bsgs2.
static const BsgsPlan *bsgs2_plan_get(PlanHold &h, const double *Ma, const double *Mb, unsigned lvl, unsigned g)
{
  const unsigned s = G.slots;
  const size_t pw = (size_t)lvl * G.n;
  return g_bsgs2.get(
    h, {s, lvl, g}, lvl, Ma, Mb, 2 * (size_t)s * s,
    [&](BsgsPlan &p) {
      bsgs_plan(p.a, Ma, g);
      bsgs_plan(p.b, Mb, g);
    },
    [&](const BsgsPlan &p, uint64_t *pts) {
      bsgs_encode(p.a, Ma, lvl, g, pts);
      bsgs_encode(p.b, Mb, lvl, g, pts + p.a.ds.size() * pw);
    });
}

static void bsgs2_run(const char *who, uint64_t *y, const double *Ma, const double *Mb, const uint64_t *xa,
                      const uint64_t *xb, const StepIn *st, size_t count, unsigned lvl, const he_evk_t rk[],
                      unsigned g)
{
  bsgs_run(
    who, y, xa, xb, st, count, lvl, rk, [&] { return bsgs_check_g(who, g); },
    [&](PlanHold &h) { return bsgs2_plan_get(h, Ma, Mb, lvl, g); });
}

extern "C" void he_gemv2_bsgs_batch(uint64_t *y, const gpqhe_complex_t Ma[], const uint64_t *xa,
                                    const gpqhe_complex_t Mb[], const uint64_t *xb, size_t count, unsigned int nlimbs,
                                    const he_evk_t rk[], unsigned int g)
{
  HPROF("gemv2_bsgs_batch");
  bsgs2_run("he_gemv2_bsgs_batch", y, (const double *)Ma, (const double *)Mb, xa, xb, nullptr, count, nlimbs, rk, g);
}

extern "C" void he_hempc_step_batch(uint64_t *up, const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                                    const uint64_t *xhat, const uint64_t *xr, const uint64_t *uhat, const uint64_t *ur,
                                    size_t count, unsigned int nlimbs, const he_evk_t rk[], unsigned int g)
{
  HPROF("hempc_step_batch");
  const StepIn st{xhat, xr, uhat, ur};
  bsgs2_run("he_hempc_step_batch", up, (const double *)Ma, (const double *)Mb, nullptr, nullptr, &st, count, nlimbs, rk,
            g);
}

// ---------------------------------------------------------------------------
// he_gemv2_rows_batch / he_hempc_step_rows_batch / he_genrk_rows
// (include/gpqhe_ext_rows_batch.h): the leading `rows` rows of Ma xa + Mb xb
// by row folding.  With m' = 2^ceil(log2 rows), each matrix has at most m'
// extended diagonals E_i (row k mod m' of the matrix at column k + i, zero
// where k mod m' >= rows); their products with rot(x, i) are summed, rescaled,
// and log2(s / m') rotate-and-add steps at level lvl - 1 gather the partial
// sums: 2 (m' - 1) + log2(s / m') key switches per ciphertext.  To bsgs_chunk
// this is a pair plan with one giant step (no giant rotation) and a fold list;
// the fold's additions are rows_batch.hip's, the last one of a step fused with
// the step's tail.
//
// The packed forms (include/gpqhe_ext_packed_batch.h: he_gemv2_packed_batch,
// he_hempc_step_packed_batch, he_genrk_packed) are the same code at a stride:
// the context's S slots hold P = S / sl loops of sl slots, entry k of loop p
// at slot k P + p, so E_i is filled over S slots from loop p's own matrix
// (nmat = P) or the shared one (nmat = 1), baby rotation i is rotation i P and
// fold step r is r P.  The entry points above are sl = S, nmat = 1 (P = 1).
// ---------------------------------------------------------------------------
static unsigned rows_pow2(unsigned rows)
{
  unsigned mp = 1;
  while (mp < rows)
    mp <<= 1;
  return mp;
}

// E_i of M ([nmat][rows][sl], loop p's matrix p mod nmat) over the context's
// slots: v [S] complex, slot k P + p from row k mod m' of loop p's matrix at
// column (k + i) mod sl; false when it is all zero.
static bool rows_diag(std::vector<double> &v, const double *Md, unsigned i, unsigned rows, unsigned mp, unsigned sl,
                      unsigned nmat)
{
  const unsigned S = G.slots, P = S / sl;
  bool nz = false;
  for (unsigned j = 0; j < S; j++) {
    const unsigned k = j / P, p = j % P, row = k % mp;
    const size_t src = ((size_t)(nmat > 1 ? p : 0) * rows + row) * sl + (k + i) % sl;
    v[2 * j] = row < rows ? Md[2 * src] : 0.0;
    v[2 * j + 1] = row < rows ? Md[2 * src + 1] : 0.0;
    nz |= v[2 * j] != 0.0 || v[2 * j + 1] != 0.0;
  }
  return nz;
}

// The non-zero E_i of M, i < m', as an operand with one giant step: ds the i,
// baby the rotations i P, tab the identity.
static void rows_plan(BsgsOp &o, const double *Md, unsigned rows, unsigned sl, unsigned nmat)
{
  const unsigned P = G.slots / sl, mp = rows_pow2(rows);
  std::vector<double> v(2 * (size_t)G.slots);
  for (unsigned i = 0; i < mp; i++)
    if (rows_diag(v, Md, i, rows, mp, sl, nmat)) {
      o.tab.push_back((int)o.ds.size());
      o.ds.push_back(i);
      o.baby.push_back(i * P);
    }
  if (!o.ds.empty())
    o.giant.push_back(0);
}

// pts <- E_i of every i in o.ds, in that order.
static void rows_encode(const BsgsOp &o, const double *Md, unsigned lvl, unsigned rows, unsigned sl, unsigned nmat,
                        uint64_t *pts)
{
  unsigned mods[GPQHE_MAXMOD];
  for (unsigned l = 0; l < lvl; l++)
    mods[l] = l;
  std::vector<double> v(2 * (size_t)G.slots);
  for (size_t e = 0; e < o.ds.size(); e++) {
    rows_diag(v, Md, o.ds[e], rows, rows_pow2(rows), sl, nmat);
    encode_limbs(pts + e * ((size_t)lvl << G.logn), v.data(), G.slots, (double)G.q[lvl - 1], mods, lvl);
  }
}

// The row plan: (the leading rows sl entries of each of Ma's, of Mb's nmat
// matrices, lvl, rows, sl, nmat) in g_rows.
static const BsgsPlan *rows_plan_get(PlanHold &h, const double *Ma, const double *Mb, unsigned lvl, unsigned rows,
                                     unsigned sl, unsigned nmat)
{
  const size_t pw = (size_t)lvl * G.n;
  return g_rows.get(
    h, {G.slots, lvl, rows, sl, nmat}, lvl, Ma, Mb, 2 * (size_t)nmat * rows * sl,
    [&](BsgsPlan &p) {
      rows_plan(p.a, Ma, rows, sl, nmat);
      rows_plan(p.b, Mb, rows, sl, nmat);
    },
    [&](const BsgsPlan &p, uint64_t *pts) {
      rows_encode(p.a, Ma, lvl, rows, sl, nmat, pts);
      rows_encode(p.b, Mb, lvl, rows, sl, nmat, pts + p.a.ds.size() * pw);
    });
}

// The loops of a packed call: P = slots / s; dies unless s, the slots of one
// loop, is a power of two dividing the context's.
static unsigned packed_loops(const char *who, unsigned s)
{
  if (!s || (s & (s - 1)) || s > G.slots)
    gpqhe_die("%s: s = %u, slots = %u", who, s, G.slots);
  return G.slots / s;
}

// ... and of a row-folded one: rows of the s, one matrix or one per loop.
static unsigned rows_loops(const char *who, unsigned s, unsigned rows, unsigned nmat)
{
  const unsigned P = packed_loops(who, s);
  if (!rows || rows > s)
    gpqhe_die("%s: rows = %u, s = %u", who, rows, s);
  if (nmat != 1 && nmat != P)
    gpqhe_die("%s: %u matrices for %u loops", who, nmat, P);
  return P;
}

static void rows_genrk(const char *who, he_evk_t rk[], const poly_mpi_t *sk, unsigned sl, unsigned rows)
{
  check_ctx();
  const unsigned P = rows_loops(who, sl, rows, 1), mp = rows_pow2(rows);
  gen_rot_keys(rk, sk, [=](unsigned r) {
    const unsigned i = r / P;                                   // the loops' own rotation (r = i P)
    const bool fold = i % mp == 0 && !(i / mp & (i / mp - 1));  // m' 2^t
    return r % P == 0 && (i < mp || fold);
  });
}

extern "C" void he_genrk_rows(he_evk_t rk[], const poly_mpi_t *sk, unsigned int rows)
{
  check_ctx();  // (G.slots is read here)
  rows_genrk("he_genrk_rows", rk, sk, G.slots, rows);
}

extern "C" void he_genrk_packed(he_evk_t rk[], const poly_mpi_t *sk, unsigned int s, unsigned int rows)
{
  rows_genrk("he_genrk_packed", rk, sk, s, rows);
}

static void rows_run(const char *who, uint64_t *y, const double *Ma, const double *Mb, const uint64_t *xa,
                     const uint64_t *xb, const StepIn *st, size_t count, unsigned lvl, const he_evk_t rk[],
                     unsigned rows, unsigned sl, unsigned nmat)
{
  bsgs_run(
    who, y, xa, xb, st, count, lvl, rk,
    [&] {
      const unsigned P = rows_loops(who, sl, rows, nmat);
      BatchKind kind{1, {}};  // the fold: the rotations m' P, 2 m' P, .. < S
      for (unsigned r = rows_pow2(rows); r < sl; r <<= 1)
        kind.fold.push_back(r * P);
      return kind;
    },
    [&](PlanHold &h) { return rows_plan_get(h, Ma, Mb, lvl, rows, sl, nmat); });
}

extern "C" void he_gemv2_rows_batch(uint64_t *y, const gpqhe_complex_t Ma[], const uint64_t *xa,
                                    const gpqhe_complex_t Mb[], const uint64_t *xb, size_t count, unsigned int nlimbs,
                                    const he_evk_t rk[], unsigned int rows)
{
  HPROF("gemv2_rows_batch");
  check_ctx();  // (G.slots is read here)
  rows_run("he_gemv2_rows_batch", y, (const double *)Ma, (const double *)Mb, xa, xb, nullptr, count, nlimbs, rk, rows,
           G.slots, 1);
}

extern "C" void he_hempc_step_rows_batch(uint64_t *up, const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                                         const uint64_t *xhat, const uint64_t *xr, const uint64_t *uhat,
                                         const uint64_t *ur, size_t count, unsigned int nlimbs, const he_evk_t rk[],
                                         unsigned int rows)
{
  HPROF("hempc_step_rows_batch");
  const StepIn st{xhat, xr, uhat, ur};
  check_ctx();  // (G.slots is read here)
  rows_run("he_hempc_step_rows_batch", up, (const double *)Ma, (const double *)Mb, nullptr, nullptr, &st, count, nlimbs,
           rk, rows, G.slots, 1);
}

extern "C" void he_gemv2_packed_batch(uint64_t *y, const gpqhe_complex_t Ma[], const uint64_t *xa,
                                      const gpqhe_complex_t Mb[], const uint64_t *xb, size_t count,
                                      unsigned int nlimbs, const he_evk_t rk[], unsigned int s, unsigned int rows,
                                      unsigned int nmat)
{
  HPROF("gemv2_packed_batch");
  rows_run("he_gemv2_packed_batch", y, (const double *)Ma, (const double *)Mb, xa, xb, nullptr, count, nlimbs, rk, rows,
           s, nmat);
}

extern "C" void he_hempc_step_packed_batch(uint64_t *up, const gpqhe_complex_t Ma[], const gpqhe_complex_t Mb[],
                                           const uint64_t *xhat, const uint64_t *xr, const uint64_t *uhat,
                                           const uint64_t *ur, size_t count, unsigned int nlimbs, const he_evk_t rk[],
                                           unsigned int s, unsigned int rows, unsigned int nmat)
{
  HPROF("hempc_step_packed_batch");
  const StepIn st{xhat, xr, uhat, ur};
  rows_run("he_hempc_step_packed_batch", up, (const double *)Ma, (const double *)Mb, nullptr, nullptr, &st, count,
           nlimbs, rk, rows, s, nmat);
}

// ---------------------------------------------------------------------------
// he_enc_pk_batch / he_dec_dcd_batch (include/gpqhe_ext_batch.h): the two ends
// of the batch entry points.  Chunks sized by GPQHE_WS_MIB (GPQHE_CHUNK: the
// test hook of he_mul_rescale_batch), a fixed number of launches per chunk.
// ---------------------------------------------------------------------------
static size_t ntt_group_polys(unsigned nlimbs);

static size_t io_chunk(size_t count, size_t per_ct_words, size_t cap)
{
  return batch_chunk_size(count, per_ct_words, cap, "GPQHE_CHUNK");
}

// k_ntt over npolys polynomials of nlimbs limbs in poly_ntt_batch's groups
static void ntt_polys(uint64_t *data, size_t npolys, unsigned nlimbs, bool inverse)
{
  const size_t per = ntt_group_polys(nlimbs), w = (size_t)nlimbs * G.n;
  for (size_t p0 = 0; p0 < npolys; p0 += per)
    k_ntt(qlimbs(data + p0 * w, nlimbs, (unsigned)std::min(per, npolys - p0), w), inverse);
}

static void io_check(const char *who, unsigned nlimbs, unsigned slots)
{
  if (nlimbs < 1 || nlimbs > G.L)
    gpqhe_die("%s: bad level %u", who, nlimbs);
  if (!slots || (slots & (slots - 1)) || slots > G.n / 2)
    gpqhe_die("%s: bad slot count %u", who, slots);
}

// The encode front end of the batch encryptions, the same under either key:
// the z upload, the packed gather, the encoder and the one overflow check of a
// call.  P = 0: z [count][s], the vectors as they are encoded.  P > 0 (the
// packed form, s = P loops' slots): z [count][P][width] loop-major, slot k P + p
// of ciphertext c from z[c][p][k], 0 for k >= width.  Takes nstreams RNG
// streams per ciphertext; chunks sized for key_words words of the caller's
// workspace per ciphertext next to the encode buffers.  back(c0, cnt, stream,
// coef): ciphertexts c0 .. c0 + cnt - 1 from their compact coefficients (coef
// [cnt][2 s], device), `stream` the first of ciphertext c0.
template <class Back>
static void enc_front(const char *who, const void *x, const gpqhe_complex_t z[], size_t count, unsigned s, double scale,
                      unsigned P, unsigned width, unsigned nstreams, size_t key_words, Back back)
{
  if (!count)
    return;
  if (!x || !z)
    gpqhe_die("%s: null argument", who);
  const size_t zw = P ? (size_t)P * width : s;  // zw: a ciphertext's values of z
  // the streams of count single encryptions: base + nstreams i + {0, ..}
  const uint64_t base = G.counter;
  G.counter += nstreams * (uint64_t)count;
  // from gpu_ecd_min() slots the special FFT runs on the GPU (one upload of
  // the chunk's z, staged: at most 64 MiB of it), below it on the host (one
  // upload of the chunk's coefficients)
  const bool gpu = s >= gpu_ecd_min();
  const size_t per_ct = key_words + 2 * (size_t)s * (gpu ? 2 : 1) + (gpu && P ? 2 * zw : 0);
  const size_t chunk = io_chunk(count, per_ct, gpu ? std::min<size_t>(16384, ((size_t)4 << 20) / s) : 16384);
  Ws ovf(gpu ? 1 : 0);
  if (gpu)
    HIP_CHECK(hipMemsetAsync(ovf.p, 0, 8, G.stream));
  std::vector<int64_t> hv;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const unsigned cnt = (unsigned)std::min(chunk, count - c0);
    Ws coef(2 * (size_t)s * cnt);
    const double *zc = (const double *)z + 2 * c0 * zw;
    if (gpu) {
      Ws work(2 * (size_t)s * cnt);
      if (P) {  // the chunk's z as given, interleaved on the device
        Ws zin(2 * zw * cnt);
        upload(zin.p, zc, (size_t)cnt * zw * 16);
        k_pack_enc_gather((double *)work.p, (const double *)zin.p, s, P, width, cnt);
      } else {
        upload(work.p, zc, (size_t)cnt * s * 16);
      }
      k_encode_slots_batch((int64_t *)coef.p, (double *)work.p, (int *)ovf.p, s, scale, cnt);
    } else {
      hv.resize(2 * (size_t)s * cnt);
      std::vector<double> il(P ? 2 * (size_t)s : 0);  // (zero for k >= width)
      for (unsigned i = 0; i < cnt; i++) {
        const double *zi = zc + 2 * zw * i;
        for (unsigned p = 0; p < P; p++)
          for (unsigned k = 0; k < width; k++) {
            il[2 * ((size_t)k * P + p)] = zi[2 * ((size_t)p * width + k)];
            il[2 * ((size_t)k * P + p) + 1] = zi[2 * ((size_t)p * width + k) + 1];
          }
        hm_encode_slots(hv.data() + 2 * (size_t)s * i, P ? il.data() : zi, s, scale);
      }
      upload(coef.p, hv.data(), hv.size() * 8);
    }
    back(c0, cnt, base + nstreams * (uint64_t)c0, (const int64_t *)coef.p);
  }
  if (gpu) {
    // the single encode's overflow check, once for the batch
    int h = 0;
    HIP_CHECK(hipMemcpyAsync(&h, ovf.p, sizeof(int), hipMemcpyDeviceToHost, G.stream));
    HIP_CHECK(hipStreamSynchronize(G.stream));
    if (h)
      gpqhe_die("encode overflow (|value * scale| >= 2^63)");
  }
}

// he_ecd_ex + he_enc_pk of count vectors (z, P, width: enc_front): per chunk
// the three noise polynomials of a ciphertext sampled, transformed, combined.
static void enc_pk_run(const char *who, uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned s, double scale,
                       unsigned lvl, const he_pk_t *pk, unsigned P, unsigned width)
{
  io_check(who, lvl, s);
  if (!pk || !pk->data || pk->nlimbs < lvl)
    gpqhe_die("%s: no public key at level %u", who, lvl);
  const size_t w = (size_t)lvl * G.n;
  enc_front(who, x, z, count, s, scale, P, width, 3, 3 * w,
            [&](size_t c0, unsigned cnt, uint64_t stream, const int64_t *coef) {
              Ws vee(3 * cnt * w);
              k_enc_sample_batch(vee.p, stream, coef, s, lvl, cnt);
              ntt_polys(vee.p, 3 * (size_t)cnt, lvl, false);
              k_enc_combine_chunk(x + c0 * 2 * w, vee.p, limb(pk, 0, 0), limb(pk, 1, 0), lvl, cnt);
            });
}

// he_ecd_ex + he_enc_sk of count vectors (include/gpqhe_ext_sk_batch.h): per
// chunk c1 sampled where it stays and e + m into the workspace, ONE transform
// per ciphertext, c0 = NTT(e + m) - c1 s.
static void enc_sk_run(const char *who, uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned s, double scale,
                       unsigned lvl, const poly_mpi_t *sk, unsigned P, unsigned width)
{
  io_check(who, lvl, s);
  if (!sk || !sk->data || sk->nlimbs < lvl)
    gpqhe_die("%s: no secret key at level %u", who, lvl);
  const size_t w = (size_t)lvl * G.n;
  enc_front(who, x, z, count, s, scale, P, width, 2, w,
            [&](size_t c0, unsigned cnt, uint64_t stream, const int64_t *coef) {
              Ws E(cnt * w);
              k_enc_sk_sample_batch(x + c0 * 2 * w, E.p, stream, coef, s, lvl, cnt);
              ntt_polys(E.p, cnt, lvl, false);
              k_enc_sk_combine_chunk(x + c0 * 2 * w, E.p, sk->data, lvl, cnt);
            });
}

extern "C" void he_enc_pk_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned int slots,
                                double scale, unsigned int nlimbs, const he_pk_t *pk)
{
  HPROF("enc_pk_batch");
  check_ctx();
  enc_pk_run("he_enc_pk_batch", x, z, count, slots, scale, nlimbs, pk, 0, 0);
}

extern "C" void he_enc_pk_packed_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned int s,
                                       unsigned int width, double scale, unsigned int nlimbs, const he_pk_t *pk)
{
  HPROF("enc_pk_packed_batch");
  check_ctx();
  const unsigned P = packed_loops("he_enc_pk_packed_batch", s);
  if (!width || width > s)
    gpqhe_die("he_enc_pk_packed_batch: width = %u, s = %u", width, s);
  // (one loop of full width: z is the vector as it is encoded)
  enc_pk_run("he_enc_pk_packed_batch", x, z, count, G.slots, scale, nlimbs, pk, P == 1 && width == s ? 0 : P, width);
}

extern "C" void he_enc_sk_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned int slots,
                                double scale, unsigned int nlimbs, const poly_mpi_t *sk)
{
  HPROF("enc_sk_batch");
  check_ctx();
  enc_sk_run("he_enc_sk_batch", x, z, count, slots, scale, nlimbs, sk, 0, 0);
}

extern "C" void he_enc_sk_packed_batch(uint64_t *x, const gpqhe_complex_t z[], size_t count, unsigned int s,
                                       unsigned int width, double scale, unsigned int nlimbs, const poly_mpi_t *sk)
{
  HPROF("enc_sk_packed_batch");
  check_ctx();
  const unsigned P = packed_loops("he_enc_sk_packed_batch", s);
  if (!width || width > s)
    gpqhe_die("he_enc_sk_packed_batch: width = %u, s = %u", width, s);
  // (one loop of full width: z is the vector as it is encoded)
  enc_sk_run("he_enc_sk_packed_batch", x, z, count, G.slots, scale, nlimbs, sk, P == 1 && width == s ? 0 : P, width);
}

// ---------------------------------------------------------------------------
// he_enc_sk_seeded_batch and its packed forms, he_expand_seeded_batch
// (include/gpqhe_ext_seeded_batch.h): c1 is the uniform sample of a PUBLIC
// ChaCha key and stream, never stored by the encrypting side.
// ---------------------------------------------------------------------------
static ChachaKey seeded_key(const char *who, const gpqhe_pubseed_t *ps, size_t count)
{
  if (!ps)
    gpqhe_die("%s: null seed", who);
  if (ps->stream + (uint64_t)count < ps->stream)
    gpqhe_die("%s: the seed's stream %llu + %zu ciphertexts wraps 2^64", who, (unsigned long long)ps->stream, count);
  ChachaKey k;
  for (unsigned i = 0; i < 8; i++)
    k.k[i] = ps->key[i];
  return k;
}

// enc_sk_run with c1 kept in registers: per chunk e + m sampled straight into
// the compact output (private stream base + 2 i + 1; base + 2 i is skipped),
// transformed there, and c0 = NTT(e + m) - a s finished in place, a from the
// public stream ps->stream + i.  No ciphertext workspace.
static void enc_sk_seeded_run(const char *who, uint64_t *c0, const gpqhe_complex_t z[], size_t count, unsigned s,
                              double scale, unsigned lvl, const poly_mpi_t *sk, unsigned P, unsigned width,
                              gpqhe_pubseed_t *ps)
{
  io_check(who, lvl, s);
  if (!sk || !sk->data || sk->nlimbs < lvl)
    gpqhe_die("%s: no secret key at level %u", who, lvl);
  const ChachaKey pub = seeded_key(who, ps, count);
  const uint64_t pstream = ps->stream;
  const size_t w = (size_t)lvl * G.n;
  enc_front(who, c0, z, count, s, scale, P, width, 2, 0,
            [&](size_t i0, unsigned cnt, uint64_t stream, const int64_t *coef) {
              uint64_t *o = c0 + i0 * w;
              k_enc_sk_sample_batch(nullptr, o, stream, coef, s, lvl, cnt, true);
              ntt_polys(o, cnt, lvl, false);
              k_enc_sk_seeded_combine(o, sk->data, pub, pstream + i0, lvl, cnt);
            });
  ps->stream += count;
}

extern "C" void he_enc_sk_seeded_batch(uint64_t *c0, const gpqhe_complex_t z[], size_t count, unsigned int slots,
                                       double scale, unsigned int nlimbs, const poly_mpi_t *sk, gpqhe_pubseed_t *ps)
{
  HPROF("enc_sk_seeded_batch");
  check_ctx();
  enc_sk_seeded_run("he_enc_sk_seeded_batch", c0, z, count, slots, scale, nlimbs, sk, 0, 0, ps);
}

extern "C" void he_enc_sk_seeded_packed_batch(uint64_t *c0, const gpqhe_complex_t z[], size_t count, unsigned int s,
                                              unsigned int width, double scale, unsigned int nlimbs,
                                              const poly_mpi_t *sk, gpqhe_pubseed_t *ps)
{
  HPROF("enc_sk_seeded_packed_batch");
  check_ctx();
  const unsigned P = packed_loops("he_enc_sk_seeded_packed_batch", s);
  if (!width || width > s)
    gpqhe_die("he_enc_sk_seeded_packed_batch: width = %u, s = %u", width, s);
  // (one loop of full width: z is the vector as it is encoded)
  enc_sk_seeded_run("he_enc_sk_seeded_packed_batch", c0, z, count, G.slots, scale, nlimbs, sk,
                    P == 1 && width == s ? 0 : P, width, ps);
}

// x [count][2][nlimbs][n] <- (c0 [count][nlimbs][n], the samples of ps): no
// key, no private stream, no workspace; chunks only for the grid's limits
extern "C" void he_expand_seeded_batch(uint64_t *x, const uint64_t *c0, size_t count, unsigned int nlimbs,
                                       const gpqhe_pubseed_t *ps)
{
  HPROF("expand_seeded_batch");
  const char *who = "he_expand_seeded_batch";
  check_ctx();
  if (nlimbs < 1 || nlimbs > G.L)
    gpqhe_die("%s: bad level %u", who, nlimbs);
  const ChachaKey pub = seeded_key(who, ps, count);
  if (!count)
    return;
  if (!x || !c0)
    gpqhe_die("%s: null argument", who);
  const size_t w = (size_t)nlimbs * G.n;
  const uintptr_t xa = (uintptr_t)x, ca = (uintptr_t)c0;
  if (xa < ca + 8 * count * w && ca < xa + 16 * count * w)
    gpqhe_die("%s: x overlaps c0", who);
  const size_t chunk = io_chunk(count, 1, 16384);
  for (size_t i0 = 0; i0 < count; i0 += chunk)
    k_seeded_expand(x + i0 * 2 * w, c0 + i0 * w, pub, ps->stream + i0, nlimbs, (unsigned)std::min(chunk, count - i0));
}

// The folded path (k_dec_fold, k_fold_decode) reads each ciphertext once and
// transforms 2 slots points per limb; it needs a gap n / 2 slots >= 2 and the
// one-workgroup decoder.  Otherwise, and under GPQHE_DCD_FOLD=0: c0 + c1 s of
// the chunk, its inverse transforms, and the single call's decoder per
// ciphertext.  Same doubles either way.
//
// P = 0: z [count][s].  P > 0 (the packed form, s = P loops' slots): z
// [count][P][rows], slot k P + p of ciphertext c into z[c][p][k], k < rows --
// up to GPQHE_DCD_ONEPASS slots by the decoders' epilogue, so only those values
// reach pinned memory; above it a gather of the chunk's decoded slots into a
// compact device buffer, copied once.
static void dec_dcd_run(const char *who, gpqhe_complex_t z[], const uint64_t *y, size_t count, unsigned nl,
                        double scale, unsigned s, const poly_mpi_t *sk, unsigned P, unsigned rows)
{
  io_check(who, nl, s);
  if (!sk || !sk->data || sk->nlimbs < nl)
    gpqhe_die("%s: no secret key at level %u", who, nl);
  if (!count)
    return;
  if (!y || !z)
    gpqhe_die("%s: null argument", who);
  const size_t zw = P ? (size_t)P * rows : s;  // a ciphertext's values of z
  const size_t n = G.n, w = (size_t)nl * n, zb = zw * 16;
  const bool fold = env_u("GPQHE_DCD_FOLD", 1) != 0 && s <= GPQHE_DCD_ONEPASS && 2 * (size_t)s < n;
  // up to GPQHE_DCD_ONEPASS slots the decoder writes each value once: straight
  // into pinned host memory (up to 64 MiB of it)
  const bool pinned = s <= GPQHE_DCD_ONEPASS && count * zb <= ((size_t)64 << 20);
  const bool gather = P && s > GPQHE_DCD_ONEPASS;
  Ws zdev(pinned ? 0 : 2 * zw * count);
  double *zd = pinned ? (double *)zpin(count * zb) : (double *)zdev.p;
  const size_t chunk = io_chunk(count, (fold ? 4 * (size_t)nl * s : w) + (gather ? 2 * (size_t)s : 0), 16384);
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const unsigned cnt = (unsigned)std::min(chunk, count - c0);
    const uint64_t *yc = y + c0 * 2 * w;
    double *zc = zd + 2 * c0 * zw;
    if (fold) {
      const size_t fw = 2 * (size_t)s * nl * cnt;
      Ws F(fw), D(fw);
      k_dec_fold(F.p, yc, sk->data, s, nl, cnt);
      if (P)
        k_fold_decode_packed(zc, D.p, F.p, nl, s, scale, cnt, P, rows);
      else
        k_fold_decode(zc, D.p, F.p, nl, s, scale, cnt);
    } else {
      Ws pt(cnt * w), full(gather ? 2 * (size_t)s * cnt : 0);
      k_dec_batch(pt.p, yc, sk->data, nl, cnt);
      ntt_polys(pt.p, cnt, nl, true);
      for (unsigned i = 0; i < cnt; i++)
        if (gather)
          k_decode((double *)full.p + 2 * (size_t)s * i, pt.p + i * w, nl, s, scale);
        else if (P)
          k_decode_packed(zc + 2 * zw * i, pt.p + i * w, nl, s, scale, P, rows);
        else
          k_decode(zc + 2 * (size_t)s * i, pt.p + i * w, nl, s, scale);
      if (gather)
        k_pack_dcd_gather(zc, (const double *)full.p, s, P, rows, cnt);
    }
  }
  if (!pinned)
    HIP_CHECK(hipMemcpyAsync(z, zd, count * zb, hipMemcpyDeviceToHost, G.stream));
  HIP_CHECK(hipStreamSynchronize(G.stream));
  if (pinned)
    memcpy(z, g_zpin, count * zb);
}

extern "C" void he_dec_dcd_batch(gpqhe_complex_t z[], const uint64_t *y, size_t count, unsigned int nlimbs,
                                 double scale, unsigned int slots, const poly_mpi_t *sk)
{
  HPROF("dec_dcd_batch");
  check_ctx();
  dec_dcd_run("he_dec_dcd_batch", z, y, count, nlimbs, scale, slots, sk, 0, 0);
}

extern "C" void he_dec_dcd_packed_batch(gpqhe_complex_t z[], const uint64_t *y, size_t count, unsigned int nlimbs,
                                        double scale, unsigned int s, unsigned int rows, const poly_mpi_t *sk)
{
  HPROF("dec_dcd_packed_batch");
  check_ctx();
  const unsigned P = rows_loops("he_dec_dcd_packed_batch", s, rows, 1);
  // (one loop read whole: z is the decoded vector)
  dec_dcd_run("he_dec_dcd_packed_batch", z, y, count, nlimbs, scale, G.slots, sk, P == 1 && rows == s ? 0 : P, rows);
}

// ---------------------------------------------------------------------------
// he_enc_gain_packed_batch / he_gemv2_encgain_packed_batch /
// he_hempc_step_encgain_packed_batch (include/gpqhe_ext_encgain_batch.h): the
// packed row-folded step whose 2 m' extended diagonals arrive encrypted.  The
// products are ciphertext x ciphertext, but their tensor terms are summed
// before anything else happens to them (encgain_batch.hip), so a ciphertext
// costs 2 (m' - 1) baby rotations, one rescale of the linear part, ONE
// relinearisation of the summed quadratic part (mul_chunk on (0, X2) x (0, 1):
// its tensor is (0, 0, X2)) and the fold: one key switch more than the packed
// step, whatever m'.  Nothing is encoded, so there is no plan.
// ---------------------------------------------------------------------------
// every E_i of M, the all-zero ones too (which diagonals vanish stays with the
// client), as enc_pk_run / enc_sk_run read them: [m'][S] complex values
static std::vector<double> gain_diags(const char *who, const gpqhe_complex_t M[], unsigned s, unsigned rows,
                                      unsigned nmat, unsigned nlimbs, unsigned &mp)
{
  check_ctx();
  rows_loops(who, s, rows, nmat);
  io_check(who, nlimbs, G.slots);
  if (!M)
    gpqhe_die("%s: null argument", who);
  mp = rows_pow2(rows);
  std::vector<double> E(2 * (size_t)mp * G.slots), v(2 * (size_t)G.slots);
  for (unsigned i = 0; i < mp; i++) {
    rows_diag(v, (const double *)M, i, rows, mp, s, nmat);
    std::copy(v.begin(), v.end(), E.begin() + 2 * (size_t)i * G.slots);
  }
  return E;
}

extern "C" void he_enc_gain_packed_batch(uint64_t *D, const gpqhe_complex_t M[], unsigned int s, unsigned int rows,
                                         unsigned int nmat, unsigned int nlimbs, const he_pk_t *pk)
{
  HPROF("enc_gain_packed_batch");
  const char *who = "he_enc_gain_packed_batch";
  unsigned mp;
  const std::vector<double> E = gain_diags(who, M, s, rows, nmat, nlimbs, mp);
  enc_pk_run(who, D, (const gpqhe_complex_t *)E.data(), mp, G.slots, (double)G.q[nlimbs - 1], nlimbs, pk, 0, 0);
}

extern "C" void he_enc_gain_sk_packed_batch(uint64_t *D, const gpqhe_complex_t M[], unsigned int s, unsigned int rows,
                                            unsigned int nmat, unsigned int nlimbs, const poly_mpi_t *sk)
{
  HPROF("enc_gain_sk_packed_batch");
  const char *who = "he_enc_gain_sk_packed_batch";
  unsigned mp;
  const std::vector<double> E = gain_diags(who, M, s, rows, nmat, nlimbs, mp);
  enc_sk_run(who, D, (const gpqhe_complex_t *)E.data(), mp, G.slots, (double)G.q[nlimbs - 1], nlimbs, sk, 0, 0);
}

extern "C" void he_enc_gain_sk_seeded_packed_batch(uint64_t *D0, const gpqhe_complex_t M[], unsigned int s,
                                                   unsigned int rows, unsigned int nmat, unsigned int nlimbs,
                                                   const poly_mpi_t *sk, gpqhe_pubseed_t *ps)
{
  HPROF("enc_gain_sk_seeded_packed_batch");
  const char *who = "he_enc_gain_sk_seeded_packed_batch";
  unsigned mp;
  const std::vector<double> E = gain_diags(who, M, s, rows, nmat, nlimbs, mp);
  enc_sk_seeded_run(who, D0, (const gpqhe_complex_t *)E.data(), mp, G.slots, (double)G.q[nlimbs - 1], nlimbs, sk, 0,
                    0, ps);
}

// One chunk of cnt ciphertexts.  W: 2 (m' - 1) + 3 (+ 2 with st) slots of cnt
// ciphertexts at level lvl -- the rotated inputs, then X01 (later quad), Q
// (0, X2), the ones (later the fold's rotated copy), then the step's two
// differences.
static void encgain_chunk(uint64_t *y, const uint64_t *DA, const uint64_t *DB, const uint64_t *xa, const uint64_t *xb,
                          const StepIn *st, unsigned cnt, unsigned lvl, unsigned mp, const BsgsKeys &kb,
                          const std::vector<unsigned> &fold, const he_evk_t rk[], const he_evk_t *rlk, size_t budget)
{
  const size_t n = G.n, pw = (size_t)lvl * n, cw = 2 * pw, sw = (size_t)cnt * cw;
  Ws W((2 * (size_t)(mp - 1) + 3 + (st ? 2 : 0)) * sw);
  uint64_t *Ra = W.p, *Rb = Ra + (mp - 1) * sw, *X01 = Rb + (mp - 1) * sw, *Q = X01 + sw, *one = Q + sw;
  if (st) {
    uint64_t *xd = one + sw, *ud = xd + sw;
    k_step_diff_batch(xd, ud, st->xhat, st->xr, st->uhat, st->ur, lvl, cnt);
    xa = xd;
    xb = ud;
  }
  // the baby rotations i P, 1 <= i < m', of each operand
  bsgs_baby_chunk(Ra, xa, cnt, lvl, kb, rk, budget);
  bsgs_baby_chunk(Rb, xb, cnt, lvl, kb, rk, budget);
  k_encgain_tensor(X01, Q, xa, xb, Ra, Rb, DA, DB, mp, lvl, cnt);
  // lin: the rescale of (X0, X1) into y; quad: (0, X2) x (0, 1) relinearised
  // and rescaled into X01's place, which the rescale has read
  k_moddown(y, (size_t)(lvl - 1) * n, X01, pw, 2 * cnt, lvl, 2);
  k_encgain_ones(one, lvl, cnt);
  uint64_t *quad = X01, *R = one;
  mul_chunk(quad, (size_t)(lvl - 1) * n, Q, one, cw, pw, cnt, lvl, rlk, true);
  k_rows_fold_add_batch(y, quad, lvl - 1, cnt);
  fold_tail_chunk(y, R, st, fold, cnt, lvl, rk);
}

// The run of both cloud-side entry points: argument checks, then keys, then
// the first launch.
static void encgain_run(const char *who, uint64_t *y, const uint64_t *DA, const uint64_t *DB, const uint64_t *xa,
                        const uint64_t *xb, const StepIn *st, size_t count, unsigned lvl, const he_evk_t rk[],
                        const he_evk_t *rlk, unsigned sl, unsigned rows)
{
  batch_check(who, y, xa, xb, st, count, lvl);
  const unsigned P = rows_loops(who, sl, rows, 1);
  if (!rlk || !rlk->data || rlk->dnum != G.dnum)
    gpqhe_die("%s: relinearization key missing or built for another dnum", who);
  const unsigned mp = rows_pow2(rows), nm = lvl + G.K, ndig = (lvl + G.alpha - 1) / G.alpha;
  const size_t pw = (size_t)lvl * G.n, in_words = 2 * pw, out_words = 2 * (size_t)(lvl - 1) * G.n;
  if (!count)
    return;
  if (!y || !DA || !DB)
    gpqhe_die("%s: null argument", who);
  for (const uint64_t *d : {DA, DB})
    if (y < d + mp * in_words && d < y + count * out_words)
      gpqhe_die("%s: output overlaps a diagonal", who);

  // every key is found before anything is launched
  std::vector<unsigned> baby, fold;
  for (unsigned i = 1; i < mp; i++)
    baby.push_back(i * P);
  for (unsigned r = mp; r < sl; r <<= 1)
    fold.push_back(r * P);
  const BsgsKeys kb = bsgs_find_keys(baby, {}, 1, rk);
  for (unsigned r : fold)
    find_rot_key(rk, r, galois_of_rot(r));

  // a ciphertext's share of a chunk: the slots of encgain_chunk, and the larger
  // of the multiply's workspace (he_mul_rescale_batch's count) and, on the
  // windowed path, k_gemv_batch's
  const size_t mul_ws = (k_mul_split_ok(lvl) ? (size_t)lvl + (size_t)ndig * nm + 2 * (G.K + 1) + 2 * (size_t)lvl
                                             : 6 * (size_t)lvl + (size_t)ndig * nm + 2 * (size_t)nm)
                        << G.logn;
  const size_t rot_ws = gemv_win_on(lvl) ? k_gemv_batch_ws_words(lvl) : 0;
  const size_t per_ct = (2 * (size_t)(mp - 1) + 3 + (st ? 2 : 0)) * 2 * pw + std::max(mul_ws, rot_ws);
  // (65535: the multiply's launch grid)
  const size_t cap = std::min<size_t>(16384, 65535 / (ndig * nm));
  const size_t chunk = batch_chunk_size(count, per_ct, cap, "GPQHE_BSGS_CHUNK");
  batch_chunks(y, xa, xb, st, count, lvl, chunk,
               [&](uint64_t *yc, const uint64_t *xac, const uint64_t *xbc, const StepIn *sc, unsigned cnt) {
                 encgain_chunk(yc, DA, DB, xac, xbc, sc, cnt, lvl, mp, kb, fold, rk, rlk, bsgs_budget());
               });
}

extern "C" void he_gemv2_encgain_packed_batch(uint64_t *y, const uint64_t *DA, const uint64_t *xa, const uint64_t *DB,
                                              const uint64_t *xb, size_t count, unsigned int nlimbs,
                                              const he_evk_t rk[], const he_evk_t *rlk, unsigned int s,
                                              unsigned int rows)
{
  HPROF("gemv2_encgain_packed_batch");
  encgain_run("he_gemv2_encgain_packed_batch", y, DA, DB, xa, xb, nullptr, count, nlimbs, rk, rlk, s, rows);
}

extern "C" void he_hempc_step_encgain_packed_batch(uint64_t *up, const uint64_t *DA, const uint64_t *DB,
                                                   const uint64_t *xhat, const uint64_t *xr, const uint64_t *uhat,
                                                   const uint64_t *ur, size_t count, unsigned int nlimbs,
                                                   const he_evk_t rk[], const he_evk_t *rlk, unsigned int s,
                                                   unsigned int rows)
{
  HPROF("hempc_step_encgain_packed_batch");
  const StepIn st{xhat, xr, uhat, ur};
  encgain_run("he_hempc_step_encgain_packed_batch", up, DA, DB, nullptr, nullptr, &st, count, nlimbs, rk, rlk, s, rows);
}

// groups of ~224 MiB (ntt_batch), at most 65535 limbs a launch
static size_t ntt_group_polys(unsigned nlimbs)
{
  static const size_t group_mib = env_u("GPQHE_NTT_GROUP_MIB", 224);
  return std::max<size_t>(1, std::min<size_t>(65535 / nlimbs, (group_mib << 20) / ((size_t)nlimbs * G.n * 8)));
}

static void ntt_batch(uint64_t *data, size_t npolys, unsigned nlimbs, bool inverse)
{
  check_ctx();
  // groups of ~224 MiB: a group's column-pass output is still in the 256 MB
  // Infinity Cache when its row pass reads it (config 2, 1024 polys x 8 limbs
  // at N=2^16: roundtrip 8.41 -> 7.84 ms; 32-64 MiB groups lose more to
  // launch gaps than they gain).  Sweep (scripts/gpu_ntt_group.sh, same box,
  // ms): 96 7.46-7.56, 160 7.20-7.26, 192 6.84-6.92, 224 6.62-6.82, 240
  // 6.76-6.77, 256 6.72-7.04, 320 7.24, 512 7.42, whole batch 7.31-7.34.
  // (GPQHE_NTT_GROUP_MIB: the group size for sweeps)
  const size_t per = ntt_group_polys(nlimbs);
  // the inverse walks the groups from the last one (GPQHE_NTT_REV): after a
  // forward batch, its last group's output is what the Infinity Cache holds
  static const bool rev = env_u("GPQHE_NTT_REV", 1) != 0;
  const size_t ngroups = (npolys + per - 1) / per;
  for (size_t i = 0; i < ngroups; i++) {
    const size_t g = inverse && rev ? ngroups - 1 - i : i, p0 = g * per;
    const unsigned cnt = (unsigned)std::min(per, npolys - p0);
    k_ntt(qlimbs(data + p0 * nlimbs * G.n, nlimbs, cnt, (size_t)nlimbs * G.n), inverse);
  }
}

extern "C" void poly_ntt_batch(uint64_t *data, size_t npolys, unsigned int nlimbs)
{
  ntt_batch(data, npolys, nlimbs, false);
}

extern "C" void poly_intt_batch(uint64_t *data, size_t npolys, unsigned int nlimbs)
{
  ntt_batch(data, npolys, nlimbs, true);
}

extern "C" void poly_fill_uniform(uint64_t *data, size_t npolys, unsigned int nlimbs, uint64_t seed)
{
  check_ctx();
  k_fill_uniform(data, npolys, nlimbs, seed);
}
