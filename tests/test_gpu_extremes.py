"""Product (libgpqhe.so on MI355X) vs oracle, bit for bit, on constructed
residues at the edges of the canonical range and under crafted switching keys
(tests/extreme_inputs.py).

The hot path's accumulating kernels are correct by worst-case bound arguments
written in their comments; uniform residues, genuine encryptions and sampled
keys stay far inside those bounds.  he_import places any canonical words in a
ciphertext or in a key (the product re-derives the key's Montgomery shadow and
bumps the key generation, api.cpp:1280-1283), so the words the bounds speak of
-- 0, 1, q - 1, +-(q - 1)/2 -- are put there directly, and "pulled back" through
the oracle's forward NTT so that the inverse transforms inside ModUp, rescale
and ModDown hand exactly those words to the basis conversions.

Every residue of every output is compared.  The pattern, key and matrix lists
are fixed here; only the rand_* patterns are drawn, from fixed seeds.
"""
import ctypes

import numpy as np
import pytest

from tests import extreme_inputs as X
from tests.bsgs_ref import bsgs_compose
from tests.test_gpu_parity import PARAMS, init_both, keys, same
from tests.test_gpu_rotations import init_slots, rot_keys, run_batch, sample_matrix

pytestmark = pytest.mark.gpu


def differ(got, want, what):
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} residues differ, first at word {bad[0]}"


def import_key(e, evk, payload):
    """payload over a generated key (its galois / dnum fields and layout stay)."""
    e.import_(evk, payload, e.L + e.K, evk.scale, evk.flags)


# ------------------------------------------------------------- a. transforms
@pytest.mark.parametrize("name", ["f13", "c14", "f15", "bench51", "c17", "c15", "bench"])
def test_transforms_on_patterns(oracle, product, name):
    """poly_ntt_batch / poly_intt_batch on one batch holding every pattern on
    every limb, direct and pulled back, padded by two mixed polynomials to 24
    (the multi-poly row pass), and on a 4-polynomial subset (one tile per
    workgroup); forward and inverse are each run on the batch itself and each
    compared with the oracle.  FP64 limbs below 2^50 (lazy stage reduction,
    ntt_device.h F64_LAZY), 51-bit FP64 limbs (reduced every stage) and, on
    c15 / bench, 60-bit integer limbs.
    A smoke case for the butterflies' own bounds, not a worst case: the
    twiddle products randomise the signs, and a float-exact emulation of the
    lazy forward chain peaks near 1.54 q for uniform, +-q/2 and {0, q - 1}
    inputs alike.  What it does pin is the edge words themselves (0, q - 1 and
    the centring at +-(q - 1)/2 on load, the canonical range on store)."""
    import torch
    init_both(oracle, product, name)
    n, L = product.n, product.L
    primes = product.primes[:L]
    direct = np.stack([X.poly([nm] * L, primes, n, seed=k) for k, nm in enumerate(X.NAMES)])
    batch = np.concatenate([direct, X.pullback(oracle, direct, L), X.mixed(0, primes, n), X.mixed(1, primes, n)])
    assert batch.shape == (24, L, n)
    sub = np.ascontiguousarray(batch[[2, 4, 13, 22]])  # qm1, half_hi, pulled-back qm1, mixed
    for arr in (batch, sub):
        for fn in ("poly_ntt_batch", "poly_intt_batch"):
            host = arr.copy()
            getattr(oracle.lib, fn)(host.ctypes.data, len(arr), L)
            dev = torch.from_numpy(arr.view(np.int64)).cuda()
            torch.cuda.synchronize()
            getattr(product.lib, fn)(dev.data_ptr(), len(arr), L)
            product.sync()
            differ(dev.cpu().numpy().view(np.uint64), host, f"{fn} of {len(arr)} polys")
            del dev


# ------------------------------------------- b. multiply under crafted keys
MUL_PAIRS = [("qm1", "qm1"), ("half_lo", "half_hi"), ("rand_half", "rand_half"), ("rand_edge", "alt_qm1"),
             ("mixed0", "mixed1"), ("pb:qm1", "one"), ("pb:rand_half", "one"), ("pb:mixed2", "pb:half_hi")]


@pytest.mark.parametrize("name,lvl", [("f13", None), ("bench51", None), ("m60", None), ("c15", None), ("c5f", None),
                                      ("a5", None), ("k5", None), ("i14", None), ("bench51", 6), ("bench51", 3)])
def test_mul_rescale_batch_crafted_keys(oracle, product, name, lvl):
    """he_mul_rescale_batch of the 8 MUL_PAIRS under the genuine
    relinearisation key and under keys whose L + K limbs and 2 dnum
    polynomials are all one / q - 1 / (q - 1)/2 / a seeded +-(q - 1)/2 mix, or
    one on digit 0 and zero on the others (a limb's accumulator then sees only
    its own controllable digit word).
    Aimed at: the tensor step's data x data FP64 products (kernels.hip:862,
    901-905, 943-946: q - 1 x q - 1, +-(q - 1)/2 products); the split key
    switch's FP64 accumulators "|.| < 3 q before each fold" (ks_split.hip:224)
    and the [0, 2q) lazy Montgomery accumulators (kernels.hip:2480-2489,
    ks_split.hip:185-188) with every key word at an extreme; the fast basis
    conversion's "sums of up to three terms stay below 2^53; longer sums are
    reduced in between" (ntt_device.h:385-389) -- the pairs (pb:X, one) make
    d2 = NTT(X), so ModUp's inverse transform hands the conversion exactly X
    (a5: one 5-limb digit, the longer sums; c5f: three digits; bench51 at
    levels 6 and 3: partial digits); the integer forms at 60- and 61-bit
    moduli (m60, c15, i14).  The rescale / ModDown inputs are sums of key
    products and not placed word by word; with the digit-0 key and (pb:X,
    one) they are P d0 + X-derived words only.
    The transforms inside are a smoke case, as in test_transforms_on_patterns."""
    import torch
    init_both(oracle, product, name)
    n, L, K = product.n, product.L, product.K
    lvl = lvl or L
    primes = product.primes[:lvl]
    pk_o, sk_o, _, rlk_o = keys(oracle, rot=False)
    pk_p, sk_p, _, rlk_p = keys(product, rot=False)
    cnt = len(MUL_PAIRS)
    a = np.concatenate([X.spec_ct(oracle, sa, primes, n, seed=2 * i).ravel() for i, (sa, _) in enumerate(MUL_PAIRS)])
    b = np.concatenate([X.spec_ct(oracle, sb, primes, n, seed=2 * i + 1).ravel() for i, (_, sb) in enumerate(MUL_PAIRS)])
    da = torch.from_numpy(a.view(np.int64)).cuda()
    db = torch.from_numpy(b.view(np.int64)).cuda()
    out_words = cnt * 2 * (lvl - 1) * n
    for kind in X.KEY_KINDS:
        payload = X.key_payload(kind, product.primes, n, rlk_p.dnum, seed=5)
        if payload is not None:
            import_key(oracle, rlk_o, payload)
            import_key(product, rlk_p, payload)
        same(oracle, product, rlk_o, rlk_p)
        want = np.full(out_words, 7, dtype=np.uint64)
        oracle.lib.he_mul_rescale_batch(want.ctypes.data, a.ctypes.data, b.ctypes.data, cnt, lvl, ctypes.byref(rlk_o))
        dout = torch.full((out_words,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        product.lib.he_mul_rescale_batch(dout.data_ptr(), da.data_ptr(), db.data_ptr(), cnt, lvl, ctypes.byref(rlk_p))
        product.sync()
        got = dout.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"key {kind}: {bad.size} residues differ, first in pair "
                               f"{MUL_PAIRS[bad[0] // (2 * (lvl - 1) * n)]}")
        for i, q in enumerate(primes[:lvl - 1]):  # canonical outputs
            assert int(got.reshape(cnt, 2, lvl - 1, n)[:, :, i].max()) < q
        del dout
    del da, db
    for e, objs in ((oracle, (pk_o, sk_o, rlk_o)), (product, (pk_p, sk_p, rlk_p))):
        for o in objs:
            e.free(o)


# ------------------------------- c. rotations and gemv under crafted keys
GEMV_CTS = ["one", "qm1", "pb:qm1", "rand_half", "mixed3"]


def gemv_matrices(s):
    return {"half": X.circulant(s, [0.5]), "alt": X.circulant(s, [0.5, -0.5]),
            "sparse": X.circulant(s, [0.5, 0.0, 0.0]), "sample": sample_matrix(s, 9)}


#: the matrices each key kind runs with (every kind runs both rotations)
GEMV_PLAN = {"genuine": ("sample", "half"), "one": ("half", "alt", "sparse"), "qm1": ("half", "sample"),
             "half_lo": ("half", "alt"), "rand_half": ("alt", "sample"), "digit0": ("half", "sparse")}


@pytest.mark.parametrize("name,slots,ncts", [("bench51", 16, 5), ("c5f", 16, 3), ("bench_d2", 16, 5), ("i14", 16, 5),
                                             ("f13", 64, 5)])
def test_gemv_rot_batch_crafted_keys(oracle, product, name, slots, ncts):
    """he_rot_batch (r = 1 and slots - 1) and he_gemv_batch over the first
    ncts GEMV_CTS pattern ciphertexts, with rk[1..slots-1] generated and then
    overwritten by each key payload (GEMV_PLAN pairs the payloads with the
    matrices; the galois / dnum fields and the layout stay the product's own).
    Aimed at the windowed inner product (gemv_win.hip:298-309):
    * LZ form (bench51, f13: FP64 slots below 2^50, two digits): accumulators
      reduced every third diagonal, "three diagonals of two products ... on
      top of |acc| <= q/2 stay below 4.7 q < 2^52.3".  A constant diagonal c
      encodes at scale q_top to the constant word round(c q_top), which on the
      top limb is the centred extreme +-(q_top -+ 1)/2; folded into a key of
      ones the key word is that extreme at every index, and against data
      words of +-1 (one, qm1) every product of the own digit is +-(q - 1)/2
      with one sign ("half"), alternating signs ("alt"), or one diagonal in
      three ("sparse": the reduction falls between different diagonals).  The
      other digit's ModUp words are not placed; the digit-0 key silences
      them.  f13 at 64 slots runs 21 groups of three diagonals.
    * C0IN and three digits (c5f): three products and the c0 term ("6.9 q <
      2^52.8") -- the same constructions, not LZ.
    * integer form (bench_d2 60-bit, i14 61-bit q0 / P): "at most ndig + 1 <=
      4 products of residues below q < 2^61" summed in 128 bits before one
      REDC: q - 1 key words on q - 1 data (key qm1 on ct qm1), the largest
      sum there is.
    The rotations' ModUp gets exactly q - 1 words from the pulled-back
    ciphertext (ntt_device.h:385-389)."""
    init_slots(oracle, product, name, slots, seed=31)
    s, n, lvl = slots, product.n, product.L
    ko, kp = rot_keys(oracle), rot_keys(product)
    specs = GEMV_CTS[:ncts]
    host = np.concatenate([X.spec_ct(oracle, sp, product.primes[:lvl], n, seed=i).ravel() for i, sp in enumerate(specs)])
    mats = {k: np.ascontiguousarray(M.ravel(), dtype=np.complex128) for k, M in gemv_matrices(s).items()}
    for kind in X.KEY_KINDS:
        payload = X.key_payload(kind, product.primes, n, kp[2][1].dnum, seed=3)
        if payload is not None:
            for r in range(1, s):
                import_key(oracle, ko[2][r], payload)
                import_key(product, kp[2][r], payload)
                assert kp[2][r].galois == ko[2][r].galois == pow(5, r, 2 * n)
        for r in (1, s - 1):
            want, got = run_batch(oracle, product, ko[2], kp[2], "he_rot_batch", host, ncts * 2 * lvl * n,
                                  "IN", ncts, lvl, r)
            differ(got, want, f"key {kind}, rot {r}")
        for m in GEMV_PLAN[kind]:
            want, got = run_batch(oracle, product, ko[2], kp[2], "he_gemv_batch", host, ncts * 2 * (lvl - 1) * n,
                                  mats[m].ctypes.data, "IN", ncts, lvl)
            differ(got, want, f"key {kind}, matrix {m}")
    for e, k in ((oracle, ko), (product, kp)):
        e.free_evks(k[2])
        e.free(k[0])
        e.free(k[1])


def test_ref_gemv_rot_bsgs_crafted_keys(oracle, product):
    """HECTR's own ring (n = 4096, L = 2: the fused small-N path): he_rot,
    he_gemv and he_gemv_bsgs (g = 4, against bsgs_compose on the oracle) of
    imported pattern ciphertexts under each key payload.  The same
    constructions as test_gemv_rot_batch_crafted_keys on the generic integer
    kernels (60-bit q0 / P: [0, 2q) accumulators, kernels.hip:2480-2489)."""
    init_both(oracle, product, "ref")
    s, n, L = product.slots, product.n, product.L
    ko, kp = rot_keys(oracle), rot_keys(product)
    mats = gemv_matrices(s)
    cts = {}
    for e in (oracle, product):
        cts[e.name] = []
        for i, sp in enumerate(("qm1", "one", "pb:rand_half")):
            c = e.ct()
            e.import_(c, X.spec_ct(oracle, sp, product.primes[:L], n, seed=i), L, scale=product.info.delta)
            cts[e.name].append(c)
    for kind in X.KEY_KINDS:
        payload = X.key_payload(kind, product.primes, n, kp[2][1].dnum, seed=3)
        if payload is not None:
            for r in range(1, s):
                import_key(oracle, ko[2][r], payload)
                import_key(product, kp[2][r], payload)
        for i in range(3):
            xo, xp = cts["oracle"][i], cts["product"][i]
            outs = []
            for e, x, k in ((oracle, xo, ko), (product, xp, kp)):
                o = [e.ct() for _ in range(2 + len(GEMV_PLAN[kind]))]
                e.rot(o[0], x, 1, k[2])
                e.rot(o[1], x, s - 1, k[2])
                for y, m in zip(o[2:], GEMV_PLAN[kind]):
                    e.gemv(y, mats[m].ravel(), x, k[2])
                outs.append(o)
            yo = bsgs_compose(oracle, mats["alt"], xo, ko[2], 4)
            yp = product.ct()
            product.gemv_bsgs(yp, mats["alt"], xp, kp[2], 4)
            outs[0].append(yo)
            outs[1].append(yp)
            for a, b in zip(*outs):
                assert a.nlimbs == b.nlimbs and a.scale == b.scale
                same(oracle, product, a, b)
            for e, o in zip((oracle, product), outs):
                for c in o:
                    e.free(c)
    for e, k in ((oracle, ko), (product, kp)):
        for c in cts[e.name]:
            e.free(c)
        e.free_evks(k[2])
        e.free(k[0])
        e.free(k[1])


# ----------------------------------- d. single-ciphertext ops above n = 2^13
def single_ops(e, a, b, pt, rlk, drop):
    """The single-ciphertext entry points on (a, b, pt), all at one level;
    `drop` he_moddown calls first bring copies of them to a partial-digit
    level.  Returns {op: ciphertext}; the caller frees them."""
    def cp(x, down=drop):
        c = e.ct()
        e.copy_ct(c, x)
        for _ in range(down):
            e.moddown(c)
        return c
    a2, b2 = cp(a), cp(b)
    out = {"copy": a2}
    c = e.ct(); e.mul(c, a2, b2, rlk); out["mul"] = c
    c = e.ct(); e.mul_rescale(c, a2, b2, rlk); out["mul_rescale"] = c
    c = cp(a); e.mul_rescale(c, c, b2, rlk); out["mul_rescale_inplace"] = c
    c = e.ct(); e.mul(c, a2, b2, rlk); e.rescale(c); out["mul_then_rescale"] = c
    c = cp(a); e.rescale(c); out["rescale"] = c
    c = e.ct(); e.mul_pt(c, a2, pt); out["mul_pt"] = c
    c = e.ct(); e.add_pt(c, a2, pt); out["add_pt"] = c
    lower = cp(b, drop + 1)
    c = e.ct(); e.add(c, a2, lower); out["add_mixed"] = c
    c = e.ct(); e.sub(c, lower, a2); out["sub_mixed"] = c
    c = cp(a); e.neg(c); out["neg"] = c
    e.free(b2)
    e.free(lower)
    return out


@pytest.mark.parametrize("name,drop", [("c14", 0), ("c14", 2), ("c15", 0), ("c15", 2), ("bench51", 0), ("bench51", 3),
                                       ("bench_d2", 0), ("bench_d2", 3), ("c5f", 0), ("c5f", 5)])
def test_single_ops_large_n(oracle, product, name, drop):
    """he_mul, he_mul_rescale (also in place), he_mul then he_rescale,
    he_rescale alone, he_mul_pt, he_add_pt, he_add / he_sub of operands one
    level apart, he_neg and he_copy_ct at the tilings above n = 2^13, at the
    top level and `drop` he_moddown calls below it (a partial last digit), on
    genuine encryptions -- decoded within the suite's 1e-6 -- and on imported
    pattern ciphertexts and a pattern plaintext: q - 1 x q - 1 and pulled-back
    +-(q - 1)/2 operands.  Aimed at the stand-alone k_moddown behind
    he_rescale (kernels.hip:2322: the pulled-back ciphertext hands its
    inverse transform exactly +-(q - 1)/2 on the dropped limb), the tensor
    step's FP64 products (kernels.hip:862, 901-905, 943-946) and the
    elementwise kernels' edge words (q - 1 + q - 1, 0 - (q - 1), -0)."""
    init_both(oracle, product, name)
    n, L, s = product.n, product.L, product.slots
    lvl = L - drop
    rng = np.random.default_rng(11)
    z1 = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    z2 = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    z3 = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    primes = product.primes[:L]
    delta = product.info.delta
    pat = [(X.spec_ct(oracle, "qm1", primes, n), X.spec_ct(oracle, "qm1", primes, n, seed=1),
            X.poly(["half_hi"] * L, primes, n)),
           (X.spec_ct(oracle, "pb:rand_half", primes, n, seed=2), X.spec_ct(oracle, "mixed4", primes, n),
            X.mixed(6, primes, n)[0])]
    res = {}
    for e in (oracle, product):
        pk, sk, _, rlk = keys(e, rot=False)
        runs = []
        a, b, pt = e.encrypt(z1, pk), e.encrypt(z2, pk), e.pt()
        e.ecd_ex(pt, z3, s, delta, lvl)
        runs.append(single_ops(e, a, b, pt, rlk, drop))
        for pa, pb, pp in pat:
            e.import_(a, pa, L, scale=delta)
            e.import_(b, pb, L, scale=delta)
            e.import_(pt, pp[None, :lvl], lvl, scale=delta)
            runs.append(single_ops(e, a, b, pt, rlk, drop))
        res[e.name] = (runs, sk)
        for o in (a, b, pt, pk, rlk):
            e.free(o)
    for i, (ro, rp) in enumerate(zip(res["oracle"][0], res["product"][0])):
        for op in ro:
            assert ro[op].nlimbs == rp[op].nlimbs and ro[op].scale == rp[op].scale, (i, op)
            A, B = oracle.export(ro[op]), product.export(rp[op])
            differ(B, A, f"run {i}, {op}")
    out, sk = res["product"][0][0], res["product"][1]
    assert out["copy"].nlimbs == lvl and out["mul"].nlimbs == lvl and out["rescale"].nlimbs == lvl - 1
    assert out["add_mixed"].nlimbs == lvl - 1 == out["mul_rescale"].nlimbs
    expect = {"copy": z1, "mul": z1 * z2, "mul_rescale": z1 * z2, "mul_rescale_inplace": z1 * z2,
              "mul_then_rescale": z1 * z2, "mul_pt": z1 * z3, "add_pt": z1 + z3, "add_mixed": z1 + z2,
              "sub_mixed": z2 - z1, "neg": -z1}
    for op, want in expect.items():
        got = product.decrypt(out[op], sk)
        assert np.abs(got - want).max() < 1e-6 * max(1.0, np.abs(want).max()), op
    for e in (oracle, product):
        runs, sk = res[e.name]
        for r in runs:
            for c in r.values():
                e.free(c)
        e.free(sk)


@pytest.mark.parametrize("name", ["ref", "c1", "bench51"])
def test_enc_sk(oracle, product, name):
    """he_enc_sk: from the same seed the ciphertext equals the oracle's bit
    for bit (the uniform a, then the error: the oracle's sampler order is the
    definition), at the top level and one below, and he_dec of it decodes to
    the input within 1e-6."""
    init_both(oracle, product, name)
    s = product.slots
    rng = np.random.default_rng(23)
    zs = [rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s) for _ in range(2)]
    res = {}
    for e in (oracle, product):
        pk, sk = e.pk(), e.sk()
        e.keypair(pk, sk)
        cts = []
        for z, nl in zip(zs, (e.L, e.L - 1)):
            pt, ct = e.pt(), e.ct()
            e.ecd_ex(pt, z, s, e.info.delta, nl)
            e.enc_sk(ct, pt, sk)
            e.free(pt)
            cts.append(ct)
        res[e.name] = (cts, pk, sk)
    for z, co, cp, nl in zip(zs, res["oracle"][0], res["product"][0], (product.L, product.L - 1)):
        assert co.nlimbs == cp.nlimbs == nl and co.scale == cp.scale
        same(oracle, product, co, cp)
        assert np.abs(product.decrypt(cp, res["product"][2]) - z).max() < 1e-6
    for e in (oracle, product):
        cts, pk, sk = res[e.name]
        for o in cts + [pk, sk]:
            e.free(o)
