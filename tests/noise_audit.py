"""Audit functions shared by the CPU tests (on the oracle) and the GPU tests
(on the product): they take an engine's *exported* objects and check them
against the independent models (tests/ckks_model.py, tests/ckks_model_rng.py).
A helper, not a test.

The only engine code they lean on is he_export and the CPU engine's
poly_ntt_batch / poly_intt_batch on host arrays (pinned to the definition by
test_oracle_model.py and test_extremes_cpu.py); the product's objects are
transformed by the CPU engine too (use_host_transforms).

The batch entry points return raw word arrays, not objects, so the audits of
one ciphertext come in an array form (exact_decrypt_words, audit_enc_pk_words,
audit_enc_sk_words, audit_enc_sk_seeded_words) that the object forms call.
measure_step runs one step family -- the reference composition on the oracle,
the batch entry point on the product -- and returns its exact noise.
"""
import ctypes

import numpy as np

import bsgs_ref
import ckks_model as M
import ckks_model_rng as R


def mulmod(a, b, q):
    """Element-wise a b mod q on uint64 arrays, exact (Python integers)."""
    return ((np.asarray(a).astype(object) * np.asarray(b).astype(object)) % int(q)).astype(np.uint64)


def addmod(a, b, q):
    q = np.uint64(q)
    return (np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)) % q  # both < 2^61: no wrap


def submod(a, b, q):
    q = np.uint64(q)
    return (np.asarray(a, dtype=np.uint64) + (q - np.asarray(b, dtype=np.uint64))) % q


def use_host_transforms(engine, host):
    """Transform engine's exported words with host's poly_(i)ntt_batch.  The
    product's batch entry points take device-resident buffers (a host array
    handed to them is an illegal access on the GPU), so its exported objects
    are transformed by the CPU engine, initialised for the same moduli."""
    assert engine.primes == host.primes
    assert list(engine.info.psi[:len(engine.primes)]) == list(host.info.psi[:len(host.primes)])
    engine.audit_host = host


def _host(engine):
    host = getattr(engine, "audit_host", engine)
    assert host.name == "oracle", "host arrays need the CPU engine's transforms (use_host_transforms)"
    assert host.primes == engine.primes and host.n == engine.n
    return host


def intt(engine, arr):
    """Coefficient form of arr [..][nl][n] (limb i modulo the context's modulus i)."""
    out = np.ascontiguousarray(arr, dtype=np.uint64).copy()
    nl = out.shape[-2]
    _host(engine).lib.poly_intt_batch(out.ctypes.data, out.size // (nl * engine.n), nl)
    return out


def ntt(engine, arr):
    out = np.ascontiguousarray(arr, dtype=np.uint64).copy()
    nl = out.shape[-2]
    _host(engine).lib.poly_ntt_batch(out.ctypes.data, out.size // (nl * engine.n), nl)
    return out


def lift(small, primes):
    """[len(primes)][n] canonical residues of a small signed polynomial."""
    small = np.asarray(small, dtype=np.int64)
    return np.stack([np.where(small < 0, small + np.int64(q), small).astype(np.uint64) for q in primes])


def small_of(coef, primes, what):
    """The small signed polynomial whose residues coef [len(primes)][n] are:
    centred per limb, and the same integer on every limb."""
    c = [R.centred(coef[i], q) for i, q in enumerate(primes)]
    for i in range(1, len(c)):
        assert np.array_equal(c[i], c[0]), f"{what}: limb {i} lifts another integer than limb 0"
    return c[0]


def automorphism_small(a, g):
    """a(X) -> a(X^g) on a signed integer coefficient vector (numpy form of
    ckks_model.automorphism, without a modulus)."""
    a = np.asarray(a, dtype=np.int64)
    n = a.size
    e = (np.arange(n, dtype=np.int64) * int(g)) % (2 * n)
    out = np.zeros(n, dtype=np.int64)
    out[e % n] = np.where(e < n, a, -a)
    return out


def subset(n, count=512):
    """A fixed index subset with 0, 1, n/2 and n - 1 (all of 0..n-1 if n <= count)."""
    if n <= count:
        return np.arange(n)
    rest = np.random.default_rng(n).choice(np.arange(2, n - 1), count - 4, replace=False)
    return np.unique(np.concatenate([[0, 1, n // 2, n - 1], rest]))


class Streams:
    """The engine's stream counter: one fresh stream per sampled polynomial."""

    def __init__(self, seed, first=0):
        self.key = R.seed_key(seed)
        self.next = first

    def take(self):
        self.next += 1
        return self.next - 1


def secret_of(engine, sk):
    """The secret's signed coefficients, from all L + K limbs of the exported key."""
    s_ntt = engine.export(sk)[0]
    return small_of(intt(engine, s_ntt), engine.primes, "secret key"), s_ntt


def audit_keypair(engine, st, pk, sk, idx=None):
    """s, a and e of he_keypair against streams st.take() x 3.  Returns the
    recovered (s, e) and the secret in NTT form."""
    n, L = engine.n, engine.L
    idx = np.arange(n) if idx is None else idx
    s, s_ntt = secret_of(engine, sk)
    assert np.array_equal(s[idx], R.sample_ternary(st.key, st.take(), n, idx)), "secret key is not the model's ternary sample"
    p = engine.export(pk)
    assert p.shape == (2, L, n)
    sa = st.take()
    for m in range(L):
        want = R.sample_uniform(st.key, sa, n, m, engine.primes[m], L + engine.K, idx)
        assert np.array_equal(p[1, m][idx], want), f"pk.a limb {m} is not the model's uniform sample"
    e_ntt = np.stack([addmod(p[0, m], mulmod(p[1, m], s_ntt[m], q), q) for m, q in enumerate(engine.primes[:L])])
    e = small_of(intt(engine, e_ntt), engine.primes[:L], "pk error")
    assert np.array_equal(e[idx], R.sample_cbd(st.key, st.take(), n, idx)), "pk error is not the model's CBD sample"
    return s, e, s_ntt


def digit_ranges(L, alpha):
    return [(lo, min(lo + alpha, L)) for lo in range(0, L, alpha)]


def audit_evk(engine, st, evk, s, s_ntt, galois, idx=None, a_limbs=None):
    """Key structure and samplers of one evaluation key: for every digit j and
    every limb m of Q u P,
        INTT(b_j + a_j s - [m in digit j] (P mod q_m) s')   (s' = s^2 or s(X^g))
    is one small integer polynomial on all limbs, equal to the model's CBD
    sample, and a_j is the model's uniform sample (on the limbs a_limbs;
    default all).  Returns the recovered errors [dnum][n]."""
    n, L, K = engine.n, engine.L, engine.K
    primes = engine.primes
    nm = L + K
    idx = np.arange(n) if idx is None else idx
    alpha = engine.info.alpha
    digits = digit_ranges(L, alpha)
    k = engine.export(evk)
    assert k.shape == (2 * len(digits), nm, n), k.shape
    P = 1
    for p in primes[L:]:
        P *= p
    sp_coef = None if galois == 1 else automorphism_small(s, galois)
    errs = []
    for j, (lo, hi) in enumerate(digits):
        sa, se = st.take(), st.take()
        for m in (range(nm) if a_limbs is None else a_limbs):
            want = R.sample_uniform(st.key, sa, n, m, primes[m], nm, idx)
            assert np.array_equal(k[2 * j + 1, m][idx], want), f"evk a_{j} limb {m} is not the model's uniform sample"
        rows = []
        for m, q in enumerate(primes):
            x = addmod(k[2 * j, m], mulmod(k[2 * j + 1, m], s_ntt[m], q), q)
            if galois == 1 and lo <= m < hi:
                x = submod(x, mulmod(mulmod(s_ntt[m], s_ntt[m], q), np.uint64(P % q), q), q)
            rows.append(x)
        coef = intt(engine, np.stack(rows))
        if galois != 1:
            for m in range(lo, hi):
                q = primes[m]
                ps = mulmod(lift(sp_coef, [q])[0], np.uint64(P % q), q)
                coef[m] = submod(coef[m], ps, q)
        e = small_of(coef, primes, f"evk (galois {galois}) digit {j} error")
        assert np.abs(e).max() <= R.CBD_ETA
        assert np.array_equal(e[idx], R.sample_cbd(st.key, se, n, idx)), f"evk digit {j} error is not the model's CBD sample"
        errs.append(e)
    return errs


def audit_enc_pk_words(engine, st, words, m_ntt, pk_words, idx=None):
    """(v, e0, e1) of one public-key encryption, words [2][nl][n], of the
    plaintext words m_ntt [nl][n] under the exported public key pk_words,
    against three fresh streams: with the model's v, INTT(c1 - v a) and
    INTT(c0 - v b - m) must be the model's e1 and e0.  v itself is the model's:
    that c1 - v a is small at all (one integer of CBD size on every limb) shows
    it is the v the engine drew, a uniform a leaving no second small solution.
    Returns (v, e0, e1)."""
    n = engine.n
    c, p, m = (np.asarray(x, dtype=np.uint64) for x in (words, pk_words, m_ntt))
    lvl = c.shape[1]
    assert c.shape == (2, lvl, n) and m.shape == (lvl, n)
    primes = engine.primes[:lvl]
    idx = np.arange(n) if idx is None else idx
    v = R.sample_ternary(st.key, st.take(), n)
    s0, s1 = st.take(), st.take()
    v_ntt = ntt(engine, lift(v, primes))
    r0 = np.stack([submod(submod(c[0, i], mulmod(v_ntt[i], p[0, i], q), q), m[i], q) for i, q in enumerate(primes)])
    r1 = np.stack([submod(c[1, i], mulmod(v_ntt[i], p[1, i], q), q) for i, q in enumerate(primes)])
    e0 = small_of(intt(engine, r0), primes, "e0")
    e1 = small_of(intt(engine, r1), primes, "e1")
    assert np.array_equal(e0[idx], R.sample_cbd(st.key, s0, n, idx)), "e0 is not the model's CBD sample"
    assert np.array_equal(e1[idx], R.sample_cbd(st.key, s1, n, idx)), "e1 is not the model's CBD sample"
    return v, e0, e1


def audit_enc_pk(engine, st, ct, pt, pk, idx=None):
    """audit_enc_pk_words on the exported objects of one he_enc_pk."""
    return audit_enc_pk_words(engine, st, engine.export(ct), engine.export(pt)[0], engine.export(pk), idx)


def sk_error_of(engine, c0, a, m_ntt, s_ntt, what="e"):
    """The small polynomial INTT(c0 + a s - m) of a secret-key encryption: one
    integer on every limb (checked), |e| <= 21."""
    lvl = np.asarray(c0).shape[0]
    primes = engine.primes[:lvl]
    r = np.stack([submod(addmod(c0[i], mulmod(a[i], s_ntt[i], q), q), m_ntt[i], q) for i, q in enumerate(primes)])
    e = small_of(intt(engine, r), primes, what)
    assert np.abs(e).max() <= R.CBD_ETA, f"{what}: |e| reaches {np.abs(e).max()}"
    return e


def audit_enc_sk_words(engine, st, words, m_ntt, s_ntt, idx=None):
    """(a, e) of one secret-key encryption, words [2][nl][n], of the plaintext
    words m_ntt [nl][n] under the secret s_ntt, against two fresh streams: every
    limb of c1 is the model's uniform sample of the first, and
    INTT(c0 + c1 s - m) is one small integer on every limb, the model's CBD
    sample of the second, |e| <= 21.  Returns (c1 [nl][n], e)."""
    n = engine.n
    c = np.asarray(words, dtype=np.uint64)
    lvl = c.shape[1]
    assert c.shape == (2, lvl, n) and np.asarray(m_ntt).shape == (lvl, n)
    idx = np.arange(n) if idx is None else idx
    sa, se = st.take(), st.take()
    for m in range(lvl):
        want = R.sample_uniform(st.key, sa, n, m, engine.primes[m], engine.L + engine.K, idx)
        assert np.array_equal(c[1, m][idx], want), f"c1 limb {m} is not the model's uniform sample of stream {sa}"
    e = sk_error_of(engine, c[0], c[1], m_ntt, s_ntt)
    assert np.array_equal(e[idx], R.sample_cbd(st.key, se, n, idx)), f"e is not the model's CBD sample of stream {se}"
    return c[1], e


def audit_enc_sk_seeded_words(engine, st, c0, m_ntt, s_ntt, pub_key, pub_stream, idx=None):
    """(a, e) of one seeded secret-key encryption, c0 [nl][n]: a is the model's
    uniform sample under the PUBLIC key words pub_key and stream pub_stream
    (nothing of the engine's enters it); the private counter advances by two,
    the first of which is skipped, and INTT(c0 + a s - m) is the model's CBD
    sample of the second.  Returns (a [nl][n], e)."""
    n = engine.n
    c0 = np.asarray(c0, dtype=np.uint64)
    lvl = c0.shape[0]
    assert c0.shape == (lvl, n) and np.asarray(m_ntt).shape == (lvl, n)
    idx = np.arange(n) if idx is None else idx
    a = np.stack([R.sample_uniform(pub_key, pub_stream, n, m, engine.primes[m], engine.L + engine.K)
                  for m in range(lvl)])
    st.take()  # the stream he_enc_sk would draw c1 from: skipped
    se = st.take()
    e = sk_error_of(engine, c0, a, m_ntt, s_ntt)
    assert np.array_equal(e[idx], R.sample_cbd(st.key, se, n, idx)), f"e is not the model's CBD sample of stream {se}"
    return a, e


def audit_enc_sk(engine, st, ct, pt, sk, idx=None):
    """audit_enc_sk_words on the exported objects of one he_enc_sk."""
    lvl = ct.nlimbs
    return audit_enc_sk_words(engine, st, engine.export(ct), engine.export(pt)[0][:lvl], engine.export(sk)[0][:lvl], idx)


def encoded_words(engine, z, slots, scale, nlimbs):
    """The plaintext words [nlimbs][n] of z: the CPU engine's he_ecd_ex,
    exported (the engines' common encoding, pinned by test_noise_cpu.py)."""
    host = _host(engine)
    pt = host.pt()
    host.ecd_ex(pt, z, slots, scale, nlimbs)
    m = host.export(pt)[0][:nlimbs].copy()
    host.free(pt)
    return m


def pairwise_distinct(polys):
    seen = {}
    for name, p in polys:
        key = np.asarray(p).tobytes()
        assert key not in seen, f"{name} equals {seen.get(key)}"
        seen[key] = name


# --------------------------------------------------------------------------- exact decryption and noise
def crt_centred(res, primes):
    """[len(primes)][n] residues -> object array of the centred integers."""
    Q = 1
    for p in primes:
        Q *= int(p)
    x = np.zeros(res.shape[-1], dtype=object)
    for r, p in zip(res, primes):
        Qi = Q // int(p)
        x = x + r.astype(object) * (Qi * pow(Qi, -1, int(p)))
    x = x % Q
    return np.where(x > Q // 2, x - Q, x)


def exact_decrypt_words(engine, words, s_ntt):
    """Centred Python-integer coefficients of c0 + c1 s modulo Q_level for the
    ciphertext words [2][nl][n] and the secret's words s_ntt (its first nl
    limbs are read): the product per limb, the engine's inverse transform
    (pinned separately), then an exact centred CRT."""
    c = np.asarray(words, dtype=np.uint64)
    lvl = c.shape[1]
    assert c.shape == (2, lvl, engine.n)
    primes = engine.primes[:lvl]
    m = np.stack([addmod(c[0, i], mulmod(c[1, i], s_ntt[i], q), q) for i, q in enumerate(primes)])
    return crt_centred(intt(engine, m), primes)


def exact_decrypt(engine, ct, sk):
    """exact_decrypt_words of an exported ciphertext and secret key."""
    return exact_decrypt_words(engine, engine.export(ct), engine.export(sk)[0])


def exact_plain(engine, pt):
    """The exact centred coefficients of a plaintext object."""
    lvl = pt.nlimbs
    return crt_centred(intt(engine, engine.export(pt)[0]), engine.primes[:lvl])


def negacyclic_int(a, b):
    """Exact product in Z[X]/(X^n + 1) of signed integer vectors, by one
    Kronecker product with balanced digits."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    n = len(a)
    bits = max(abs(x) for x in a).bit_length() + max(abs(x) for x in b).bit_length() + n.bit_length() + 2
    width = (bits + 7) // 8
    half = 1 << (8 * width - 1)

    def pack(v):
        pos = b"".join(max(x, 0).to_bytes(width, "little") for x in v)
        neg = b"".join(max(-x, 0).to_bytes(width, "little") for x in v)
        return int.from_bytes(pos, "little") - int.from_bytes(neg, "little")

    offset = int.from_bytes(half.to_bytes(width, "little") * (2 * n), "little")
    raw = (pack(a) * pack(b) + offset).to_bytes(2 * n * width + 1, "little")
    c = [int.from_bytes(raw[i * width:(i + 1) * width], "little") - half for i in range(2 * n)]
    return np.array([c[i] - c[i + n] for i in range(n)], dtype=object)


def noise_stats(got, want, div=1):
    """(max |d|, mean d) of d = got - want / div as floats; got, want exact
    integer vectors (the difference is formed exactly before the division)."""
    d = (np.asarray(got, dtype=object) * div - np.asarray(want, dtype=object)).astype(np.float64) / float(div)
    return float(np.abs(d).max()), float(d.mean())


def model_params(engine, lvl=None):
    return dict(n=engine.n, primes=[int(p) for p in engine.primes], L=engine.L, alpha=engine.info.alpha,
                lvl=lvl or engine.L)


#: operations measure_ops() reports, with the number of model-encoded
#: plaintexts in the expected message (each may differ from the engine's own
#: encoding by one unit: two roundings of values that agree to 2^40 2^-50)
OPS = {"enc_pk": 1, "enc_sk": 1, "add": 2, "sub": 2, "neg": 1, "moddown": 1, "add_pt": 2, "mul_pt": 0,
       "rot": 0, "mul": 0, "mul+rescale": 0, "mul_rescale": 0}
SCALE = 2.0 ** 40
SLOTS = 16


def measure_ops(e, seed, ops=None, rot=1):
    """{op: (max |noise|, mean noise)} on engine e (context initialised) after
    gpqhe_set_seed(seed), and {"mul_pt": pt_norm2} extras.  noise = exact
    decryption - expected message; the expected message is the model's
    encoding for fresh and additive operations and the exact image of the
    operands' exact decryptions for rotations and products."""
    ops = set(OPS if ops is None else ops)
    n, L = e.n, e.L
    e.set_seed(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(seed)
    z = [rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS) for _ in range(2)]
    m = [np.array(M.encode_coeffs(list(v), n, SCALE), dtype=object) for v in z]
    pts, cts = [], []
    for v in z:
        pt, ct = e.pt(), e.ct()
        e.ecd_ex(pt, v, SLOTS, SCALE, L)
        e.enc_pk(ct, pt, pk)
        pts.append(pt)
        cts.append(ct)
    dec = [exact_decrypt(e, c, sk) for c in cts]
    out, extra = {}, {}
    tmp = e.ct()
    out["enc_pk"] = noise_stats(dec[0], m[0])
    if "enc_sk" in ops:
        e.enc_sk(tmp, pts[0], sk)
        out["enc_sk"] = noise_stats(exact_decrypt(e, tmp, sk), m[0])
    if "add" in ops:
        e.add(tmp, cts[0], cts[1])
        out["add"] = noise_stats(exact_decrypt(e, tmp, sk), m[0] + m[1])
    if "sub" in ops:
        e.sub(tmp, cts[0], cts[1])
        out["sub"] = noise_stats(exact_decrypt(e, tmp, sk), m[0] - m[1])
    if "neg" in ops:
        e.copy_ct(tmp, cts[0])
        e.neg(tmp)
        out["neg"] = noise_stats(exact_decrypt(e, tmp, sk), -m[0])
    if "moddown" in ops:
        e.copy_ct(tmp, cts[0])
        e.moddown(tmp)
        assert tmp.nlimbs == L - 1
        out["moddown"] = noise_stats(exact_decrypt(e, tmp, sk), m[0])
    if "add_pt" in ops:
        e.add_pt(tmp, cts[0], pts[1])
        out["add_pt"] = noise_stats(exact_decrypt(e, tmp, sk), m[0] + m[1])
    if "mul_pt" in ops:
        e.mul_pt(tmp, cts[0], pts[1])
        p1 = exact_plain(e, pts[1])
        extra["mul_pt"] = dict(pt_norm2=SCALE ** 2 * float(np.mean(np.abs(z[1]) ** 2)))
        assert abs(float(sum(int(x) ** 2 for x in p1)) / extra["mul_pt"]["pt_norm2"] - 1) < 1e-6
        out["mul_pt"] = noise_stats(exact_decrypt(e, tmp, sk), negacyclic_int(m[0], p1))
    if "rot" in ops:
        rk = e.evks(e.slots)
        e.lib.he_genrot(ctypes.byref(rk[rot]), rot, ctypes.byref(sk))
        e.rot(tmp, cts[0], rot, rk)
        want = M.automorphism_int([int(x) for x in dec[0]], pow(5, rot, 2 * n))
        out["rot"] = noise_stats(exact_decrypt(e, tmp, sk), want)
        e.free_evks(rk)
    if ops & {"mul", "mul+rescale", "mul_rescale"}:
        rlk = e.evk()
        e.genrlk(rlk, sk)
        prod = negacyclic_int(dec[0], dec[1])
        qtop = int(e.primes[L - 1])
        if ops & {"mul", "mul+rescale"}:
            e.mul(tmp, cts[0], cts[1], rlk)
            out["mul"] = noise_stats(exact_decrypt(e, tmp, sk), prod)
            e.rescale(tmp)
            out["mul+rescale"] = noise_stats(exact_decrypt(e, tmp, sk), prod, qtop)
        if "mul_rescale" in ops:
            e.mul_rescale(tmp, cts[0], cts[1], rlk)
            out["mul_rescale"] = noise_stats(exact_decrypt(e, tmp, sk), prod, qtop)
        e.free(rlk)
    for o in pts + cts + [tmp, pk, sk]:
        e.free(o)
    return {k: v for k, v in out.items() if k in ops}, extra


def ceiling_of(e, op, extra):
    return M.noise_ceilings(model_params(e), op, **extra.get(op, {})) + OPS[op]


def matrix_with_diagonals(s, diags, rng):
    """A real s x s matrix, entries uniform in [-2, 2] on the diagonals
    (M[i][(i + d) mod s]) listed and exactly zero elsewhere."""
    Mx = np.zeros((s, s))
    i = np.arange(s)
    for d in diags:
        Mx[i, (i + d) % s] = rng.uniform(-2, 2, s)
    return Mx


def measure_gemv(e, seed, diags):
    """(max |noise|, mean noise), {"diags": encoded diagonals} of he_gemv with
    the listed non-zero diagonals, one he_genrot per diagonal d != 0.  The
    expected message is sum_d pt_d * dec(x)(X^(5^d)) / q_top with pt_d the
    model's encoding of diagonal d at scale q_top."""
    n, L, s = e.n, e.L, e.slots
    e.set_seed(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = e.evks(s)
    for d in diags:
        if d:
            e.lib.he_genrot(ctypes.byref(rk[d]), d, ctypes.byref(sk))
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    Mx = matrix_with_diagonals(s, diags, np.random.default_rng(0))  # the same matrix for every seed
    pt, x, y = e.pt(), e.ct(), e.ct()
    e.ecd_ex(pt, z, s, SCALE, L)
    e.enc_pk(x, pt, pk)
    e.gemv(y, Mx.ravel(), x, rk)
    assert y.nlimbs == L - 1
    dx = [int(v) for v in exact_decrypt(e, x, sk)]
    qtop = int(e.primes[L - 1])
    want = np.zeros(n, dtype=object)
    enc = {}
    for d in diags:
        ptd = M.encode_coeffs([complex(Mx[i, (i + d) % s]) for i in range(s)], n, float(qtop))
        want = want + negacyclic_int(ptd, M.automorphism_int(dx, pow(5, d, 2 * n)))
        if d:
            enc[d] = ptd
    stats = noise_stats(exact_decrypt(e, y, sk), want, qtop)
    for o in (pt, x, y, pk, sk):
        e.free(o)
    e.free_evks(rk)
    return stats, dict(diags=enc)


#: slack of the gemv comparison: the model's double-precision encoding of a
#: diagonal at scale q_top may differ from the engine's by q_top 2^-46 per
#: coefficient (|M| <= 2, 2 s = 32 non-zero coefficients), times the message
#: coefficients (<= SCALE) and divided by q_top: 32 2^-46 2^40 = 0.5; one more
#: unit for the rounding of the comparison itself
GEMV_SLACK = 2


def gemv_ceiling(e, extra):
    return M.noise_ceilings(model_params(e), "gemv", **extra) + GEMV_SLACK


def measure_bsgs(e, seed, diags, g):
    """(max |noise|, mean noise), {"steps", "g"} of the baby-step
    giant-step product with g baby steps: he_gemv_bsgs on the product, its
    defining composition (bsgs_ref.bsgs_compose) on the oracle, which has no
    entry point of that name.  The expected message is
    sum_{j,i} pt_{j,i}(X^(5^jg)) * dec(x)(X^(5^(jg+i))) / q_top with pt_{j,i}
    the model's encoding of diagonal jg + i rolled by jg, at scale q_top."""
    n, L, s = e.n, e.L, e.slots
    e.set_seed(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = bsgs_ref.bsgs_keys(e, sk, g)
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    Mx = matrix_with_diagonals(s, diags, np.random.default_rng(0))  # the same matrix for every seed
    pt, x = e.pt(), e.ct()
    e.ecd_ex(pt, z, s, SCALE, L)
    e.enc_pk(x, pt, pk)
    if hasattr(e.lib, "he_gemv_bsgs"):
        y = e.ct()
        e.gemv_bsgs(y, Mx.ravel(), x, rk, g)
    else:
        y = bsgs_ref.bsgs_compose(e, Mx.astype(np.complex128), x, rk, g)
    assert y.nlimbs == L - 1
    dx = [int(v) for v in exact_decrypt(e, x, sk)]
    qtop = int(e.primes[L - 1])
    want = np.zeros(n, dtype=object)
    steps = {}
    for d in diags:
        j, i = divmod(d, g)
        diag = np.roll(Mx[np.arange(s), (np.arange(s) + d) % s], j * g)
        ptd = M.encode_coeffs([complex(v) for v in diag], n, float(qtop))
        rolled = M.automorphism_int(ptd, pow(5, j * g, 2 * n))
        want = want + negacyclic_int(rolled, M.automorphism_int(dx, pow(5, d, 2 * n)))
        steps.setdefault(j, {})
        if i:
            steps[j][i] = ptd
    stats = noise_stats(exact_decrypt(e, y, sk), want, qtop)
    for o in (pt, x, y, pk, sk):
        e.free(o)
    e.free_evks(rk)
    return stats, dict(steps=steps, g=g)


def bsgs_ceiling(e, extra):
    return M.noise_ceilings(model_params(e), "gemv_bsgs", **extra) + GEMV_SLACK


# --------------------------------------------------------------------------- the step products
#: the step families: the reference composition (on the oracle) and the
#: product's entry point that it defines
STEP_KINDS = ("step", "rows", "packed", "encgain")
#: slack of the step comparisons: the expected message is built from exact
#: integers throughout (exact decryptions, the engine's own plaintexts), so the
#: only allowance is one unit for the rounding of the comparison itself
STEP_SLACK = 1


def automorphism_obj(a, g):
    """a(X) -> a(X^g) on an object (Python integer) coefficient vector."""
    a = np.asarray(a, dtype=object)
    n = a.size
    e = (np.arange(n, dtype=np.int64) * int(g)) % (2 * n)
    out = np.zeros(n, dtype=object)
    out[e % n] = np.where(e < n, a, -a)
    return out


def plain_coeffs(engine, z, slots, scale, nlimbs):
    """The exact centred coefficients of the engine's encoding of z."""
    return crt_centred(intt(engine, encoded_words(engine, z, slots, scale, nlimbs)), engine.primes[:nlimbs])


def _device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).ravel().view(np.int64)).cuda()


def _words_out(engine, count, nl):
    import torch
    t = torch.zeros(count * 2 * nl * engine.n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def _read(engine, t, count, nl):
    engine.sync()
    return t.cpu().numpy().view(np.uint64).reshape(count, 2, nl, engine.n)


def step_matrices(kind, S, s, rows, diags):
    """The gains of a step case, the same for every seed: entries uniform in
    [-2, 2].  step: two s x s matrices with the non-zero diagonals diags =
    (of Ma, of Mb); the other kinds: [nmat][rows][s] leading rows, nmat = 1
    for rows and P = S / s (every loop its own) for packed and encgain."""
    rng = np.random.default_rng(0)
    if kind == "step":
        return matrix_with_diagonals(s, diags[0], rng), matrix_with_diagonals(s, diags[1], rng)
    nmat = 1 if kind == "rows" else S // s
    return rng.uniform(-2, 2, (nmat, rows, s)), rng.uniform(-2, 2, (nmat, rows, s))


def measure_step(e, seed, kind, s=None, rows=None, g=0, diags=None, count=1, sym=False):
    """([(max |noise|, mean noise) per ciphertext], model arguments) of one
    step family on engine e (context of S = e.slots slots initialised) after
    gpqhe_set_seed(seed): on the oracle the reference composition of
    tests/{step,rows,packed,encgain}_ref.py, on the product its batch entry
    point over `count` ciphertexts in device memory.

    up = moddown(uhat) - W(xhat - xr, uhat - ur); the expected message is, in
    exact integers,
        dec(uhat) - F(sum_r pt^A_r * xd(X^(5^r)) + pt^B_r * ud(X^(5^r))) / q_top
    with xd = dec(xhat) - dec(xr), ud = dec(uhat) - dec(ur) from the exact
    decryptions of the four inputs, pt_r the engine's own plaintext of the
    diagonal (for encgain: the exact decryption of the gain ciphertext), and F
    the giant rotations of the BSGS (step) or the row fold prod (1 + sigma_r).
    So the noise is what the key switches, ModDowns and rescales add.
    sym: the encgain gains encrypted under the secret key."""
    import bsgs_ref as B
    from tests import encgain_ref, packed_ref, rows_ref, sk_ref, step_ref
    assert kind in STEP_KINDS
    product = e.name != "oracle"
    n, L, S = e.n, e.L, e.slots
    s = s or S
    P = S // s
    if kind in ("step", "rows"):
        assert s == S
    qtop = int(e.primes[L - 1])
    e.set_seed(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = None
    if kind == "step":
        g = g or B.default_g(S)
        rk = B.bsgs_keys(e, sk, g)
    elif kind == "rows":
        rk = rows_ref.rows_keys(e, sk, rows)
    else:
        rk = packed_ref.packed_keys(e, sk, s, rows)
    if kind == "encgain":
        rlk = e.evk()
        e.genrlk(rlk, sk)
    Ma, Mb = step_matrices(kind, S, s, rows, diags)
    nmat = 1 if kind == "rows" else P
    s_ntt = e.export(sk)[0]
    # the gains: {rotation r: (plaintext of Ma, of Mb)} and the images F sums over
    gains, DA, DB = {}, None, None
    if kind == "step":
        da, db = B.diagonals(Ma, S), B.diagonals(Mb, S)
        for d in sorted(set(da) | set(db)):
            j = d // g
            gains[d] = tuple(plain_coeffs(e, np.roll(dd[d], j * g), S, float(qtop), L) if d in dd else None
                             for dd in (da, db))
        folds = []
    else:
        mp = rows_ref.pow2(rows)
        if kind == "rows":
            da, db = rows_ref.extended_diagonals(Ma, S, rows), rows_ref.extended_diagonals(Mb, S, rows)
        else:
            da, db = packed_ref.packed_diagonals(Ma, S, s, rows, nmat), packed_ref.packed_diagonals(Mb, S, s, rows, nmat)
        if kind == "encgain":
            if sym:
                DA = sk_ref.enc_gain_sk_compose(e, Ma, sk, s, rows, nmat, L)
                DB = sk_ref.enc_gain_sk_compose(e, Mb, sk, s, rows, nmat, L)
            else:
                DA = encgain_ref.enc_gain_compose(e, Ma, pk, s, rows, nmat, L)
                DB = encgain_ref.enc_gain_compose(e, Mb, pk, s, rows, nmat, L)
            for i in range(mp):
                gains[i * P] = (exact_decrypt(e, DA[i], sk), exact_decrypt(e, DB[i], sk))
        else:
            for i in sorted(set(da) | set(db)):
                gains[i * P] = tuple(plain_coeffs(e, dd[i], S, float(qtop), L) if i in dd else None for dd in (da, db))
        folds = []
        r = mp
        while r < s:
            folds.append(r * P)
            r *= 2
    rng = np.random.default_rng(seed)
    zs = rng.uniform(-1, 1, (count, 4, S)) + 1j * rng.uniform(-1, 1, (count, 4, S))
    cts = [[e.encrypt(zs[c, b], pk, S, SCALE, L) for b in range(4)] for c in range(count)]
    words = np.stack([[e.export(x) for x in blk] for blk in cts])  # [count][4][2][L][n]
    if product:
        din = _device(np.ascontiguousarray(words.transpose(1, 0, 2, 3, 4)))  # blocks xhat, xr, uhat, ur
        ptr = [din.data_ptr() + 8 * b * count * 2 * L * n for b in range(4)]
        dout = _words_out(e, count, L - 1)
        if kind == "step":
            e.hempc_step_batch(dout.data_ptr(), Ma, Mb, *ptr, count, L, rk, g)
        elif kind == "rows":
            e.hempc_step_rows_batch(dout.data_ptr(), Ma, Mb, *ptr, count, L, rk, rows)
        elif kind == "packed":
            e.hempc_step_packed_batch(dout.data_ptr(), Ma, Mb, *ptr, count, L, rk, s, rows, nmat)
        else:
            dg = _device(np.stack([e.export(x) for x in DA + DB]))
            e.hempc_step_encgain_packed_batch(dout.data_ptr(), dg.data_ptr(), dg.data_ptr() + 8 * mp * 2 * L * n,
                                              *ptr, count, L, rk, rlk, s, rows)
        out = _read(e, dout, count, L - 1)
    else:
        out = []
        for xhat, xr, uhat, ur in cts:
            if kind == "step":
                up = step_ref.step_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, g)
            elif kind == "rows":
                up = rows_ref.step_rows_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, rows)
            elif kind == "packed":
                up = packed_ref.step_packed_compose(e, Ma, Mb, xhat, xr, uhat, ur, rk, s, rows, nmat)
            else:
                up = encgain_ref.step_encgain_compose(e, DA, DB, xhat, xr, uhat, ur, rk, rlk, s, rows)
            assert up.nlimbs == L - 1
            out.append(e.export(up).copy())
            e.free(up)
    stats = []
    for c in range(count):
        dec = [exact_decrypt_words(e, words[c, b], s_ntt) for b in range(4)]
        dx, du = dec[0] - dec[1], dec[2] - dec[3]
        w = np.zeros(n, dtype=object)
        for r, pts in gains.items():
            # step: the plaintext of diagonal r = j g + i was rolled by j g and rides the giant rotation
            giant = pow(5, r // g * g, 2 * n) if kind == "step" else 1
            for ptv, d in zip(pts, (dx, du)):
                if ptv is not None:
                    w = w + negacyclic_int(automorphism_obj(ptv, giant), automorphism_obj(d, pow(5, r, 2 * n)))
        for r in folds:
            w = w + automorphism_obj(w, pow(5, r, 2 * n))
        stats.append(noise_stats(exact_decrypt_words(e, out[c], s_ntt), dec[2] * qtop - w, qtop))
    # what the model needs: the plaintexts of every rotation r != 0, per operand
    if kind == "step":
        steps = {}
        for d, pts in gains.items():
            j, i = divmod(d, g)
            steps.setdefault(j, {})
            if i:
                steps[j].setdefault(i, [])
                steps[j][i] += [np.array(p, dtype=float) for p in pts if p is not None]
        extra = dict(steps=steps, g=g)
    else:
        extra = dict(babies={r: [np.array(p, dtype=float) for p in pts if p is not None]
                             for r, pts in gains.items() if r}, folds=folds)
    for blk in cts:
        for x in blk:
            e.free(x)
    for o in [pk, sk] + ([rlk] if rlk is not None else []) + (DA or []) + (DB or []):
        e.free(o)
    e.free_evks(rk)
    return stats, extra


def step_ceiling(e, kind, extra):
    return M.noise_ceilings(model_params(e), kind, **extra) + STEP_SLACK
