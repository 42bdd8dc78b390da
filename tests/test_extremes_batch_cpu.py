"""The constructions behind tests/test_gpu_extremes_batch.py pinned to exact
integers, without a GPU: the identity switching key, the decoder's centred
lift at its edge values, the constant diagonals, and the accumulator maxima
the batch kernels' bound comments speak of.  The oracle is compared with the
big-integer model (tests/ckks_model.py), Python integers and
extreme_inputs.horner_double at the prime sizes of tests/test_extremes_cpu.py,
so a disagreement on the GPU between product and oracle on these inputs is the
product's."""
import numpy as np
import pytest

import ckks_model as M
import extreme_inputs as X
from test_extremes_cpu import BITS, LOGN, ints

#: crafted secret keys: the pattern on every limb (the constant polynomials 1
#: and -1, and NTT words at the centred extremes)
SK_KINDS = ("one", "qm1", "half_lo", "rand_half")


def ctx(oracle, logn, qb, nlimbs=3, nspecial=1, dnum=None, slots=None):
    oracle.init_params(logn=logn, nlimbs=nlimbs, nspecial=nspecial, dnum=dnum or nlimbs,
                       slots=slots or (1 << (logn - 1)), q0_bits=qb[0], qi_bits=qb[1], p_bits=qb[2], seed=5)
    assert [q.bit_length() for q in oracle.primes] == [qb[0]] + [qb[1]] * (nlimbs - 1) + [qb[2]] * nspecial
    return oracle


def prod(v):
    out = 1
    for x in v:
        out *= int(x)
    return out


def craft_sk(oracle, sk, kind):
    """kind on every one of sk's L + K limbs; returns the words [L + K][n]."""
    w = X.poly([kind] * sk.nlimbs, oracle.primes[:sk.nlimbs], oracle.n, seed=41)
    oracle.import_(sk, w[None], sk.nlimbs, sk.scale, sk.flags)
    assert np.array_equal(oracle.export(sk)[0], w)
    return w


# ------------------------------------------------------------ 1. identity key
#            nlimbs, nspecial, dnum: digits
DIGITS = [(3, 3, 1),   # one digit of three limbs
          (3, 2, 2),   # alpha 2: digits {0, 1}, {2}, the last partial; partial again at level 1
          (3, 1, 3)]   # a digit per limb


@pytest.mark.parametrize("nl,K,dnum", DIGITS)
@pytest.mark.parametrize("qb", BITS)
@pytest.mark.parametrize("logn", LOGN)
def test_rot_under_identity_key_is_the_index_permutation(oracle, logn, qb, nl, K, dnum):
    """he_rot under X.identity_key: both output polynomials equal the model's
    transform of the model's X -> X^g on the pulled-back patterns, for r = 1
    and r = slots - 1, at the top level and every level down to 1."""
    s = 8
    ctx(oracle, logn, qb, nl, K, dnum, slots=s)
    n, L, primes = oracle.n, oracle.L, oracle.primes
    pk, sk = oracle.pk(), oracle.sk()
    oracle.keypair(pk, sk)
    rk = oracle.evks(s)
    oracle.genrk(rk, sk)
    for r in (1, s - 1):
        ident = X.key_payload("identity", primes, n, rk[r].npoly // 2, L=L)
        assert ident.shape == (rk[r].npoly, L + K, n) and rk[r].npoly // 2 == oracle.info.dnum
        oracle.import_(rk[r], ident, len(primes), rk[r].scale, rk[r].flags)
    ct, out = oracle.ct(), oracle.ct()
    for lvl in range(L, 0, -1):
        for k in (0, 4, 7):  # mixed(k): every NAMES pattern lands on some limb of some polynomial
            coef = X.mixed(k, primes[:lvl], n, npolys=2)
            oracle.import_(ct, X.pullback(oracle, coef, lvl), lvl, scale=1.0)
            for r in (1, s - 1):
                g = rk[r].galois
                assert g == pow(5, r, 2 * n)
                oracle.rot(out, ct, r, rk)
                got = oracle.export(out)
                assert out.nlimbs == lvl
                for p in range(2):
                    for i in range(lvl):
                        want = M.ntt_eval(M.automorphism(ints(coef[p, i]), g, primes[i]), primes[i], oracle.info.psi[i])
                        assert ints(got[p, i]) == want, (lvl, k, r, p, i)
    # a constant ciphertext (q - 1, q - 1) stays what it is under every rotation
    const = np.stack([X.poly(["qm1"] * L, primes[:L], n)] * 2)
    oracle.import_(ct, const, L, scale=1.0)
    for r in (1, s - 1):
        oracle.rot(out, ct, r, rk)
        assert np.array_equal(oracle.export(out), const)
    for o in (ct, out, pk, sk):
        oracle.free(o)
    oracle.free_evks(rk)


def test_identity_key_layout():
    primes, n = [97, 193, 257, 769, 12289], 8
    key = X.identity_key(primes, 3, 2, n, 2)
    P = 769 * 12289
    assert key.shape == (4, 5, n)
    assert not key[0].any() and not key[2].any() and not key[:, 3:].any()
    assert ints(key[1, :, 3]) == [P % 97, P % 193, 0, 0, 0] and ints(key[3, :, 5]) == [0, 0, P % 257, 0, 0]
    assert not X.key_payload("zero", primes, n, 2).any()
    assert np.array_equal(X.key_payload("identity", primes, n, 2, L=3), key)
    assert set(X.KEY_KINDS) < set(X.BATCH_KEY_KINDS) and {"zero", "identity"} < set(X.BATCH_KEY_KINDS)


# ------------------------------------------------------------ 2. decoder lift
#          nlimbs, (q0, qi, P bits): q0 wider than the other limbs, up to the longest chains of the GPU tests
CHAINS = ([(nl, qb) for nl in (1, 2, 3) for qb in BITS] +
          [(6, (51, 48, 51)), (6, (61, 48, 61)), (8, (60, 50, 60)), (8, (51, 50, 51))])


def test_lift_edges_and_horner_double():
    primes = [(1 << 61) - 1, 281474976710597, 281474976710567]
    Q = prod(primes)
    E = X.lift_edges(primes)
    for name in ("0", "1", "Q-1", "(Q-1)/2", "(Q+1)/2", "2^64-1", "2^64", "Q-2^64", "Q-2^128", "Q-1-2^64", "2^128",
                 "lowQ", "2^53+1", "Q-2^53-1", "q0", "q0..q0", "q0..q1", "Q0-1", "Q1-1", "Q2-1", "floor(Q/2)-2^64",
                 "ceil(Q/2)+2^64", "Q-2^128+1"):
        assert name in E, name
    assert all(0 <= v < Q for v in E.values())
    assert E["lowQ"] % (1 << 64) == Q % (1 << 64) and E["q0..q1"] == primes[0] * primes[1]
    assert E["Q1-1"] % primes[0] == primes[0] - 1 and E["Q1-1"] % primes[1] == primes[1] - 1
    # Q - X = 2^128 - 1: the low word of X is one above Q's, the next equals Q's
    x = E["Q-2^128+1"]
    assert x % (1 << 64) == (Q + 1) % (1 << 64) and (x >> 64) % (1 << 64) == (Q >> 64) % (1 << 64) and 2 * x > Q
    assert X.lift_edges(primes[:1]).keys() >= {"0", "1", "Q-1", "(Q-1)/2", "(Q+1)/2"}
    assert "2^64" not in X.lift_edges(primes[:1])
    assert X.horner_double(0, primes) == 0.0 and X.horner_double(1, primes) == 1.0
    assert X.horner_double(Q - 1, primes) == -1.0 and X.horner_double(Q - (1 << 64), primes) == -(2.0 ** 64)
    assert X.horner_double((1 << 64) - 1, primes) == 2.0 ** 64  # the word itself rounds
    assert X.horner_double((1 << 53) + 1, primes) == 2.0 ** 53
    assert X.horner_double((Q - 1) // 2, primes) > 0 > X.horner_double((Q + 1) // 2, primes)
    w = X.const_words(Q - 1, primes, 4)
    assert w.shape == (3, 4) and ints(w[:, 2]) == [q - 1 for q in primes]


@pytest.mark.parametrize("nl,qb", CHAINS)
def test_decode_of_constant_polynomials_is_the_lift(oracle, nl, qb):
    """he_dec + he_dcd_ex of c0 + c1 s = the constant polynomial X, for every
    X of lift_edges at levels 1 and nl (the chains in between are parametrised
    themselves): every slot bit-equal to
    horner_double(X) / scale, imaginary part 0.  sk = 1 with c0 = X - (Q - 1),
    c1 = Q - 1, and sk = -1 (the word q - 1) with c0 = (Q - 1)/2, c1 = c0 - X."""
    logn = 5
    ctx(oracle, logn, qb, nl, 1, nl)
    n, primes = oracle.n, oracle.primes
    pk, sk = oracle.pk(), oracle.sk()
    oracle.keypair(pk, sk)
    ct = oracle.ct()
    scale = 2.0 ** qb[1]
    for lvl in sorted({1, nl}):
        Q = prod(primes[:lvl])
        for kind in ("one", "qm1"):
            craft_sk(oracle, sk, kind)
            for name, v in X.lift_edges(primes[:lvl]).items():
                if kind == "one":
                    c0, c1 = (v - (Q - 1)) % Q, Q - 1
                else:
                    c0 = (Q - 1) // 2
                    c1 = (c0 - v) % Q
                oracle.import_(ct, np.stack([X.const_words(c0, primes[:lvl], n), X.const_words(c1, primes[:lvl], n)]),
                               lvl, scale=scale)
                want = np.float64(X.horner_double(v, primes[:lvl])) / np.float64(scale)
                for slots in (n // 2, 4):
                    z = oracle.decrypt(ct, sk, slots)
                    assert np.all(z.real.view(np.uint64) == want.view(np.uint64)), (lvl, kind, name, slots)
                    assert np.all(z.imag.view(np.uint64) == 0), (lvl, kind, name, slots)
    for o in (ct, pk, sk):
        oracle.free(o)


@pytest.mark.parametrize("qb", BITS)
def test_dec_under_crafted_sk_is_exact_on_every_pattern_pair(oracle, qb):
    """he_dec of (c0, c1) = every ordered pair of NAMES patterns under each
    crafted secret key: (c0 + c1 s) mod q, word by word in Python integers."""
    ctx(oracle, 5, qb)
    n, L, primes = oracle.n, oracle.L, oracle.primes
    pk, sk = oracle.pk(), oracle.sk()
    oracle.keypair(pk, sk)
    ct, pt = oracle.ct(), oracle.pt()
    q = np.array(primes[:L], dtype=object).reshape(L, 1)
    pats = [X.poly([nm] * L, primes[:L], n, seed=k) for k, nm in enumerate(X.NAMES)]
    for kind in SK_KINDS:
        s = craft_sk(oracle, sk, kind)[:L].astype(object)
        for a in pats:
            for b in pats:
                oracle.import_(ct, np.stack([a, b]), L, scale=1.0)
                oracle.dec(pt, ct, sk)
                want = (a.astype(object) + b.astype(object) * s) % q
                assert np.array_equal(oracle.export(pt)[0].astype(object), want), kind
    for o in (ct, pt, pk, sk):
        oracle.free(o)


# ------------------------------------------------------ 3. constant diagonals
@pytest.mark.parametrize("qb", BITS)
def test_unit_constant_diagonals_encode_to_one_and_q_minus_one(oracle, qb):
    """The BSGS, row-folded and packed products encode every diagonal with
    he_ecd_ex(diag, slots, q_top, lvl), q_top = primes[lvl - 1] the top limb of
    the operands' level (bsgs_ref.bsgs_compose, rows_ref.gemv2_rows_compose,
    packed_ref; api.cpp encode_limbs(.., (double)G.q[lvl - 1], ..)), and the
    encrypted gains are encrypted at that scale.  At it the constant diagonal
    -1 / q_top is the word q - 1 on every limb and +1 / q_top the word 1, at
    every level, also as diagonals of const_diag_matrix."""
    s = 16
    ctx(oracle, 6, qb, slots=s)
    pt = oracle.pt()
    for lvl in range(1, oracle.L + 1):
        q_top = oracle.primes[lvl - 1]
        for c, word in ((-1.0 / q_top, lambda q: q - 1), (1.0 / q_top, lambda q: 1)):
            Mx = X.const_diag_matrix(s, c)
            assert Mx.shape == (s, s) and np.all(Mx == c)
            for d in (0, 5):
                diag = Mx[np.arange(s), (np.arange(s) + d) % s]
                oracle.ecd_ex(pt, diag, s, float(q_top), lvl)
                w = oracle.export(pt)[0]
                for i, q in enumerate(oracle.primes[:lvl]):
                    assert np.all(w[i] == word(q)), (lvl, c, i)
    oracle.free(pt)


# ------------------------------------------------------ 4. bounds are reached
def q61(oracle):
    ctx(oracle, 6, (61, 48, 61))
    q = int(oracle.primes[0])
    assert q.bit_length() == 61
    return q


def test_bsgs_tile_sum_attains_its_stated_maximum(oracle):
    """bsgs_inner_batch_kernel, one output word of a full baby tile of 16
    slots: under the identity key a constant (q - 1, q - 1) ciphertext rotates
    to itself, and every diagonal of const_diag_matrix(s, -1 / q_top) is the
    word q - 1, so the 128-bit sum is exactly 16 (q - 1)^2 -- the largest sum
    of 16 products of canonical residues -- on the 61-bit limb; it fits 128 bits
    with its high word below 2^62 (bsgs_red128's precondition)."""
    q = q61(oracle)
    acc = 0
    for _ in range(16):
        acc += (q - 1) * (q - 1)
    assert acc == 16 * (q - 1) ** 2 == max(16 * a * b for a in (q - 1, q - 2) for b in (q - 1, 1))
    assert acc < 1 << 128 and acc >> 64 < 1 << 62
    assert 16 * ((1 << 61) - 1) ** 2 >> 64 < 1 << 62  # the comment's own statement, any q < 2^61
    assert acc % q == 16


def test_encgain_x1_attains_its_stated_maximum(oracle):
    """EgAcc<false>, 2 m' = 32 terms (rows 16), reduced when (t & 15) == 15:
    with constant (q - 1, q - 1) inputs and gains every term adds 2 (q - 1)^2 to
    x1, so before the reductions x1 is 32 (q - 1)^2 and then the residue 32 plus
    32 (q - 1)^2: the stated "32 products and one residue", the products at
    their maximum, below 2^128.
    A reduction every 32 terms would hold 64 (q - 1)^2 + residue.  For a prime
    below 2^61 that is 2^128 - 2^68 (c + 1) + .. with q = 2^61 - c: still below
    2^128, so the comment's bound has a factor two of slack and no canonical
    input can make that change overflow; every 64 terms would."""
    q = q61(oracle)
    x1, peak = 0, 0
    for t in range(32):
        x1 += (q - 1) * (q - 1)
        x1 += (q - 1) * (q - 1)
        peak = max(peak, x1)
        if t & 15 == 15:
            x1 %= q
    assert peak == 32 * (q - 1) ** 2 + 32
    assert 32 * (q - 1) ** 2 <= peak <= 32 * (q - 1) ** 2 + (q - 1) < 1 << 128
    assert x1 == 64 % q
    assert 64 * (q - 1) ** 2 + (q - 1) < 1 << 128 <= 128 * (q - 1) ** 2
