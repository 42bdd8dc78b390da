"""The oracle pinned to the big-integer model (tests/ckks_model.py) at the
prime sizes where it judges the product -- 51/50-, 60/50- and 61/48-bit
moduli -- on the constructed edge residues of tests/extreme_inputs.py, and the
properties of those helpers.  CPU only."""
import numpy as np
import pytest

import ckks_model as M
import extreme_inputs as X

BITS = [(51, 50, 51), (60, 50, 60), (61, 48, 61)]
LOGN = [4, 5, 6]


def ctx(oracle, logn, qb, nlimbs=3, slots=None):
    oracle.init_params(logn=logn, nlimbs=nlimbs, nspecial=1, dnum=nlimbs, slots=slots or (1 << (logn - 1)),
                       q0_bits=qb[0], qi_bits=qb[1], p_bits=qb[2], seed=5)
    assert [q.bit_length() for q in oracle.primes] == [qb[0]] + [qb[1]] * (nlimbs - 1) + [qb[2]]
    return oracle


def ints(v):
    return [int(x) for x in v]


@pytest.mark.parametrize("qb", BITS)
@pytest.mark.parametrize("logn", LOGN)
def test_ntt_and_inverse_match_model(oracle, logn, qb):
    """Forward: the oracle's transform of every pattern equals the evaluation
    at psi^(2 brev(k) + 1).  Inverse: the model's evaluation of the oracle's
    inverse transform of the pattern gives the pattern back.  All L + K limbs
    (q0, q1, q2 and the special prime)."""
    ctx(oracle, logn, qb)
    n, primes = oracle.n, oracle.primes
    nl = len(primes)
    for name in X.NAMES:
        src = X.poly([name] * nl, primes, n, seed=3)
        fwd = X.pullback(oracle, src, nl)
        inv = src.copy()
        oracle.lib.poly_intt_batch(inv.ctypes.data, 1, nl)
        for i, q in enumerate(primes):
            psi = oracle.info.psi[i]
            assert ints(fwd[i]) == M.ntt_eval(ints(src[i]), q, psi), (name, i)
            assert int(inv[i].max()) < q
            assert M.ntt_eval(ints(inv[i]), q, psi) == ints(src[i]), (name, i)


@pytest.mark.parametrize("qb", BITS)
@pytest.mark.parametrize("logn", LOGN)
def test_rescale_is_exact_floor_division_on_patterns(oracle, logn, qb):
    """he_rescale output = (X - X mod q_top) / q_top on every coefficient, for
    coefficient vectors that are each pattern on all three limbs (polynomial 0)
    beside a mixed one (polynomial 1)."""
    ctx(oracle, logn, qb)
    n, primes = oracle.n, oracle.primes[:3]
    ct = oracle.ct()
    for k, name in enumerate(X.NAMES):
        coef = np.stack([X.poly([name] * 3, primes, n, seed=k), X.mixed(k, primes, n)[0]])
        oracle.import_(ct, X.pullback(oracle, coef, 3), 3, scale=float(primes[2]))
        oracle.rescale(ct)
        assert ct.nlimbs == 2 and ct.scale == 1.0
        out = oracle.export(ct).copy()
        oracle.lib.poly_intt_batch(out.ctypes.data, 2, 2)
        for p in range(2):
            for j in range(n):
                v, _ = M.crt([int(coef[p, i, j]) for i in range(3)], primes)
                y = (v - v % primes[2]) // primes[2]
                assert [int(out[p, i, j]) for i in range(2)] == [y % q for q in primes[:2]], (name, p, j)
    oracle.free(ct)


@pytest.mark.parametrize("qb", BITS)
@pytest.mark.parametrize("logn", LOGN)
def test_automorphism_matches_model(oracle, logn, qb):
    """he_rot under an all-zero rotation key: the key switch adds nothing, the
    division by P of P sigma(c0) is exact, so the output is (sigma_g(c0), 0).
    c0 is each pattern pulled back, and the output's limbs must equal the
    model's transform of the model's X -> X^g on the pattern."""
    s = 8
    ctx(oracle, logn, qb, slots=s)
    n, L, primes = oracle.n, oracle.L, oracle.primes
    pk, sk = oracle.pk(), oracle.sk()
    oracle.keypair(pk, sk)
    rk = oracle.evks(s)
    oracle.genrk(rk, sk)
    for r in (1, s - 1):
        zero = X.key_payload("zero", primes, n, rk[r].npoly // 2)
        oracle.import_(rk[r], zero, len(primes), rk[r].scale, rk[r].flags)
    ct, out = oracle.ct(), oracle.ct()
    for k, name in enumerate(X.NAMES):
        coef = X.poly([name] * L, primes[:L], n, seed=k)
        c1 = X.mixed(k, primes[:L], n)[0]
        oracle.import_(ct, np.stack([X.pullback(oracle, coef, L), c1]), L, scale=1.0)
        for r in (1, s - 1):
            g = rk[r].galois
            assert g == pow(5, r, 2 * n)
            oracle.rot(out, ct, r, rk)
            got = oracle.export(out)
            assert not got[1].any()
            for i in range(L):
                want = M.ntt_eval(M.automorphism(ints(coef[i]), g, primes[i]), primes[i], oracle.info.psi[i])
                assert ints(got[0, i]) == want, (name, r, i)
    for o in (ct, out, pk, sk):
        oracle.free(o)
    oracle.free_evks(rk)


# ------------------------------------------------------------------- helpers
@pytest.mark.parametrize("q", [(1 << 50) - 27, (1 << 61) - 1, 97])
@pytest.mark.parametrize("n", [16, 33])
def test_patterns_are_canonical_and_hit_their_extremes(q, n):
    lo, hi = (q - 1) // 2, (q + 1) // 2
    assert (lo + hi) % q == 0  # the two centred extremes are each other's negatives
    want = {"zero": {0}, "one": {1}, "qm1": {q - 1}, "half_lo": {lo}, "half_hi": {hi}, "alt_qm1": {0, q - 1},
            "alt_half": {lo, hi}, "rand_half": {lo, hi}, "rand_edge": {0, 1, q - 1}, "imp0": {0, q - 1},
            "impN": {0, q - 1}}
    assert sorted(want) == sorted(X.NAMES)
    for name in X.NAMES:
        v = X.pattern(name, q, n, seed=4)
        assert v.dtype == np.uint64 and v.shape == (n,)
        assert int(v.max()) < q
        assert set(ints(v)) == want[name], name  # every named value really occurs
        assert np.array_equal(v, X.pattern(name, q, n, seed=4))
    assert ints(X.pattern("alt_qm1", q, n))[:3] == [q - 1, 0, q - 1]
    assert ints(X.pattern("alt_half", q, n))[:3] == [lo, hi, lo]
    assert int(X.pattern("imp0", q, n)[0]) == q - 1 and int(X.pattern("impN", q, n)[n - 1]) == q - 1
    assert not np.array_equal(X.pattern("rand_half", q, n, 1), X.pattern("rand_half", q, n, 2))


def test_poly_mixed_and_key_payload():
    primes, n = [97, 193, 257, 769], 8
    p = X.poly(["qm1", "one", "half_lo", "zero"], primes, n)
    assert ints(p[:, 0]) == [96, 1, 128, 0]
    for k in range(len(X.NAMES)):
        m = X.mixed(k, primes, n, npolys=3)
        assert m.shape == (3, 4, n)
        for i, q in enumerate(primes):
            assert int(m[:, i].max()) < q
        for pi in range(3):
            for i in range(3):  # neighbouring limbs hold different patterns
                a, b = (m[pi, j].astype(object) * 1000 // primes[j] for j in (i, i + 1))
                assert list(a) != list(b), (k, pi, i)
    key = X.key_payload("digit0", primes, n, dnum=3)
    assert key.shape == (6, 4, n) and np.all(key[:2] == 1) and not key[2:].any()
    key = X.key_payload("qm1", primes, n, dnum=2)
    assert key.shape == (4, 4, n) and ints(key[3, :, 5]) == [q - 1 for q in primes]
    assert X.key_payload("genuine", primes, n, 2) is None


@pytest.mark.parametrize("qb", BITS)
def test_pullback_inverts_to_the_pattern(oracle, qb):
    ctx(oracle, 6, qb)
    n, primes = oracle.n, oracle.primes
    for spec in list(X.NAMES) + ["mixed0", "mixed5"]:
        coef = X.spec_ct(oracle, spec, primes, n, seed=2)
        back = X.spec_ct(oracle, "pb:" + spec, primes, n, seed=2)
        assert back.shape == coef.shape == (2, len(primes), n)
        oracle.lib.poly_intt_batch(back.ctypes.data, 2, len(primes))
        assert np.array_equal(back, coef), spec


def test_circulant_diagonals_encode_to_constants(oracle):
    """Diagonal d of circulant(s, consts) is the constant consts[d]; a constant
    slot vector encodes to a constant polynomial, whose NTT-domain words are all
    c scale rounded, mod q -- at c = +-1/2 and scale q_top the centred extremes
    +-(q_top -+ 1)/2 on the top limb."""
    s = 16
    Mx = X.circulant(s, [0.5, -0.5, 0.0])
    idx = np.arange(s)
    for d in range(s):
        assert np.all(Mx[idx, (idx + d) % s] == [0.5, -0.5, 0.0][d % 3])
    ctx(oracle, 6, (51, 50, 51), slots=s)
    q_top = oracle.primes[oracle.L - 1]
    pt = oracle.pt()
    for c in (0.5, -0.5, 1.0):
        oracle.ecd_ex(pt, np.full(s, c, dtype=np.complex128), s, float(q_top), oracle.L)
        w = oracle.export(pt)[0]
        for i, q in enumerate(oracle.primes[:oracle.L]):
            assert np.all(w[i] == w[i][0])
            # c q_top is a tie at c = +-1/2 (q_top is odd): either neighbour
            near = {int(np.floor(c * q_top)) % q, int(np.ceil(c * q_top)) % q}
            assert int(w[i][0]) in near
    oracle.free(pt)
