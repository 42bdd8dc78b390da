"""The hybrid key switch restated exactly (tests/ckks_model.HybridModel, Python
integers) against the oracle, bit for bit, and the structure of the keys it
consumes.  CPU only; no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

import ckks_model as M
import extreme_inputs as X
import noise_audit as A

#: name -> (L, K, dnum, (q0, qi, p bits))
CONTEXTS = {
    "a1": (3, 1, 3, (55, 40, 58)),        # alpha = 1, K = 1
    "a2": (4, 2, 2, (55, 40, 58)),        # alpha = 2, K = 2
    "partial": (5, 2, 3, (55, 40, 58)),   # digits {0,1} {2,3} {4}
    "onedigit": (4, 4, 1, (55, 40, 58)),  # one digit of all limbs, K = 4
    "fp51": (4, 2, 2, (51, 48, 51)),      # every prime below 2^51
    "q61": (4, 2, 2, (61, 48, 61)),       # 61-bit q0 and P
}


def ctx(oracle, name, logn, seed=5):
    L, K, dnum, qb = CONTEXTS[name]
    oracle.init_params(logn=logn, nlimbs=L, nspecial=K, dnum=dnum, q0_bits=qb[0], qi_bits=qb[1], p_bits=qb[2],
                       seed=seed)
    assert (oracle.L, oracle.K, oracle.info.dnum) == (L, K, dnum)
    return oracle


def ints(v):
    return [int(x) for x in v]


def genrot(e, r, sk, evk=None):
    evk = e.evk() if evk is None else evk
    e.lib.he_genrot(ctypes.byref(evk), r, ctypes.byref(sk))
    return evk


def coef(e, arr):
    """[..][nl][n] NTT words -> nested lists of coefficient residues, by the
    definition (ckks_model.intt_eval)."""
    if arr.ndim == 2:
        return [M.intt_eval(ints(arr[m]), e.primes[m], e.info.psi[m]) for m in range(arr.shape[0])]
    return [coef(e, a) for a in arr]


def words(e, c):
    """[2][nl][n] coefficient residues -> NTT words, by the definition."""
    return np.array([[M.ntt_eval(c[p][m], e.primes[m], e.info.psi[m]) for m in range(len(c[p]))] for p in range(2)],
                    dtype=np.uint64)


# --------------------------------------------------------------------------- model self-checks
def test_model_helpers():
    q, n = 12289, 8
    psi = next(h for h in range(2, q) if pow(h, n, q) == q - 1)
    rng = np.random.default_rng(0)
    a, b = ints(rng.integers(0, q, n)), ints(rng.integers(0, q, n))
    assert M.intt_eval(M.ntt_eval(a, q, psi), q, psi) == a
    assert [v % q for v in M.negacyclic_mul_int(a, b)] == M.negacyclic_mul(a, b, q)
    assert [v % q for v in M.automorphism_int(a, 5)] == M.automorphism(a, 5, q)
    mods = [97, 101, 103]
    F = 97 * 101 * 103
    for x in (0, 1, F - 1, F // 2, 123456):
        xt = M.basis_convert([[x % f] for f in mods], mods)[0]
        assert xt % F == x and 0 <= xt // F < len(mods)
    # the largest overshoot: y_i = f_i - 1 on every limb
    res = [[(-(F // f)) % f] for f in mods]
    assert M.basis_convert(res, mods)[0] // F == len(mods) - 1


# --------------------------------------------------------------------------- key structure
@pytest.mark.parametrize("name,logn", [("a1", 8), ("a2", 8), ("partial", 10), ("onedigit", 8), ("fp51", 6), ("q61", 7)])
def test_key_structure(oracle, name, logn):
    """b_j + a_j s - [m in digit j] (P mod q_m) s' is the model's CBD sample of
    that digit's stream, as one small integer on every limb of Q u P, for the
    relinearisation key (s' = s^2) and two rotation keys (s' = s(X^g))."""
    e = ctx(oracle, name, logn, seed=11)
    st = A.Streams(11)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rots = [(r, genrot(e, r, sk)) for r in (1, e.slots - 1)]
    s, _, s_ntt = A.audit_keypair(e, st, pk, sk)
    errs = A.audit_evk(e, st, rlk, s, s_ntt, 1)
    for r, k in rots:
        g = pow(5, r, 2 * e.n)
        assert k.galois == g and k.dnum == e.info.dnum
        errs += A.audit_evk(e, st, k, s, s_ntt, g)
    assert len(errs) == 3 * e.info.dnum
    A.pairwise_distinct([(i, x) for i, x in enumerate(errs)])
    for o in [pk, sk, rlk] + [k for _, k in rots]:
        e.free(o)


# --------------------------------------------------------------------------- exact key switch
def ymax_payload(e, lvl):
    """c1 whose coefficient limbs make every y_i of its digit f_i - 1: the
    conversion overshoots by (digit size - 1) F on every coefficient."""
    alpha = e.info.alpha
    out = np.zeros((lvl, e.n), dtype=np.uint64)
    for lo in range(0, lvl, alpha):
        mods = e.primes[lo:min(lo + alpha, lvl)]
        F = 1
        for f in mods:
            F *= f
        for i, f in enumerate(mods):
            out[lo + i, :] = (-(F // f)) % f
    return out


def inputs(e, pk, lvl, rng):
    """(label, a, b) payload pairs [2][lvl][n] in NTT form at level lvl."""
    n, primes = e.n, e.primes[:lvl]
    out = []
    z = [rng.uniform(-1, 1, e.slots) + 1j * rng.uniform(-1, 1, e.slots) for _ in range(2)]
    cts = [e.encrypt(v, pk, scale=2.0 ** 30, nlimbs=lvl) for v in z]
    out.append(("genuine", e.export(cts[0]).copy(), e.export(cts[1]).copy()))
    for c in cts:
        e.free(c)
    ones = np.ones((lvl, n), dtype=np.uint64)  # the constant polynomial 1: d2 = a1 b1 = a1
    other = np.stack([X.mixed(3, primes, n)[0], ones])
    qm1 = X.pullback(e, np.stack([X.mixed(1, primes, n)[0], X.poly(["qm1"] * lvl, primes, n)]), lvl)
    out.append(("c1 = q - 1", qm1, other))
    ymax = X.pullback(e, np.stack([X.mixed(5, primes, n)[0], ymax_payload(e, lvl)]), lvl)
    out.append(("y = f - 1", ymax, other))
    return out


@pytest.mark.parametrize("logn", [4, 5, 6])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_exact_key_switch(oracle, name, logn):
    """he_mul, he_mul + he_rescale, he_mul_rescale and he_rot(1), he_rot(slots - 1)
    equal the integer restatement on every output word, at every level L ... 1
    (every ndig and every size of the last digit the chain has; he_rescale and
    he_mul_rescale from level 2, the lowest with a limb to drop), on genuine
    ciphertexts and on constructed c1 (all limbs q - 1; all y_i = f_i - 1,
    where the conversion overshoots by alpha - 1).  The GPU level sweep
    (tests/test_gpu_levels.py) compares the product with this oracle at the
    same levels."""
    e = ctx(oracle, name, logn)
    L, n = e.L, e.n
    model = M.HybridModel(e.primes, L, e.info.alpha)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rk = e.evks(e.slots)
    rot_r = (1, e.slots - 1)
    for r in rot_r:
        genrot(e, r, sk, rk[r])
    rlk_c = coef(e, e.export(rlk))
    rk_c = {r: coef(e, e.export(rk[r])) for r in rot_r}
    rng = np.random.default_rng(logn)
    a, b, out = e.ct(), e.ct(), e.ct()
    seen_overshoot = 0
    for lvl in range(L, 0, -1):
        for label, pa, pb in inputs(e, pk, lvl, rng):
            where = (name, logn, lvl, label)
            # he_moddown only drops the top limb: import at L, then step down
            top = np.zeros((2, L - lvl, n), dtype=np.uint64)
            e.import_(a, np.concatenate([pa, top], axis=1), L, scale=2.0 ** 30)
            e.import_(b, np.concatenate([pb, top], axis=1), L, scale=2.0 ** 30)
            for _ in range(L - lvl):
                e.moddown(a)
                e.moddown(b)
            assert a.nlimbs == lvl and b.nlimbs == lvl
            ca, cb = coef(e, pa), coef(e, pb)
            for lo, hi in model.digits(lvl):
                F = 1
                for f in e.primes[lo:hi]:
                    F *= f
                u = max(x // F for x in M.basis_convert(ca[1][lo:hi], e.primes[lo:hi]))
                assert u <= hi - lo - 1
                if label == "y = f - 1":
                    assert u == hi - lo - 1
                seen_overshoot = max(seen_overshoot, u)
            for r in rot_r:
                e.rot(out, a, r, rk)
                want = model.rot(ca, rk_c[r], pow(5, r, 2 * n))
                assert out.nlimbs == lvl and np.array_equal(e.export(out), words(e, want)), where + ("rot", r)
            e.mul(out, a, b, rlk)
            want = model.mul(ca, cb, rlk_c)
            assert out.nlimbs == lvl and np.array_equal(e.export(out), words(e, want)), where + ("mul",)
            if lvl < 2:
                continue  # one limb: nothing to rescale away
            e.rescale(out)
            want = model.rescale(want)
            assert out.nlimbs == lvl - 1 and np.array_equal(e.export(out), words(e, want)), where + ("rescale",)
            e.mul_rescale(out, a, b, rlk)
            want = model.mul(ca, cb, rlk_c, rescale=True)
            assert out.nlimbs == lvl - 1 and np.array_equal(e.export(out), words(e, want)), where + ("mul_rescale",)
    assert seen_overshoot == e.info.alpha - 1
    for o in (a, b, out, pk, sk, rlk):
        e.free(o)
    e.free_evks(rk)
