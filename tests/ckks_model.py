"""Independent pure-Python big-integer model of the arithmetic the engine
claims to compute (test infrastructure only).

Nothing here shares code with the oracle (C) or the product (HIP): NTTs are
evaluated from the definition, polynomials are multiplied by schoolbook
negacyclic convolution, RNS values are recombined with exact Python
integers.  Used to pin the oracle (tests/test_oracle_model.py) and to make
the committed known-answer vectors (tests/make_golden.py).
"""
from __future__ import annotations

import cmath
import math


def brev(x: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def is_prime(n: int) -> bool:
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_eval(a, q, psi):
    """A[k] = a(psi^(2 brev(k) + 1)) mod q (bit-reversed evaluation order)."""
    n = len(a)
    logn = n.bit_length() - 1
    out = []
    for k in range(n):
        x = pow(psi, 2 * brev(k, logn) + 1, q)
        acc, p = 0, 1
        for c in a:
            acc = (acc + c * p) % q
            p = p * x % q
        out.append(acc)
    return out


def negacyclic_mul(a, b, q):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if not x:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] = (out[k] + x * y) % q
            else:
                out[k - n] = (out[k - n] - x * y) % q
    return out


def automorphism(a, g, q):
    """a(X) -> a(X^g) in Z_q[X]/(X^n + 1)."""
    n = len(a)
    out = [0] * n
    for j, c in enumerate(a):
        e = j * g % (2 * n)
        if e < n:
            out[e] = (out[e] + c) % q
        else:
            out[e - n] = (out[e - n] - c) % q
    return out


def crt(residues, primes):
    """Exact value in [0, prod primes)."""
    Q = 1
    for p in primes:
        Q *= p
    x = 0
    for r, p in zip(residues, primes):
        Qi = Q // p
        x += r * Qi * pow(Qi, -1, p)
    return x % Q, Q


def center(x, Q):
    return x - Q if x > Q // 2 else x


def special_decode(u):
    """z_j = sum_k u_k xi^(k 5^j), xi = exp(2 pi i / 4s)."""
    s = len(u)
    M = 4 * s
    return [sum(u[k] * cmath.exp(2j * math.pi * k * pow(5, j, M) / M) for k in range(s)) for j in range(s)]


def special_encode(z):
    s = len(z)
    M = 4 * s
    return [sum(z[j] * cmath.exp(-2j * math.pi * k * pow(5, j, M) / M) for j in range(s)) / s for k in range(s)]


def encode_coeffs(z, n, scale):
    """Coefficients of the CKKS encoding of z (len s) at `scale`."""
    s = len(z)
    u = special_encode(z)
    gap = n // (2 * s)
    coef = [0] * n
    for k in range(s):
        coef[k * gap] = round(u[k].real * scale)
        coef[(k + s) * gap] = round(u[k].imag * scale)
    return coef


def intt_eval(A, q, psi):
    """Inverse of ntt_eval, from the definition:
    a_j = n^-1 sum_k A[k] psi^(-(2 brev(k) + 1) j) mod q."""
    n = len(A)
    logn = n.bit_length() - 1
    ninv = pow(n, -1, q)
    xs = [pow(psi, -(2 * brev(k, logn) + 1), q) for k in range(n)]
    pw = [1] * n
    out = []
    for _ in range(n):
        out.append(sum(a * p for a, p in zip(A, pw)) % q * ninv % q)
        pw = [p * x % q for p, x in zip(pw, xs)]
    return out


def negacyclic_mul_int(a, b):
    """Exact product in Z[X]/(X^n + 1) of non-negative integer coefficient
    lists, by Kronecker substitution (one big-integer multiplication)."""
    n = len(a)
    width = (max(a).bit_length() + max(b).bit_length() + n.bit_length() + 7) // 8 + 1
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(width, "little") for x in v), "little")
    raw = (pack(a) * pack(b)).to_bytes(2 * n * width, "little")
    c = [int.from_bytes(raw[i * width:(i + 1) * width], "little") for i in range(2 * n)]
    return [c[i] - c[i + n] for i in range(n)]


def automorphism_int(a, g):
    """a(X) -> a(X^g) in Z[X]/(X^n + 1) (no modulus: signs stay signs)."""
    n = len(a)
    out = [0] * n
    for j, c in enumerate(a):
        e = j * g % (2 * n)
        if e < n:
            out[e] += c
        else:
            out[e - n] -= c
    return out


def basis_convert(res, mods):
    """The engine's approximate basis conversion, as an integer: for residues
    res[i][k] modulo mods[i] with F = prod mods,
        y_i = x_i (F / f_i)^-1 mod f_i,   x~ = sum_i y_i (F / f_i),
    kept unreduced.  x~ = x + u F for the x in [0, F) the residues name and an
    overshoot u in [0, len(mods))."""
    F = 1
    for f in mods:
        F *= f
    hat = [F // f for f in mods]
    inv = [pow(h, -1, f) for h, f in zip(hat, mods)]
    n = len(res[0])
    return [sum(res[i][k] * inv[i] % mods[i] * hat[i] for i in range(len(mods))) for k in range(n)]


class HybridModel:
    """Exact restatement, in Python integers on coefficient vectors, of the
    engine's hybrid key switch and of the three operations built on it.

    primes: the L + K moduli (q_0 .. q_{L-1}, then the special primes, P their
    product); alpha: limbs per digit.  A ciphertext is [2][lvl][n] coefficient
    residues; an evaluation key is [2 dnum][L + K][n] coefficient residues
    (b_0, a_0, b_1, a_1, ...).

    key_switch(d, key, lvl, g):
      1. digit split: digit j is limbs [j alpha, min((j+1) alpha, lvl));
      2. ModUp: x~_j = basis_convert(digit j) as an unreduced integer vector;
      3. if g != 1, x~_j <- x~_j(X^g) -- the automorphism acts on the
         *converted digits*, after the decomposition (the order matters: the
         conversion of q - x is not minus the conversion of x);
      4. inner product over the basis Q_lvl u P: acc0 = sum_j x~_j b_j,
         acc1 = sum_j x~_j a_j modulo every modulus of the basis.
    mod_down(X, lvl, top): (X - x~_D) D^-1 on the kept limbs, D = P or P q_top
      and x~_D = basis_convert of X's residues on the dropped moduli.

    he_rot   = mod_down(key_switch(c1, rot key, g) + (P c0(X^g), 0))
               -- c0 is folded in before the single ModDown, times P;
    he_mul   = mod_down(key_switch(d2, rlk) + P (d0, d1)), d the tensor;
    he_mul_rescale = the same with the single ModDown by P q_top;
    he_rescale = mod_down by q_top alone (exact floor division).
    """

    def __init__(self, primes, L, alpha):
        self.primes = list(primes)
        self.L = L
        self.K = len(primes) - L
        self.alpha = alpha
        self.P = 1
        for p in primes[L:]:
            self.P *= p

    def basis(self, lvl):
        return list(range(lvl)) + list(range(self.L, self.L + self.K))

    def digits(self, lvl):
        return [(lo, min(lo + self.alpha, lvl)) for lo in range(0, lvl, self.alpha)]

    def mod_up(self, d, lvl):
        return [basis_convert(d[lo:hi], self.primes[lo:hi]) for lo, hi in self.digits(lvl)]

    def key_switch(self, d, key, lvl, g=1):
        """{modulus index: (acc0, acc1)} over basis(lvl)."""
        dig = self.mod_up(d, lvl)
        if g != 1:
            dig = [automorphism_int(x, g) for x in dig]
        out = {}
        for m in self.basis(lvl):
            q = self.primes[m]
            acc = [[0] * len(d[0]), [0] * len(d[0])]
            for j, x in enumerate(dig):
                xm = [v % q for v in x]
                for p in range(2):
                    prod = negacyclic_mul_int(xm, key[2 * j + p][m])
                    acc[p] = [(u + v) % q for u, v in zip(acc[p], prod)]
            out[m] = acc
        return out

    def mod_down(self, X, lvl, top=False):
        """X: {modulus index: coefficients} over basis(lvl) -> [kept limbs][n]."""
        drop = ([lvl - 1] if top else []) + list(range(self.L, self.L + self.K))
        keep = range(lvl - 1 if top else lvl)
        D = 1
        for m in drop:
            D *= self.primes[m]
        conv = basis_convert([X[m] for m in drop], [self.primes[m] for m in drop])
        out = []
        for t in keep:
            q = self.primes[t]
            dinv = pow(D, -1, q)
            out.append([(x - c) * dinv % q for x, c in zip(X[t], conv)])
        return out

    def _finish(self, acc, add0, add1, lvl, top):
        for t in range(lvl):
            q = self.primes[t]
            acc[t][0] = [(u + self.P * v) % q for u, v in zip(acc[t][0], add0[t])]
            if add1 is not None:
                acc[t][1] = [(u + self.P * v) % q for u, v in zip(acc[t][1], add1[t])]
        return [self.mod_down({m: acc[m][p] for m in acc}, lvl, top) for p in range(2)]

    def rot(self, ct, key, g):
        lvl = len(ct[0])
        acc = self.key_switch(ct[1], key, lvl, g)
        return self._finish(acc, [automorphism(ct[0][t], g, self.primes[t]) for t in range(lvl)], None, lvl, False)

    def mul(self, a, b, rlk, rescale=False):
        lvl = min(len(a[0]), len(b[0]))
        d0, d1, d2 = [], [], []
        for t in range(lvl):
            q = self.primes[t]
            a0, a1, b0, b1 = a[0][t], a[1][t], b[0][t], b[1][t]
            d0.append([v % q for v in negacyclic_mul_int(a0, b0)])
            d1.append([(u + v) % q for u, v in zip(negacyclic_mul_int(a0, b1), negacyclic_mul_int(a1, b0))])
            d2.append([v % q for v in negacyclic_mul_int(a1, b1)])
        return self._finish(self.key_switch(d2, rlk, lvl), d0, d1, lvl, rescale)

    def rescale(self, ct):
        lvl = len(ct[0])
        out = []
        for p in range(2):
            top = ct[p][lvl - 1]
            out.append([[(x - c) * pow(self.primes[lvl - 1], -1, self.primes[t]) % self.primes[t]
                         for x, c in zip(ct[p][t], top)] for t in range(lvl - 1)])
        return out


# --------------------------------------------------------------------------- noise model
CBD_VAR = 10.5   # centred binomial, eta = 21: variance eta / 2, |e| <= 21
TERNARY_DENSITY = 0.5  # P(s_i != 0); s_i = +-1 equally likely, so E s_i = 0, E s_i^2 = 1/2
SIGMAS = 6.0


class Term:
    """One modelled noise term: every coefficient has mean `bias` and variance
    `var` (over keys, encryption randomness and uniform ciphertext words)."""

    def __init__(self, bias=0.0, var=0.0):
        self.bias, self.var = float(bias), float(var)

    def __add__(self, o):  # independent terms
        return Term(self.bias + o.bias, self.var + o.var)

    def scaled(self, c):
        return Term(self.bias * c, self.var * c * c)

    @property
    def ceiling(self):
        return abs(self.bias) + SIGMAS * math.sqrt(self.var)


def _uniform_sum_moments(k):
    """Mean and mean square of a sum of k independent uniforms on [0, 1)."""
    return k / 2.0, k / 12.0 + k * k / 4.0


def noise_terms(params, op, **kw):
    """The modelled noise of `op` as a Term; noise_ceilings() is its ceiling.

    params: n; primes (all L + K); L; alpha; lvl (the level of the operands).
    Noise is dec(ct) - expected, in coefficient units, dec = c0 + c1 s centred.

    Derivations (n coefficients; e ~ CBD with variance V = 10.5 and mean 0;
    s, v ternary with E x = 0, E x^2 = 1/2; a negacyclic product of independent
    zero-mean polynomials a, b has coefficient variance n Var a Var b, and with
    one factor of non-zero mean, n E[a^2] Var b):

    enc_sk   c0 + c1 s = m + e: bias 0, variance V.
    enc_pk   m + e_pk v + e0 + e1 s: variance n V/2 + V + n V/2 = V (n + 1).
    add, sub of independent ciphertexts: variances add.  neg, moddown (which
             drops a limb and leaves the centred value alone): unchanged.
    add_pt   unchanged (the plaintext is exact).
    mul_pt   noise(X) * pt(X): variance var_in ||pt||_2^2, with
             ||pt||_2^2 = scale^2 mean|z_j|^2 (kw pt_norm2), because the special
             FFT is unitary up to 1/s: sum_k |u_k|^2 = (1/s) sum_j |z_j|^2.  The
             fresh noise it multiplies has uncorrelated coefficients.
    ks       the key switch before ModDown decrypts to P m' + E with
             E = sum_j d~_j * e_j (digit j's converted integer d~_j times that
             digit's key error, permuted by the automorphism for a rotation,
             which changes no moment).  d~_j / Q_j is a sum of alpha_j
             independent uniforms on [0, 1) -- the conversion is unsigned --
             so E[d~_j^2] = Q_j^2 (alpha_j/12 + alpha_j^2/4) and, e_j having
             mean 0, E has bias 0 and variance n V sum_j E[d~_j^2].  After the
             division by D (P, or P q_top): variance / D^2.
             The non-zero mean of d~_j does not bias E but makes its
             coefficients correlated: coefficient k carries
             mean(d~_j) (sum_{t<=k} e_j[t] - sum_{t>k} e_j[t]), a random walk in
             the key's error that is the same for every ciphertext under one
             key.  Averaged over the coefficients of one output it looks like
             an offset; over keys it has mean 0.
    md       ModDown by D = product of k dropped moduli computes, per polynomial,
             (X - x~_D) / D with x~_D / D a sum of k independent uniforms
             r in [0, k); so dec changes by -(r0 + r1 * s): bias -k/2 (from
             r0; r1 * s has mean 0 because E s = 0), variance
             k/12 + (n/2) (k/12 + k^2/4).  Again the non-zero mean of r1 makes
             (k/2) (sum_{t<=k} s[t] - sum_{t>k} s[t]) a walk in the secret,
             common to all outputs under one key.  k = 1 is he_rescale (exact
             floor division), k = K the ModDown by P, k = K + 1 the fused one.
    rot           = ks / P + md(K)
    mul           = ks / P + md(K)            against dec(a) dec(b)
    mul+rescale   = (the above) / q_top + md(1)     against dec(a) dec(b) / q_top
    mul_rescale   = ks / (P q_top) + md(K + 1)      against dec(a) dec(b) / q_top
    gemv     y = sum_d pt_d * rot_d(x) with one ModDown by D = P q_top (pt_d:
             diagonal d encoded at scale q_top; kw diags: the coefficient
             vectors of the non-zero diagonals d != 0; diagonal 0 multiplies
             P (c0, c1) and adds no noise).  Each diagonal has its own key, so
             the terms are independent: term d is (pt_d * d~_j(X^g)) * e_{d,j}
             with variance V ||pt_d * d~_j(X^g)||_2^2 (kw diags: {d: coefficients}).
             With d~_j's coefficients independent of mean mu_j = Q_j alpha_j / 2
             and variance Q_j^2 alpha_j / 12,
               E ||pt * d~(X^g)||^2 = n ||pt||_2^2 Var d~ + mu^2 ||pt * 1(X^g)||_2^2,
             1 the all-ones polynomial: the automorphism acts on the converted
             digit, so the digit's mean becomes a vector of signs.
             gemv = sum_d term_d / (P q_top) + md(K + 1), against
             sum_d pt_d * dec(x)(X^g_d) / q_top.
    gemv_bsgs  y = rescale(sum_j rot_{jg}(u_j)), u_j = sum_i pt_{j,i} * b_i,
             b_i = rot_i(x) (kw g; kw steps: {giant step j: {baby i != 0:
             coefficients of pt_{j,i}}}).  Baby i carries
             N_i = E_i / P - r0_i - r1_i * s (rot above), so u_j's noise is
             sum_i pt_{j,i} * N_i, which the giant rotation maps to X^(5^jg).
             With S_j = sum_i pt_{j,i} and T_k(S) = sum_{i<=k} S[i] - sum_{i>k} S[i]
             (= S times the all-ones polynomial):
               walk     the means K/2 of the r1_i give (K/2) T(S_j) * s.  All
                        giant steps share the one secret, so the variance of
                        their sum is computed exactly per output coefficient:
                        coefficient k of step j reads coefficient
                        k 5^(-jg) mod 2n of the antiperiodic extension, the
                        cross terms are negacyclic cross-correlations of the
                        T(S_j) at the difference of those indices, and the
                        largest coefficient's variance is taken;
               bias     the means K/2 of the r0_i give -(K/2) T_k(S_j),
                        summed over j after the rotation; largest |.| taken;
               rest     per step: sum_i (the he_gemv term of pt_{j,i} with
                        D = P and rotation i; independent keys), r0_i about
                        its mean (K/12) ||pt_{j,i}||^2, (r1_i about its mean)
                        * s: (1/2) n (K/12) ||pt_{j,i}||^2.  Steps reuse the
                        babies, so these are correlated across j in a way not
                        modelled: their standard deviations are added (the
                        standard deviation of a sum is at most the sum of the
                        standard deviations).  The rest is uncorrelated with
                        the walk (zero-mean fluctuations, independent keys),
                        so its variance adds to the walk's.
             Each step j != 0 adds one more rot noise; all of it is divided
             by q_top, and he_rescale adds md(1).  Against
             sum_{j,i} pt_{j,i}(X^(5^jg)) * dec(x)(X^(5^(jg+i))) / q_top.
    step     up = moddown(uhat) - y, y the gemv_bsgs of TWO operands with shared
             giants: u_j = sum_i pt^A_{j,i} * a_i + pt^B_{j,i} * b_i, a_i =
             rot_i(xa), b_i = rot_i(xb) (kw g; kw steps: {j: {i != 0: [the
             plaintexts of every operand that has diagonal jg + i]}}).  The
             subtractions before and after and he_moddown add nothing, so the
             noise is -noise(y): the gemv_bsgs terms with, per giant step,
             S_j = sum over both operands, and one change: a_i and b_i are
             rotated by the SAME key, so in E^a_i = sum_j d~^a_j(X^g) * e_{i,j}
             and E^b_i the key errors are shared.  The digits of the two
             ciphertexts are independent words, so their fluctuations add in
             variance, V n (||pt^A||^2 + ||pt^B||^2) Var d~, but their common
             mean mu_j adds before it is squared: V mu^2 ||(pt^A + pt^B) *
             1(X^g)||^2 (ks_shared).  r0 and r1 of the two ModDowns are
             independent; their means go into the walk and the bias through S_j.
    rows, packed   y = F(rescale(u)), u = sum_r sum_o pt_{r,o} * rot_r(x_o) over
             the baby rotations r (kw babies: {r != 0: [plaintexts]}; rows: r = i,
             packed: r = i P), F = prod_t (1 + sigma_{r_t}) the fold
             u <- u + rot(u, r_t) (kw folds: r_0, r_1, ..: m', 2m', .. times P).
             With R = -(K/2) - (K/2) 1 * s + rho one rotation's noise (rho of
             mean 0: E / P and the fluctuations of r0, r1 * s; rot above),
               u1 = rescale(u) carries -(b1 + w1 * s) + rho1,
               b1 = w1 = (K/2) T(S) / q_top + 1/2,   S = sum of all pt_{r,o},
               Var rho1 = [sum_r ks_shared + ||pt||^2 (K/12)(1 + n/2)] / q_top^2
                          + (1/12)(1 + n/2)           (the rescale is md(1)),
             and fold step t adds R_t (at the level below) AFTER doubling what
             is there: u_{t+1} = u_t + sigma_{r_t}(u_t) + R_t.  Unrolled,
               noise(y) = sum_{g in G_0} sigma_g(u1's) + sum_t sum_{g in G_{t+1}} sigma_g(R_t),
             G_t the 2^(T-t) rotations that are sums of subsets of r_t .. r_{T-1}:
             the baby term appears under all 2^T images, the noise of fold step
             t under 2^(T-1-t).  An automorphism permutes coefficients (with
             signs), so for a typical output coefficient the images are
             different coefficients and the variance doubles per fold step --
             but coefficient 0 (and every k with k (5^r - 1) = 0 mod 2n) is
             fixed by all of them, where the images add coherently.  A ceiling
             on the max-norm has to hold there, so:
               walk, bias  every term -(b + w * s) of every image is a fixed
                        polynomial times the one secret: variance and bias per
                        output coefficient are exact (images(): the
                        cross-correlations of the w at the index differences,
                        as for gemv_bsgs), the largest is taken;
               rest     the rho of the images of one polynomial are taken as
                        fully coherent (standard deviations added: |G_0|
                        sqrt(Var rho1) + sum_t |G_{t+1}| sqrt(Var rho_t)),
                        which is what coefficient 0 sees; uncorrelated with
                        the walk, so the variances of the two add.
             This is why the ceiling of 2^T images is about sqrt(2^T) above a
             typical coefficient's 6 sigma; T = 3 in the audited shapes.
             Against F(sum pt_{r,o} * dec(x_o)(X^(5^r))) / q_top.
    encgain  the same with the gains encrypted: the 2 m' pairs (rot_r(x_o),
             D_{r,o}) are tensored and summed, X0 + X1 s + X2 s^2 =
             sum dec(rot_r(x_o)) dec(D_{r,o}) exactly, so the babies' noise is
             sum_r R_r * dec(D_{r,o}): the baby terms above with the exact
             decryption of the gain ciphertext (diagonal at scale q_top plus
             its fresh noise) in the place of the plaintext (dense, so the
             products are taken by FFT).  The division is not one rescale but
             two: (X0, X1) by he_rescale, md(1), and the quadratic term by one
             relinearisation with the fused ModDown, ks(P q_top) + md(K + 1)
             (mul_rescale above, of (0, X2) and (0, 1): no other term).  So
               b1 = w1 = (K/2) T(S) / q_top + (K + 2)/2,
               Var rho1 = [babies] / q_top^2 + ks(P q_top)
                          + ((K + 1)/12 + 1/12)(1 + n/2),
             then the fold as above.  Against
             F(sum dec(D_{r,o}) * dec(x_o)(X^(5^r))) / q_top.
    """
    n, primes, L, alpha, lvl = params["n"], params["primes"], params["L"], params["alpha"], params["lvl"]
    K = len(primes) - L
    V = CBD_VAR
    P = 1
    for p in primes[L:]:
        P *= p
    fresh_pk = Term(0, V * (n + 1))
    fresh_sk = Term(0, V)

    def md(k):
        mean, sq = _uniform_sum_moments(k)
        return Term(-mean, k / 12.0 + n * TERNARY_DENSITY * sq)

    def ks(D, level=None):
        level = lvl if level is None else level
        tot = 0.0
        for lo in range(0, level, alpha):
            hi = min(lo + alpha, level)
            Q = 1
            for f in primes[lo:hi]:
                Q *= f
            tot += (Q / D) ** 2 * _uniform_sum_moments(hi - lo)[1]
        return Term(0, n * V * tot)

    import numpy as np

    def shifted(c, i):
        """c(X) X^i in R[X]/(X^n + 1)."""
        return np.concatenate([-c[n - i:], c[:n - i]]) if i else c

    def times(pt, c):
        """pt * c for a sparse integer pt and a float vector c."""
        out = np.zeros(n)
        for i, v in enumerate(pt):
            if v:
                out += float(v) * shifted(c, i)
        return out

    ones = np.ones(n)

    def ks_times(pt, D, r):
        """Variance per coefficient of pt * (sum_j d~_j(X^(5^r)) * e_j) / D: V times
        E ||pt * d~(X^g)||^2 = n ||pt||^2 Var d~ + mu^2 ||pt * 1(X^g)||^2, 1 the
        all-ones polynomial (whose image under the automorphism is a vector of
        signs: the mean of the rotated digit)."""
        norm2 = float(sum(c * c for c in pt))
        signs = np.array(automorphism_int([1] * n, pow(5, r, 2 * n)), dtype=float)
        mean2 = float(np.sum(times(pt, signs) ** 2))
        tot = 0.0
        for lo in range(0, lvl, alpha):
            a = min(lo + alpha, lvl) - lo
            Q = 1
            for f in primes[lo:lo + a]:
                Q *= f
            tot += (Q / D) ** 2 * (n * norm2 * a / 12.0 + (a / 2.0) ** 2 * mean2)
        return V * tot

    def conv(a, b):
        """a * b in R[X]/(X^n + 1) for float vectors (one FFT of length 2 n)."""
        c = np.fft.irfft(np.fft.rfft(a, 2 * n) * np.fft.rfft(b, 2 * n), 2 * n)
        return c[:n] - c[n:]

    def ks_shared(pts, D, r, level=None):
        """ks_times for operands rotated by the SAME key (rotation r): the
        variance per coefficient of (sum_o pt_o * d~_{o,j}(X^(5^r))) * e_j / D.
        The operands' digits are independent ciphertext words, so the
        fluctuations of the d~_{o,j} add in variance (n ||pt_o||^2 Var d~ each),
        but they have one mean mu_j, whose terms add before they are squared:
        mu^2 ||(sum_o pt_o) * 1(X^g)||^2."""
        level = lvl if level is None else level
        pts = [np.asarray(pt, dtype=float) for pt in pts]
        norm2 = float(sum(np.dot(pt, pt) for pt in pts))
        signs = np.array(automorphism_int([1] * n, pow(5, r, 2 * n)), dtype=float)
        mean2 = float(np.sum(conv(sum(pts), signs) ** 2))
        tot = 0.0
        for lo in range(0, level, alpha):
            a = min(lo + alpha, level) - lo
            Q = 1
            for f in primes[lo:lo + a]:
                Q *= f
            tot += (Q / D) ** 2 * (n * norm2 * a / 12.0 + (a / 2.0) ** 2 * mean2)
        return V * tot

    def images(items):
        """(largest |bias|, largest walk variance / E s^2) over the output
        coefficients of sum_m sigma_m(b_m + w_m * s), sigma_m the automorphism
        X -> X^(5^r_m), for items (r_m, b_m, w_m) of fixed real polynomials.
        Coefficient k of image m reads coefficient k 5^(-r_m) mod 2n of the
        antiperiodic extension; the sum is linear in the one secret, so its
        variance per output coefficient is exact: (E s^2) || sum_m w_m^(k) ||^2,
        whose cross terms are negacyclic cross-correlations of the w_m at the
        difference of those indices."""
        ext = lambda v: np.concatenate([v, -v])  # one period of the antiperiodic extension
        full = lambda v: np.full(n, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=float)
        items = [(r, full(b), full(w)) for r, b, w in items]
        at = [(np.arange(n) * pow(pow(5, r, 2 * n), -1, 2 * n)) % (2 * n) for r, _, _ in items]
        fw = [np.fft.fft(ext(w)) for _, _, w in items]
        bias, var = np.zeros(n), np.zeros(n)
        for a, (_, b, w) in enumerate(items):
            bias += ext(b)[at[a]]
            var += float(np.sum(w * w))
            for c in range(a + 1, len(items)):
                rho = np.real(np.fft.ifft(np.conj(fw[a]) * fw[c])) / 2.0
                var += 2.0 * rho[(at[c] - at[a]) % (2 * n)]
        return float(np.abs(bias).max()), float(var.max())

    def baby_terms(babies, level_D=P):
        """For u = sum over rotations r != 0 and operands o of pt_{r,o} * rot_r(x_o)
        (babies: {r: [pt_{r,o}]}): (T(S), variance of the rest).  Every rotated
        operand carries N = E / P - r0 - r1 * s (rot above), so u's noise is
        sum pt * N: the means K/2 of the r0 and r1 give (K/2) T(S) and
        (K/2) T(S) * s, S the sum of all the plaintexts, T(S) = S * 1 (partial
        sums: T_k = 2 sum_{i<=k} S_i - sum_i S_i); the rest is the key-switch
        term of every rotation (ks_shared: one key per rotation, shared by the
        operands), r0 about its mean (K/12) ||pt||^2 and (r1 about its mean) * s,
        (1/2) n (K/12) ||pt||^2, of every plaintext."""
        S, var = np.zeros(n), 0.0
        for r, pts in babies.items():
            pts = [np.asarray(pt, dtype=float) for pt in pts]
            norm2 = float(sum(np.dot(pt, pt) for pt in pts))
            S = S + sum(pts)
            var += ks_shared(pts, level_D, r) + norm2 * (K / 12.0) * (1.0 + TERNARY_DENSITY * n)
        return 2.0 * np.cumsum(S) - S.sum(), var

    def bsgs(steps, g):
        """steps: {giant step j: {baby i != 0: [coefficients of pt_{j,i} of every operand]}}"""
        qtop = primes[lvl - 1]
        mean, sq = _uniform_sum_moments(K)
        items, rest_sigma = [], 0.0
        for j, pts in steps.items():
            if not pts:
                continue
            T, var = baby_terms(pts)
            rest_sigma += math.sqrt(var)
            # the means of the r0_i and of the r1_i, after the giant rotation:
            # (K/2) T(S_j) and (K/2) T(S_j) * s
            items.append((j * g, mean * T, mean * T))
        # the walks of all giant steps are linear in the one secret: exact
        # variance per output coefficient k, (1/2) || sum_j w_j^(k) ||^2
        bias, var_walk = images(items) if items else (0.0, 0.0)
        giants = sum(1 for j in steps if j)
        giant = ks(P) + md(K)
        rest_sigma += giants * math.sqrt(giant.var)
        # the walk (the secret times fixed polynomials) is uncorrelated with the
        # rest (zero-mean fluctuations and key errors): variances add
        var = TERNARY_DENSITY * var_walk + rest_sigma ** 2
        return Term((bias + giants * abs(giant.bias)) / qtop, var / qtop ** 2) + md(1)

    if op == "gemv":
        D = P * primes[lvl - 1]
        return Term(0, sum(ks_times(pt, D, d) for d, pt in kw["diags"].items())) + md(K + 1)
    if op == "gemv_bsgs":
        return bsgs({j: {i: [pt] for i, pt in pts.items()} for j, pts in kw["steps"].items()}, kw["g"])
    if op == "step":
        return bsgs(kw["steps"], kw["g"])
    if op in ("rows", "packed", "encgain"):
        qtop = primes[lvl - 1]
        mean = K / 2.0
        T, var1 = baby_terms(kw["babies"])
        var1 /= float(qtop) ** 2
        # the division: he_rescale, or for the encrypted gains one relinearisation
        # of X2 with the fused ModDown by P q_top beside he_rescale of (X0, X1)
        drop = (K + 2) if op == "encgain" else 1
        if op == "encgain":
            var1 += ks(P * qtop).var
        first = mean * T / qtop + drop / 2.0
        var1 += (drop / 12.0) * (1.0 + TERNARY_DENSITY * n)
        folds = list(kw["folds"])
        sums = lambda rs: [sum(r for b, r in enumerate(rs) if m >> b & 1) for m in range(1 << len(rs))]
        items = [(r, first, first) for r in sums(folds)]
        rest_sigma = len(items) * math.sqrt(var1)
        var_rot = ks(P, lvl - 1).var + (K / 12.0) * (1.0 + TERNARY_DENSITY * n)
        for t in range(len(folds)):
            later = sums(folds[t + 1:])
            items += [(r, mean, mean) for r in later]
            rest_sigma += len(later) * math.sqrt(var_rot)
        bias, var_walk = images(items)
        return Term(bias, TERNARY_DENSITY * var_walk + rest_sigma ** 2)
    if op == "enc_pk":
        return fresh_pk
    if op == "enc_sk":
        return fresh_sk
    if op in ("add", "sub"):
        return fresh_pk + fresh_pk
    if op in ("neg", "moddown", "add_pt"):
        return fresh_pk
    if op == "mul_pt":
        return fresh_pk.scaled(math.sqrt(kw["pt_norm2"]))
    if op in ("rot", "mul"):
        return ks(P) + md(K)
    if op == "mul+rescale":
        return (ks(P) + md(K)).scaled(1.0 / primes[lvl - 1]) + md(1)
    if op == "mul_rescale":
        return ks(P * primes[lvl - 1]) + md(K + 1)
    raise ValueError(op)


def noise_ceilings(params, op, **kw):
    """|bias| + 6 standard deviations of the modelled noise of op (max-norm
    ceiling per coefficient; see noise_terms for the derivations)."""
    return noise_terms(params, op, **kw).ceiling


# --------------------------------------------------------------------------- encoding error
UNIT_ROUNDOFF = 2.0 ** -53
#: modelled mean of |table entry - exp(2 pi i k / M)|^2 over the engine's
#: twiddle table, in units of u^2 (fft_error_factor derives it;
#: test_twiddle_table_error measures 4.2 .. 4.7 against mpmath)
TWIDDLE_VAR = 6.0
#: relative error variance one FFT stage leaves, in u^2: 4/3 + TWIDDLE_VAR, rounded up
STAGE_VAR = 7.5


def fft_error_factor(slots):
    """gamma: six standard deviations of the relative error a double-precision
    radix-2 special FFT leaves on one output, relative to the root mean square
    output magnitude.

    A butterfly output a + w b costs four roundings per real component (two
    products, their difference, the sum), each of relative variance at most
    u^2 / 3 (u = 2^-53), on components that carry half of |w b|^2 each:
    (4/3) u^2 |b|^2 per complex output.  The engine's twiddle table is
    cos, sin of fl(2 pi k / M): the angle carries the rounding of the product
    (relative variance u^2 / 3; the division by the power of two M is exact)
    and of pi (0.35 u), so its absolute error has variance
    ang^2 (1/3 + 0.35^2) u^2, which averaged over angles uniform on [0, 2 pi)
    (mean ang^2 = (2 pi)^2 / 3) is 6.0 u^2: the twiddle, not the arithmetic,
    dominates.  One stage leaves a relative error of variance at most
    (4/3 + 6.0) u^2 < 7.5 u^2; the stages are unitary up to a common factor
    (they neither shrink nor amplify earlier errors relative to the signal) and
    their errors are independent, so after t stages the relative error has
    standard deviation u sqrt(7.5 t).  t = log2(4 slots) counts the log2(slots)
    butterfly stages plus two for the scalings by 1/slots and by the scale.
    gamma = 6 u sqrt(7.5 log2(4 slots))."""
    assert 4.0 / 3.0 + TWIDDLE_VAR <= STAGE_VAR
    return SIGMAS * UNIT_ROUNDOFF * math.sqrt(STAGE_VAR * math.log2(4 * slots))


def encode_error_ceiling(scale, slots, z_rms):
    """Ceiling on |coefficient - scale u_k| of he_ecd_ex: 0.5 for the rounding
    to an integer plus scale ||u|| gamma, where ||u|| = z_rms / sqrt(slots) is
    the root mean square of the |u_k| (sum_k |u_k|^2 = (1/s) sum_j |z_j|^2)."""
    return 0.5 + scale * (z_rms / math.sqrt(slots)) * fft_error_factor(slots)


def decode_error_ceiling(scale, slots, z_rms):
    """Ceiling on |he_dcd(he_ecd(z))_j - z_j|, six standard deviations of two
    independent errors whose variances add: the 2 s coefficient errors
    (rounding, variance 1/12 each, plus the encoding FFT's) pass through the
    unitary-up-to-scale decoding transform, z_j = sum_k u_k xi^(..), so
    E |dz_j|^2 = 2 s (1/12 + sigma_fft^2) / scale^2; the decoding FFT adds its
    own relative error, variance (z_rms gamma / 6)^2."""
    sig_fft = scale * (z_rms / math.sqrt(slots)) * fft_error_factor(slots) / SIGMAS
    var_coef = 2 * slots * (1.0 / 12.0 + sig_fft ** 2) / scale ** 2
    var_fft = (z_rms * fft_error_factor(slots) / SIGMAS) ** 2
    return SIGMAS * math.sqrt(var_coef + var_fft)
