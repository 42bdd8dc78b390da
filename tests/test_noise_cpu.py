"""Noise audit of the oracle against the analytic model
(tests/ckks_model.noise_terms): exact decryption minus the exact expected
message stays under |bias| + 6 sigma of every modelled term, and no ceiling is
more than 4x the largest noise measured over the three seeds (so two lost bits
of precision fail).  Also the encoding error at HECTR's scale 2^50 against a
100-bit mpmath encoding.  CPU only; the product runs the same audit in
tests/test_gpu_noise_audit.py."""
import numpy as np
import pytest

import ckks_model as M
import noise_audit as A

SEEDS = (1, 7, 99)
CTX = {
    "n10a1": dict(logn=10, nlimbs=3, nspecial=1, dnum=3, q0_bits=60, qi_bits=50, p_bits=60),
    "n10p": dict(logn=10, nlimbs=5, nspecial=2, dnum=3, q0_bits=58, qi_bits=45, p_bits=59),
    "n10one": dict(logn=10, nlimbs=4, nspecial=4, dnum=1, q0_bits=51, qi_bits=48, p_bits=51),
    "f13": dict(logn=13, nlimbs=6, nspecial=3, dnum=2, q0_bits=51, qi_bits=48, p_bits=51),
}
#: the non-zero diagonals of the he_gemv cases (16 slots)
GEMV = {"gemv_dense": list(range(16)), "gemv_sparse": [3, 7, 12], "gemv_0_1": [0, 1]}
#: the baby-step giant-step cases: (non-zero diagonals, baby steps g); g = 4 is
#: the default for 16 slots (four giant steps), g = 8 has two
BSGS = {"bsgs_dense": (list(range(16)), 4), "bsgs_sparse": ([0, 1, 5, 9, 12], 4), "bsgs_g8": (list(range(16)), 8)}
NON_VACUITY = 4.0

_cache = {}


def measured(oracle, name, op):
    """([(max, mean) per seed], [ceiling per seed]) of one operation in a
    context; the single-operation measurements of a context are made together,
    once, each he_gemv case on its own."""
    group = op if op in GEMV or op in BSGS else "ops"
    if (name, group) not in _cache:
        oracle.init_params(slots=A.SLOTS, seed=1, **CTX[name])
        if group == "ops":
            per_seed = [A.measure_ops(oracle, seed) for seed in SEEDS]
            _cache[name, group] = {o: ([r[o] for r, _ in per_seed], [A.ceiling_of(oracle, o, x) for _, x in per_seed])
                                   for o in A.OPS}
        elif op in BSGS:
            runs = [A.measure_bsgs(oracle, seed, *BSGS[op]) for seed in SEEDS]
            _cache[name, group] = {op: ([st for st, _ in runs], [A.bsgs_ceiling(oracle, x) for _, x in runs])}
        else:
            runs = [A.measure_gemv(oracle, seed, GEMV[op]) for seed in SEEDS]
            _cache[name, group] = {op: ([st for st, _ in runs], [A.gemv_ceiling(oracle, x) for _, x in runs])}
    return _cache[name, group][op]


#: every operation in every context (the dense cases at n = 2^13 generate
#: fifteen rotation keys per seed on the CPU and take a few seconds each)
CASES = [(name, op) for name in CTX for op in list(A.OPS) + list(GEMV) + list(BSGS)]


@pytest.mark.parametrize("name,op", CASES)
def test_noise_under_ceiling_and_ceiling_not_vacuous(oracle, name, op):
    runs, ceils = measured(oracle, name, op)
    for seed, (mx, mean), c in zip(SEEDS, runs, ceils):
        print(f"{name} {op} seed {seed}: max |noise| {mx:.6g} mean {mean:.6g} ceiling {c:.6g}")
        assert mx <= c, (name, op, seed)
    assert max(ceils) <= NON_VACUITY * max(mx for mx, _ in runs), (name, op)


def test_offsets_are_key_dependent_not_a_bias(oracle):
    """The mean over one output's coefficients of the key-switch noise is an
    offset of tens of units, but a different one per key: the walk of
    noise_terms' `md` and `ks` notes, not a bias.  Over these three seeds the
    offsets of one rotation have both signs (a fact of these seeds' streams,
    recorded here; any three keys may agree in sign one time in four), and
    each stays under the walk's own ceiling: md(K) alone puts
    (K/2) (2 S_k - S_n) on coefficient k, S the partial sums of the secret,
    whose average over k has variance (K/2)^2 (n/2) / 3; 6 sigma of that, plus
    the bias K/2."""
    name = "n10one"
    n, K = 1 << CTX[name]["logn"], CTX[name]["nspecial"]
    means = [m for _, m in measured(oracle, name, "rot")[0]]
    assert min(means) < 0 < max(means)
    assert max(abs(m) for m in means) <= K / 2 + 6 * (K / 2) * np.sqrt(n / 2 / 3)


# --------------------------------------------------------------------------- encoding error
def mp_encode(z, scale):
    """scale u_k (real, imaginary parts) of the special inverse FFT at 120 bits."""
    import mpmath as mp
    mp.mp.prec = 120
    s = len(z)
    Mm = 4 * s
    root = [mp.expjpi(mp.mpf(-2 * k) / Mm) for k in range(Mm)]
    zz = [mp.mpc(v.real, v.imag) for v in z]
    rot = [pow(5, j, Mm) for j in range(s)]
    out = []
    for k in range(s):
        acc = mp.mpc(0)
        for j in range(s):
            acc += zz[j] * root[k * rot[j] % Mm]
        out.append(acc * scale / s)
    return out


@pytest.mark.parametrize("slots", [16, 128])
def test_encoding_error_at_scale_2_50(oracle, slots):
    """he_ecd_ex at Delta = 2^50, |z| <= 4, slots 16 and n/2, against mpmath:
    every coefficient within encode_error_ceiling, the ceiling within 4x the
    largest error seen, and decode(encode(z)) within decode_error_ceiling."""
    import mpmath as mp
    scale = 2.0 ** 50
    oracle.init_params(logn=8, nlimbs=2, nspecial=1, dnum=2, slots=slots, q0_bits=60, qi_bits=50, p_bits=60, seed=3)
    n = oracle.n
    gap = n // (2 * slots)
    worst = worst_z = 0.0
    pt = oracle.pt()
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        r, phi = 4 * np.sqrt(rng.uniform(0, 1, slots)), rng.uniform(0, 2 * np.pi, slots)
        z = r * np.exp(1j * phi)
        assert np.abs(z).max() <= 4
        z_rms = float(np.sqrt(np.mean(np.abs(z) ** 2)))
        oracle.ecd_ex(pt, z, slots, scale, 2)
        coef = A.exact_plain(oracle, pt)
        ref = mp_encode(z, mp.mpf(scale))
        ceil = M.encode_error_ceiling(scale, slots, z_rms)
        used = set()
        for k in range(slots):
            for idx, want in ((k * gap, ref[k].real), ((k + slots) * gap, ref[k].imag)):
                used.add(idx)
                err = float(abs(int(coef[idx]) - want))
                assert err <= ceil, (slots, seed, idx, err, ceil)
                worst = max(worst, err)
        assert all(int(coef[i]) == 0 for i in range(n) if i not in used)
        back = oracle.dcd(pt, slots)
        dz = float(np.abs(back - z).max())
        assert dz <= M.decode_error_ceiling(scale, slots, z_rms), (slots, seed, dz)
        worst_z = max(worst_z, dz)
        print(f"slots {slots} seed {seed}: coefficient error {worst:.4f} ceiling {ceil:.4f}; "
              f"decode error {dz:.3e} ceiling {M.decode_error_ceiling(scale, slots, z_rms):.3e}")
    assert ceil <= NON_VACUITY * worst
    assert M.decode_error_ceiling(scale, slots, z_rms) <= NON_VACUITY * worst_z
    oracle.free(pt)


@pytest.mark.parametrize("slots", [16, 128, 4096])
def test_twiddle_table_error(slots):
    """The figure fft_error_factor rests on, measured and not inferred from the
    encoding test: the engine's table is cos, sin of fl(2 pi k / M), M = 4 slots,
    k = 0..M (the same double expression is formed here), and its
    mean squared distance from the exact root, by mpmath at 120 bits, must lie
    under the modelled TWIDDLE_VAR u^2 and above a quarter of it -- and well
    above the (4/3) u^2 of a stage's arithmetic, which is the claim that the
    table dominates."""
    import math

    import mpmath as mp
    mp.mp.prec = 120
    Mm = 4 * slots
    tot = 0.0
    for k in range(Mm + 1):
        ang = 2.0 * math.pi * float(k) / float(Mm)
        t = 2 * mp.pi * k / Mm
        tot += float((mp.mpf(math.cos(ang)) - mp.cos(t)) ** 2 + (mp.mpf(math.sin(ang)) - mp.sin(t)) ** 2)
    mean = tot / (Mm + 1) / M.UNIT_ROUNDOFF ** 2
    print(f"M = {Mm}: mean |twiddle error|^2 = {mean:.2f} u^2 (model {M.TWIDDLE_VAR})")
    assert M.TWIDDLE_VAR / NON_VACUITY <= mean <= M.TWIDDLE_VAR
    assert mean > 2 * 4.0 / 3.0
