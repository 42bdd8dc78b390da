"""Noise audit of the step compositions (tests/step_ref.py, rows_ref.py,
packed_ref.py, encgain_ref.py: the definitions of he_hempc_step_batch and its
rows, packed and encrypted-gain forms) run on the oracle, against the analytic
model (tests/ckks_model.noise_terms, ops step / rows / packed / encgain).

The bit-for-bit tests prove that the product computes these compositions; this
one asks whether the compositions lose more precision than they must.  Exact
decryption of the result minus the exact expected message -- built from the
exact decryptions of the four inputs and the engine's own plaintexts of the
gains (for the encrypted gains, their exact decryptions), so that the noise is
what the key switches, ModDowns and rescales add -- stays under |bias| + 6
sigma for every seed, and no ceiling is more than 4x the largest noise measured
over the three seeds: a composition that loses two bits more fails.  The
constants are test_noise_cpu.py's.  CPU only; the product's outputs are held to
the same ceilings in tests/test_gpu_batch_audit.py."""
import pytest

import noise_audit as A
from tests.test_noise_cpu import CTX, NON_VACUITY, SEEDS

DENSE, SPARSE = list(range(16)), [0, 1, 5, 9, 12]
#: context, slots S, arguments of noise_audit.measure_step
CASES = {
    # the BSGS step over two operands: default g = 4 (four giant steps), Ma dense, Mb five diagonals
    "n10p-step": ("n10p", 16, dict(kind="step", diags=(DENSE, SPARSE))),
    "n10one-step": ("n10one", 16, dict(kind="step", diags=(DENSE, SPARSE))),
    "n10p-step-g8": ("n10p", 16, dict(kind="step", g=8, diags=(SPARSE, DENSE))),
    # the row fold: rows 2 of 16 slots is one baby rotation and three folds (8 images)
    "n10p-rows2": ("n10p", 16, dict(kind="rows", rows=2)),
    "n10one-rows2": ("n10one", 16, dict(kind="rows", rows=2)),
    "n10p-rows3": ("n10p", 16, dict(kind="rows", rows=3)),  # m' = 4: a padded zero row, two folds
    # S = 16, s = 8, P = 2: rotations in steps of P, two folds
    "n10p-packed": ("n10p", 16, dict(kind="packed", s=8, rows=2)),
    "n10one-packed": ("n10one", 16, dict(kind="packed", s=8, rows=2)),
    "n10p-encgain": ("n10p", 16, dict(kind="encgain", s=8, rows=2)),
    "n10one-encgain": ("n10one", 16, dict(kind="encgain", s=8, rows=2)),
    "n10p-encgain-sk": ("n10p", 16, dict(kind="encgain", s=8, rows=2, sym=True)),
    # n = 2^13, K = 3, two digits of three limbs; S = 64, s = 16, P = 4: three folds
    "f13-packed": ("f13", 64, dict(kind="packed", s=16, rows=2)),
    "f13-encgain": ("f13", 64, dict(kind="encgain", s=16, rows=2)),
}

_cache = {}


def measured(oracle, case):
    """([(max, mean) per seed], [ceiling per seed]), computed once per case."""
    if case not in _cache:
        name, S, kw = CASES[case]
        oracle.init_params(slots=S, seed=1, **CTX[name])
        runs, ceils = [], []
        for seed in SEEDS:
            stats, extra = A.measure_step(oracle, seed, **kw)
            runs.append(stats[0])
            ceils.append(A.step_ceiling(oracle, kw["kind"], extra))
        _cache[case] = (runs, ceils)
    return _cache[case]


@pytest.mark.parametrize("case", list(CASES))
def test_step_noise_under_ceiling_and_ceiling_not_vacuous(oracle, case):
    runs, ceils = measured(oracle, case)
    for seed, (mx, mean), c in zip(SEEDS, runs, ceils):
        print(f"{case} seed {seed}: max |noise| {mx:.6g} mean {mean:.6g} ceiling {c:.6g}")
        assert mx <= c, (case, seed)
    worst = max(mx for mx, _ in runs)
    print(f"{case}: ceiling / maximum = {max(ceils) / worst:.2f}")
    assert max(ceils) <= NON_VACUITY * worst, case

