"""What the key-switch dispatch branches on at one level of one parameter set.

The host code picks its kernels from the level alone (kernels.hip
k_mul_split_ok / mul_split_launch, ks_split.hip ksq_dispatch / ksq_stage,
gemv_win.hip k_gemv_win_ok): the number of digits, the size of the last digit,
the number of conversion targets per digit, the ModDown's dropped and kept
slots, and the arithmetic class (modulus below 2^51: the FP64 forms; else the
integer forms) of each of them.  shape() restates those quantities in plain
Python from the parameters and the engine's primes, label() prints them; every
failure message of the level sweeps (tests/test_gpu_levels.py) carries the
label, so a failing level says what is special about it.

SWEEPS lists which sets and levels each sweep runs; tests/test_levels_cpu.py
asserts that together they reach every distinct label of every set.
"""
from collections import namedtuple

#: ndig, na_min (size of the last digit), targets (nm - na_min: conversion
#: targets of the last digit, the most any digit has), and per form of the
#: ModDown (plain: he_mul / he_rot; rescale: he_mul_rescale) the number of
#: dropped moduli nd, of kept limbs, and the class string of the kept and the
#: dropped slots ("f": modulus below 2^51, "i": 2^51 or more)
Shape = namedtuple("Shape", "ndig na_min targets nd keep kept_cls drop_cls nd_rs keep_rs kept_cls_rs drop_cls_rs")


def geometry(kw):
    """(L, K, alpha) of a PARAMS entry's keyword dict (hectx_init_params:
    nspecial defaults to 1, dnum to nlimbs, alpha = ceil(L / dnum))."""
    L = kw["nlimbs"]
    K = kw.get("nspecial", 1)
    dnum = kw.get("dnum") or L
    return L, K, (L + dnum - 1) // dnum


def cls(q):
    return "f" if q < (1 << 51) else "i"


def shape(L, K, alpha, primes, lvl):
    """primes: the engine's list, L chain moduli then K special ones."""
    assert 1 <= lvl <= L and len(primes) == L + K
    ndig = (lvl + alpha - 1) // alpha
    na_min = lvl - (ndig - 1) * alpha
    nm = lvl + K
    special = "".join(cls(q) for q in primes[L:])
    chain = "".join(cls(q) for q in primes[:lvl])
    return Shape(ndig, na_min, nm - na_min,
                 K, lvl, chain, special,
                 K + 1, lvl - 1, chain[:lvl - 1], chain[lvl - 1:] + special)


def label(sh):
    return (f"ndig={sh.ndig} na_min={sh.na_min} targets={sh.targets} "
            f"plain(nd={sh.nd} keep={sh.keep} kept={sh.kept_cls or '-'} drop={sh.drop_cls}) "
            f"rescale(nd={sh.nd_rs} keep={sh.keep_rs} kept={sh.kept_cls_rs or '-'} drop={sh.drop_cls_rs})")


def engine_label(e, lvl):
    """The label of level lvl on an initialised engine."""
    return label(shape(e.L, e.K, e.info.alpha, e.primes, lvl))


def levels(L, lo):
    return list(range(lo, L + 1))


#: sweep -> (sets, lowest level); every sweep runs each level from there to L
SWEEPS = {
    "mul_rescale_batch": (["bench", "bench_d2", "bench51", "c5", "c5f", "c17", "c14", "c15", "i14", "f13", "f15", "a5",
                           "m60", "c1", "hyb", "k5"], 2),
    "single": (["f13", "hyb", "a5", "c14", "i14", "c15", "f15", "bench51", "bench_d2", "m60", "c17", "c5"], 1),
    "rot_gemv_batch": (["f13", "c1", "hyb", "c14", "c15", "i14", "k5", "bench51", "bench_d2", "m60", "c5f", "c5"], 1),
    "families": (["f13", "hyb", "c1", "c15"], 2),
}

def sweep_vectors(cnt, s, seed):
    """The slot vectors sweep c encrypts: both parts uniform in [-1/4, 1/4].

    A result must still fit one limb: on the sets whose q0 has 51 bits at
    Delta = 2^50 (bench51, c5f, c17) a level-1 ciphertext holds coefficients
    below q0 / 2, about Delta.  A coefficient of an encoding is Delta times an
    average of the 2 s slot values and their conjugates under unit-modulus
    weights, so at most Delta max|z|: here 0.36 Delta for the rotations'
    results and, with sweep_matrix, 0.5 Delta for M z."""
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.25, 0.25, (cnt, s)) + 1j * rng.uniform(-0.25, 0.25, (cnt, s))


def sweep_matrix(s, seed):
    """Sweep c's matrix: entries of modulus at most sqrt(2) / s (so |M z| <=
    sqrt(2) max|z|), every third diagonal zero (skipped by both engines)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    M = (rng.uniform(-1, 1, (s, s)) + 1j * rng.uniform(-1, 1, (s, s))) / s
    return M * (np.add.outer(-np.arange(s), np.arange(s)) % s % 3 != 2)


#: the 2^17 sets run their levels as several tests (the oracle's time there):
#: sweep -> set -> the first level of each part
PARTS = {
    "mul_rescale_batch": {"c5": [2, 8], "c5f": [2, 8], "c17": [2, 5]},
    "single": {"c5": [1, 8], "c17": [1, 5]},
    # (generating the 16 rotation keys on both engines is most of a part's
    # time at n = 2^17: about 15 s of each part's 16 to 19 s)
    "rot_gemv_batch": {"c5": [1, 6, 9, 11], "c5f": [1, 6, 9, 11]},
}


def sweep_levels(sweep, name, L):
    """The levels sweep `sweep` runs on set `name`."""
    sets, lo = SWEEPS[sweep]
    return levels(L, lo) if name in sets else []


def sweep_parts(sweep, name, L):
    """sweep_levels cut into the tests that run them: [(first, last), ...]."""
    lv = sweep_levels(sweep, name, L)
    starts = PARTS.get(sweep, {}).get(name, lv[:1])
    assert not lv or starts[0] == lv[0]
    return [(a, b - 1) for a, b in zip(starts, starts[1:] + [L + 1])]
