"""The CPU side of the level sweeps and of the small-ring tests: nothing there
may be right only because both engines are wrong in the same way.

* The shape labels (tests/level_shapes.py) and the sweep lists: the sweeps of
  tests/test_gpu_levels.py reach every distinct label of every parameter set.
* The oracle alone through the reference side of sweeps b and c (the single
  calls, he_rot_batch and he_gemv_batch) on genuine encryptions at every
  level: nlimbs, scale and the decoded values.  The bound is 1e-8, two decades
  over the 5e-11 measured for the oracle at these levels; it guards the
  sweeps' inputs and reference and says nothing about the kernels.
* The small-N step sequences (tests/small_n_steps.py) on the oracle at the
  other rings of tests/test_gpu_small_rings.py: every decoded vector within
  1e-6 of the plaintext step.
(tests/test_model_keyswitch.py pins the oracle's words to the exact integer
model at every level.)"""
import ctypes

import numpy as np
import pytest

from tests import level_shapes as LS
from tests import small_n_steps as S
from tests.test_gpu_parity import PARAMS


# --------------------------------------------------------------------------- labels
def test_shape_hand_checked():
    """hyb (L = 5, K = 2, alpha = 2; q0 58 bits, the rest below 2^51 except
    the 59-bit special primes) by hand."""
    primes = [1 << 57] + [1 << 44] * 4 + [1 << 58] * 2
    sh = LS.shape(5, 2, 2, primes, 5)
    assert (sh.ndig, sh.na_min, sh.targets) == (3, 1, 6)
    assert (sh.nd, sh.keep, sh.kept_cls, sh.drop_cls) == (2, 5, "iffff", "ii")
    assert (sh.nd_rs, sh.keep_rs, sh.kept_cls_rs, sh.drop_cls_rs) == (3, 4, "ifff", "fii")
    sh = LS.shape(5, 2, 2, primes, 2)
    assert (sh.ndig, sh.na_min, sh.targets, sh.keep_rs, sh.drop_cls_rs) == (1, 2, 2, 1, "fii")
    sh = LS.shape(5, 2, 2, primes, 1)
    assert (sh.ndig, sh.na_min, sh.targets, sh.keep, sh.kept_cls) == (1, 1, 2, 1, "i")
    assert "ndig=1 na_min=1 targets=2" in LS.label(sh)


def test_sweeps_cover_every_label(oracle):
    """Per set: the labels of every level he_mul_rescale_batch accepts (2..L)
    and, for the sets whose rotations and single calls are swept, of level 1
    too, are all reached by some sweep.  (Each level has its own label, so this
    holds while every sweep runs every level; it fails once one is thinned.)
    Also the path switches the sweeps exist for are where they are said to be."""
    labels = {}
    for name, (kind, kw) in PARAMS.items():
        if kind == "init":
            oracle.init(**kw)
        else:
            oracle.init_params(**kw)
        assert (kind == "init") or (oracle.L, oracle.K, oracle.info.alpha) == LS.geometry(kw)
        L = oracle.L
        labels[name] = {lvl: LS.engine_label(oracle, lvl) for lvl in range(1, L + 1)}
        assert len(set(labels[name].values())) == L
        reached = set()
        for sweep in LS.SWEEPS:
            reached |= {labels[name][lvl] for lvl in LS.sweep_levels(sweep, name, L)}
        low = 1 if name in LS.SWEEPS["single"][0] + LS.SWEEPS["rot_gemv_batch"][0] else 2
        missing = [lvl for lvl in range(low, L + 1) if labels[name][lvl] not in reached]
        if name != "ref":  # HECTR's own chain: n = 4096, not a key-switch tiling of these sweeps
            assert not missing, (name, missing)
        # the parts a sweep's levels run in leave none out
        for sweep in LS.SWEEPS:
            lv = LS.sweep_levels(sweep, name, L)
            if lv:
                parts = LS.sweep_parts(sweep, name, L)
                assert [x for a, b in parts for x in range(a, b + 1)] == lv, (sweep, name, parts)
    for sweep, sets in LS.PARTS.items():
        for name in sets:
            assert PARAMS[name][1]["logn"] == 17 and name in LS.SWEEPS[sweep][0]
    # c5 at level 8 and below: 8 conversion targets on a mixed prime set
    # (levels 9..12 have three digits and 12; at most 8 lets ks_cols4_kernel
    # run the column INTT itself)
    assert all("targets=8 " in labels["c5"][lvl] for lvl in range(5, 9)) and "targets=12 " in labels["c5"][9]
    assert "kept=ifffffff drop=iiii" in labels["c5"][8]
    # c1 and bench (alpha = 1): at most three digits from level 3 down
    for name in ("c1", "bench"):
        assert "ndig=3 " in labels[name][3] and "ndig=4 " in labels[name][4]
    # one digit at n = 2^14, 2^15 and 2^17
    for name in ("c14", "c15", "c17", "c5"):
        assert "ndig=1 " in labels[name][2]


# --------------------------------------------------------------------------- the reference side of sweeps b and c
TOL = 1e-8


def close(got, want, what):
    err = np.abs(got - want).max()
    assert err < TOL, (what, err)


@pytest.mark.parametrize("name", ["f13", "hyb", "c1"])
def test_oracle_single_calls_every_level(oracle, name):
    e = oracle
    kind, kw = PARAMS[name]
    e.init_params(**kw)
    e.set_seed(1234)
    s, delta = e.slots, e.info.delta
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rk = e.evks(s)
    rots = (1, s - 1)
    for r in rots:
        e.lib.he_genrot(ctypes.byref(rk[r]), r, ctypes.byref(sk))
    rng = np.random.default_rng(7)
    for lvl in range(1, e.L + 1):
        where = (name, lvl, LS.engine_label(e, lvl))
        z1 = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
        z2 = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
        a, b = e.encrypt(z1, pk, nlimbs=lvl), e.encrypt(z2, pk, nlimbs=lvl)
        assert a.nlimbs == lvl and a.scale == delta
        c = e.ct()
        for r in rots:
            e.rot(c, a, r, rk)
            assert c.nlimbs == lvl and c.scale == delta, where
            close(e.decrypt(c, sk), np.roll(z1, -r), where + ("rot", r))
        e.mul(c, a, b, rlk)
        assert c.nlimbs == lvl and c.scale == delta * delta, where
        if lvl >= 2:  # (at level 1 the scale exceeds q0: only the bits mean anything)
            close(e.decrypt(c, sk), z1 * z2, where + ("mul",))
            q = e.primes[lvl - 1]
            e.rescale(c)
            assert c.nlimbs == lvl - 1 and c.scale == delta * delta / q, where
            close(e.decrypt(c, sk), z1 * z2, where + ("mul_then_rescale",))
            e.mul_rescale(c, a, b, rlk)
            assert c.nlimbs == lvl - 1 and c.scale == delta * delta / q, where
            close(e.decrypt(c, sk), z1 * z2, where + ("mul_rescale",))
            e.copy_ct(c, a)
            e.mul_rescale(c, c, b, rlk)
            assert c.nlimbs == lvl - 1 and c.scale == delta * delta / q, where
            close(e.decrypt(c, sk), z1 * z2, where + ("mul_rescale_inplace",))
        for o in (a, b, c):
            e.free(o)
    for o in (pk, sk, rlk):
        e.free(o)
    e.free_evks(rk)


@pytest.mark.parametrize("name", ["f13", "hyb", "c1"])
def test_oracle_rot_gemv_batch_every_level(oracle, name):
    e = oracle
    kind, kw = PARAMS[name]
    e.init_params(**dict(kw, slots=16))
    e.set_seed(31)
    s, n, cnt, delta = 16, e.n, 2, e.info.delta
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = e.evks(s)
    e.genrk(rk, sk)
    M = LS.sweep_matrix(s, 9)
    Mc = np.ascontiguousarray(M.ravel(), dtype=np.complex128)

    def decoded(words, nl):
        ct = e.ct()
        e.import_(ct, words, nl, scale=delta)
        z = e.decrypt(ct, sk)
        e.free(ct)
        return z

    for lvl in range(1, e.L + 1):
        where = (name, lvl, LS.engine_label(e, lvl))
        zs = LS.sweep_vectors(cnt, s, 1000 + lvl)
        cts = [e.encrypt(z, pk, nlimbs=lvl) for z in zs]
        host = np.concatenate([e.export(c).ravel() for c in cts])
        for c in cts:
            e.free(c)
        for r in (1, s - 1):
            out = np.full(cnt * 2 * lvl * n, 7, dtype=np.uint64)
            e.lib.he_rot_batch(out.ctypes.data, host.ctypes.data, cnt, lvl, r, rk)
            for i in range(cnt):
                close(decoded(out.reshape(cnt, -1)[i], lvl), np.roll(zs[i], -r), where + ("rot_batch", r, i))
        if lvl >= 2:
            out = np.full(cnt * 2 * (lvl - 1) * n, 7, dtype=np.uint64)
            e.lib.he_gemv_batch(out.ctypes.data, Mc.ctypes.data, host.ctypes.data, cnt, lvl, rk)
            for i in range(cnt):
                close(decoded(out.reshape(cnt, -1)[i], lvl - 1), M @ zs[i], where + ("gemv_batch", i))
    for o in (pk, sk):
        e.free(o)
    e.free_evks(rk)


# --------------------------------------------------------------------------- the small rings on the oracle
@pytest.mark.parametrize("ring", list(S.PARAMS_RINGS))
@pytest.mark.parametrize("seq", list(S.SEQUENCES))
def test_oracle_small_ring_sequences(oracle, ring, seq):
    plain = []
    res = S.SEQUENCES[seq](oracle, params=S.PARAMS_RINGS[ring], plain=plain)
    assert plain, "no decoded vector"
    decoded = [i for i, x in enumerate(res) if np.iscomplexobj(x)]
    assert decoded == [i for i, _ in plain]
    for i, want in plain:
        err = np.abs(res[i] - want).max()
        assert err < 1e-6, (ring, seq, i, err)
