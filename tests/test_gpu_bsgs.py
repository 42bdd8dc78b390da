"""he_gemv_bsgs / he_genrk_bsgs (include/gpqhe_ext.h) on the MI355X against
the composition that defines them, run on the oracle (tests/bsgs_ref.py):
every residue equal, level and scale as defined, and the decoded result
within the he_gemv tests' bound of M z.  Only the BSGS key subset exists on
either engine, so no other key can be read.  The shapes are the smallest that
reach each code path (see the table in each parametrisation)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bsgs_ref import bsgs_compose, bsgs_keys, bsgs_rotations, default_g
from tests.test_gpu_parity import PARAMS, same
from tests.test_gpu_rotations import init_slots

pytestmark = pytest.mark.gpu


def init(oracle, product, name, slots, seed=77):
    kind, kw = PARAMS[name]
    if kind != "init":
        return init_slots(oracle, product, name, slots, seed)
    for e in (oracle, product):
        e.init(**dict(kw, slots=slots))
        e.set_seed(seed)
    assert oracle.primes == product.primes


def matrix(s, seed, only=None):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (s, s)) + 1j * rng.uniform(-1, 1, (s, s))
    if only is not None:
        M = M * np.isin(np.add.outer(-np.arange(s), np.arange(s)) % s, only)
    return M


def vector(s, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)


class Side:
    """One engine's keys (the BSGS subset only) and an encrypted z."""

    def __init__(self, e, g, z, level=None, product_keys=False):
        self.e = e
        self.pk, self.sk = e.pk(), e.sk()
        e.keypair(self.pk, self.sk)
        if product_keys:
            self.rk = e.evks(e.slots)
            e.genrk_bsgs(self.rk, self.sk, g)
        else:
            self.rk = bsgs_keys(e, self.sk, g)
        self.x = self.enc(z, level)

    def enc(self, z, level=None):
        x = self.e.encrypt(z, self.pk)
        while level and x.nlimbs > level:
            self.e.moddown(x)
        return x

    def close(self):
        for o in (self.x, self.pk, self.sk):
            self.e.free(o)
        self.e.free_evks(self.rk)


def check(oracle, product, O, P, M, z, g, x_o=None, x_p=None):
    """he_gemv_bsgs on the product == bsgs_compose on the oracle."""
    x_o, x_p = x_o or O.x, x_p or P.x
    lvl, scale = x_p.nlimbs, x_p.scale
    yo = bsgs_compose(oracle, M, x_o, O.rk, g)
    yp = product.ct()
    product.gemv_bsgs(yp, M, x_p, P.rk, g)
    assert yp.nlimbs == lvl - 1 == yo.nlimbs
    assert yp.scale == scale and yp.flags == 0
    same(oracle, product, yo, yp)
    want = np.asarray(M).reshape(len(z), len(z)) @ z
    err = np.abs(product.decrypt(yp, P.sk) - want).max()
    assert err < 1e-6 * max(1.0, np.abs(want).max()), err
    oracle.free(yo)
    return yp


# ---------------------------------------------------------------------- keys
@pytest.mark.parametrize("name,slots,g,count", [("ref", 16, 4, 6), ("f13", 256, 0, 30)])
def test_genrk_bsgs_equals_genrot_sequence(oracle, product, name, slots, g, count):
    init(oracle, product, name, slots)
    assert product.bsgs_default_g() == default_g(slots)
    so, sp = oracle.sk(), product.sk()
    pko, pkp = oracle.pk(), product.pk()
    oracle.keypair(pko, so)
    product.keypair(pkp, sp)
    ro = bsgs_keys(oracle, so, g)
    rp = product.evks(slots)
    product.genrk_bsgs(rp, sp, g)
    held = [r for r in range(slots) if rp[r].data]
    assert held == bsgs_rotations(slots, g) and len(held) == count
    assert rp[0].galois == 1
    for r in held:
        assert rp[r].galois == pow(5, r, 2 * product.n) == ro[r].galois
        same(oracle, product, ro[r], rp[r])
    for e, objs, rk in ((oracle, (so, pko), ro), (product, (sp, pkp), rp)):
        for o in objs:
            e.free(o)
        e.free_evks(rk)


# -------------------------------------------------------------------- parity
# set, slots, g, level, diagonals: what it reaches
PARITY = [
    ("ref", 16, 4, 2, None),    # HECTR's ring, generic integer path, result at the lowest level
    ("ref", 16, 16, 2, None),   # G = 1: no giant rotation
    ("ref", 16, 1, 2, None),    # no baby rotation, 15 giants
    ("ref", 16, 6, 2, None),    # g does not divide s: the last giant step is partial
    ("ref", 32, 8, 2, (0, 1, 2, 9, 17, 31)),  # skipped babies and a j with one diagonal
    ("hyb", 32, 4, 5, None),    # K = 2, dnum = 3, partial last digit
    ("hyb", 32, 4, 4, None),    # ... input below the top level
    ("c1", 64, 0, 4, None),     # n = 2^13, 60-bit q0 / P: integer forms at a windowed-path ring size
    ("f13", 256, 0, 6, None),   # all-FP64 set; giants 64..240 wrap the Galois orbit; 256 diagonals in one launch
    ("bench51", 64, 0, 8, None),  # the headline ring, N = 2^16
    # more than 16 baby slots: bsgs_inner_kernel's later tiles add to what the first wrote
    ("ref", 32, 32, 2, None),   # G = 1, two full tiles of baby slots
    ("ref", 64, 24, 2, None),   # a partial second tile, giants present, the last giant step partial
    ("ref", 64, 32, 2, tuple(range(21)) + (33,)),  # giant step 1 has no diagonal in the second tile
    ("ref", 16, 4, 2, (5, 9, 14)),  # no diagonal in giant step 0: the sum starts without u_0
]


@pytest.mark.parametrize("name,slots,g,level,only", PARITY)
def test_gemv_bsgs_equals_composition(oracle, product, name, slots, g, level, only):
    init(oracle, product, name, slots)
    z, M = vector(slots, slots + level), matrix(slots, 3 * slots + g, only)
    O = Side(oracle, g, z, level)
    P = Side(product, g, z, level, product_keys=True)
    assert P.x.nlimbs == level == O.x.nlimbs
    yp = check(oracle, product, O, P, M, z, g)
    product.free(yp)
    O.close()
    P.close()


def test_zero_matrix(oracle, product):
    init(oracle, product, "ref", 16)
    z = vector(16, 5)
    P = Side(product, 4, z)
    y = product.ct()
    product.gemv_bsgs(y, np.zeros((16, 16)), P.x, P.rk, 4)
    assert y.nlimbs == P.x.nlimbs - 1 and y.scale == P.x.scale
    assert not product.export(y).any()
    product.free(y)
    P.close()


@pytest.mark.parametrize("g", [1, 16])
def test_workspace_chunks_do_not_change_bits(oracle, product, g, monkeypatch):
    """GPQHE_WS_MIB = 1: the key-switch workspaces of the 15 giant steps
    (g = 1) / the 15 baby steps (g = 16) are cut into several chunks."""
    monkeypatch.setenv("GPQHE_WS_MIB", "1")
    init(oracle, product, "ref", 16)
    z, M = vector(16, 8), matrix(16, 80 + g)
    O, P = Side(oracle, g, z), Side(product, g, z)
    product.free(check(oracle, product, O, P, M, z, g))
    O.close()
    P.close()


def test_small_diagonal_cache():
    """GPQHE_DIAG_MIB = 1 (read once per process, so a process of its own):
    a set larger than the cap is encoded into workspace on every call, and
    three plans rotate through a cache that holds two -- in each of the three
    plan caches (he_gemv_bsgs, he_gemv2_bsgs_batch, he_gemv2_rows_batch), their
    calls interleaved (tests/bsgs_cache_worker.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "bsgs_cache_worker.py")],
                       env=dict(os.environ, GPQHE_DIAG_MIB="1"), cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]) == {
        "ok": True, "calls": {"bsgs": 12, "pair": 12, "rows": 12}}


# --------------------------------------------------------------------- state
@pytest.mark.parametrize("name,slots,g,other", [("ref", 16, 4, ("hyb", 32)), ("f13", 256, 0, ("ref", 16))])
def test_state(oracle, product, name, slots, g, other):
    init(oracle, product, name, slots)
    z = vector(slots, 11)
    A, B = matrix(slots, 21), matrix(slots, 22)
    O, P = Side(oracle, g, z), Side(product, g, z)
    ya, yb = (oracle.export(y) for y in (bsgs_compose(oracle, A, O.x, O.rk, g), bsgs_compose(oracle, B, O.x, O.rk, g)))

    def run(M, x=None, y=None):
        y = y or product.ct()
        product.gemv_bsgs(y, M, x or P.x, P.rk, g)
        out = product.export(y)
        product.free(y)
        return out

    # the same call twice (the second is a cache hit), then alternated matrices
    for M, want in ((A, ya), (A, ya), (B, yb), (A, ya), (B, yb)):
        assert np.array_equal(run(M), want)
    # in place
    x2 = product.ct()
    product.copy_ct(x2, P.x)
    assert np.array_equal(run(A, x2, x2), ya)
    # one entry changed after the matrix was cached (in the caller's own buffer)
    A2 = A.copy()
    A2[3, 5] += 0.25
    y2 = bsgs_compose(oracle, A2, O.x, O.rk, g)
    assert np.array_equal(run(A2), oracle.export(y2))
    assert np.array_equal(run(A), ya)
    oracle.free(y2)
    O.close()
    P.close()
    # another parameter set after hectx_exit: nothing of the old cache is used
    for e in (oracle, product):
        e.exit()
    name2, slots2 = other
    init(oracle, product, name2, slots2)
    z2 = vector(slots2, 12)
    M2 = np.zeros((slots2, slots2), dtype=complex)
    M2[:min(slots, slots2), :min(slots, slots2)] = A[:min(slots, slots2), :min(slots, slots2)]
    O, P = Side(oracle, 0, z2), Side(product, 0, z2)
    product.free(check(oracle, product, O, P, M2, z2, 0))
    O.close()
    P.close()


# ------------------------------------------------------------ queue interplay
def test_queued_neighbours(oracle, product):
    """he_sub (queued on the product) -> he_gemv_bsgs -> he_add -> decrypt."""
    init(oracle, product, "ref", 16)
    za, zb, M = vector(16, 31), vector(16, 32), matrix(16, 33)
    outs = []
    for e in (oracle, product):
        S = Side(e, 4, za)
        b, d = S.enc(zb), e.ct()
        e.sub(d, S.x, b)
        if e is product:
            y = e.ct()
            e.gemv_bsgs(y, M, d, S.rk, 4)
        else:
            y = bsgs_compose(e, M, d, S.rk, 4)
        e.add(y, y, y)
        outs.append((e.export(y), e.decrypt(y, S.sk)))
        for o in (b, d, y):
            e.free(o)
        S.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    want = 2 * (M @ (za - zb))
    assert np.abs(outs[1][1] - want).max() < 1e-6 * max(1.0, np.abs(want).max())


# ---------------------------------------------------------------- statistics
def test_kernel_classes_are_reported(oracle, product):
    init(oracle, product, "ref", 16)
    z = vector(16, 41)
    P = Side(product, 4, z)
    y = product.ct()
    product.sync()
    product.prof_enable(True)
    try:
        product.prof_collect()
        product.gemv_bsgs(y, matrix(16, 42), P.x, P.rk, 4)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k, launches in (("bsgs_ks_kernel", 2), ("bsgs_inner_kernel", 1), ("bsgs_sum_kernel", 1)):
        assert k in stats, sorted(stats)
        assert stats[k][0] == launches and stats[k][2] > 0
    product.free(y)
    P.close()
