"""he_gemv2_bsgs_batch / he_hempc_step_batch (include/gpqhe_ext_step_batch.h)
on the MI355X against the compositions that define them, run on the oracle per
ciphertext (tests/step_ref.py), never against the product's own calls.

The scheme is test_gpu_bsgs_batch.py's: the product encrypts distinct vectors;
their exported words are the device input and, he_import-ed, the oracle's
ciphertexts; both engines hold the he_genrk_bsgs key subset from one seed.
Every word of every output must equal the oracle's, every up_i decode to
within 1e-6 max(1, |expected|) of the plaintext step (the BSGS tests' bound;
the reference alone stays near 1e-11), the 4096 guard words behind the output
and every input stay as they were.  The oracle's results are computed once per
shape (_REF).  The shapes are the smallest that reach each path."""
import ctypes as C

import numpy as np
import pytest

from hectr_amd import cstr
from tests.bsgs_ref import bsgs_compose
from tests.step_ref import gemv2_compose, step_compose
from tests.test_gpu_bsgs import matrix
from tests.test_gpu_bsgs_batch import FILL, GUARD, Pair, vectors

pytestmark = pytest.mark.gpu

_REF = {}  # (shape key) -> (input words, oracle words): computed once, shared, read-only


class StepPair(Pair):
    """Both engines, the same BSGS keys; inputs as blocks [k][cnt][2 level n]."""

    def blocks(self, slots, cnt, level, seed, k=4):
        """k blocks of cnt encryptions (the product's): (vectors [k][cnt], words [k][cnt][W], scale)."""
        zs = [vectors(slots, cnt, seed + 17 * b) for b in range(k)]
        words = []
        for b in range(k):
            w, scale = self.inputs(zs[b], level)
            words.append(w)
        return zs, np.stack(words), scale

    def reference(self, key, compose, H, level, scale, alias=None):
        """compose(e, [ciphertext of block b], rk, g) on the oracle for every
        ciphertext of the batch; alias {b: b'}: block b is block b' itself."""
        if key in _REF and np.array_equal(_REF[key][0], H):
            return _REF[key][1]
        rows = []
        for c in range(H.shape[1]):
            cts = []
            for b in range(H.shape[0]):
                x = self.o.ct()
                self.o.import_(x, H[b, c], level, scale=scale)
                cts.append(x)
            use = [cts[(alias or {}).get(b, b)] for b in range(H.shape[0])]
            y = compose(self.o, use, self.O.rk, self.g)
            assert y.nlimbs == level - 1 and np.isclose(y.scale, scale, rtol=1e-12)
            rows.append(self.o.export(y).ravel().copy())
            for x in cts + [y]:
                self.o.free(x)
        _REF[key] = (H.copy(), np.stack(rows))
        _REF[key][1].setflags(write=False)
        return _REF[key][1]

    def run(self, Ma, Mb, H, level, count=None, alias=None):
        """The product's call on device copies of the blocks (two blocks:
        he_gemv2_bsgs_batch, four: he_hempc_step_batch): output words [cnt][..];
        guard and inputs checked."""
        import torch
        k, n_ct = H.shape[0], H.shape[1]
        cnt = n_ct if count is None else count
        ow = 2 * (level - 1) * self.p.n
        din = torch.from_numpy(H.ravel().view(np.int64)).cuda()
        dout = torch.full((n_ct * ow + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptr = [din.data_ptr() + 8 * (alias or {}).get(b, b) * n_ct * H.shape[2] for b in range(k)]
        if k == 2:
            self.p.gemv2_bsgs_batch(dout.data_ptr(), Ma, ptr[0], Mb, ptr[1], cnt, level, self.P.rk, self.g)
        else:
            self.p.hempc_step_batch(dout.data_ptr(), Ma, Mb, ptr[0], ptr[1], ptr[2], ptr[3], cnt, level, self.P.rk,
                                    self.g)
        self.p.sync()
        got = dout.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[n_ct * ow:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        assert np.array_equal(din.cpu().numpy().view(np.uint64), H.ravel()), "an input was written"
        return got[:n_ct * ow].reshape(n_ct, ow)

    def decodes(self, got, want_z, level, scale):
        for i, w in enumerate(want_z):
            ct = self.p.ct()
            self.p.import_(ct, got[i], level - 1, scale=scale)
            err = np.abs(self.p.decrypt(ct, self.P.sk) - w).max()
            self.p.free(ct)
            assert err < 1e-6 * max(1.0, np.abs(w).max()), (i, err)

    def check_step(self, key, Ma, Mb, zs, H, level, scale, alias=None):
        """he_hempc_step_batch == step_compose, blocks (xhat, xr, uhat, ur)."""
        want = self.reference(key, lambda e, c, rk, g: step_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, g), H,
                              level, scale, alias)
        got = self.run(Ma, Mb, H, level, alias=alias)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        z = [zs[(alias or {}).get(b, b)] for b in range(4)]
        s = len(z[0][0])
        A, B = np.asarray(Ma).reshape(s, s), np.asarray(Mb).reshape(s, s)
        self.decodes(got, [z[2][i] - (A @ (z[0][i] - z[1][i]) + B @ (z[2][i] - z[3][i])) for i in range(len(got))],
                     level, scale)
        return want

    def check_gemv2(self, key, Ma, Mb, zs, H, level, scale, alias=None):
        """he_gemv2_bsgs_batch == gemv2_compose, blocks (xa, xb)."""
        want = self.reference(key, lambda e, c, rk, g: gemv2_compose(e, Ma, c[0], Mb, c[1], rk, g), H, level, scale,
                              alias)
        got = self.run(Ma, Mb, H, level, alias=alias)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        z = [zs[(alias or {}).get(b, b)] for b in range(2)]
        s = len(z[0][0])
        A, B = np.asarray(Ma).reshape(s, s), np.asarray(Mb).reshape(s, s)
        self.decodes(got, [A @ z[0][i] + B @ z[1][i] for i in range(len(got))], level, scale)
        return want


def matrices(slots, g, only_a=None, only_b=None):
    return matrix(slots, 3 * slots + g, only_a), matrix(slots, 5 * slots + g + 1, only_b)


# set, slots, g, level, cnt, diagonals of Ma, of Mb: what it reaches
PARITY = [
    # generic rotations (n = 4096)
    ("ref", 16, 4, 2, 1, None, None),   # a lone ciphertext tile; 8 combined baby slots: the TB 8 form
    ("ref", 16, 4, 2, 5, None, None),   # a partial last ciphertext tile
    ("ref", 16, 8, 2, 3, None, None),   # 16 combined slots: one TB 16 tile
    ("ref", 16, 16, 2, 3, None, None),  # G = 1: no giant rotation, no sum; 32 combined slots, two tiles
    ("ref", 64, 24, 2, 3, None, None),  # 48 combined slots: a partial last baby tile, a partial last giant step
    ("ref", 16, 1, 2, 3, None, None),   # no rotated baby
    ("ref", 16, 4, 2, 3, (0, 1, 2, 5), (9, 14)),  # disjoint giant steps; Mb has no unrotated slot
    ("ref", 16, 4, 2, 3, (5, 9, 14), (6, 13)),    # nothing in giant step 0, no unrotated slot in either
    # windowed rotations (folded keys, k_gemv_batch over the chunk)
    ("hyb", 32, 4, 5, 3, None, None),   # K = 2, three digits, the last partial, integer slots
    ("hyb", 32, 4, 4, 3, None, None),   # ... below the top level
    ("f13", 64, 0, 6, 3, None, None),   # all-FP64
    ("bench51", 64, 0, 8, 2, None, None),  # the headline ring, N = 2^16
    # a large ring without the windowed path: four digits
    ("c1", 64, 0, 4, 2, None, None),
]
GEMV2 = [c for c in PARITY if c[0] == "ref"] + [PARITY[8]]  # the operands given: slot 0 is a copy of them


@pytest.mark.parametrize("name,slots,g,level,cnt,da,db", PARITY)
def test_step_equals_composition(oracle, product, name, slots, g, level, cnt, da, db):
    pr = StepPair(oracle, product, name, slots, g)
    Ma, Mb = matrices(slots, g, da, db)
    zs, H, scale = pr.blocks(slots, cnt, level, level)
    pr.check_step(("step", name, slots, g, level, cnt, da, db), Ma, Mb, zs, H, level, scale)
    pr.close()


@pytest.mark.parametrize("name,slots,g,level,cnt,da,db", GEMV2)
def test_gemv2_equals_composition(oracle, product, name, slots, g, level, cnt, da, db):
    pr = StepPair(oracle, product, name, slots, g)
    Ma, Mb = matrices(slots, g, da, db)
    zs, H, scale = pr.blocks(slots, cnt, level, level, k=2)
    pr.check_gemv2(("gemv2", name, slots, g, level, cnt, da, db), Ma, Mb, zs, H, level, scale)
    pr.close()


def test_one_matrix_zero_is_the_single_product(oracle, product):
    """Mb = 0: the bits of bsgs_compose(Ma, xa); likewise Ma = 0.  And the step with them."""
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    Z = np.zeros((16, 16))
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    wa = pr.reference(("bsgs a",), lambda e, c, rk, g: bsgs_compose(e, Ma, c[0], rk, g), H[:2], 2, scale)
    wb = pr.reference(("bsgs b",), lambda e, c, rk, g: bsgs_compose(e, Mb, c[1], rk, g), H[:2], 2, scale)
    assert np.array_equal(pr.run(Ma, Z, H[:2], 2), wa)
    assert np.array_equal(pr.run(Z, Mb, H[:2], 2), wb)
    pr.check_step(("step Mb=0",), Ma, Z, zs, H, 2, scale)
    pr.check_step(("step Ma=0",), Z, Mb, zs, H, 2, scale)
    pr.close()


def test_zero_matrices_and_empty_batch(oracle, product):
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    Z = np.zeros((16, 16))
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    assert not pr.run(Z, Z, H[:2], 2).any()  # y zeroed: the sentinel is overwritten
    low = H[2].reshape(3, 2, 2, -1)[:, :, :1, :].reshape(3, -1)
    assert np.array_equal(pr.run(Z, Z, H, 2), low)  # up = he_moddown(uhat) exactly
    assert (pr.run(Ma, Mb, H[:2], 2, count=0) == FILL).all()  # nothing touched
    assert (pr.run(Ma, Mb, H, 2, count=0) == FILL).all()
    pr.close()


def test_operands_that_are_one_array(oracle, product):
    """xa and xb the same array; the step with xr the same array as xhat (a zero difference)."""
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    pr.check_gemv2(("gemv2 xa is xb",), Ma, Mb, zs, H[:2], 2, scale, alias={1: 0})
    pr.check_step(("step xr is xhat",), Ma, Mb, zs, H, 2, scale, alias={1: 0})
    pr.close()


@pytest.mark.parametrize("name,level", [("ref", 2), ("f13", 6)])
def test_forced_chunks_do_not_change_bits(oracle, product, name, level, monkeypatch):
    """GPQHE_BSGS_CHUNK = 2: five ciphertexts as 2 + 2 + 1."""
    monkeypatch.setenv("GPQHE_BSGS_CHUNK", "2")
    pr = StepPair(oracle, product, name, 16, 4)
    Ma, Mb = matrices(16, 4)
    zs, H, scale = pr.blocks(16, 5, level, level)
    pr.check_step(("step", name, 16, 4, level, 5, None, None), Ma, Mb, zs, H, level, scale)
    pr.close()


def test_workspace_chunks_do_not_change_bits(oracle, product, monkeypatch):
    """GPQHE_WS_MIB = 1: every chunk holds one ciphertext and the stages' own workspaces are cut."""
    monkeypatch.setenv("GPQHE_WS_MIB", "1")
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    zs, H, scale = pr.blocks(16, 5, 2, 2)
    pr.check_step(("step", "ref", 16, 4, 2, 5, None, None), Ma, Mb, zs, H, 2, scale)
    pr.close()


def test_state(oracle, product):
    """A repeat call (a pair-plan hit), the swapped pair (an entry of its
    own), re-keyed rotations (no stale fold), another parameter set after
    hectx_exit."""
    name, slots, g, level = "f13", 16, 4, 6
    pr = StepPair(oracle, product, name, slots, g)
    Ma, Mb = matrices(slots, g)
    zs, H, scale = pr.blocks(slots, 2, level, 9)
    w = pr.check_step((name, "ab"), Ma, Mb, zs, H, level, scale)
    assert np.array_equal(pr.run(Ma, Mb, H, level), w)  # a hit
    wba = pr.check_step((name, "ba"), Mb, Ma, zs, H, level, scale)
    assert not np.array_equal(wba, w)
    assert np.array_equal(pr.run(Ma, Mb, H, level), w)
    # a baby and a giant rotation re-keyed on the product, copied to the oracle
    for r in (1, 2 * g):
        product.lib.he_free_evk(C.byref(pr.P.rk[r]))
        product.lib.he_genrot(C.byref(pr.P.rk[r]), r, C.byref(pr.P.sk))
        oracle.import_(pr.O.rk[r], product.export(pr.P.rk[r]), pr.P.rk[r].nlimbs)
    w2 = pr.check_step((name, "ab rekeyed"), Ma, Mb, zs, H, level, scale)
    assert not np.array_equal(w2, w)
    pr.close()
    for e in (oracle, product):
        e.exit()
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    zs, H, scale = pr.blocks(16, 3, 2, 4)
    pr.check_step(("ref", "after exit"), Ma, Mb, zs, H, 2, scale)
    pr.close()


def test_kernel_classes_are_reported(oracle, product):
    pr = StepPair(oracle, product, "ref", 16, 4)
    Ma, Mb = matrices(16, 4)
    zs, H, scale = pr.blocks(16, 3, 2, 6)
    pr.run(Ma, Mb, H, 2)  # warm
    product.prof_enable(True)
    try:
        product.prof_collect()
        pr.run(Ma, Mb, H, 2)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k in ("step_diff_batch_kernel", "step_tail_batch_kernel", "bsgs_inner_batch_kernel"):
        assert k in stats, sorted(stats)
        assert stats[k][0] == 1 and stats[k][2] > 0, (k, stats[k])
    pr.close()


def test_closed_loop_of_three_plants(product):
    """simulate_batch of three CstrProblem(40) with different disturbance steps
    through BatchedEncryptedRegulator on HECTR's parameters: every step's u
    within 1e-8 max(1, |u|) of regulator_plain on that step's own inputs (the
    reference composition's worst error on six such steps: 1.9e-11)."""
    problems = [cstr.CstrProblem(40) for _ in range(3)]
    for pb, (k0, amp) in zip(problems[1:], ((5, -0.05), (20, 0.08))):
        pb.p = np.zeros(40)
        pb.p[k0:] = amp * cstr.F0S
    reg = cstr.BatchedEncryptedRegulator(product, problems[0], 3, seed=2024)
    worst = [0.0]

    def on_step(k, xhat, uhat, xr, ur, u):
        for i, pb in enumerate(problems):
            want = pb.regulator_plain(xhat[i], uhat[i], xr[i], ur[i])
            err = np.abs(u[i] - want).max()
            worst[0] = max(worst[0], err)
            assert err < 1e-8 * max(1.0, np.abs(want).max()), (k, i, err)

    x, u = cstr.simulate_batch(problems, reg, on_step)
    print(f"closed loop: worst |u - plain| {worst[0]:.3e}")
    assert len(reg.timings) == 40 and x.shape == (3, 41, 3) and u.shape == (3, 40, 2)
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[1], u[2])
    reg.close()
