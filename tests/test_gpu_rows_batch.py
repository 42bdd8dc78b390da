"""he_genrk_rows / he_gemv2_rows_batch / he_hempc_step_rows_batch
(include/gpqhe_ext_rows_batch.h) on the MI355X against the compositions that
define them, run on the oracle per ciphertext (tests/rows_ref.py), never
against the product's own calls.

The scheme is test_gpu_step_batch.py's: the product encrypts distinct vectors;
their exported words are the device input and, he_import-ed, the oracle's
ciphertexts; both engines hold the row-folding key subset from one seed.  Every
word of every output must equal the oracle's, the first `rows` slots of every
result decode to within 1e-6 max(1, |expected|) of the plaintext (the BSGS
tests' bound; the reference alone stays below 2e-9), the 4096 guard words
behind the output and every input stay as they were.  The oracle's results are
computed once per shape.  The shapes are the smallest that reach each path:
HECTR's ring (generic rotations, the fold at level 1), the windowed rotations
at two levels, a large ring without them, and the long-horizon shape (256
slots at N = 2^16: 8 keys, 9 key switches)."""
import ctypes as C

import numpy as np
import pytest

from hectr_amd import cstr
from tests.rows_ref import expected_rows, gemv2_rows_compose, pow2, rows_keys, rows_rotations, step_rows_compose
from tests.test_gpu_bsgs import init, matrix
from tests.test_gpu_bsgs_batch import FILL, GUARD
from tests.test_gpu_parity import same
from tests.test_gpu_step_batch import StepPair

pytestmark = pytest.mark.gpu


class RowsSide:
    """One engine's keys: the pair and the row-folding rotations only."""

    def __init__(self, e, rows, product_keys=False):
        self.e = e
        self.pk, self.sk = e.pk(), e.sk()
        e.keypair(self.pk, self.sk)
        if product_keys:
            self.rk = e.evks(e.slots)
            e.genrk_rows(self.rk, self.sk, rows)
        else:
            self.rk = rows_keys(e, self.sk, rows)

    def enc(self, z, level=None):
        x = self.e.encrypt(z, self.pk)
        while level and x.nlimbs > level:
            self.e.moddown(x)
        return x

    def close(self):
        for o in (self.pk, self.sk):
            self.e.free(o)
        self.e.free_evks(self.rk)


class RowsPair(StepPair):
    """Both engines, the same he_genrk_rows(keys_rows) keys; self.g is the
    `rows` of the calls (it may be smaller than keys_rows where that subset of
    the keys serves)."""

    def __init__(self, oracle, product, name, slots, rows, seed=77, keys_rows=None):
        init(oracle, product, name, slots, seed)
        self.o, self.p, self.g = oracle, product, rows
        self.O = RowsSide(oracle, keys_rows or rows)
        self.P = RowsSide(product, keys_rows or rows, product_keys=True)

    def run(self, Ma, Mb, H, level, count=None, alias=None):
        """The product's call on device copies of the blocks (two blocks:
        he_gemv2_rows_batch, four: he_hempc_step_rows_batch): output words
        [cnt][..]; guard and inputs checked."""
        import torch
        k, n_ct = H.shape[0], H.shape[1]
        cnt = n_ct if count is None else count
        ow = 2 * (level - 1) * self.p.n
        din = torch.from_numpy(H.ravel().view(np.int64)).cuda()
        dout = torch.full((n_ct * ow + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptr = [din.data_ptr() + 8 * (alias or {}).get(b, b) * n_ct * H.shape[2] for b in range(k)]
        if k == 2:
            self.p.gemv2_rows_batch(dout.data_ptr(), Ma, ptr[0], Mb, ptr[1], cnt, level, self.P.rk, self.g)
        else:
            self.p.hempc_step_rows_batch(dout.data_ptr(), Ma, Mb, ptr[0], ptr[1], ptr[2], ptr[3], cnt, level,
                                         self.P.rk, self.g)
        self.p.sync()
        got = dout.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[n_ct * ow:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        assert np.array_equal(din.cpu().numpy().view(np.uint64), H.ravel()), "an input was written"
        return got[:n_ct * ow].reshape(n_ct, ow)

    def decodes(self, got, want_z, level, scale):
        """The first `rows` slots of every result."""
        rows = self.g
        for i, w in enumerate(want_z):
            ct = self.p.ct()
            self.p.import_(ct, got[i], level - 1, scale=scale)
            err = np.abs(self.p.decrypt(ct, self.P.sk)[:rows] - w[:rows]).max()
            self.p.free(ct)
            assert err < 1e-6 * max(1.0, np.abs(w[:rows]).max()), (i, err)

    def check_step(self, key, Ma, Mb, zs, H, level, scale, alias=None):
        """he_hempc_step_rows_batch == step_rows_compose, blocks (xhat, xr, uhat, ur)."""
        want = self.reference(("rows",) + key,
                              lambda e, c, rk, rows: step_rows_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, rows), H,
                              level, scale, alias)
        got = self.run(Ma, Mb, H, level, alias=alias)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        z = [zs[(alias or {}).get(b, b)] for b in range(4)]
        s = len(z[0][0])
        self.decodes(got, [z[2][i] - expected_rows(Ma, z[0][i] - z[1][i], Mb, z[2][i] - z[3][i], s, self.g)
                           for i in range(len(got))], level, scale)
        return want

    def check_gemv2(self, key, Ma, Mb, zs, H, level, scale, alias=None):
        """he_gemv2_rows_batch == gemv2_rows_compose, blocks (xa, xb)."""
        want = self.reference(("rows",) + key,
                              lambda e, c, rk, rows: gemv2_rows_compose(e, Ma, c[0], Mb, c[1], rk, rows), H, level,
                              scale, alias)
        got = self.run(Ma, Mb, H, level, alias=alias)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        z = [zs[(alias or {}).get(b, b)] for b in range(2)]
        s = len(z[0][0])
        self.decodes(got, [expected_rows(Ma, z[0][i], Mb, z[1][i], s, self.g) for i in range(len(got))], level, scale)
        return want


def without_e(M, s, rows, i):
    """M with its extended diagonal E_i zeroed: entries [r][(k + i) mod s], k mod m' = r."""
    M = M.copy()
    mp = pow2(rows)
    for k in range(s):
        M[k % mp, (k + i) % s] = 0
    return M


def matrices(slots, rows, form=None):
    Ma, Mb = matrix(slots, 3 * slots + rows), matrix(slots, 5 * slots + rows + 1)
    if form == "no E0":  # Ma without its unrotated diagonal, Mb without its rotated one (rows = 2)
        Ma, Mb = without_e(Ma, slots, rows, 0), without_e(Mb, slots, rows, 1)
    return Ma, Mb


# set, slots, rows, level, cnt, form: what it reaches
PARITY = [
    # generic rotations (n = 4096), the fold at level 1
    ("ref", 16, 2, 2, 1, None),     # a lone ciphertext; one rotated baby per operand, three fold steps
    ("ref", 16, 2, 2, 5, None),     # a partial last ciphertext tile
    ("ref", 16, 3, 2, 3, None),     # m' = 4: a padded zero row, two fold steps
    ("ref", 16, 1, 2, 3, None),     # no rotated baby, four fold steps
    ("ref", 16, 16, 2, 3, None),    # no fold: k_step_tail_batch; 32 combined slots
    ("ref", 16, 2, 2, 3, "no E0"),  # E^A_0 zero: xhat - xr lives in a workspace; Mb has its slot 0 only
    # windowed rotations (folded keys, k_gemv_batch over the chunk), the fold one level down
    ("hyb", 32, 2, 5, 3, None),     # K = 2, three digits, the last partial, integer slots
    ("hyb", 32, 2, 4, 3, None),     # ... below the top level
    ("f13", 64, 2, 6, 3, None),     # all-FP64
    # a large ring without the windowed path: four digits
    ("c1", 64, 2, 4, 2, None),
    # the long-horizon shape: N = 2^16, L = 8, 256 slots: 8 keys, 9 key switches
    ("bench51", 256, 2, 8, 3, None),
]
GEMV2 = [c for c in PARITY if c[0] == "ref"] + [PARITY[6]]  # the operands given: slot 0 is a copy of them


@pytest.mark.parametrize("name,slots,rows,level,cnt,form", PARITY)
def test_step_rows_equals_composition(oracle, product, name, slots, rows, level, cnt, form):
    pr = RowsPair(oracle, product, name, slots, rows)
    held = [r for r in range(slots) if pr.P.rk[r].data]
    assert held == rows_rotations(slots, rows)
    Ma, Mb = matrices(slots, rows, form)
    zs, H, scale = pr.blocks(slots, cnt, level, level)
    pr.check_step(("step", name, slots, rows, level, cnt, form), Ma, Mb, zs, H, level, scale)
    pr.close()


@pytest.mark.parametrize("name,slots,rows,level,cnt,form", GEMV2)
def test_gemv2_rows_equals_composition(oracle, product, name, slots, rows, level, cnt, form):
    pr = RowsPair(oracle, product, name, slots, rows)
    Ma, Mb = matrices(slots, rows, form)
    zs, H, scale = pr.blocks(slots, cnt, level, level, k=2)
    pr.check_gemv2(("gemv2", name, slots, rows, level, cnt, form), Ma, Mb, zs, H, level, scale)
    pr.close()


def test_one_matrix_zero(oracle, product):
    """Mb = 0, Ma = 0 (in their leading rows only: the rows below are not read)."""
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    Z = matrix(16, 99)
    Z[:2] = 0
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    pr.check_gemv2(("gemv2 Mb=0",), Ma, Z, zs, H[:2], 2, scale)
    pr.check_gemv2(("gemv2 Ma=0",), Z, Mb, zs, H[:2], 2, scale)
    pr.check_step(("step Mb=0",), Ma, Z, zs, H, 2, scale)
    pr.check_step(("step Ma=0",), Z, Mb, zs, H, 2, scale)
    pr.close()


def test_zero_matrices_and_empty_batch(oracle, product):
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    Z = matrix(16, 99)
    Z[:2] = 0
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    assert not pr.run(Z, Z, H[:2], 2).any()  # y zeroed: the sentinel is overwritten
    low = H[2].reshape(3, 2, 2, -1)[:, :, :1, :].reshape(3, -1)
    assert np.array_equal(pr.run(Z, Z, H, 2), low)  # up = he_moddown(uhat) exactly
    pr.check_step(("step both zero",), Z, Z, zs, H, 2, scale)
    assert (pr.run(Ma, Mb, H[:2], 2, count=0) == FILL).all()  # nothing touched
    assert (pr.run(Ma, Mb, H, 2, count=0) == FILL).all()
    pr.close()


def test_operands_that_are_one_array(oracle, product):
    """xa and xb the same array; the step with xr the same array as xhat (a zero difference)."""
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    zs, H, scale = pr.blocks(16, 3, 2, 2)
    pr.check_gemv2(("gemv2 xa is xb",), Ma, Mb, zs, H[:2], 2, scale, alias={1: 0})
    pr.check_step(("step xr is xhat",), Ma, Mb, zs, H, 2, scale, alias={1: 0})
    pr.close()


@pytest.mark.parametrize("name,level", [("ref", 2), ("f13", 6)])
def test_forced_chunks_do_not_change_bits(oracle, product, name, level, monkeypatch):
    """GPQHE_BSGS_CHUNK = 2: five ciphertexts as 2 + 2 + 1."""
    monkeypatch.setenv("GPQHE_BSGS_CHUNK", "2")
    pr = RowsPair(oracle, product, name, 16, 2)
    Ma, Mb = matrices(16, 2)
    zs, H, scale = pr.blocks(16, 5, level, level)
    pr.check_step(("step", name, 16, 2, level, 5, None), Ma, Mb, zs, H, level, scale)
    pr.close()


def test_workspace_chunks_do_not_change_bits(oracle, product, monkeypatch):
    """GPQHE_WS_MIB = 1: every chunk holds one ciphertext and the stages' own workspaces are cut."""
    monkeypatch.setenv("GPQHE_WS_MIB", "1")
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    zs, H, scale = pr.blocks(16, 5, 2, 2)
    pr.check_step(("step", "ref", 16, 2, 2, 5, None), Ma, Mb, zs, H, 2, scale)
    pr.close()


def test_state(oracle, product):
    """A repeat call (a row-plan hit), the swapped pair (an entry of its own),
    the same matrices at rows 2 then rows 4 (no stale hit; the rows-4 keys
    contain the rows-2 ones), a fold key re-keyed (no stale fold), another
    parameter set after hectx_exit."""
    name, slots, level = "f13", 16, 6
    pr = RowsPair(oracle, product, name, slots, 2, keys_rows=4)
    assert set(rows_rotations(slots, 2)) <= set(rows_rotations(slots, 4))
    Ma, Mb = matrices(slots, 2)
    zs, H, scale = pr.blocks(slots, 2, level, 9)
    w = pr.check_step((name, "ab"), Ma, Mb, zs, H, level, scale)
    assert np.array_equal(pr.run(Ma, Mb, H, level), w)  # a hit
    wba = pr.check_step((name, "ba"), Mb, Ma, zs, H, level, scale)
    assert not np.array_equal(wba, w)
    assert np.array_equal(pr.run(Ma, Mb, H, level), w)
    pr.g = 4
    w4 = pr.check_step((name, "ab rows 4"), Ma, Mb, zs, H, level, scale)
    assert not np.array_equal(w4, w)
    pr.g = 2
    assert np.array_equal(pr.run(Ma, Mb, H, level), w)
    # a fold rotation re-keyed on the product, copied to the oracle
    r = 8
    product.lib.he_free_evk(C.byref(pr.P.rk[r]))
    product.lib.he_genrot(C.byref(pr.P.rk[r]), r, C.byref(pr.P.sk))
    oracle.import_(pr.O.rk[r], product.export(pr.P.rk[r]), pr.P.rk[r].nlimbs)
    w2 = pr.check_step((name, "ab rekeyed"), Ma, Mb, zs, H, level, scale)
    assert not np.array_equal(w2, w)
    pr.close()
    for e in (oracle, product):
        e.exit()
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    zs, H, scale = pr.blocks(16, 3, 2, 4)
    pr.check_step(("ref", "after exit"), Ma, Mb, zs, H, 2, scale)
    pr.close()


def test_kernel_classes_are_reported(oracle, product):
    pr = RowsPair(oracle, product, "ref", 16, 2)
    Ma, Mb = matrices(16, 2)
    zs, H, scale = pr.blocks(16, 3, 2, 6)
    pr.run(Ma, Mb, H, 2)  # warm
    product.prof_enable(True)
    try:
        product.prof_collect()
        pr.run(Ma, Mb, H, 2)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    # rotations 2, 4, 8: two plain fold steps and the one fused with the tail
    for k, launches in (("rows_fold_add_batch_kernel", 2), ("rows_fold_tail_batch_kernel", 1),
                        ("step_diff_batch_kernel", 1), ("bsgs_inner_batch_kernel", 1)):
        assert k in stats, sorted(stats)
        assert stats[k][0] == launches and stats[k][2] > 0, (k, stats[k])
    assert "step_tail_batch_kernel" not in stats
    pr.close()


@pytest.mark.parametrize("name,slots,rows,count", [("ref", 16, 3, 5), ("f13", 256, 2, 8)])
def test_genrk_rows_equals_genrot_sequence(oracle, product, name, slots, rows, count):
    """Word for word the oracle's he_genrot calls from the same seed, and the
    RNG goes on from where they left it: one more he_genrot matches."""
    init(oracle, product, name, slots)
    so, sp = oracle.sk(), product.sk()
    pko, pkp = oracle.pk(), product.pk()
    oracle.keypair(pko, so)
    product.keypair(pkp, sp)
    ro = rows_keys(oracle, so, rows)
    rp = product.evks(slots)
    product.genrk_rows(rp, sp, rows)
    held = [r for r in range(slots) if rp[r].data]
    assert held == rows_rotations(slots, rows) and len(held) == count
    assert rp[0].galois == 1
    for r in held:
        assert rp[r].galois == pow(5, r, 2 * product.n) == ro[r].galois
        same(oracle, product, ro[r], rp[r])
    extra = next(r for r in range(1, slots) if r not in held)
    for e, rk, sk in ((oracle, ro, so), (product, rp, sp)):
        e.lib.he_genrot(C.byref(rk[extra]), extra, C.byref(sk))
    same(oracle, product, ro[extra], rp[extra])
    for e, objs, rk in ((oracle, (so, pko), ro), (product, (sp, pkp), rp)):
        for o in objs:
            e.free(o)
        e.free_evks(rk)


def test_closed_loop_of_three_plants(product):
    """simulate_batch of three CstrProblem(40) with different disturbance steps
    through BatchedEncryptedRegulator(rows=nu) on HECTR's parameters: every
    step's u within 1e-8 max(1, |u|) of regulator_plain on that step's own
    inputs (the existing closed-loop bound)."""
    problems = [cstr.CstrProblem(40) for _ in range(3)]
    for pb, (k0, amp) in zip(problems[1:], ((5, -0.05), (20, 0.08))):
        pb.p = np.zeros(40)
        pb.p[k0:] = amp * cstr.F0S
    reg = cstr.BatchedEncryptedRegulator(product, problems[0], 3, seed=2024, rows=problems[0].nu)
    held = [r for r in range(problems[0].slots) if reg.rk[r].data]
    assert held == rows_rotations(problems[0].slots, problems[0].nu)
    worst = [0.0]

    def on_step(k, xhat, uhat, xr, ur, u):
        for i, pb in enumerate(problems):
            want = pb.regulator_plain(xhat[i], uhat[i], xr[i], ur[i])
            err = np.abs(u[i] - want).max()
            worst[0] = max(worst[0], err)
            assert err < 1e-8 * max(1.0, np.abs(want).max()), (k, i, err)

    x, u = cstr.simulate_batch(problems, reg, on_step)
    print(f"closed loop by row folding: worst |u - plain| {worst[0]:.3e}")
    assert len(reg.timings) == 40 and x.shape == (3, 41, 3) and u.shape == (3, 40, 2)
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[1], u[2])
    reg.close()
