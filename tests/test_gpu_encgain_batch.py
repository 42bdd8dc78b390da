"""The packed step with encrypted gains (include/gpqhe_ext_encgain_batch.h) on
the MI355X against the compositions that define the calls, run on the oracle
per ciphertext (tests/encgain_ref.py), never against the product's own calls.

The scheme is test_gpu_packed_batch.py's: the product encrypts distinct vectors
of S packed slots and the gains' diagonals (he_enc_gain_packed_batch); their
exported words are the device input and, he_import-ed, the oracle's
ciphertexts; both engines hold the packed key subset and a relinearisation key
from one seed.  Every word of every output must equal the oracle's, each loop's
first `rows` values decode to within 1e-6 max(1, |expected|) of the plaintext
(the reference alone stays below 4e-8), the 4096 guard words behind
the output, every input and every diagonal stay as they were.  The oracle's
results are computed once per shape.  The shapes are the smallest that reach
each path."""
import ctypes as C

import numpy as np
import pytest

from hectr_amd import cstr
from tests.encgain_ref import (RefGainRegulator, gain_diagonals, gemv2_encgain_compose, step_encgain_compose)
from tests.packed_ref import expected_packed, packed_rotations
from tests.rows_ref import pow2
from tests.test_gpu_bsgs import vector
from tests.test_gpu_bsgs_batch import FILL, GUARD
from tests.test_gpu_packed_batch import PackedPair, matrices
from tests.test_gpu_parity import same

pytestmark = pytest.mark.gpu


class GainPair(PackedPair):
    """PackedPair with a relinearisation key on both engines (generated after
    the rotation keys, from the same streams) and encrypted gains: the
    product's he_enc_gain_packed_batch, imported into the oracle."""

    def __init__(self, oracle, product, name, S, s, rows, seed=77):
        super().__init__(oracle, product, name, S, s, rows, S // s, seed)
        self.genrlk()
        self.D, self.oD = {}, []

    def genrlk(self):
        for side in (self.O, self.P):
            side.rlk = side.e.evk()
            side.e.genrlk(side.rlk, side.sk)
        same(self.o, self.p, self.O.rlk, self.P.rlk)

    def gains(self, M, level):
        """The product's encryption of M's m' diagonals at `level`: words [m'][2 level n]."""
        import torch
        mp, cw = pow2(self.g), 2 * level * self.p.n
        d = torch.full((mp * cw + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.p.enc_gain_packed_batch(d.data_ptr(), M, self.P.pk, self.s, self.g, level, self.nmat)
        self.p.sync()
        got = d.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[mp * cw:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        return got[:mp * cw].reshape(mp, cw).copy()

    def oracle_gains(self, W, level):
        out = []
        for w in W:
            x = self.o.ct()
            self.o.import_(x, w, level, scale=float(self.o.primes[level - 1]))
            out.append(x)
        self.oD += out
        return out

    def run(self, DA, DB, H, level, count=None, alias=None):
        """The product's call on device copies (two blocks: the product alone,
        four: the step): output words [cnt][..]; guard, inputs and diagonals checked."""
        import torch
        k, n_ct = H.shape[0], H.shape[1]
        cnt = n_ct if count is None else count
        ow = 2 * (level - 1) * self.p.n
        din = torch.from_numpy(H.ravel().view(np.int64)).cuda()
        dd = torch.from_numpy(np.concatenate([DA.ravel(), DB.ravel()]).view(np.int64)).cuda()
        dout = torch.full((n_ct * ow + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptr = [din.data_ptr() + 8 * (alias or {}).get(b, b) * n_ct * H.shape[2] for b in range(k)]
        da, db = dd.data_ptr(), dd.data_ptr() + 8 * DA.size
        if k == 2:
            self.p.gemv2_encgain_packed_batch(dout.data_ptr(), da, ptr[0], db, ptr[1], cnt, level, self.P.rk,
                                              self.P.rlk, self.s, self.g)
        else:
            self.p.hempc_step_encgain_packed_batch(dout.data_ptr(), da, db, ptr[0], ptr[1], ptr[2], ptr[3], cnt, level,
                                                   self.P.rk, self.P.rlk, self.s, self.g)
        self.p.sync()
        got = dout.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[n_ct * ow:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        assert np.array_equal(din.cpu().numpy().view(np.uint64), H.ravel()), "an input was written"
        assert np.array_equal(dd.cpu().numpy().view(np.uint64), np.concatenate([DA.ravel(), DB.ravel()])), \
            "a diagonal was written"
        return got[:n_ct * ow].reshape(n_ct, ow)

    def check(self, key, Ma, Mb, DA, DB, zs, H, level, scale, alias=None):
        """Both calls' words against the compositions on the oracle (H with two
        blocks: the product alone; four: the step), and the decoded loops."""
        s, rows = self.s, self.g
        oa, ob = self.oracle_gains(DA, level), self.oracle_gains(DB, level)
        key = ("encgain", s, DA.tobytes()[:64], DB.tobytes()[:64]) + key
        if H.shape[0] == 2:
            want = self.reference(
                key, lambda e, c, rk, r: gemv2_encgain_compose(e, oa, c[0], ob, c[1], rk, self.O.rlk, s, r), H, level,
                scale, alias)
        else:
            want = self.reference(
                key, lambda e, c, rk, r: step_encgain_compose(e, oa, ob, c[0], c[1], c[2], c[3], rk, self.O.rlk, s, r),
                H, level, scale, alias)
        got = self.run(DA, DB, H, level, alias=alias)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        z = [zs[(alias or {}).get(b, b)] for b in range(H.shape[0])]
        if H.shape[0] == 2:
            exp = [expected_packed(Ma, z[0][i], Mb, z[1][i], s, rows, self.nmat) for i in range(len(got))]
        else:
            exp = [z[2][i] - expected_packed(Ma, z[0][i] - z[1][i], Mb, z[2][i] - z[3][i], s, rows, self.nmat)
                   for i in range(len(got))]
        self.decodes(got, exp, level, scale)
        return want

    def close(self):
        for x in self.oD:
            self.o.free(x)
        for side in (self.O, self.P):
            side.e.free(side.rlk)
        super().close()


def case(pr, S, s, rows, level, cnt, k=4, zero=False):
    Ma, Mb = matrices(S // s, rows, s)
    if zero:
        Ma, Mb = np.zeros_like(Ma), np.zeros_like(Mb)
    DA, DB = pr.gains(Ma, level), pr.gains(Mb, level)
    zs, H, scale = pr.blocks(S, cnt, level, level, k=k)
    return Ma, Mb, DA, DB, zs, H, scale


# set, S, s, rows, level, cnt: what it reaches
PARITY = [
    # generic rotations and the generic multiply (n = 4096); P = 4
    ("ref", 64, 16, 2, 2, 1),       # a lone ciphertext
    ("ref", 64, 16, 2, 2, 5),       # a partial last ciphertext group
    ("ref", 64, 16, 3, 2, 3),       # m' = 4: eight terms
    ("ref", 64, 16, 1, 2, 3),       # no baby rotation
    ("ref", 64, 16, 16, 2, 2),      # no fold; 32 terms: the integer sums' in-loop reduction
    ("ref", 2048, 16, 2, 2, 2),     # full packing S = n / 2
    # windowed rotations; a partial digit one level down
    ("hyb", 128, 32, 2, 5, 3),
    ("hyb", 128, 32, 2, 4, 3),
    # all-FP64 sums and split key switch
    ("f13", 256, 64, 2, 6, 3),
    ("f13", 4096, 16, 2, 6, 2),
    # 60-bit moduli: the integer sums
    ("c1", 256, 64, 2, 4, 2),
    # the workload's own packing: N = 2^16, 2048 loops a ciphertext
    ("bench51", 32768, 16, 2, 8, 1),
]
GEMV2 = [c for c in PARITY if c[:2] == ("ref", 64)]


@pytest.mark.parametrize("name,S,s,rows,level,cnt", PARITY)
def test_step_encgain_equals_composition(oracle, product, name, S, s, rows, level, cnt):
    pr = GainPair(oracle, product, name, S, s, rows)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, S, s, rows, level, cnt)
    pr.check(("step", name, S, rows, level, cnt), Ma, Mb, DA, DB, zs, H, level, scale)
    pr.close()


@pytest.mark.parametrize("name,S,s,rows,level,cnt", GEMV2)
def test_gemv2_encgain_equals_composition(oracle, product, name, S, s, rows, level, cnt):
    pr = GainPair(oracle, product, name, S, s, rows)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, S, s, rows, level, cnt, k=2)
    pr.check(("gemv2", name, S, rows, level, cnt), Ma, Mb, DA, DB, zs, H, level, scale)
    pr.close()


@pytest.mark.parametrize("name,S,s,level", [("ref", 64, 16, 2), ("f13", 256, 64, 6)])
def test_forced_chunks_do_not_change_bits(oracle, product, name, S, s, level, monkeypatch):
    """GPQHE_BSGS_CHUNK = 2: five ciphertexts as 2 + 2 + 1."""
    monkeypatch.setenv("GPQHE_BSGS_CHUNK", "2")
    pr = GainPair(oracle, product, name, S, s, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, S, s, 2, level, 5)
    pr.check(("step", name, S, 2, level, 5), Ma, Mb, DA, DB, zs, H, level, scale)
    pr.close()


def test_workspace_chunks_do_not_change_bits(oracle, product, monkeypatch):
    """GPQHE_WS_MIB = 1: every chunk holds one ciphertext."""
    monkeypatch.setenv("GPQHE_WS_MIB", "1")
    pr = GainPair(oracle, product, "ref", 64, 16, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, 64, 16, 2, 2, 5)
    pr.check(("step", "ref", 64, 2, 2, 5), Ma, Mb, DA, DB, zs, H, 2, scale)
    pr.close()


def test_empty_batch_aliases_and_zero_diagonals(oracle, product):
    pr = GainPair(oracle, product, "ref", 64, 16, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, 64, 16, 2, 2, 3)
    assert (pr.run(DA, DB, H[:2], 2, count=0) == FILL).all()  # nothing touched
    assert (pr.run(DA, DB, H, 2, count=0) == FILL).all()
    pr.check(("gemv2 xa is xb",), Ma, Mb, DA, DB, zs, H[:2], 2, scale, alias={1: 0})
    pr.check(("step xr is xhat",), Ma, Mb, DA, DB, zs, H, 2, scale, alias={1: 0})
    # encryptions of all-zero diagonals are ciphertexts like any other: the
    # product part decodes to 0, the step to uhat (check()'s decode)
    Z = np.zeros_like(Ma)
    ZA, ZB = pr.gains(Z, 2), pr.gains(Z, 2)
    assert ZA.any(axis=1).all() and ZB.any(axis=1).all()
    pr.check(("gemv2 zero",), Z, Z, ZA, ZB, zs, H[:2], 2, scale)
    pr.check(("step zero",), Z, Z, ZA, ZB, zs, H, 2, scale)
    pr.close()


def test_state(oracle, product):
    """A repeat call; the relinearisation key regenerated between calls; the
    new step and he_hempc_step_packed_batch interleaved on one context; another
    parameter set after hectx_exit."""
    from tests.packed_ref import step_packed_compose
    name, S, s, level = "f13", 64, 16, 6
    pr = GainPair(oracle, product, name, S, s, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, S, s, 2, level, 2)
    w = pr.check((name, "first"), Ma, Mb, DA, DB, zs, H, level, scale)
    assert np.array_equal(pr.run(DA, DB, H, level), w)
    wp = pr.reference(("encgain", name, "packed between"),
                      lambda e, c, rk, r: step_packed_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, s, r, pr.nmat),
                      H, level, scale)
    assert np.array_equal(PackedPair.run(pr, Ma, Mb, H, level), wp) and not np.array_equal(wp, w)
    assert np.array_equal(pr.run(DA, DB, H, level), w)
    assert np.array_equal(PackedPair.run(pr, Ma, Mb, H, level), wp)
    # regenerated on the product (whose streams have moved on), copied to the oracle
    product.lib.he_free_evk(C.byref(pr.P.rlk))
    product.genrlk(pr.P.rlk, pr.P.sk)
    oracle.import_(pr.O.rlk, product.export(pr.P.rlk), pr.P.rlk.nlimbs)
    w2 = pr.check((name, "rekeyed"), Ma, Mb, DA, DB, zs, H, level, scale)
    assert not np.array_equal(w2, w)
    pr.close()
    for e in (oracle, product):
        e.exit()
    pr = GainPair(oracle, product, "ref", 64, 16, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, 64, 16, 2, 2, 3)
    pr.check(("ref", "after exit"), Ma, Mb, DA, DB, zs, H, 2, scale)
    pr.close()


def test_kernel_classes_are_reported(oracle, product):
    pr = GainPair(oracle, product, "f13", 64, 16, 2)
    Ma, Mb, DA, DB, zs, H, scale = case(pr, 64, 16, 2, 6, 2)
    pr.run(DA, DB, H, 6)  # warm
    product.prof_enable(True)
    try:
        product.prof_collect()
        pr.run(DA, DB, H, 6)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k in ("encgain_tensor_kernel", "encgain_ones_kernel"):
        assert k in stats, sorted(stats)
        assert stats[k][0] >= 1 and stats[k][2] > 0, (k, stats[k])
    pr.close()


@pytest.mark.parametrize("name,S,s,rows", [("ref", 64, 16, 3), ("f13", 4096, 16, 2)])
def test_enc_gain_equals_the_oracles_single_calls(oracle, product, name, S, s, rows):
    """Word for word the oracle's he_ecd_ex + he_enc_pk over the m' diagonals
    from the same seed, at nmat 1 and P (the zero diagonals included), and one
    more single encryption after them."""
    pr = GainPair(oracle, product, name, S, s, rows)
    lvl, P = product.L, S // s
    q_top = float(oracle.primes[lvl - 1])
    M = matrices(P, rows, s)[0]
    for k in range(s):  # E_1 zero in every loop
        if k % pow2(rows) < rows:
            M[:, k % pow2(rows), (k + 1) % s] = 0
    for nmat, Mn in ((1, M[:1]), (P, M)):
        pr.nmat = nmat
        E = gain_diagonals(Mn, S, s, rows, nmat)
        assert len(E) == pow2(rows) and not E[1].any()
        want = []
        for d in E:
            ct = oracle.encrypt(d, pr.O.pk, S, q_top, lvl)
            want.append(oracle.export(ct).ravel().copy())
            oracle.free(ct)
        got = pr.gains(Mn, lvl)
        bad = np.argwhere(got != np.stack(want))
        assert bad.size == 0, f"nmat {nmat}: {len(bad)} words differ, first at {bad[0].tolist()}"
    z = vector(S, 5)
    co = oracle.encrypt(z, pr.O.pk, S, product.info.delta, lvl)
    cp = product.encrypt(z, pr.P.pk, S, product.info.delta, lvl)
    same(oracle, product, co, cp)
    oracle.free(co)
    product.free(cp)
    pr.close()


#: worst |u - regulator_plain| of this closed loop run through RefGainRegulator
#: on the oracle alone (a CPU run)
ORACLE_LOOP_WORST = 1.15e-10


def test_closed_loop_of_six_plants(oracle, product):
    """simulate_batch of six CstrProblem(40) with different disturbance steps
    through EncryptedGainRegulator on S = 64 (P = 4, two ciphertexts).  Every
    step's u within min(100 x the oracle loop's own worst deviation, 1e-6
    max(1, |u|)) of regulator_plain on that step's inputs; the first three
    steps' u equal bit for bit what the reference loop on the oracle gives for
    the same inputs (the same seed, so the same keys, gains and encryptions)."""
    problems = [cstr.CstrProblem(40) for _ in range(6)]
    for pb, (k0, amp) in zip(problems[1:], ((5, -0.05), (20, 0.08), (12, 0.03), (30, -0.07), (2, 0.1))):
        pb.p = np.zeros(40)
        pb.p[k0:] = amp * cstr.F0S
    reg = cstr.EncryptedGainRegulator(product, problems, 64, rows=problems[0].nu, seed=2024)
    assert (reg.P, reg.count, reg.nmat, reg.mp) == (4, 2, 4, 2)
    assert [r for r in range(64) if reg.rk[r].data] == packed_rotations(64, problems[0].slots, problems[0].nu)
    worst, first = [0.0], []

    def on_step(k, xhat, uhat, xr, ur, u):
        if k < 3:
            first.append((np.array(xhat), np.array(uhat), np.array(xr), np.array(ur), np.array(u)))
        for i, pb in enumerate(problems):
            want = pb.regulator_plain(xhat[i], uhat[i], xr[i], ur[i])
            err = np.abs(u[i] - want).max()
            worst[0] = max(worst[0], err)
            assert err < min(100 * ORACLE_LOOP_WORST, 1e-6 * max(1.0, np.abs(want).max())), (k, i, err)

    x, u = cstr.simulate_batch(problems, reg, on_step)
    print(f"closed loop, encrypted gains: worst |u - plain| {worst[0]:.3e}")
    assert len(reg.timings) == 40 and x.shape == (6, 41, 3) and u.shape == (6, 40, 2)
    assert all(not np.array_equal(u[0], u[i]) for i in range(1, 6))
    reg.close()
    ref = RefGainRegulator(oracle, problems, 64, 2024)
    for xhat, uhat, xr, ur, got in first:
        assert np.array_equal(ref(xhat, uhat, xr, ur), got)
    ref.close()
