"""he_enc_sk_batch, he_enc_sk_packed_batch and he_enc_gain_sk_packed_batch
(include/gpqhe_ext_sk_batch.h) on the MI355X against the oracle's sequential
he_ecd_ex + he_enc_sk from the same gpqhe_set_seed (tests/sk_ref.py), never
against the product's own single calls: every word of x bit for bit, the RNG
left where the single calls leave it, guard words and inputs intact; then the
ciphertexts through the batch decode and the packed steps against the
reference compositions on the oracle, and the closed loops of
cstr.*Regulator(sym=True).  Both engines generate their keys from one seed.
The shapes are the smallest that reach each path: host and GPU encoder, one and
several ChaCha blocks per coefficient of c1 (nb = ceil((L + K) / 4)), FP64 and
integer moduli, full and partial ciphertext groups."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ckks_model_rng as R
import noise_audit as A
from hectr_amd import cstr
from tests.encgain_ref import gain_diagonals, step_encgain_compose
from tests.packed_ref import deinterleave, expected_packed, interleave, packed_rotations, step_packed_compose
from tests.rows_ref import pow2
from tests.sk_ref import (RefSymGainRegulator, RefSymPackedRegulator, enc_gain_sk_compose, enc_sk_packed_words,
                          enc_sk_words, encrypt_sk)
from tests.test_gpu_bsgs import init, vector
from tests.test_gpu_encgain_batch import ORACLE_LOOP_WORST, GainPair
from tests.test_gpu_io_batch import FILL, GUARD, SEED, Ends, bits, vectors
from tests.test_gpu_packed_batch import PackedPair, loops, matrices
from tests.test_gpu_parity import same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENC = {}  # case -> (zs, oracle words [cnt][2 nl n]): computed once, shared, read-only


def dev(nwords):
    """A device array of nwords words and GUARD more, all FILL."""
    import torch
    t = torch.full((nwords + GUARD,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def words_of(t, nwords):
    got = t.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[nwords:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
    return got[:nwords]


def assert_words(got, want, what="words"):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {bad[0].tolist()}"


class SkEnds(Ends):
    """Ends (one key pair on each engine from one seed) with the secret-key
    calls; slots: the context's slot count instead of the set's own."""

    def __init__(self, oracle, product, name, slots=None, seed=SEED):
        if slots is None:
            super().__init__(oracle, product, name, seed)
            return
        init(oracle, product, name, slots, seed)
        self.o, self.p, self.name = oracle, product, name
        self.n, self.L, self.scale = product.n, product.L, product.info.delta
        self.ko = (oracle.pk(), oracle.sk())
        self.kp = (product.pk(), product.sk())
        oracle.keypair(*self.ko)
        product.keypair(*self.kp)

    def oracle_enc_sk(self, zs, slots, nl):
        return enc_sk_words(self.o, zs, self.ko[1], slots, self.scale, nl)

    def enc_sk_batch(self, zs, slots, nl, count=None):
        """he_enc_sk_batch: the output words [len(zs)][2 nl n]; guard and input checked."""
        cw = 2 * nl * self.n
        dout = dev(len(zs) * cw)
        zz = np.asarray(zs, dtype=np.complex128).reshape(len(zs), slots)
        keep = zz.copy()
        self.p.enc_sk_batch(dout.data_ptr(), zz[:len(zs) if count is None else count], self.kp[1], slots,
                            self.scale, nl)
        self.p.sync()
        assert np.array_equal(bits(zz), bits(keep)), "input written"
        return words_of(dout, len(zs) * cw).reshape(len(zs), cw)

    def enc_sk_packed(self, zs, s, width, nl):
        cw = 2 * nl * self.n
        dout = dev(len(zs) * cw)
        zz = np.stack(zs)
        keep = zz.copy()
        self.p.enc_sk_packed_batch(dout.data_ptr(), zz, self.kp[1], s, width, self.scale, nl)
        self.p.sync()
        assert np.array_equal(bits(zz), bits(keep)), "input written"
        return words_of(dout, len(zs) * cw).reshape(len(zs), cw)

    def rng_continued(self, slots, nl):
        """One more single he_enc_sk and one he_enc_pk on both engines."""
        z = vector(slots, 5)
        co = encrypt_sk(self.o, z, self.ko[1], slots, self.scale, nl)
        cp = encrypt_sk(self.p, z, self.kp[1], slots, self.scale, nl)
        same(self.o, self.p, co, cp)
        do = self.o.encrypt(z, self.ko[0], slots, self.scale, nl)
        dp = self.p.encrypt(z, self.kp[0], slots, self.scale, nl)
        same(self.o, self.p, do, dp)
        for e, cts in ((self.o, (co, do)), (self.p, (cp, dp))):
            for c in cts:
                e.free(c)


def encryptions(E, case):
    """(zs, oracle words) of a case right after E's key pair, from the cache or
    computed now (which advances the oracle's RNG by 2 streams a ciphertext)."""
    name, slots, nl, cnt = case
    if case not in _ENC:
        zs = vectors(slots, cnt, slots + cnt)
        words = E.oracle_enc_sk(zs, slots, nl or E.L)
        words.setflags(write=False)
        _ENC[case] = (zs, words)
    return _ENC[case]


# set, slots, level (None: top), count: what it reaches
CASES = [
    ("ref", 16, None, 3),       # n = 4096, nb = 1; a queued single he_enc_pk right before the call
    ("f13", 64, None, 1),       # nb = 3, level 6: c1 from two blocks; a partial ciphertext group alone
    ("f13", 64, None, 3),
    ("f13", 64, None, 17),      # more than two groups of 8, the last partial
    ("f13", 64, 1, 3),          # level 1: one limb of the first block
    ("c1", 64, None, 3),        # 60-bit q0: the integer combine beside the FP64 one
    ("c1", 64, None, 17),
    ("hyb", 32, None, 3),       # K = 2, level 5
    ("f13", 2048, None, 3),     # GPU encoder, gap 2
    ("f13", 4096, None, 3),     # GPU encoder, gap 1
    ("bench51", 16, None, 5),   # n = 2^16, nb = 3
    ("bench_d2", 16, None, 5),  # ... with a 60-bit q0
]


@pytest.mark.parametrize("name,slots,nl,cnt", CASES)
def test_enc_sk_batch_equals_sequential_single_calls(oracle, product, name, slots, nl, cnt):
    E = SkEnds(oracle, product, name)
    lvl = nl or E.L
    pre = None
    if name == "ref":  # a single encryption first: queued on the product, its streams already taken
        z0 = vector(slots, 6)
        pre = (oracle.encrypt(z0, E.ko[0], slots, E.scale, lvl), product.encrypt(z0, E.kp[0], slots, E.scale, lvl))
        zs = vectors(slots, cnt, slots + cnt)
        want = E.oracle_enc_sk(zs, slots, lvl)
    else:
        _ENC.pop((name, slots, nl, cnt), None)  # from this seed state: the RNG must end where the oracle's does
        zs, want = encryptions(E, (name, slots, nl, cnt))
    got = E.enc_sk_batch(zs, slots, lvl)
    assert_words(got, want)
    if pre:
        same(oracle, product, *pre)
        oracle.free(pre[0])
        product.free(pre[1])
    E.rng_continued(slots, lvl)
    E.close()


@pytest.mark.parametrize("env", [{"GPQHE_CHUNK": "5"}, {"GPQHE_WS_MIB": "1"}])
def test_chunks_do_not_change_bits(oracle, product, env, monkeypatch):
    """17 ciphertexts as 5/5/5/2 (GPQHE_CHUNK) or cut by a 1 MiB workspace."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E = SkEnds(oracle, product, "f13")
    zs, want = encryptions(E, ("f13", 64, None, 17))
    assert_words(E.enc_sk_batch(zs, 64, E.L), want)
    E.close()


def test_empty_batch_and_zero_vectors(oracle, product):
    E = SkEnds(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 2, 4)
    # count = 0: nothing written, no stream taken
    assert (E.enc_sk_batch(zs, slots, lvl, count=0) == FILL).all()
    E.rng_continued(slots, lvl)
    # an all-zero batch: ciphertexts like any other
    zero = [np.zeros(slots, dtype=np.complex128)] * 3
    want = E.oracle_enc_sk(zero, slots, lvl)
    got = E.enc_sk_batch(zero, slots, lvl)
    assert_words(got, want)
    assert got.reshape(3, 2, -1).any(axis=2).all()
    zd = E.dec_batch(got, lvl, slots)
    assert np.array_equal(bits(zd), bits(E.oracle_dec(want, lvl, slots)))
    assert np.abs(zd).max() < 1e-6
    E.close()


@pytest.mark.parametrize("name,S,s,width", [("ref", 64, 16, 3), ("f13", 4096, 16, 2)])
def test_enc_sk_packed_equals_the_oracles_single_calls(oracle, product, name, S, s, width):
    """At width = s and at a width below it, against the oracle on the interleaved vectors."""
    E = SkEnds(oracle, product, name, S)
    P, lvl = S // s, product.L
    full, part = loops(P, s, 2, S), loops(P, width, 2, S + 1)
    want = enc_sk_packed_words(oracle, full + part, E.ko[1], E.scale, lvl)
    got = np.concatenate([E.enc_sk_packed(full, s, s, lvl), E.enc_sk_packed(part, s, width, lvl)])
    assert_words(got, want)
    E.rng_continued(S, lvl)
    z = E.dec_batch(got, lvl, S)
    for i, v in enumerate(full + part):
        assert np.abs(z[i] - interleave(v, S)).max() < 1e-6  # (they do decrypt)
    E.close()


def test_enc_gain_sk_equals_the_oracles_single_calls(oracle, product):
    """ref 64/16, rows 3 (m' = 4) with E_1 zero in every loop, still a full
    ciphertext; nmat 1 and P; one more pair of single encryptions after them."""
    S, s, rows = 64, 16, 3
    E = SkEnds(oracle, product, "ref", S)
    lvl, P, mp = product.L, S // s, pow2(rows)
    cw = 2 * lvl * E.n
    M = matrices(P, rows, s)[0]
    for k in range(s):
        if k % mp < rows:
            M[:, k % mp, (k + 1) % s] = 0
    for nmat, Mn in ((1, M[:1]), (P, M)):
        assert not gain_diagonals(Mn, S, s, rows, nmat)[1].any()
        oc = enc_gain_sk_compose(oracle, Mn, E.ko[1], s, rows, nmat, lvl)
        want = np.stack([oracle.export(c).ravel() for c in oc])
        for c in oc:
            oracle.free(c)
        d = dev(mp * cw)
        product.enc_gain_sk_packed_batch(d.data_ptr(), Mn, E.kp[1], s, rows, lvl, nmat)
        product.sync()
        got = words_of(d, mp * cw).reshape(mp, cw)
        assert_words(got, want, f"nmat {nmat}")
        assert got.reshape(mp, 2, -1).any(axis=2).all()
    E.rng_continued(S, lvl)
    E.close()


def test_noise_audit_of_the_exported_words(oracle, product):
    """f13, 64 slots: c1 and the exact noise of the product's ciphertexts are
    the model's samples from the seed alone (the key pair took streams 0..2,
    ciphertext i takes 3 + 2 i and 3 + 2 i + 1): integers, no tolerance."""
    E = SkEnds(oracle, product, "f13")
    A.use_host_transforms(product, oracle)
    n, lvl, nmod, key = E.n, E.L, product.L + product.K, R.seed_key(SEED)
    zs = vectors(64, 3, 9)
    got = E.enc_sk_batch(zs, 64, lvl)
    for i, z in enumerate(zs):
        ct, pt = product.ct(), product.pt()
        product.import_(ct, got[i], lvl, scale=E.scale)
        product.ecd_ex(pt, z, 64, E.scale, lvl)
        noise = A.exact_decrypt(product, ct, E.kp[1]) - A.exact_plain(product, pt)
        assert np.abs(noise).max() <= R.CBD_ETA
        assert np.array_equal(noise.astype(np.int64), R.sample_cbd(key, 3 + 2 * i + 1, n)), f"e of ciphertext {i}"
        c1 = got[i].reshape(2, lvl, n)[1]
        for m in range(lvl):
            assert np.array_equal(c1[m], R.sample_uniform(key, 3 + 2 * i, n, m, product.primes[m], nmod)), (i, m)
        product.free(ct)
        product.free(pt)
    E.close()


@pytest.mark.parametrize("case", [("ref", 16, None, 3), ("f13", 64, None, 3), ("f13", 4096, None, 3)])
def test_decode_of_sk_encryptions(oracle, product, case, monkeypatch):
    """sk encryptions -> he_dec_dcd_batch, double for double the oracle's he_dec + he_dcd_ex."""
    name, slots, nl, cnt = case
    E = SkEnds(oracle, product, name)
    lvl = nl or E.L
    zs, want_x = encryptions(E, case)
    got = E.enc_sk_batch(zs, slots, lvl)
    assert_words(got, want_x)
    want = E.dec_check(got, lvl, slots, monkeypatch)
    assert np.abs(want - np.stack(zs)).max() < 1e-6
    E.close()


def loop_bound(got, want, P, rows):
    g, w = deinterleave(got, P, rows) if got.ndim == 1 else got, deinterleave(want, P, rows)
    err = np.abs(g - w).max(axis=1)
    assert (err < 1e-6 * np.maximum(1.0, np.abs(w).max(axis=1))).all(), err.max()


def packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, seed):
    """4 cnt loop sets through he_enc_sk_packed_batch into one device array
    (blocks xhat, xr, uhat, ur): (vectors, the array, the oracle's words [4][cnt][W])."""
    cw = 2 * level * product.n
    zs = loops(S // s, width, 4 * cnt, seed)
    x = dev(4 * cnt * cw)
    product.enc_sk_packed_batch(x.data_ptr(), np.stack(zs), pr.P.sk, s, width, scale, level)
    product.sync()
    want = enc_sk_packed_words(oracle, zs, pr.O.sk, scale, level)
    assert_words(words_of(x, 4 * cnt * cw).reshape(4 * cnt, cw), want, "input words")
    return zs, x, want.reshape(4, cnt, cw)


def check_step_output(pr, oracle, product, up, want_up, zs, Ma, Mb, S, s, rows, level, cnt, scale):
    """up (device) against the reference words, its batch decode double for
    double against the oracle's, each loop's leading rows within the bound."""
    P, ow = S // s, 2 * (level - 1) * product.n
    assert_words(words_of(up, cnt * ow).reshape(cnt, ow), want_up, "step words")
    z = product.dec_dcd_packed_batch(up.data_ptr(), cnt, level - 1, scale, pr.P.sk, s, rows)
    for c in range(cnt):
        ct = oracle.ct()
        oracle.import_(ct, want_up[c], level - 1, scale=scale)
        wz = deinterleave(oracle.decrypt(ct, pr.O.sk, S), P, rows)
        oracle.free(ct)
        assert np.array_equal(bits(z[c]), bits(wz)), f"ciphertext {c}: decoded doubles differ"
        v = [interleave(zs[b * cnt + c], S) for b in range(4)]
        loop_bound(z[c], v[2] - expected_packed(Ma, v[0] - v[1], Mb, v[2] - v[3], s, rows, P), P, rows)


@pytest.mark.parametrize("name,S,s,level,cnt", [("ref", 64, 16, 2, 2), ("f13", 4096, 16, 6, 1)])
def test_pipeline_packed_step(oracle, product, name, S, s, level, cnt):
    """he_enc_sk_packed_batch -> he_hempc_step_packed_batch -> he_dec_dcd_packed_batch on one device array."""
    rows, width, P = 2, 3, S // s
    pr = PackedPair(oracle, product, name, S, s, rows)
    scale = product.info.delta
    Ma, Mb = matrices(P, rows, s)
    zs, x, H = packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, S + 3)
    cw, ow = 2 * level * product.n, 2 * (level - 1) * product.n
    up = dev(cnt * ow)
    ptr = [x.data_ptr() + 8 * b * cnt * cw for b in range(4)]
    product.hempc_step_packed_batch(up.data_ptr(), Ma, Mb, *ptr, cnt, level, pr.P.rk, s, rows, P)
    product.sync()
    want_up = pr.reference(("sk packed", name, S, cnt),
                           lambda e, c, rk, r: step_packed_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, s, r, P),
                           H, level, scale)
    assert_words(words_of(x, 4 * cnt * cw), H.ravel(), "inputs after the step")
    check_step_output(pr, oracle, product, up, want_up, zs, Ma, Mb, S, s, rows, level, cnt, scale)
    pr.close()


def test_pipeline_encgain_step(oracle, product):
    """The same through he_hempc_step_encgain_packed_batch with the gains from
    he_enc_gain_sk_packed_batch, ref S = 64."""
    name, S, s, rows, width, level, cnt = "ref", 64, 16, 2, 3, 2, 2
    P, mp = S // s, pow2(rows)
    pr = GainPair(oracle, product, name, S, s, rows)
    scale = product.info.delta
    cw, ow = 2 * level * product.n, 2 * (level - 1) * product.n
    Ma, Mb = matrices(P, rows, s)
    D = dev(2 * mp * cw)
    DA, DB = D.data_ptr(), D.data_ptr() + 8 * mp * cw
    product.enc_gain_sk_packed_batch(DA, Ma, pr.P.sk, s, rows, level, P)
    product.enc_gain_sk_packed_batch(DB, Mb, pr.P.sk, s, rows, level, P)
    product.sync()
    oa = enc_gain_sk_compose(oracle, Ma, pr.O.sk, s, rows, P, level)
    ob = enc_gain_sk_compose(oracle, Mb, pr.O.sk, s, rows, P, level)
    pr.oD += oa + ob
    want_d = np.stack([oracle.export(c).ravel() for c in oa + ob])
    assert_words(words_of(D, 2 * mp * cw).reshape(2 * mp, cw), want_d, "gain words")
    zs, x, H = packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, S + 4)
    up = dev(cnt * ow)
    ptr = [x.data_ptr() + 8 * b * cnt * cw for b in range(4)]
    product.hempc_step_encgain_packed_batch(up.data_ptr(), DA, DB, *ptr, cnt, level, pr.P.rk, pr.P.rlk, s, rows)
    product.sync()
    want_up = pr.reference(
        ("sk encgain", name, S, cnt),
        lambda e, c, rk, r: step_encgain_compose(e, oa, ob, c[0], c[1], c[2], c[3], rk, pr.O.rlk, s, r), H, level,
        scale)
    assert_words(words_of(D, 2 * mp * cw).reshape(2 * mp, cw), want_d, "gains after the step")
    check_step_output(pr, oracle, product, up, want_up, zs, Ma, Mb, S, s, rows, level, cnt, scale)
    pr.close()


def six_plants():
    problems = [cstr.CstrProblem(40) for _ in range(6)]
    for pb, (k0, amp) in zip(problems[1:], ((5, -0.05), (20, 0.08), (12, 0.03), (30, -0.07), (2, 0.1))):
        pb.p = np.zeros(40)
        pb.p[k0:] = amp * cstr.F0S
    return problems


def closed_loop(oracle, reg, ref_class, problems, bound, what):
    """simulate_batch through reg; every step's u within bound(|plain u|) of
    regulator_plain on that step's inputs; the first three steps' u bit for bit
    the sym reference loop's on the oracle for the same inputs."""
    assert (reg.P, reg.count, reg.nmat, reg.sym) == (4, 2, 4, True)
    assert [r for r in range(64) if reg.rk[r].data] == packed_rotations(64, problems[0].slots, problems[0].nu)
    worst, first = [0.0], []

    def on_step(k, xhat, uhat, xr, ur, u):
        if k < 3:
            first.append((np.array(xhat), np.array(uhat), np.array(xr), np.array(ur), np.array(u)))
        for i, pb in enumerate(problems):
            want = pb.regulator_plain(xhat[i], uhat[i], xr[i], ur[i])
            err = np.abs(u[i] - want).max()
            worst[0] = max(worst[0], err)
            assert err < bound(np.abs(want).max()), (k, i, err)

    x, u = cstr.simulate_batch(problems, reg, on_step)
    print(f"closed loop, {what}, secret-key encryptions: worst |u - plain| {worst[0]:.3e}")
    assert len(reg.timings) == 40 and x.shape == (6, 41, 3) and u.shape == (6, 40, 2)
    assert all(not np.array_equal(u[0], u[i]) for i in range(1, 6))
    reg.close()
    ref = ref_class(oracle, problems, 64, 2024)
    for xhat, uhat, xr, ur, got in first:
        assert np.array_equal(ref(xhat, uhat, xr, ur), got)
    ref.close()


def test_closed_loop_packed_sym(oracle, product):
    """Six CstrProblem(40) through PackedEncryptedRegulator(sym=True) on S = 64:
    within 1e-8 max(1, |u|) of regulator_plain, the bound of the public-key loop."""
    problems = six_plants()
    reg = cstr.PackedEncryptedRegulator(product, problems, 64, rows=problems[0].nu, seed=2024, sym=True)
    closed_loop(oracle, reg, RefSymPackedRegulator, problems, lambda w: 1e-8 * max(1.0, w), "plain gains")


def test_closed_loop_encrypted_gains_sym(oracle, product):
    """... through EncryptedGainRegulator(sym=True): within min(1.15e-8, 1e-6
    max(1, |u|)), the bound of the public-key loop (100 x the oracle loop's own
    worst deviation)."""
    problems = six_plants()
    reg = cstr.EncryptedGainRegulator(product, problems, 64, rows=problems[0].nu, seed=2024, sym=True)
    assert reg.mp == 2
    closed_loop(oracle, reg, RefSymGainRegulator, problems,
                lambda w: min(100 * ORACLE_LOOP_WORST, 1e-6 * max(1.0, w)), "encrypted gains")


def test_state(oracle, product):
    """A repeat call; pk and sk batch calls interleaved on one context, each
    against the oracle's single calls in that order; another parameter set
    after hectx_exit."""
    E = SkEnds(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 3, 11)
    for kind in ("sk", "sk", "pk", "sk", "pk"):
        if kind == "sk":
            assert_words(E.enc_sk_batch(zs, slots, lvl), E.oracle_enc_sk(zs, slots, lvl), kind)
        else:
            assert_words(E.enc_batch(zs, slots, lvl), E.oracle_enc(zs, slots, lvl), kind)
    E.rng_continued(slots, lvl)
    E.close()
    for e in (oracle, product):
        e.exit()
    E = SkEnds(oracle, product, "ref")
    zs = vectors(16, 3, 12)
    assert_words(E.enc_sk_batch(zs, 16, E.L), E.oracle_enc_sk(zs, 16, E.L))
    E.rng_continued(16, E.L)
    E.close()


def test_kernel_classes_are_reported(oracle, product):
    E = SkEnds(oracle, product, "f13")
    product.prof_enable(True)
    try:
        product.prof_collect()
        E.enc_sk_batch(vectors(64, 3, 1), 64, E.L)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k in ("enc_sk_sample_batch_kernel", "enc_sk_combine_batch_kernel"):
        assert k in stats, sorted(stats)
        assert stats[k][0] >= 1 and stats[k][2] > 0, (k, stats[k])
    assert "enc_sample_batch_kernel" not in stats and "enc_combine_batch_kernel" not in stats
    E.close()


def test_teardown_clean_exit():
    """The three calls, hectx_exit, a second context, the calls again, exit: rc 0."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sk_batch_worker.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rc {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert res == {"first": True, "second": True}, res
