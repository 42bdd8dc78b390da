"""he_enc_pk_batch / he_dec_dcd_batch (include/gpqhe_ext_batch.h) on the MI355X
against the oracle's sequential single calls from the same gpqhe_set_seed:
every word of x, every double of z bit for bit, the RNG left where the single
calls leave it, guard words and inputs intact.  Both engines generate their
key pair from the same seed, so a test can rebuild the context and still use
the oracle words another test computed (_ENC).  The shapes are the smallest
that reach each path: host and GPU encoder, gap T = n / 2 slots of 1, 2 and
more, the folded decoder and the general one, FP64 and integer moduli."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_bsgs import matrix, vector
from tests.test_gpu_parity import init_both, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL, SEED = 4096, 7, 77
_ENC = {}  # case -> (zs, oracle words [cnt][2 nl n]): computed once, shared, read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Ends:
    """Both engines on one parameter set, one key pair each from the same seed."""

    def __init__(self, oracle, product, name, seed=SEED):
        init_both(oracle, product, name, seed)
        self.o, self.p, self.name = oracle, product, name
        self.n, self.L, self.scale = product.n, product.L, product.info.delta
        self.ko = (oracle.pk(), oracle.sk())
        self.kp = (product.pk(), product.sk())
        oracle.keypair(*self.ko)
        product.keypair(*self.kp)

    def close(self):
        for e, k in ((self.o, self.ko), (self.p, self.kp)):
            for obj in k:
                e.free(obj)

    # ------------------------------------------------------------ oracle side
    def oracle_enc(self, zs, slots, nl):
        """The oracle's he_ecd_ex + he_enc_pk of every z in order: words [cnt][2 nl n]."""
        rows = []
        for z in zs:
            ct = self.o.encrypt(z, self.ko[0], slots, self.scale, nl)
            assert ct.nlimbs == nl
            rows.append(self.o.export(ct).ravel().copy())
            self.o.free(ct)
        return np.stack(rows) if rows else np.zeros((0, 2 * nl * self.n), dtype=np.uint64)

    def oracle_dec(self, words, nl, slots):
        """The oracle's he_dec + he_dcd_ex of every imported ciphertext: [cnt][slots]."""
        out = []
        for w in words:
            ct = self.o.ct()
            self.o.import_(ct, w, nl, scale=self.scale)
            out.append(self.o.decrypt(ct, self.ko[1], slots))
            self.o.free(ct)
        return np.stack(out)

    def oracle_moddown(self, words, nl):
        rows = []
        for w in words:
            ct = self.o.ct()
            self.o.import_(ct, w, nl, scale=self.scale)
            self.o.moddown(ct)
            assert ct.nlimbs == nl - 1
            rows.append(self.o.export(ct).ravel().copy())
            self.o.free(ct)
        return np.stack(rows)

    # ----------------------------------------------------------- product side
    def enc_batch(self, zs, slots, nl, count=None):
        """he_enc_pk_batch: the output words [len(zs)][2 nl n]; guard checked."""
        import torch
        cw = 2 * nl * self.n
        dout = torch.full((len(zs) * cw + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        zz = np.asarray(zs, dtype=np.complex128).reshape(len(zs), slots)
        self.p.enc_pk_batch(dout.data_ptr(), zz[:len(zs) if count is None else count], self.kp[0], slots,
                            self.scale, nl)
        self.p.sync()
        got = dout.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[len(zs) * cw:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        return got[:len(zs) * cw].reshape(len(zs), cw)

    def dec_batch(self, words, nl, slots):
        """he_dec_dcd_batch of host words: [cnt][slots]; the input must stay as it was."""
        import torch
        din = torch.from_numpy(np.array(words).ravel().view(np.int64)).cuda()  # (a writable copy)
        torch.cuda.synchronize()
        z = self.p.dec_dcd_batch(din.data_ptr(), len(words), nl, self.scale, self.kp[1], slots)
        assert np.array_equal(din.cpu().numpy().view(np.uint64), np.asarray(words).ravel()), "input written"
        return z

    def dec_check(self, words, nl, slots, monkeypatch, want=None):
        """Folded (where the shape folds) and general path against the oracle."""
        want = self.oracle_dec(words, nl, slots) if want is None else want
        for fold in ("1", "0"):
            monkeypatch.setenv("GPQHE_DCD_FOLD", fold)
            got = self.dec_batch(words, nl, slots)
            bad = np.argwhere(bits(got) != bits(want))
            assert bad.size == 0, f"GPQHE_DCD_FOLD={fold}: {len(bad)} doubles differ, first at {bad[0].tolist()}"
        monkeypatch.delenv("GPQHE_DCD_FOLD")
        return want


def vectors(slots, cnt, seed):
    return [vector(slots, 1000 * seed + i) for i in range(cnt)]


def encryptions(E, case):
    """(zs, oracle words) of a case, from the cache or computed now (which
    advances the oracle's RNG by 3 streams a ciphertext)."""
    name, slots, nl, cnt = case
    if case not in _ENC:
        zs = vectors(slots, cnt, slots + cnt)
        words = E.oracle_enc(zs, slots, nl or E.L)
        words.setflags(write=False)
        _ENC[case] = (zs, words)
    return _ENC[case]


# set, slots, level (None: top), count: what it reaches
CASES = [
    ("ref", 16, None, 3),       # n = 4096: the small-N single calls queue; host encoder
    ("f13", 64, None, 1),       # all-FP64 moduli; a partial ciphertext group alone
    ("f13", 64, None, 3),
    ("f13", 64, None, 17),      # more than two groups of 8, the last partial
    ("c1", 64, None, 1),        # 60-bit q0: integer forms
    ("c1", 64, None, 3),
    ("c1", 64, None, 17),
    ("f13", 64, 1, 3),          # level 1
    ("f13", 2048, None, 3),     # GPU encoder, T = 2
    ("f13", 4096, None, 3),     # GPU encoder, T = 1: general decoder only
    ("bench51", 16, None, 5),   # n = 2^16, T = 2048
    ("bench_d2", 16, None, 5),  # ... with a 60-bit q0
]


@pytest.mark.parametrize("name,slots,nl,cnt", CASES)
def test_encrypt_equals_sequential_single_calls(oracle, product, name, slots, nl, cnt):
    E = Ends(oracle, product, name)
    case = (name, slots, nl, cnt)
    _ENC.pop(case, None)  # from this seed state: the RNG must end where the oracle's does
    zs, want = encryptions(E, case)
    got = E.enc_batch(zs, slots, nl or E.L)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} words differ, first at {bad[0].tolist()}"
    # the RNG continued: one more single encryption on both engines
    z = vector(slots, 5)
    co = oracle.encrypt(z, E.ko[0], slots, E.scale, nl or E.L)
    cp = product.encrypt(z, E.kp[0], slots, E.scale, nl or E.L)
    same(oracle, product, co, cp)
    oracle.free(co)
    product.free(cp)
    E.close()


@pytest.mark.parametrize("name,slots,nl,cnt", CASES)
def test_decode_of_encryptions(oracle, product, name, slots, nl, cnt, monkeypatch):
    """The encryptions at their level and one level lower (he_moddown)."""
    E = Ends(oracle, product, name)
    zs, words = encryptions(E, (name, slots, nl, cnt))
    lvl = nl or E.L
    want = E.dec_check(words, lvl, slots, monkeypatch)
    assert np.abs(want - np.stack(zs)).max() < 1e-6  # (they do decrypt)
    if lvl > 1:
        E.dec_check(E.oracle_moddown(words, lvl), lvl - 1, slots, monkeypatch)
    E.close()


def random_words(E, cnt, nl, seed):
    """poly_fill_uniform residues [cnt][2][nl][n] made on the device."""
    import torch
    buf = torch.zeros(cnt * 2 * nl * E.n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    E.p.lib.poly_fill_uniform(buf.data_ptr(), cnt * 2, nl, seed)
    E.p.sync()
    return buf.cpu().numpy().view(np.uint64).reshape(cnt, -1)


RANDOM = ([("f13", lvl, s, 3) for lvl in (1, 2, None) for s in (16, 64, 2048, 4096)] +
          [("ref", None, 16, 5), ("ref", 1, 2048, 2), ("c1", None, 64, 9), ("c1", 2, 4096, 2), ("c1", 1, 2, 2),
           ("bench51", None, 16, 5), ("bench51", 2, 64, 2), ("bench_d2", None, 16, 5), ("bench_d2", 1, 2048, 2)])


@pytest.mark.parametrize("name,nl,slots,cnt", RANDOM)
def test_decode_of_random_residues(oracle, product, name, nl, slots, cnt, monkeypatch):
    """Full-width residues: the folded sum is exact on any input."""
    E = Ends(oracle, product, name)
    lvl = nl or E.L
    E.dec_check(random_words(E, cnt, lvl, 100 + slots), lvl, slots, monkeypatch)
    E.close()


@pytest.mark.parametrize("env", [{"GPQHE_CHUNK": "5"}, {"GPQHE_WS_MIB": "1"}])
def test_chunks_do_not_change_bits(oracle, product, env, monkeypatch):
    """17 ciphertexts as 5/5/5/2 (GPQHE_CHUNK) or cut by a 1 MiB workspace (one
    ciphertext an encryption chunk, two a general decode chunk) against one chunk."""
    E = Ends(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 17, 3)
    product.set_seed(SEED + 1)
    one = E.enc_batch(zs, slots, lvl)
    zone = {f: None for f in ("1", "0")}
    for f in zone:
        monkeypatch.setenv("GPQHE_DCD_FOLD", f)
        zone[f] = E.dec_batch(one, lvl, slots)
    assert np.array_equal(bits(zone["1"]), bits(zone["0"]))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    product.set_seed(SEED + 1)
    assert np.array_equal(E.enc_batch(zs, slots, lvl), one)
    for f in zone:
        monkeypatch.setenv("GPQHE_DCD_FOLD", f)
        assert np.array_equal(bits(E.dec_batch(one, lvl, slots)), bits(zone[f]))
    E.close()


def test_empty_batch_and_zero_vectors(oracle, product):
    E = Ends(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 2, 4)
    # count = 0: nothing written, no stream taken
    got = E.enc_batch(zs, slots, lvl, count=0)
    assert (got == FILL).all()
    z = np.full((2, slots), 3 + 4j)
    product._ext("he_dec_dcd_batch")(z.ctypes.data, None, 0, lvl, E.scale, slots, C.byref(E.kp[1]))
    assert (z == 3 + 4j).all()
    co = oracle.encrypt(zs[0], E.ko[0], slots, E.scale, lvl)
    cp = product.encrypt(zs[0], E.kp[0], slots, E.scale, lvl)
    same(oracle, product, co, cp)
    oracle.free(co)
    product.free(cp)
    # an all-zero batch
    zero = [np.zeros(slots, dtype=np.complex128)] * 3
    want = E.oracle_enc(zero, slots, lvl)
    got = E.enc_batch(zero, slots, lvl)
    assert np.array_equal(got, want)
    zd = E.dec_batch(got, lvl, slots)
    assert np.array_equal(bits(zd), bits(E.oracle_dec(want, lvl, slots)))
    assert np.abs(zd).max() < 1e-6
    E.close()


def test_end_to_end_gemv(oracle, product):
    """enc_pk_batch -> he_gemv_batch -> dec_dcd_batch against M z, within the he_gemv tests' bound."""
    import torch
    E = Ends(oracle, product, "f13")
    slots, lvl, cnt = product.slots, E.L, 3
    rk = product.evks(slots)
    product.genrk(rk, E.kp[1])
    zs = vectors(slots, cnt, 8)
    Mx = matrix(slots, 31)
    x = torch.zeros(cnt * 2 * lvl * E.n, dtype=torch.int64, device="cuda")
    y = torch.zeros(cnt * 2 * (lvl - 1) * E.n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    product.enc_pk_batch(x.data_ptr(), np.stack(zs), E.kp[0], slots, E.scale, lvl)
    product.lib.he_gemv_batch(y.data_ptr(), np.ascontiguousarray(Mx).ctypes.data, x.data_ptr(), cnt, lvl, rk)
    got = product.dec_dcd_batch(y.data_ptr(), cnt, lvl - 1, E.scale, E.kp[1], slots)
    for i, z in enumerate(zs):
        want = Mx @ z
        err = np.abs(got[i] - want).max()
        assert err < 1e-6 * max(1.0, np.abs(want).max()), (i, err)
    product.free_evks(rk)
    E.close()


def test_kernel_classes_are_reported(oracle, product, monkeypatch):
    E = Ends(oracle, product, "f13")
    lvl = E.L
    product.prof_enable(True)
    try:
        product.prof_collect()
        x = E.enc_batch(vectors(64, 3, 1), 64, lvl)
        E.dec_batch(x, lvl, 64)
        monkeypatch.setenv("GPQHE_DCD_FOLD", "0")
        E.dec_batch(x, lvl, 64)
        E.enc_batch(vectors(2048, 2, 1), 2048, lvl)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k in ("enc_sample_batch_kernel", "enc_combine_batch_kernel", "dec_fold_kernel", "fold_dcd_kernel",
              "dec_batch_kernel", "fft_enc_batch_kernel"):
        assert k in stats, sorted(stats)
        assert stats[k][0] >= 1 and stats[k][2] > 0, (k, stats[k])
    E.close()


def test_teardown_clean_exit():
    """Both calls, hectx_exit, a second context, both calls again, exit: rc 0."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "io_batch_worker.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rc {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert res == {"first": True, "second": True}, res
