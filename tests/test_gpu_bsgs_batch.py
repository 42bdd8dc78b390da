"""he_gemv_bsgs_batch (include/gpqhe_ext_batch.h) on the MI355X against the
composition that defines he_gemv_bsgs, run on the oracle per ciphertext
(tests/bsgs_ref.bsgs_compose), never against the product's own single call.

The product encrypts cnt distinct vectors; their exported words are the device
input (a torch buffer) and, he_import-ed, the oracle's ciphertexts; both
engines hold the BSGS key subset generated from the same seed.  Every word of
every y_i must equal the oracle's, every y_i decode to within the he_gemv
tests' bound of M z_i, the 4096 guard words behind the output and the input
stay as they were.  The shapes are the smallest that reach each path."""
import numpy as np
import pytest

from tests.bsgs_ref import bsgs_compose
from tests.test_gpu_bsgs import Side, init, matrix, vector

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 7
_REF = {}  # (shape key) -> (input words, oracle words): computed once, shared by the tests of a shape


class Pair:
    """Both engines on one parameter set with the same BSGS keys."""

    def __init__(self, oracle, product, name, slots, g, seed=77):
        init(oracle, product, name, slots, seed)
        self.o, self.p, self.g = oracle, product, g
        z = vector(slots, 1)
        self.O, self.P = Side(oracle, g, z), Side(product, g, z, product_keys=True)

    def inputs(self, zs, level):
        """The product's encryptions of zs at `level`: (words [cnt][2 level n], scale)."""
        out = []
        for z in zs:
            x = self.P.enc(z, level)
            assert x.nlimbs == level
            scale = x.scale
            out.append(self.p.export(x).ravel().copy())
            self.p.free(x)
        return np.stack(out), scale

    def reference(self, key, M, host, level, scale):
        """bsgs_compose on the oracle of every imported ciphertext."""
        if key in _REF and np.array_equal(_REF[key][0], host):
            return _REF[key][1]
        rows = []
        for w in host:
            x = self.o.ct()
            self.o.import_(x, w, level, scale=scale)
            y = bsgs_compose(self.o, M, x, self.O.rk, self.g)
            assert y.nlimbs == level - 1
            rows.append(self.o.export(y).ravel().copy())
            self.o.free(x)
            self.o.free(y)
        _REF[key] = (host.copy(), np.stack(rows))
        _REF[key][1].setflags(write=False)
        return _REF[key][1]

    def batch(self, M, host, level, count=None):
        """he_gemv_bsgs_batch on the product: (output words [cnt][..], guard ok, input unchanged)."""
        import torch
        cnt = len(host) if count is None else count
        ow = 2 * (level - 1) * self.p.n
        din = torch.from_numpy(host.ravel().view(np.int64)).cuda()
        dout = torch.full((len(host) * ow + GUARD,), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.p.gemv_bsgs_batch(dout.data_ptr(), M, din.data_ptr(), cnt, level, self.P.rk, self.g)
        self.p.sync()
        got = dout.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[len(host) * ow:], np.full(GUARD, FILL, dtype=np.uint64)), "guard words written"
        assert np.array_equal(din.cpu().numpy().view(np.uint64), host.ravel()), "input written"
        return got[:len(host) * ow].reshape(len(host), ow)

    def check(self, key, M, zs, level):
        host, scale = self.inputs(zs, level)
        want = self.reference(key, M, host, level, scale)
        got = self.batch(M, host, level)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} residues differ"
        Mz = np.asarray(M).reshape(len(zs[0]), -1)
        for i, z in enumerate(zs):
            ct = self.p.ct()
            self.p.import_(ct, got[i], level - 1, scale=scale)
            err = np.abs(self.p.decrypt(ct, self.P.sk) - Mz @ z).max()
            self.p.free(ct)
            assert err < 1e-6 * max(1.0, np.abs(Mz @ z).max()), (i, err)
        return host, scale, want

    def close(self):
        self.O.close()
        self.P.close()


def vectors(slots, cnt, seed):
    return [vector(slots, 1000 * seed + i) for i in range(cnt)]


# set, slots, g, level, cnt, diagonals: what it reaches
PARITY = [
    # generic rotations (n = 4096) with the batched inner and sum kernels
    ("ref", 16, 4, 2, 1, None),     # one ciphertext: a partial ciphertext tile alone
    ("ref", 16, 4, 2, 5, None),     # a partial last ciphertext tile
    ("ref", 16, 4, 2, 9, None),     # more than one tile for any tile of up to 8 ciphertexts
    ("ref", 16, 16, 2, 3, None),    # G = 1: no giant rotation, no sum
    ("ref", 16, 1, 2, 3, None),     # no babies
    ("ref", 16, 6, 2, 3, None),     # partial last giant step
    ("ref", 32, 8, 2, 3, (0, 1, 2, 9, 17, 31)),  # skipped babies, a giant step with one diagonal
    ("ref", 16, 4, 2, 3, (5, 9, 14)),  # nothing in giant step 0: the sum starts without u_0
    ("ref", 64, 24, 2, 3, None),    # partial second baby tile
    ("ref", 64, 32, 2, 3, tuple(range(21)) + (33,)),  # a giant step with nothing in the second tile
    # windowed rotations (folded keys, k_gemv_batch over the chunk)
    ("hyb", 32, 4, 5, 3, None),     # K = 2, three digits, the last partial, integer slots
    ("hyb", 32, 4, 4, 3, None),     # ... below the top level
    ("f13", 256, 0, 6, 2, None),    # all-FP64; giants wrap the Galois orbit; 30 folds
    ("f13", 64, 24, 6, 3, None),
    ("bench_d2", 16, 4, 8, 3, None),
    ("bench51", 64, 0, 8, 2, None),
    # a large ring without the windowed path: four digits
    ("c1", 64, 0, 4, 2, None),
]


@pytest.mark.parametrize("name,slots,g,level,cnt,only", PARITY)
def test_batch_equals_composition(oracle, product, name, slots, g, level, cnt, only):
    pr = Pair(oracle, product, name, slots, g)
    M = matrix(slots, 3 * slots + g, only)
    pr.check((name, slots, g, level, cnt, only), M, vectors(slots, cnt, level), level)
    pr.close()


@pytest.mark.parametrize("name,level", [("ref", 2), ("f13", 6)])
def test_forced_chunks_do_not_change_bits(oracle, product, name, level, monkeypatch):
    """GPQHE_BSGS_CHUNK = 2: five ciphertexts as 2 + 2 + 1."""
    monkeypatch.setenv("GPQHE_BSGS_CHUNK", "2")
    pr = Pair(oracle, product, name, 16, 4)
    pr.check((name, 16, 4, level, 5, None), matrix(16, 3 * 16 + 4), vectors(16, 5, level), level)
    pr.close()


def test_workspace_chunks_do_not_change_bits(oracle, product, monkeypatch):
    """GPQHE_WS_MIB = 1: a ciphertext's slot-major buffers alone exceed it, so
    every chunk holds one ciphertext and the stages' own workspaces are cut."""
    monkeypatch.setenv("GPQHE_WS_MIB", "1")
    pr = Pair(oracle, product, "ref", 16, 4)
    pr.check(("ref", 16, 4, 2, 5, None), matrix(16, 3 * 16 + 4), vectors(16, 5, 2), 2)
    pr.close()


def test_zero_matrix_and_empty_batch(oracle, product):
    pr = Pair(oracle, product, "ref", 16, 4)
    host, _ = pr.inputs(vectors(16, 3, 2), 2)
    got = pr.batch(np.zeros((16, 16)), host, 2)
    assert not got.any()  # every y_i zero: the sentinel is overwritten
    got = pr.batch(matrix(16, 5), host, 2, count=0)
    assert (got == FILL).all()  # nothing touched
    pr.close()


def test_state(oracle, product):
    """Plan-cache hits, a single call sharing the entry, re-keyed rotations
    (no stale fold), and another parameter set after hectx_exit."""
    import ctypes as C
    name, slots, g, level = "f13", 16, 4, 6
    pr = Pair(oracle, product, name, slots, g)
    A, B = matrix(slots, 21), matrix(slots, 22)
    zs = vectors(slots, 3, 9)
    host, scale, wa = pr.check((name, "A"), A, zs, level)
    assert np.array_equal(pr.batch(A, host, level), wa)  # a hit
    wb = pr.reference((name, "B"), B, host, level, scale)
    assert np.array_equal(pr.batch(B, host, level), wb)
    # the single call with A (the entry a batch call made)
    x, y = product.ct(), product.ct()
    product.import_(x, host[1], level, scale=scale)
    product.gemv_bsgs(y, A, x, pr.P.rk, g)
    assert np.array_equal(product.export(y).ravel(), wa[1])
    product.free(x)
    product.free(y)
    # a baby and a giant rotation re-keyed on the product, copied to the oracle
    for r in (1, 2 * g):
        product.lib.he_free_evk(C.byref(pr.P.rk[r]))
        product.lib.he_genrot(C.byref(pr.P.rk[r]), r, C.byref(pr.P.sk))
        oracle.import_(pr.O.rk[r], product.export(pr.P.rk[r]), pr.P.rk[r].nlimbs)
    wa2 = pr.reference((name, "A rekeyed"), A, host, level, scale)
    assert not np.array_equal(wa2, wa)
    assert np.array_equal(pr.batch(A, host, level), wa2)
    pr.close()
    for e in (oracle, product):
        e.exit()
    pr = Pair(oracle, product, "ref", 16, 4)
    pr.check(("ref", "after exit"), matrix(16, 23), vectors(16, 3, 4), 2)
    pr.close()


def test_kernel_classes_are_reported(oracle, product):
    pr = Pair(oracle, product, "ref", 16, 4)
    host, _ = pr.inputs(vectors(16, 3, 6), 2)
    M = matrix(16, 42)
    pr.batch(M, host, 2)  # warm
    product.prof_enable(True)
    try:
        product.prof_collect()
        pr.batch(M, host, 2)
        stats = product.prof_collect()
    finally:
        product.prof_enable(False)
    for k in ("bsgs_inner_batch_kernel", "bsgs_sum_batch_kernel"):
        assert k in stats, sorted(stats)
        assert stats[k][0] >= 1 and stats[k][2] > 0
    pr.close()
