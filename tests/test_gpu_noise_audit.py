"""The audit of tests/test_model_sampling.py, test_model_keyswitch.py and
test_noise_cpu.py run on the product's own exported objects (not through the
oracle): samplers and stream numbering predicted from the seed, the key
identity on every digit and limb, and the noise of the product's results under
the analytic ceilings.  The oracle takes part only as the CPU transform of the
exported words (noise_audit.use_host_transforms).  One context per kernel
family; one he_genrot per key instead of a full he_genrk.  That the product's
bits equal the oracle's is the parity tests' business and is not repeated
here."""
import ctypes
import time

import numpy as np
import pytest

import noise_audit as A
from tests.test_gpu_parity import PARAMS

pytestmark = pytest.mark.gpu

CONTEXTS = ["ref", "hyb", "f13", "a5", "k5", "c15", "bench51"]
SEED = 4242


def init(oracle, product, name):
    """The product at context `name` (16 slots) and seed SEED; the oracle is
    initialised for the same moduli only to transform host arrays."""
    kind, kw = PARAMS[name]
    kw = dict(kw, slots=A.SLOTS)
    for e in (oracle, product):
        if kind == "init":
            e.init(**kw)
        else:
            e.init_params(**kw)
    product.set_seed(SEED)
    A.use_host_transforms(product, oracle)
    return product


def genrot(e, r, sk):
    evk = e.evk()
    e.lib.he_genrot(ctypes.byref(evk), r, ctypes.byref(sk))
    return evk


@pytest.mark.parametrize("name", CONTEXTS)
def test_samplers_and_key_structure(oracle, product, name):
    """he_keypair, he_genrlk, he_genrot(1) and one he_enc_pk in that order: the
    secret, the public key's a and every error polynomial are the model's
    samples of streams 0, 1, 2, ...; every digit and limb of both evaluation
    keys satisfies b + a s - [m in digit] P s' = e.  At n = 2^16 the samples
    are compared on a fixed subset of 512 coefficients (0, 1, n/2, n - 1
    among them); the same-integer-on-every-limb check is always on all n."""
    t0 = time.time()
    e = init(oracle, product, name)
    n = e.n
    idx = A.subset(n) if n >= 1 << 16 else None
    st = A.Streams(SEED)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rot = genrot(e, 1, sk)
    z = np.random.default_rng(1).uniform(-1, 1, A.SLOTS) + 0j
    pt, ct = e.pt(), e.ct()
    e.ecd_ex(pt, z, A.SLOTS, A.SCALE, e.L)
    e.enc_pk(ct, pt, pk)
    s, epk, s_ntt = A.audit_keypair(e, st, pk, sk, idx)
    ends = (0, e.L + e.K - 1)  # the evk's a on the first and the last modulus; pk.a is checked on every limb
    small = [("s", s), ("e_pk", epk)]
    small += [(f"e_rlk{j}", x) for j, x in enumerate(A.audit_evk(e, st, rlk, s, s_ntt, 1, idx, a_limbs=ends))]
    g = pow(5, 1, 2 * n)
    assert rot.galois == g
    small += [(f"e_rot{j}", x) for j, x in enumerate(A.audit_evk(e, st, rot, s, s_ntt, g, idx, a_limbs=ends))]
    small += list(zip(("v", "e0", "e1"), A.audit_enc_pk(e, st, ct, pt, pk, idx)))
    assert st.next == 3 + 4 * e.info.dnum + 3
    A.pairwise_distinct(small)
    for o in (pk, sk, rlk, rot, pt, ct):
        e.free(o)
    print(f"{name}: samplers and key structure in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("name", CONTEXTS)
def test_noise_under_ceilings(oracle, product, name):
    """Exact decryption of the product's he_enc_pk, he_rot, he_mul_rescale and
    he_gemv (diagonals 0 and 1) minus the exact expected message, under
    ckks_model.noise_ceilings; at n = 2^16 he_enc_pk and he_mul_rescale only;
    on ref and f13 also he_gemv_bsgs (default baby-step count, diagonals
    0, 1, 5, 9, 12: two babies, every giant step)."""
    t0 = time.time()
    e = init(oracle, product, name)
    big = e.n >= 1 << 16
    ops = ("enc_pk", "mul_rescale") if big else ("enc_pk", "rot", "mul_rescale")
    got, extra = A.measure_ops(e, SEED, ops)
    assert set(got) == set(ops)
    for op, (mx, mean) in got.items():
        c = A.ceiling_of(e, op, extra)
        print(f"{name} {op}: max |noise| {mx:.6g} mean {mean:.6g} ceiling {c:.6g}")
        assert mx <= c, (name, op)
    if not big:
        (mx, mean), x = A.measure_gemv(e, SEED, [0, 1])
        c = A.gemv_ceiling(e, x)
        print(f"{name} gemv: max |noise| {mx:.6g} mean {mean:.6g} ceiling {c:.6g}")
        assert mx <= c, (name, "gemv")
    if name in ("ref", "f13"):
        (mx, mean), x = A.measure_bsgs(e, SEED, [0, 1, 5, 9, 12], 4)
        c = A.bsgs_ceiling(e, x)
        print(f"{name} gemv_bsgs: max |noise| {mx:.6g} mean {mean:.6g} ceiling {c:.6g}")
        assert mx <= c, (name, "gemv_bsgs")
    print(f"{name}: noise in {time.time() - t0:.2f} s")


def test_queued_encryptions_use_disjoint_streams(oracle, product):
    """HECTR's step on its own ring: five encodes, then five encryptions (queued
    at n = 2^12), read only afterwards.  Each takes the next stream triple:
    (v, e0, e1) of every one is the model's, and all fifteen differ."""
    e = init(oracle, product, "ref")
    st = A.Streams(SEED)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    st.next = 3
    rng = np.random.default_rng(5)
    pts, cts = [], []
    for _ in range(5):
        pt = e.pt()
        e.ecd_ex(pt, rng.uniform(-1, 1, A.SLOTS) + 1j * rng.uniform(-1, 1, A.SLOTS), A.SLOTS, e.info.delta, e.L)
        pts.append(pt)
    for pt in pts:
        ct = e.ct()
        e.enc_pk(ct, pt, pk)
        cts.append(ct)
    small = []
    for i, (pt, ct) in enumerate(zip(pts, cts)):
        small += list(zip((f"v{i}", f"e0_{i}", f"e1_{i}"), A.audit_enc_pk(e, st, ct, pt, pk)))
    assert st.next == 18 and len(small) == 15
    A.pairwise_distinct(small)
    for o in pts + cts + [pk, sk]:
        e.free(o)
