"""The engine's random number generation pinned to an independent model
(tests/ckks_model_rng.py): ChaCha20 against openssl's keystream, the three
sampling maps, the stream numbering (one fresh stream per sampled polynomial,
restarted by a reseed) and the default seed.  CPU only, on the oracle; the same
audit runs on the product in tests/test_gpu_noise_audit.py, and on its batch
encrypting calls in tests/test_gpu_batch_audit.py."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

import ckks_model_rng as R
import make_golden
import noise_audit as A

HERE = os.path.dirname(os.path.abspath(__file__))

CTX = {"n64": dict(logn=6, nlimbs=2, nspecial=1, dnum=2),
       "n256": dict(logn=8, nlimbs=3, nspecial=2, dnum=2)}


def init(oracle, name, seed):
    oracle.init_params(slots=8, q0_bits=55, qi_bits=45, p_bits=58, seed=seed, **CTX[name])
    return oracle


def golden():
    with open(os.path.join(HERE, "golden", "chacha_vectors.json")) as f:
        return json.load(f)["blocks"]


def test_chacha_known_answers():
    """Scalar and vectorised blocks equal openssl's committed keystream; the
    key of a seed is the splitmix64 derivation."""
    blocks = golden()
    assert {(c["seed"], c["stream"], c["counter"]) for c in blocks} == set(make_golden.CHACHA_CASES)
    assert any(c["counter"] == 2 ** 32 - 1 for c in blocks) and any(c["stream"] >= 2 ** 32 for c in blocks)
    assert any(not any(c["key"]) for c in blocks)
    for c in blocks:
        if c["seed"] is not None:
            assert R.seed_key(c["seed"]) == c["key"]
        want = bytes.fromhex(c["keystream"])
        assert R.block_bytes(R.chacha20_block(c["key"], c["stream"], c["counter"])) == want
        assert R.block_bytes(R.chacha20_blocks(c["key"], c["stream"], [c["counter"]])[0]) == want


def test_chacha_vectorised_equals_scalar():
    key = R.seed_key(31)
    counters = [0, 1, 2, 255, 256, 65535, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    got = R.chacha20_blocks(key, 2 ** 40 + 3, counters)
    for i, c in enumerate(counters):
        assert got[i].tolist() == R.chacha20_block(key, 2 ** 40 + 3, c)


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on the path to re-derive the vectors live")
def test_chacha_vectors_rederived_from_openssl():
    assert make_golden.chacha_vectors() == golden()


def test_sampler_maps_on_crafted_words(monkeypatch):
    """The three maps on keystream words chosen by hand: bits above the masks
    are ignored, the ternary table, the 128-bit little-endian word order and
    the block / word a modulus reads."""
    words = {}

    def fake(key, stream, counters):
        out = np.zeros((len(counters), 16), dtype=np.uint32)
        for i, c in enumerate(np.asarray(counters).tolist()):
            out[i] = words.get(c, [0] * 16)
        return out

    monkeypatch.setattr(R, "chacha20_blocks", fake)
    words.update({0: [0xFFFFFFFC] + [0] * 15, 1: [0x1D] + [0] * 15, 2: [0x12] + [0] * 15, 3: [0x7] + [0] * 15})
    assert R.sample_ternary(None, 0, 4).tolist() == [0, 0, 1, -1]
    words.clear()
    words.update({0: [0xFFFFFFFF, 0xFFE00000] + [0] * 14, 1: [0xFFE00000, 0x001FFFFF] + [0] * 14,
                  2: [0x00100001, 0x00000002] + [0] * 14})
    assert R.sample_cbd(None, 0, 3).tolist() == [21, -21, 1]
    words.clear()
    # 6 moduli: nb = 2 blocks per coefficient; modulus 5 of coefficient 3 reads block 7, words 4..7
    words[7] = [9] * 4 + [1, 2, 3, 4] + [9] * 8
    q = (1 << 61) - 1
    assert int(R.sample_uniform(None, 0, 4, 5, q, 6, idx=[3])[0]) == (1 + (2 << 32) + (3 << 64) + (4 << 96)) % q


def genrot(e, r, sk):
    evk = e.evk()
    e.lib.he_genrot(ctypes.byref(evk), r, ctypes.byref(sk))
    return evk


def run_documented_order(e, seed):
    """he_keypair, he_genrlk, he_genrot(1), 3 x he_enc_pk, 2 x he_enc_sk and
    one more he_enc_pk against streams 0, 1, 2, ...; returns the named small
    polynomials recovered (the uniform c1 of the secret-key encryptions are
    compared with each other and the public key's a here)."""
    st = A.Streams(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rot = genrot(e, 1, sk)
    s, epk, s_ntt = A.audit_keypair(e, st, pk, sk)
    assert st.next == 3
    small = [("s", s), ("e_pk", epk)]
    small += [(f"e_rlk{j}", x) for j, x in enumerate(A.audit_evk(e, st, rlk, s, s_ntt, 1))]
    g = pow(5, 1, 2 * e.n)
    assert rot.galois == g
    small += [(f"e_rot{j}", x) for j, x in enumerate(A.audit_evk(e, st, rot, s, s_ntt, g))]
    assert st.next == 3 + 4 * e.info.dnum
    rng = np.random.default_rng(seed)
    for i in range(3):
        z = rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8)
        pt, ct = e.pt(), e.ct()
        e.ecd(pt, z)
        e.enc_pk(ct, pt, pk)
        v, e0, e1 = A.audit_enc_pk(e, st, ct, pt, pk)
        small += [(f"v{i}", v), (f"e0_{i}", e0), (f"e1_{i}", e1)]
        e.free(pt)
        e.free(ct)
    assert st.next == 12 + 4 * e.info.dnum
    # he_enc_sk: a (uniform) from the next stream, e (CBD) from the one after
    firsts = []
    for i in range(2):
        z = rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8)
        pt, ct = e.pt(), e.ct()
        e.ecd(pt, z)
        e.enc_sk(ct, pt, sk)
        t = st.next
        a, err = A.audit_enc_sk(e, st, ct, pt, sk)
        assert st.next == t + 2
        small.append((f"e_sk{i}", err))
        firsts.append((f"a_sk{i}", a))
        e.free(pt)
        e.free(ct)
    assert st.next == 16 + 4 * e.info.dnum
    # ... and a public-key encryption after them sees the next three
    z = rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8)
    pt, ct = e.pt(), e.ct()
    e.ecd(pt, z)
    e.enc_pk(ct, pt, pk)
    small += list(zip(("v3", "e0_3", "e1_3"), A.audit_enc_pk(e, st, ct, pt, pk)))
    e.free(pt)
    e.free(ct)
    assert st.next == 19 + 4 * e.info.dnum
    A.pairwise_distinct(firsts + [("a_pk", e.export(pk)[1])])
    for o in (pk, sk, rlk, rot):
        e.free(o)
    return small


@pytest.mark.parametrize("seed", [1, 99])
@pytest.mark.parametrize("name", list(CTX))
def test_documented_stream_order(oracle, name, seed):
    """Every sampled polynomial of the documented call order is the model's
    sample from the stream that order assigns, the same integer is lifted to
    every limb (checked inside the audit), the CBD range holds and no two small
    polynomials coincide."""
    small = run_documented_order(init(oracle, name, seed), seed)
    A.pairwise_distinct(small)
    for nm, p in small:
        bound = 1 if nm[0] in "sv" else R.CBD_ETA
        assert np.abs(p).max() <= bound, nm
    # the samplers are not degenerate: ternary density 1/2, CBD variance 10.5
    # (n = 64 and 256 draws: 5 sigma of a binomial / chi-square estimate)
    n = oracle.n
    s = dict(small)["s"]
    assert abs(np.count_nonzero(s) - n / 2) <= 5 * np.sqrt(n / 4)
    e = np.concatenate([p for nm, p in small if nm[0] == "e"])
    assert abs(e.astype(float).var() - R.CBD_VAR) <= 5 * R.CBD_VAR * np.sqrt(2.0 / e.size)


def secret(e):
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    s, _ = A.secret_of(e, sk)
    e.free(pk)
    e.free(sk)
    return s


def test_set_seed_restarts_the_stream_count(oracle):
    init(oracle, "n64", 1)
    first = secret(oracle)
    second = secret(oracle)  # streams 3, 4, 5
    key = R.seed_key(1)
    assert np.array_equal(first, R.sample_ternary(key, 0, 64))
    assert np.array_equal(second, R.sample_ternary(key, 3, 64))
    oracle.set_seed(1)
    assert np.array_equal(secret(oracle), first)
    oracle.set_seed(2)
    other = secret(oracle)
    assert np.array_equal(other, R.sample_ternary(R.seed_key(2), 0, 64))
    assert not np.array_equal(other, first)


def test_default_seed(oracle, monkeypatch):
    """seed = 0: a fresh seed per initialisation unless GPQHE_SEED names one
    (the environment is read at every initialisation, so no child process)."""
    monkeypatch.delenv("GPQHE_SEED", raising=False)
    a = secret(init(oracle, "n256", 0))
    b = secret(init(oracle, "n256", 0))
    assert not np.array_equal(a, b)
    monkeypatch.setenv("GPQHE_SEED", "77")
    c = secret(init(oracle, "n256", 0))
    d = secret(init(oracle, "n256", 0))
    explicit = secret(init(oracle, "n256", 77))
    assert np.array_equal(c, d) and np.array_equal(c, explicit)
    assert np.array_equal(c, R.sample_ternary(R.seed_key(77), 0, 256))
