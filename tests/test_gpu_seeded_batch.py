"""he_enc_sk_seeded_batch, its packed and gain forms and he_expand_seeded_batch
(include/gpqhe_ext_seeded_batch.h) on the MI355X against tests/seeded_ref on
the oracle -- the sequential he_ecd_ex + he_enc_sk from the same
gpqhe_set_seed, c1 replaced by the model's sample under the public key in exact
integers -- never against the product's own calls: every word of the compact
c0 and of the expanded x bit for bit, both seeds' streams left where the
contract says, guard words and inputs intact; then the ciphertexts through the
batch decode and the packed steps against the reference compositions on the
oracle, and the closed loops of cstr.*Regulator(sym="seeded").  Both engines
generate their keys from one seed.  The shapes are the smallest that reach
each path: host and GPU encoder, one and several ChaCha blocks per coefficient
(nb = ceil((L + K) / 4)), a partial last group of four limbs, FP64 and integer
moduli inside one block, full and partial ciphertext groups, a carry into the
public stream's high word."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hectr_amd import cstr
from hectr_amd.gpqhe import Engine, PubSeed
from tests.encgain_ref import gain_diagonals, step_encgain_compose
from tests.packed_ref import interleave, packed_rotations, step_packed_compose
from tests.rows_ref import pow2
from tests.seeded_ref import (RefSeededGainRegulator, RefSeededPackedRegulator, enc_gain_sk_seeded_compose,
                              enc_sk_seeded_packed_words, enc_sk_seeded_words)
from tests.test_gpu_bsgs import vector
from tests.test_gpu_encgain_batch import ORACLE_LOOP_WORST, GainPair
from tests.test_gpu_io_batch import FILL, SEED, bits, vectors
from tests.test_gpu_packed_batch import PackedPair, loops, matrices
from tests.test_gpu_parity import PARAMS, same
from tests.test_gpu_sk_batch import SkEnds, assert_words, check_step_output, dev, six_plants, words_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBKEY = bytes(range(101, 133))
PUBSTREAM = 2 ** 32 - 1  # ciphertext 1 of a call carries into the stream's high word
_ENC = {}  # case -> (zs, c0 words, expanded words, plain words) of the oracle: computed once, shared, read-only


def seed_at(stream=PUBSTREAM):
    return Engine.pubseed(PUBKEY, stream)


def copy_of(ps):
    return PubSeed.from_buffer_copy(ps)


def expand(product, c0_words, cnt, nl, ps):
    """he_expand_seeded_batch of host c0 words [cnt][nl n] under the seed value
    ps: x words [cnt][2 nl n]; guards, c0 and ps checked unchanged."""
    import torch
    w = nl * product.n
    din = torch.from_numpy(np.array(c0_words).ravel().view(np.int64)).cuda()
    x = dev(len(c0_words) * 2 * w)
    keep = bytes(ps)
    product.expand_seeded_batch(x.data_ptr(), din.data_ptr(), cnt, nl, ps)
    product.sync()
    assert bytes(ps) == keep, "the seed was written"
    assert np.array_equal(din.cpu().numpy().view(np.uint64), np.asarray(c0_words).ravel()), "c0 written"
    return words_of(x, len(c0_words) * 2 * w).reshape(len(c0_words), 2 * w)


class SeededEnds(SkEnds):
    """SkEnds with the seeded calls."""

    def oracle_seeded(self, zs, slots, nl, stream=PUBSTREAM, scale=None):
        return enc_sk_seeded_words(self.o, zs, self.ko[1], slots, scale or self.scale, nl, PUBKEY, stream)

    def enc_seeded(self, zs, slots, nl, ps, count=None):
        """he_enc_sk_seeded_batch: the c0 words [len(zs)][nl n]; guard, input and the seed's advance checked."""
        w = nl * self.n
        dout = dev(len(zs) * w)
        zz = np.asarray(zs, dtype=np.complex128).reshape(len(zs), slots)
        keep, cnt, before = zz.copy(), len(zs) if count is None else count, copy_of(ps)
        self.p.enc_sk_seeded_batch(dout.data_ptr(), zz[:cnt], self.kp[1], slots, self.scale, nl, ps)
        self.p.sync()
        assert np.array_equal(bits(zz), bits(keep)), "input written"
        assert bytes(ps)[:32] == bytes(before)[:32] and ps.stream == before.stream + cnt
        return words_of(dout, len(zs) * w).reshape(len(zs), w)

    def enc_seeded_packed(self, zs, s, width, nl, ps):
        w = nl * self.n
        dout = dev(len(zs) * w)
        zz = np.stack(zs)
        keep, before = zz.copy(), copy_of(ps)
        self.p.enc_sk_seeded_packed_batch(dout.data_ptr(), zz, self.kp[1], s, width, self.scale, nl, ps)
        self.p.sync()
        assert np.array_equal(bits(zz), bits(keep)), "input written"
        assert ps.stream == before.stream + len(zs)
        return words_of(dout, len(zs) * w).reshape(len(zs), w)

    def both(self, zs, slots, nl, want, stream=PUBSTREAM):
        """Encrypt and expand against want = (c0, expanded, plain) words."""
        ps = seed_at(stream)
        c0 = self.enc_seeded(zs, slots, nl, ps)
        assert_words(c0, want[0], "c0")
        x = expand(self.p, c0, len(zs), nl, seed_at(stream))
        assert_words(x, want[1], "expanded")
        return x


def encryptions(E, case):
    """(zs, oracle c0 / expanded / plain words) of a case right after E's key
    pair, from the cache or computed now (which advances the oracle's RNG by 2
    streams a ciphertext)."""
    name, slots, nl, cnt = case
    if case not in _ENC:
        zs = vectors(slots, cnt, slots + cnt)
        words = E.oracle_seeded(zs, slots, nl or E.L)
        for w in words:
            w.setflags(write=False)
        _ENC[case] = (zs, words)
    return _ENC[case]


# set, slots, level (None: top), count: what it reaches
CASES = [
    ("ref", 16, None, 3),       # n = 4096, nb = 1: an FP64 and an integer limb in one block; a queued he_enc_pk before
    ("f13", 64, None, 1),       # nb = 3, level 6: groups of 4 and 2 limbs; a partial ciphertext group alone
    ("f13", 64, None, 3),
    ("f13", 64, None, 17),      # more than two groups of 8, the last partial
    ("f13", 64, 1, 3),          # level 1: one limb of the first block
    ("c1", 64, None, 3),        # 60-bit q0 beside 50-bit limbs
    ("hyb", 32, None, 3),       # K = 2, level 5: groups of 4 and 1
    ("f13", 2048, None, 3),     # GPU encoder, gap 2
    ("f13", 4096, None, 3),     # GPU encoder, gap 1
    ("bench51", 16, None, 1),   # n = 2^16, nb = 3
]


@pytest.mark.parametrize("name,slots,nl,cnt", CASES)
def test_encrypt_and_expand_equal_the_reference(oracle, product, name, slots, nl, cnt):
    E = SeededEnds(oracle, product, name)
    lvl = nl or E.L
    pre = None
    if name == "ref":  # a single encryption first: queued on the product, its streams already taken
        z0 = vector(slots, 6)
        pre = (oracle.encrypt(z0, E.ko[0], slots, E.scale, lvl), product.encrypt(z0, E.kp[0], slots, E.scale, lvl))
        zs = vectors(slots, cnt, slots + cnt)
        want = E.oracle_seeded(zs, slots, lvl)
    else:
        _ENC.pop((name, slots, nl, cnt), None)  # from this seed state: the RNG must end where the oracle's does
        zs, want = encryptions(E, (name, slots, nl, cnt))
    E.both(zs, slots, lvl, want)
    if pre:
        same(oracle, product, *pre)
        oracle.free(pre[0])
        product.free(pre[1])
    E.rng_continued(slots, lvl)  # the private streams: 2 a ciphertext, as after he_enc_sk_batch
    E.close()


def test_public_stream_carry(oracle, product):
    """Streams 2^32 - 2 .. 2^32 + 2: the low word wraps inside the call."""
    E = SeededEnds(oracle, product, "ref")
    start, zs = 2 ** 32 - 2, vectors(16, 5, 21)
    want = E.oracle_seeded(zs, 16, E.L, start)
    ps = seed_at(start)
    assert_words(E.enc_seeded(zs, 16, E.L, ps), want[0], "c0")
    assert ps.stream == start + 5 == 2 ** 32 + 3
    assert_words(expand(product, want[0], 5, E.L, seed_at(start)), want[1], "expanded")
    # ... and the last two alone, from the seed value in between
    assert_words(expand(product, want[0][3:], 2, E.L, seed_at(start + 3)), want[1][3:], "expanded tail")
    E.rng_continued(16, E.L)
    E.close()


@pytest.mark.parametrize("env", [{"GPQHE_CHUNK": "5"}, {"GPQHE_WS_MIB": "1"}])
def test_chunks_do_not_change_bits(oracle, product, env, monkeypatch):
    """17 ciphertexts as 5/5/5/2 (GPQHE_CHUNK) or under a 1 MiB workspace."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E = SeededEnds(oracle, product, "f13")
    zs, want = encryptions(E, ("f13", 64, None, 17))
    E.both(zs, 64, E.L, want)
    E.close()


def test_empty_batch_and_zero_vectors(oracle, product):
    E = SeededEnds(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 2, 4)
    # count = 0: nothing written, no stream of either kind taken
    ps = seed_at()
    assert (E.enc_seeded(zs, slots, lvl, ps, count=0) == FILL).all()
    assert bytes(ps) == bytes(seed_at())
    assert (expand(product, np.zeros((2, lvl * E.n), dtype=np.uint64), 0, lvl, ps) == FILL).all()
    E.rng_continued(slots, lvl)
    # an all-zero batch: ciphertexts like any other
    zero = [np.zeros(slots, dtype=np.complex128)] * 3
    want = E.oracle_seeded(zero, slots, lvl)
    x = E.both(zero, slots, lvl, want)
    assert x.reshape(3, 2, -1).any(axis=2).all()
    zd = E.dec_batch(x, lvl, slots)
    assert np.array_equal(bits(zd), bits(E.oracle_dec(want[2], lvl, slots)))  # the plain he_enc_sk decode
    assert np.abs(zd).max() < 1e-6
    E.close()


@pytest.mark.parametrize("name,S,s,width", [("ref", 64, 16, 3), ("f13", 4096, 16, 2)])
def test_packed_form_equals_the_reference(oracle, product, name, S, s, width):
    """At width = s and at a width below it, against the oracle on the interleaved vectors."""
    E = SeededEnds(oracle, product, name, S)
    P, lvl = S // s, product.L
    full, part = loops(P, s, 2, S), loops(P, width, 2, S + 1)
    want = enc_sk_seeded_packed_words(oracle, full + part, E.ko[1], E.scale, lvl, PUBKEY, PUBSTREAM)
    ps = seed_at()
    c0 = np.concatenate([E.enc_seeded_packed(full, s, s, lvl, ps), E.enc_seeded_packed(part, s, width, lvl, ps)])
    assert_words(c0, want[0], "c0")
    assert ps.stream == PUBSTREAM + 4
    x = expand(product, c0, 4, lvl, seed_at())
    assert_words(x, want[1], "expanded")
    E.rng_continued(S, lvl)
    z = E.dec_batch(x, lvl, S)
    assert np.array_equal(bits(z), bits(E.oracle_dec(want[2], lvl, S)))
    for i, v in enumerate(full + part):
        assert np.abs(z[i] - interleave(v, S)).max() < 1e-6
    E.close()


def gains_with_a_zero_diagonal(P, rows, s):
    M, mp = matrices(P, rows, s)[0], pow2(rows)
    for k in range(s):
        if k % mp < rows:
            M[:, k % mp, (k + 1) % s] = 0
    return M


def test_gain_form_equals_the_reference(oracle, product):
    """ref 64/16, rows 3 (m' = 4) with E_1 zero in every loop, still a full
    ciphertext; nmat 1 and P on one running seed."""
    S, s, rows = 64, 16, 3
    E = SeededEnds(oracle, product, "ref", S)
    lvl, P, mp = product.L, S // s, pow2(rows)
    w = lvl * E.n
    M = gains_with_a_zero_diagonal(P, rows, s)
    ps = seed_at()
    for nmat, Mn in ((1, M[:1]), (P, M)):
        assert not gain_diagonals(Mn, S, s, rows, nmat)[1].any()
        start = ps.stream
        oc = enc_gain_sk_seeded_compose(oracle, Mn, E.ko[1], s, rows, nmat, lvl, PUBKEY, start)
        want = np.stack([oracle.export(c).ravel() for c in oc])
        for c in oc:
            oracle.free(c)
        d = dev(mp * w)
        product.enc_gain_sk_seeded_packed_batch(d.data_ptr(), Mn, E.kp[1], s, rows, lvl, ps, nmat)
        product.sync()
        assert ps.stream == start + mp
        got = words_of(d, mp * w).reshape(mp, w)
        assert_words(got, want[:, :w], f"nmat {nmat}: c0")
        assert got.any(axis=1).all()
        assert_words(expand(product, got, mp, lvl, seed_at(start)), want, f"nmat {nmat}: expanded")
    E.rng_continued(S, lvl)
    E.close()


def test_expansion_without_the_secret_key(oracle, product):
    """The two machines' shape: c0 and the 40-byte seed are all that reaches a
    second context, equal in its parameters, that never held the key; the
    first key re-imported afterwards decodes the expanded ciphertexts double
    for double like the oracle's plain he_enc_sk ones."""
    E = SeededEnds(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs, want = encryptions(E, ("f13", 64, None, 3))
    c0 = E.enc_seeded(zs, slots, lvl, seed_at())
    assert_words(c0, want[0], "c0")
    skw, sk_nl, sk_scale, sk_flags = product.export(E.kp[1]), E.kp[1].nlimbs, E.kp[1].scale, E.kp[1].flags
    want_z = E.oracle_dec(want[2], lvl, slots)
    for o in E.kp:
        product.free(o)
    product.exit()
    product.init_params(**PARAMS["f13"][1])  # no seed, no key pair
    x = expand(product, c0, 3, lvl, seed_at())
    assert_words(x, want[1], "expanded")
    sk = product.sk()
    product.import_(sk, skw, sk_nl, sk_scale, sk_flags)
    E.kp = (product.pk(), sk)
    z = E.dec_batch(x, lvl, slots)
    assert np.array_equal(bits(z), bits(want_z))
    assert np.abs(z - np.stack(zs)).max() < 1e-6
    E.close()


def packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, seed, ps):
    """4 cnt loop sets through he_enc_sk_seeded_packed_batch and
    he_expand_seeded_batch into one device array (blocks xhat, xr, uhat, ur):
    (vectors, the array, the oracle's expanded words [4][cnt][W])."""
    w = level * product.n
    zs = loops(S // s, width, 4 * cnt, seed)
    before = copy_of(ps)
    c0, x = dev(4 * cnt * w), dev(4 * cnt * 2 * w)
    product.enc_sk_seeded_packed_batch(c0.data_ptr(), np.stack(zs), pr.P.sk, s, width, scale, level, ps)
    product.expand_seeded_batch(x.data_ptr(), c0.data_ptr(), 4 * cnt, level, before)
    product.sync()
    want = enc_sk_seeded_packed_words(oracle, zs, pr.O.sk, scale, level, PUBKEY, before.stream)
    assert_words(words_of(c0, 4 * cnt * w).reshape(4 * cnt, w), want[0], "c0 words")
    assert_words(words_of(x, 4 * cnt * 2 * w).reshape(4 * cnt, 2 * w), want[1], "input words")
    return zs, x, want[1].reshape(4, cnt, 2 * w)


@pytest.mark.parametrize("name,S,s,level,cnt", [("ref", 64, 16, 2, 2), ("f13", 4096, 16, 6, 1)])
def test_pipeline_packed_step(oracle, product, name, S, s, level, cnt):
    """seeded packed encrypt -> expand -> he_hempc_step_packed_batch -> he_dec_dcd_packed_batch."""
    rows, width, P = 2, 3, S // s
    pr = PackedPair(oracle, product, name, S, s, rows)
    scale = product.info.delta
    Ma, Mb = matrices(P, rows, s)
    zs, x, H = packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, S + 3, seed_at())
    cw, ow = 2 * level * product.n, 2 * (level - 1) * product.n
    up = dev(cnt * ow)
    ptr = [x.data_ptr() + 8 * b * cnt * cw for b in range(4)]
    product.hempc_step_packed_batch(up.data_ptr(), Ma, Mb, *ptr, cnt, level, pr.P.rk, s, rows, P)
    product.sync()
    want_up = pr.reference(("seeded packed", name, S, cnt),
                           lambda e, c, rk, r: step_packed_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, s, r, P),
                           H, level, scale)
    assert_words(words_of(x, 4 * cnt * cw), H.ravel(), "inputs after the step")
    check_step_output(pr, oracle, product, up, want_up, zs, Ma, Mb, S, s, rows, level, cnt, scale)
    pr.close()


def test_pipeline_encgain_step(oracle, product):
    """The same through he_hempc_step_encgain_packed_batch with the gains from
    he_enc_gain_sk_seeded_packed_batch, ref S = 64, all on one running seed."""
    name, S, s, rows, width, level, cnt = "ref", 64, 16, 2, 3, 2, 2
    P, mp = S // s, pow2(rows)
    pr = GainPair(oracle, product, name, S, s, rows)
    scale = product.info.delta
    w, cw, ow = level * product.n, 2 * level * product.n, 2 * (level - 1) * product.n
    Ma, Mb = matrices(P, rows, s)
    ps = seed_at()
    D0, D = dev(2 * mp * w), dev(2 * mp * cw)
    DA, DB = D.data_ptr(), D.data_ptr() + 8 * mp * cw
    product.enc_gain_sk_seeded_packed_batch(D0.data_ptr(), Ma, pr.P.sk, s, rows, level, ps, P)
    product.enc_gain_sk_seeded_packed_batch(D0.data_ptr() + 8 * mp * w, Mb, pr.P.sk, s, rows, level, ps, P)
    assert ps.stream == PUBSTREAM + 2 * mp
    product.expand_seeded_batch(DA, D0.data_ptr(), 2 * mp, level, seed_at())  # both sets: consecutive streams
    product.sync()
    oa = enc_gain_sk_seeded_compose(oracle, Ma, pr.O.sk, s, rows, P, level, PUBKEY, PUBSTREAM)
    ob = enc_gain_sk_seeded_compose(oracle, Mb, pr.O.sk, s, rows, P, level, PUBKEY, PUBSTREAM + mp)
    pr.oD += oa + ob
    want_d = np.stack([oracle.export(c).ravel() for c in oa + ob])
    assert_words(words_of(D0, 2 * mp * w).reshape(2 * mp, w), want_d[:, :w], "gain c0 words")
    assert_words(words_of(D, 2 * mp * cw).reshape(2 * mp, cw), want_d, "gain words")
    zs, x, H = packed_inputs(pr, oracle, product, S, s, width, level, cnt, scale, S + 4, ps)
    assert ps.stream == PUBSTREAM + 2 * mp + 4 * cnt
    up = dev(cnt * ow)
    ptr = [x.data_ptr() + 8 * b * cnt * cw for b in range(4)]
    product.hempc_step_encgain_packed_batch(up.data_ptr(), DA, DB, *ptr, cnt, level, pr.P.rk, pr.P.rlk, s, rows)
    product.sync()
    want_up = pr.reference(
        ("seeded encgain", name, S, cnt),
        lambda e, c, rk, r: step_encgain_compose(e, oa, ob, c[0], c[1], c[2], c[3], rk, pr.O.rlk, s, r), H, level,
        scale)
    assert_words(words_of(D, 2 * mp * cw).reshape(2 * mp, cw), want_d, "gains after the step")
    check_step_output(pr, oracle, product, up, want_up, zs, Ma, Mb, S, s, rows, level, cnt, scale)
    pr.close()


def closed_loop(oracle, reg, ref_class, problems, bound, what, streams):
    """simulate_batch through reg; every step's u within bound(|plain u|) of
    regulator_plain on that step's inputs; the first three steps' u bit for bit
    the seeded reference loop's on the oracle for the same inputs; the public
    seed advanced by `streams`."""
    assert (reg.P, reg.count, reg.nmat, reg.sym) == (4, 2, 4, "seeded")
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
    print(f"closed loop, {what}, seeded secret-key encryptions: worst |u - plain| {worst[0]:.3e}")
    assert len(reg.timings) == 40 and x.shape == (6, 41, 3) and u.shape == (6, 40, 2)
    assert all(not np.array_equal(u[0], u[i]) for i in range(1, 6))
    assert reg.ps.stream == PUBSTREAM + streams and bytes(reg.ps)[:32] == PUBKEY
    reg.close()
    ref = ref_class(oracle, problems, 64, 2024, PUBKEY, PUBSTREAM)
    for xhat, uhat, xr, ur, got in first:
        assert np.array_equal(ref(xhat, uhat, xr, ur), got)
    ref.close()


def test_closed_loop_packed_seeded(oracle, product):
    """Six CstrProblem(40) through PackedEncryptedRegulator(sym="seeded") on S =
    64: within 1e-8 max(1, |u|) of regulator_plain, the bound of the public-key
    and secret-key loops; 8 public streams a step."""
    problems = six_plants()
    reg = cstr.PackedEncryptedRegulator(product, problems, 64, rows=problems[0].nu, seed=2024, sym="seeded",
                                        pubseed=seed_at())
    closed_loop(oracle, reg, RefSeededPackedRegulator, problems, lambda w: 1e-8 * max(1.0, w), "plain gains", 40 * 8)


def test_closed_loop_encrypted_gains_seeded(oracle, product):
    """... through EncryptedGainRegulator(sym="seeded"): within min(1.15e-8, 1e-6
    max(1, |u|)), the bound of the public-key and secret-key loops; 2 m' public
    streams for the gains first."""
    problems = six_plants()
    reg = cstr.EncryptedGainRegulator(product, problems, 64, rows=problems[0].nu, seed=2024, sym="seeded",
                                      pubseed=seed_at())
    assert reg.mp == 2
    closed_loop(oracle, reg, RefSeededGainRegulator, problems,
                lambda w: min(100 * ORACLE_LOOP_WORST, 1e-6 * max(1.0, w)), "encrypted gains", 4 + 40 * 8)


def test_state(oracle, product):
    """A repeat call; seeded, sk and pk batch calls interleaved on one context
    and one running seed, each against the oracle in that order; another
    parameter set after hectx_exit."""
    E = SeededEnds(oracle, product, "f13")
    slots, lvl = 64, E.L
    zs = vectors(slots, 3, 11)
    ps = seed_at()
    for kind in ("seeded", "seeded", "sk", "seeded", "pk", "seeded"):
        if kind == "seeded":
            start = ps.stream
            want = E.oracle_seeded(zs, slots, lvl, start)
            c0 = E.enc_seeded(zs, slots, lvl, ps)
            assert_words(c0, want[0], kind)
            assert_words(expand(product, c0, 3, lvl, seed_at(start)), want[1], "expanded")
        elif kind == "sk":
            assert_words(E.enc_sk_batch(zs, slots, lvl), E.oracle_enc_sk(zs, slots, lvl), kind)
        else:
            assert_words(E.enc_batch(zs, slots, lvl), E.oracle_enc(zs, slots, lvl), kind)
    assert ps.stream == PUBSTREAM + 12
    E.rng_continued(slots, lvl)
    E.close()
    for e in (oracle, product):
        e.exit()
    E = SeededEnds(oracle, product, "ref")
    zs = vectors(16, 3, 12)
    E.both(zs, 16, E.L, E.oracle_seeded(zs, 16, E.L, ps.stream), ps.stream)
    E.rng_continued(16, E.L)
    E.close()


def test_kernel_classes_are_reported(oracle, product):
    E = SeededEnds(oracle, product, "f13")
    n, lvl, cnt = E.n, E.L, 3
    product.prof_enable(True)
    try:
        product.prof_collect()
        c0 = E.enc_seeded(vectors(64, cnt, 1), 64, lvl, seed_at())
        enc = product.prof_collect()
        expand(product, c0, cnt, lvl, seed_at())
        exp = product.prof_collect()
    finally:
        product.prof_enable(False)
    # the noise alone, the in-place combine (a word read, a word written, the key words once), no c1 anywhere
    assert enc["enc_sk_sample_batch_kernel"][0] == 1
    assert enc["enc_sk_sample_batch_kernel"][2] == 8.0 * n * lvl * cnt + 16.0 * 64 * cnt
    assert enc["enc_sk_seeded_combine_kernel"][0] == 1
    assert enc["enc_sk_seeded_combine_kernel"][2] == 8.0 * n * lvl * (2 * cnt + 1)
    assert not {"enc_sk_combine_batch_kernel", "seeded_expand_kernel", "enc_sample_batch_kernel"} & set(enc)
    assert set(exp) == {"seeded_expand_kernel"}
    assert exp["seeded_expand_kernel"][0] == 1 and exp["seeded_expand_kernel"][2] == 8.0 * n * lvl * 3 * cnt
    E.close()


def test_teardown_clean_exit():
    """The four calls, hectx_exit, a second context, the calls again, exit: rc 0."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seeded_batch_worker.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rc {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert res == {"first": True, "second": True, "streams": 32}, res
