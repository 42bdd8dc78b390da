"""The batch kernels (BSGS product, step, row-folded and packed steps, encrypted
gains, batch encrypt / decode ends, secret-key and seeded ends) on constructed
residues at the edges of the canonical range and under crafted keys
(tests/extreme_inputs.py): product vs oracle, bit for bit, on every output
word, every decoded double's bit pattern and the guard words.

Those kernels are correct by bound arguments written in their comments; the
encryptions, sampled keys and random matrices of their own tests are uniform
residues, far inside every bound.  Every batch entry point takes raw device
words, so the words the bounds speak of -- 0, 1, q - 1, +-(q - 1)/2 -- go in
directly, and three constructions (pinned to exact integers by
tests/test_extremes_batch_cpu.py) carry them through the rotations:
* the identity switching key (X.identity_key): a rotation is the index
  permutation of both polynomials, so a constant ciphertext stays what it is
  and the kernels behind the rotations see exactly the words placed;
* the constant diagonals -1 / q_top and +1 / q_top at the products' own scale
  q_top: the words q - 1 and 1 on every limb;
* constant polynomials under a constant secret key for the decoder's lift.
The oracle side is always the reference composition (tests/*_ref.py) on the
oracle, never another product call.  Only the rand_* patterns and the sampled
matrix are drawn, from fixed seeds.  Nothing above n = 2^14.
"""
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

from tests import extreme_inputs as X
from tests.bsgs_ref import bsgs_compose, bsgs_rotations
from tests.encgain_ref import gemv2_encgain_compose, step_encgain_compose
from tests.packed_ref import (deinterleave, gemv2_packed_compose, interleave, packed_rotations,
                              step_packed_compose)
from tests.rows_ref import gemv2_rows_compose, pow2, rows_rotations, step_rows_compose
from tests.sk_ref import enc_sk_packed_words
from tests.seeded_ref import enc_sk_seeded_packed_words
from tests.step_ref import gemv2_compose, step_compose
from tests.test_gpu_encgain_batch import GainPair
from tests.test_gpu_io_batch import bits, vectors
from tests.test_gpu_packed_batch import PackedPair, loops
from tests.test_gpu_rotations import sample_matrix
from tests.test_gpu_rows_batch import RowsPair
from tests.test_gpu_seeded_batch import PUBKEY, PUBSTREAM, SeededEnds, expand, seed_at
from tests.test_gpu_sk_batch import SkEnds, assert_words, dev, words_of
from tests.test_gpu_step_batch import StepPair

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "hectr_amd" / "csrc"


def constant(fname, name):
    """The integer a kernel source gives `name` (#define or constexpr)."""
    text = (CSRC / fname).read_text()
    m = re.search(r"(?:#define\s+%s\s+|\b%s\s*=\s*)(\d+)" % (name, name), text)
    assert m, (fname, name)
    return int(m.group(1))


def test_counts_leave_a_partial_last_group():
    """The counts below against the kernels' ciphertext group sizes, read
    from the sources: each leaves a partial last group (and a full one)."""
    assert 3 > constant("bsgs.hip", "BSGS_BATCH_CB") and 3 % constant("bsgs.hip", "BSGS_BATCH_CB")
    for nm in ("EG_CG_F64", "EG_CG_INT"):
        assert 5 > constant("encgain_batch.hip", nm) and 5 % constant("encgain_batch.hip", nm)
    assert 5 > constant("kernels.hip", "FOLD_CG") and 5 % constant("kernels.hip", "FOLD_CG")
    assert 9 > constant("gpqhe_internal.h", "IOB_CG") and 9 % constant("gpqhe_internal.h", "IOB_CG")
    assert constant("kernels.hip", "FOLD_TPB") == 256  # T = n / 2 slots on both sides of it below


def reference(pr, compose, H, lvl, scale):
    """compose(oracle, [the ciphertext of every block], rk, pr.g) for every
    ciphertext column of H [blocks][cnt][2 lvl n], identical columns computed
    once: the oracle's words [cnt][2 (lvl - 1) n]."""
    done, rows = {}, []
    for c in range(H.shape[1]):
        key = hashlib.sha1(np.ascontiguousarray(H[:, c]).tobytes()).digest()
        if key not in done:
            cts = []
            for b in range(H.shape[0]):
                x = pr.o.ct()
                pr.o.import_(x, H[b, c], lvl, scale=scale)
                cts.append(x)
            y = compose(pr.o, cts, pr.O.rk, pr.g)
            assert y.nlimbs == lvl - 1 and np.isclose(y.scale, scale, rtol=1e-12)
            done[key] = pr.o.export(y).ravel().copy()
            for x in cts + [y]:
                pr.o.free(x)
        rows.append(done[key])
    return np.stack(rows)


# ============================================================ a. decode end
SK_KINDS = ("one", "qm1", "half_lo", "rand_half", "genuine")
DEC_SPECS = [("qm1", "qm1"), ("half_lo", "half_hi"), ("rand_half", "rand_half"), ("rand_edge", "rand_edge"),
             ("mixed3", "mixed3")]


def place(holder, tag, pairs, payload):
    """Import payload [npoly][nlimbs][n] into the object of every (engine,
    object) pair, the same object on each engine; payload None: the words the
    object was generated with, which the first call for `tag` saves on holder
    (so every call for it goes through here).  Returns the words in place."""
    saved = holder.__dict__.setdefault("_generated", {})
    if tag not in saved:
        gen = [e.export(o).copy() for e, o in pairs]
        assert all(np.array_equal(g, gen[0]) for g in gen), f"{tag}: the engines generated different keys"
        assert gen[0].any()
        saved[tag] = gen[0]
    w = saved[tag] if payload is None else np.asarray(payload, dtype=np.uint64).reshape(saved[tag].shape)
    for e, o in pairs:
        e.import_(o, w, o.nlimbs, o.scale, o.flags)
        assert np.array_equal(e.export(o), w), f"{tag}: the payload is not in place"
    return w


def craft_sk(E, kind):
    """kind on every limb of both engines' secret key ("genuine": the
    generated words again); the words [L + K][n]."""
    sk = E.kp[1]
    w = None if kind == "genuine" else X.poly([kind] * sk.nlimbs, E.p.primes[:sk.nlimbs], E.n, seed=41)[None]
    w = place(E, "sk", [(E.o, E.ko[1]), (E.p, E.kp[1])], w)[0]
    if kind == "genuine":  # the ternary key: more than two values, unlike every crafted kind
        assert len(np.unique(w[0])) > 2
    return w


def prod(v):
    out = 1
    for x in v:
        out *= int(x)
    return out


def decode_inputs(E, lvl, slots, kind, s_words):
    """(words [cnt][2 lvl n], {index: X}): the ciphertexts of the decode tests
    under the secret key s_words, and the lift value X of those that decrypt
    to the constant polynomial X."""
    o, n = E.o, E.n
    primes = E.p.primes[:lvl]
    Q = prod(primes)
    q = np.array(primes, dtype=object).reshape(lvl, 1)
    cts, lifts = [], {}
    edges = X.lift_edges(primes)
    if kind in ("one", "qm1"):  # c0 + c1 s = X exactly, all three constant polynomials
        for v in edges.values():
            if kind == "one":
                c0, c1 = (v - (Q - 1)) % Q, Q - 1
            else:
                c0 = (Q - 1) // 2
                c1 = (c0 - v) % Q
            lifts[len(cts)] = v
            cts.append(np.stack([X.const_words(c0, primes, n), X.const_words(c1, primes, n)]))
    # the decoded coefficients j T, j < 2 slots, each an edge value; c1 a +-(q - 1)/2 mix
    T, vals = n // (2 * slots), list(edges.values())
    D = np.zeros((lvl, n), dtype=np.uint64)
    for j in range(2 * slots):
        for i, p in enumerate(primes):
            D[i, j * T] = vals[j % len(vals)] % int(p)
    c1 = X.poly(["rand_half"] * lvl, primes, n, seed=9)
    Y = X.pullback(o, D, lvl).astype(object)
    c0 = ((Y - c1.astype(object) * s_words[:lvl].astype(object)) % q).astype(np.uint64)
    cts.append(np.stack([c0, c1]))
    for i, (a, b) in enumerate(DEC_SPECS):
        cts.append(np.stack([X.spec_ct(o, a, primes, n, seed=i)[0], X.spec_ct(o, b, primes, n, seed=i + 50)[1]]))
    k = 0
    while len(cts) % 4 == 0 or len(cts) % 8 == 0 or len(cts) < 9:  # a partial last group of FOLD_CG and of IOB_CG
        cts.append(X.spec_ct(o, f"pb:mixed{k}", primes, n))
        k += 1
    return np.stack(cts).reshape(len(cts), -1), lifts


# set, slots, level (None: top): T = n / 2 slots, the path
DECODE = [
    ("ref", 16, None),    # T = 128 < FOLD_TPB; 60-bit q0: the Barrett fold beside the FP64 one
    ("ref", 8, 1),        # T = 256; one limb: the lift's nl = 1 branch
    ("f13", 16, None),    # T = 256 >= FOLD_TPB: a block a workgroup; all-FP64 fold, six limbs
    ("f13", 64, None),    # T = 64: four blocks a workgroup, the LDS tree over segments
    ("f13", 2048, None),  # the largest folding slot count, T = 2
    ("f13", 4096, None),  # T = 1: no fold; the multi-launch decoder above GPQHE_DCD_ONEPASS
    ("c1", 64, None),     # 60-bit q0 beside 50-bit limbs: reduce64 of a 60-bit Garner digit
    ("i14", 16, None),    # T = 512: two words a thread; 61-bit q0
    ("i14", 64, 2),       # T = 128; two limbs: Q below 2^128
]


@pytest.mark.parametrize("name,slots,nl", DECODE)
def test_decode_at_the_lift_edges_under_crafted_sk(oracle, product, name, slots, nl, monkeypatch):
    """he_dec_dcd_batch with GPQHE_DCD_FOLD = 1 and 0 against the oracle's
    he_dec + he_dcd_ex, every double's bits, under each SK_KINDS secret key.
    Placed exactly: every word of c0, c1 and s.  Under sk = 1 and -1 one
    ciphertext per X.lift_edges value decrypts to the constant polynomial X,
    and every slot must also equal horner_double(X) / scale with imaginary part
    0: dcd_crt_center's Garner digits (kernels.hip:1354-1367: reduce64 of a
    60/61-bit digit against a 48/50-bit modulus at Q_k - 1, digits 0 and 1 at
    q_0 .. q_k), the Horner carries "hi += lo < cv" (1382-1393), the "2 val > Q"
    comparison at (Q +- 1)/2 and floor/ceil(Q/2) -+ 2^64 (1397-1409), the
    borrow chain "(Q[w] < val[w]) | (d < b)" (1410-1418; Q - 2^(64 j) + 1 sends a
    borrow through words equal to Q's, which a uniform coefficient does with
    probability 2^-64) and the conversion to double (1419-1423).  One
    pulled-back ciphertext holds a different edge value at every decoded
    coefficient j T under every key.  FoldMul<true>'s "one correction each
    way" (kernels.hip:4424-4442) and the add_mod chains and LDS tree of
    dec_fold_kernel (4463-4485) and dec_batch_kernel's c0 + c1 s get q - 1 x
    q - 1, +-(q - 1)/2 products and q - 1 + q - 1 from the DEC_SPECS patterns
    under the qm1 / half_lo / rand_half keys.  The FFT behind the lift is a
    smoke case except on the constant polynomials, where it only adds zeros."""
    E = SkEnds(oracle, product, name)
    lvl = nl or E.L
    for kind in SK_KINDS if slots <= 2048 else ("one", "qm1", "rand_half"):  # (8192 lifts a ciphertext at 4096)
        s_words = craft_sk(E, kind)
        words, lifts = decode_inputs(E, lvl, slots, kind, s_words)
        assert len(words) % 4 and len(words) % 8
        want = E.dec_check(words, lvl, slots, monkeypatch)
        for i, v in lifts.items():
            d = np.float64(X.horner_double(v, E.p.primes[:lvl])) / np.float64(E.scale)
            assert np.all(bits(want[i].real) == bits(d)) and not bits(want[i].imag).any(), (kind, i, v)
    E.close()


@pytest.mark.parametrize("name,S,s,rows", [("ref", 64, 16, 3), ("f13", 4096, 16, 2)])
def test_packed_decode_at_the_lift_edges(oracle, product, name, S, s, rows, monkeypatch):
    """he_dec_dcd_packed_batch (S = 64: the folded decoder's packed store;
    S = 4096 above GPQHE_DCD_ONEPASS: the multi-launch decoder and the packed
    gather) on the same ciphertexts under sk = -1 and a +-(q - 1)/2 key: the
    first `rows` entries of every loop of the oracle's decode, bit for bit."""
    import torch
    E = SkEnds(oracle, product, name, S)
    lvl, P = E.L, S // s
    for kind in ("qm1", "rand_half"):
        s_words = craft_sk(E, kind)
        words, _ = decode_inputs(E, lvl, S, kind, s_words)
        full = E.oracle_dec(words, lvl, S)
        want = np.stack([deinterleave(z, P, rows) for z in full])
        din = torch.from_numpy(words.ravel().view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        for fold in ("1", "0"):
            monkeypatch.setenv("GPQHE_DCD_FOLD", fold)
            got = product.dec_dcd_packed_batch(din.data_ptr(), len(words), lvl, E.scale, E.kp[1], s, rows)
            bad = np.argwhere(bits(got) != bits(want))
            assert bad.size == 0, f"{kind}, GPQHE_DCD_FOLD={fold}: {len(bad)} doubles differ, first at {bad[0].tolist()}"
        monkeypatch.delenv("GPQHE_DCD_FOLD")
        assert np.array_equal(din.cpu().numpy().view(np.uint64), words.ravel()), "input written"
    E.close()


# ========================================================== b. encrypt ends
@pytest.mark.parametrize("name", ["ref", "f13", "c1"])
def test_encrypt_ends_under_crafted_keys(oracle, product, name):
    """he_enc_pk_batch, he_enc_sk_batch, he_enc_sk_seeded_batch +
    he_expand_seeded_batch (9 ciphertexts: a full and a partial group of
    IOB_CG) and the packed form of each (3), at the top level and at level 1, under a
    public key whose two polynomials are each key kind and a secret key of the
    same kind, imported over generated ones on both engines.  Both engines draw
    from one seed: every word must agree and the RNG end where the oracle's
    does (rng_continued).  Placed exactly: the key words that
    enc_combine_batch_kernel (pk v + e + m), the sk_batch.hip / seeded_batch.hip
    combines ("e - p is one below 2.25 q < 2^53") multiply the samples by --
    q - 1 and +-(q - 1)/2 against uniform a and small v, e; the samples
    themselves are the RNG's."""
    S, s, width, cnt = 64, 16, 3, 9
    E = SeededEnds(oracle, product, name, S)
    P = S // s
    zs, zp = vectors(S, cnt, 3), loops(P, width, 3, 5)
    for k, kind in enumerate(SK_KINDS):
        craft_sk(E, kind)
        w = None if kind == "genuine" else np.stack([X.poly([kind] * E.L, E.p.primes[:E.L], E.n, seed=60 + p)
                                                     for p in range(2)])
        w = place(E, "pk", [(E.o, E.ko[0]), (E.p, E.kp[0])], w)
        assert kind != "genuine" or len(np.unique(w[0, 0])) > 3  # uniform words
        for e in (E.o, E.p):
            e.set_seed(500 + k)
        for lvl in (E.L, 1):
            what = f"key {kind}, level {lvl}"
            assert_words(E.enc_batch(zs, S, lvl), E.oracle_enc(zs, S, lvl), what + ": enc_pk")
            assert_words(E.enc_sk_batch(zs, S, lvl), E.oracle_enc_sk(zs, S, lvl), what + ": enc_sk")
            E.both(zs, S, lvl, E.oracle_seeded(zs, S, lvl))
        lvl = E.L
        # the packed forms, on the interleaved vectors
        cw = 2 * lvl * E.n
        d = dev(len(zp) * cw)
        product.enc_pk_packed_batch(d.data_ptr(), np.stack(zp), E.kp[0], s, width, E.scale, lvl)
        product.sync()
        assert_words(words_of(d, len(zp) * cw).reshape(len(zp), cw),
                     E.oracle_enc([interleave(z, S) for z in zp], S, lvl), f"key {kind}: enc_pk_packed")
        assert_words(E.enc_sk_packed(zp, s, width, lvl), enc_sk_packed_words(oracle, zp, E.ko[1], E.scale, lvl),
                     f"key {kind}: enc_sk_packed")
        want = enc_sk_seeded_packed_words(oracle, zp, E.ko[1], E.scale, lvl, PUBKEY, PUBSTREAM)
        c0 = E.enc_seeded_packed(zp, s, width, lvl, seed_at())
        assert_words(c0, want[0], f"key {kind}: seeded packed c0")
        assert_words(expand(product, c0, len(zp), lvl, seed_at()), want[1], f"key {kind}: seeded packed expanded")
        E.rng_continued(S, lvl)
    E.close()


# ================================== c. BSGS batch product and the step
def payload_for(e, kind, evk):
    return X.key_payload(kind, e.primes, e.n, evk.npoly // 2, seed=3, L=e.L)


def craft_key(pr, tag, ko, kp, kind):
    """One switching key on both engines: the payload of `kind`, or
    ("genuine") the words it was generated with."""
    assert ko.nlimbs == kp.nlimbs == pr.p.L + pr.p.K and ko.npoly == kp.npoly
    w = place(pr, tag, [(pr.o, ko), (pr.p, kp)], payload_for(pr.p, kind, kp))
    if kind == "genuine":  # uniform words: neither the zero nor the identity nor a pattern key
        assert len(np.unique(w[0, 0])) > 3 and len(np.unique(w[1, 0])) > 3


def craft_rot_keys(pr, kind, rots):
    """Overwrite the rotation keys `rots` on both engines."""
    for r in rots:
        assert pr.P.rk[r].galois == pr.O.rk[r].galois == pow(5, r, 2 * pr.p.n)
        craft_key(pr, ("rk", r), pr.O.rk[r], pr.P.rk[r], kind)


def ct_words(oracle, specs, primes, n, seed=0):
    """[len(specs)][2 lvl n]; a spec "a|b": polynomial 0 from a, 1 from b."""
    out = []
    for i, sp in enumerate(specs, seed):
        a, b = sp.split("|") if "|" in sp else (sp, sp)
        out.append(np.stack([X.spec_ct(oracle, a, primes, n, seed=i)[0], X.spec_ct(oracle, b, primes, n, seed=i)[1]]))
    return np.stack(out).reshape(len(specs), -1)


#: the input ciphertexts of the products: constant q - 1 on both polynomials, one, pulled-back q - 1, +-(q - 1)/2, mixed
GEMV_CTS = ["qm1", "one", "pb:qm1", "rand_half", "mixed3"]
#: the step's (xhat, xr, uhat, ur) per ciphertext.  Differences: 0 - (q - 1) (A, B), equal operands (C and the
#: u pairs), (q - 1) - 0 (D).  Under the identity key and the matrix -1 / q_top, xd = 1 gives the sum -slots, which
#: rescales to w = q - 1 on every limb: the tail sees uhat - w with w = uhat (A: up = 0), 0 - (q - 1) (B), and
#: w = 0 from xd = ud = 0 (C); D and E are a smoke case of it.
STEP_CTS = {"A": ("zero", "qm1", "qm1", "qm1"), "B": ("zero", "qm1", "zero", "zero"), "C": ("qm1", "qm1", "one", "one"),
            "D": ("qm1", "zero", "rand_half", "rand_edge"), "E": ("mixed3", "pb:rand_half", "mixed5", "half_hi")}


def step_blocks(oracle, primes, n, names):
    """[4][len(names)][2 lvl n]"""
    return np.stack([ct_words(oracle, [STEP_CTS[c][b] for c in names], primes, n) for b in range(4)])


def const_matrices(s, q_top):
    return {"neg": X.const_diag_matrix(s, -1.0 / q_top), "pos": X.const_diag_matrix(s, 1.0 / q_top),
            "alt": X.circulant(s, [0.5, -0.5]), "sample": sample_matrix(s, 9)}


#: the matrices each rotation-key kind runs with
BSGS_PLAN = {"genuine": ("sample",), "zero": ("neg",), "identity": ("neg", "pos", "alt"), "one": ("alt",),
             "qm1": ("neg",), "half_lo": ("alt",), "rand_half": ("sample",), "digit0": ("pos",)}

# set, slots, g, GPQHE_BSGS_INNER_TB, key kinds (None: all), matrices (None: all of BSGS_PLAN's)
BSGS = [
    ("ref", 16, 4, None, None, None),     # the generic rotations; two tiles of 8 in the step (TB 8 form)
    ("ref", 64, 16, None, None, None),    # a full tile of 16 baby slots
    ("ref", 64, 32, None, ("identity", "qm1", "rand_half"), None),  # two tiles: the add-to-own-words path
    ("f13", 64, 16, None, ("identity", "zero", "genuine"), ("neg", "sample")),  # all-FP64, windowed rotations
    ("f13", 64, 32, None, ("identity", "qm1"), ("neg", "alt")),
    ("i14", 64, 16, None, ("identity",), None),  # 61-bit q0: the stated maximum 16 (q - 1)^2 (see the docstring)
    ("i14", 64, 16, None, ("qm1", "genuine"), None),
    ("i14", 64, 16, None, ("zero", "half_lo"), None),
    ("i14", 64, 16, None, ("rand_half", "digit0"), None),
    ("i14", 64, 16, "8", ("identity",), ("neg", "alt")),  # the tile of 8: two of them a giant step
    ("i14", 64, 32, None, ("identity",), ("neg", "alt")),
]


@pytest.mark.parametrize("name,slots,g,tb,kinds,only", BSGS, ids=[
    "ref-16-g4", "ref-64-g16", "ref-64-g32", "f13-64-g16", "f13-64-g32", "i14-64-g16-identity-max-16(q-1)^2",
    "i14-64-g16-qm1-genuine", "i14-64-g16-zero-half_lo", "i14-64-g16-rand_half-digit0", "i14-64-g16-tb8", "i14-64-g32"])
def test_bsgs_batch_and_step_on_patterns_under_crafted_keys(oracle, product, name, slots, g, tb, kinds, only,
                                                            monkeypatch):
    """he_gemv_bsgs_batch (3 pattern ciphertexts), he_hempc_step_batch (3
    STEP_CTS) and, under the identity key, he_gemv2_bsgs_batch, with the BSGS
    rotation keys generated and then overwritten by each key kind
    (BSGS_PLAN pairs the kinds with the matrices), against bsgs_compose /
    step_compose / gemv2_compose on the oracle.
    Aimed at bsgs_inner_batch_kernel's 128-bit tile sums and bsgs_red128,
    "(hi : lo) mod q for hi < 2^62: what a sum of 16 products of residues
    below 2^61 fits" (bsgs.hip:70-76, the batch kernel's sums at 236-276):
    under the identity key every rotation of the constant (q - 1, q - 1)
    ciphertext is that ciphertext, and every diagonal of the matrix -1 / q_top
    is the word q - 1, so each output of a full tile (g = 16) is exactly
    16 (q - 1)^2 -- on i14's 61-bit q0 the largest sum there is; g = 32 adds a
    second tile's reduced sum to the first one's own words (q - 1 + .. in
    add_mod); GPQHE_BSGS_INNER_TB = 8 runs the other tile form on the same
    words.  bsgs_sum_batch_kernel adds G giant-step words that are all
    16 (q - 1)^2 mod q (identity key, exact) before the rescale.
    step_diff_batch_kernel's sub_mod gets 0 - (q - 1), (q - 1) - 0 and equal
    operands exactly, and step_tail_batch_kernel uhat - w with w = uhat,
    0 - (q - 1) and w = 0 (STEP_CTS; exact under the identity key with the
    matrix -1 / q_top, which the test asserts on the oracle's words).
    Behind a non-identity key switch (one, qm1, half_lo, rand_half, digit0,
    genuine) the words reaching the inner product, the sum and the tail are
    key products and not placed: those kinds are a smoke case for the batch
    kernels and aim at the rotations themselves, as in
    test_gpu_extremes.test_gemv_rot_batch_crafted_keys."""
    if tb:
        monkeypatch.setenv("GPQHE_BSGS_INNER_TB", tb)
    pr = StepPair(oracle, product, name, slots, g)
    n, lvl, primes = product.n, product.L, product.primes[:product.L]
    scale = product.info.delta
    rots = bsgs_rotations(slots, g)
    mats = const_matrices(slots, primes[lvl - 1])
    for ki, kind in enumerate(kinds or X.BATCH_KEY_KINDS):
        craft_rot_keys(pr, kind, rots)
        for mi, m in enumerate(x for x in BSGS_PLAN[kind] if only is None or x in only):
            M = mats[m]
            specs = ["qm1"] + [GEMV_CTS[1 + (2 * (ki + mi) + j) % 4] for j in range(2)]
            host = ct_words(oracle, specs, primes, n)
            want = reference(pr, lambda e, c, rk, gg: bsgs_compose(e, M, c[0], rk, gg), host[None],
                                lvl, scale)
            assert_words(pr.batch(M, host, lvl), want, f"bsgs, key {kind}, matrix {m}")
            names = ["A", "BC"[(ki + mi) % 2], "DE"[(ki + mi) % 2]]
            H = step_blocks(oracle, primes, n, names)
            want = reference(pr, lambda e, c, rk, gg: step_compose(e, M, M, c[0], c[1], c[2], c[3], rk, gg), H, lvl, scale)
            assert_words(pr.run(M, M, H, lvl), want, f"step, key {kind}, matrix {m}")
            if kind == "identity" and m == "neg":
                assert not want[0].any(), "A: up = uhat - w with w = uhat"
                assert np.all(want[1] == 1), "B: 0 - (q - 1); C: w = 0, up = he_moddown(uhat) = 1"
                Mb = mats["pos"]
                want = reference(pr, lambda e, c, rk, gg: gemv2_compose(e, M, c[0], Mb, c[1], rk, gg), H[:2], lvl, scale)
                assert_words(pr.run(M, Mb, H[:2], lvl), want, "gemv2, identity key")
    pr.close()


# ======================================= d. row-folded and packed steps
ROWS_PLAN = {"genuine": ("sample",), "zero": ("neg",), "identity": ("neg", "pos"), "one": ("alt",), "qm1": ("neg",),
             "half_lo": ("pos",), "rand_half": ("sample",), "digit0": ("alt",)}


@pytest.mark.parametrize("name,rows,kinds", [("ref", 2, None), ("ref", 3, None),
                                             ("f13", 2, ("identity", "zero", "qm1", "genuine")),
                                             ("f13", 3, ("identity", "rand_half", "digit0"))])
def test_rows_step_on_patterns_under_crafted_keys(oracle, product, name, rows, kinds):
    """he_hempc_step_rows_batch and (identity key) he_gemv2_rows_batch at 64
    slots, rows 2 and 3 (m' = 2, 4), 5 ciphertexts, the he_genrk_rows keys
    overwritten by each key kind, against step_rows_compose /
    gemv2_rows_compose on the oracle.  Under the identity key with constant
    ciphertexts and the constant matrices every word is placed:
    rows_fold_add_kernel adds a constant ciphertext to its own rotation -- q - 1
    + q - 1 (ciphertext B, matrix +1 / q_top: w = 1 per row before the fold
    doubles it up; matrix -1 / q_top: w = q - 1 per live row) -- and
    rows_fold_tail_kernel forms c - (v + r) with v + r = q - 1 + q - 1 wrapping
    to q - 2.  step_diff's words are STEP_CTS's.  Other key kinds: a smoke
    case, as in the BSGS test."""
    slots, cnt = 64, 5
    pr = RowsPair(oracle, product, name, slots, rows)
    n, lvl, primes = product.n, product.L, product.primes[:product.L]
    scale = product.info.delta
    rots = rows_rotations(slots, rows)
    mats = const_matrices(slots, primes[lvl - 1])
    H = step_blocks(oracle, primes, n, "ABCDE")
    for kind in kinds or X.BATCH_KEY_KINDS:
        craft_rot_keys(pr, kind, rots)
        for m in ROWS_PLAN[kind]:
            M = mats[m]
            want = reference(pr, lambda e, c, rk, r: step_rows_compose(e, M, M, c[0], c[1], c[2], c[3], rk, r), H, lvl,
                                scale)
            assert_words(pr.run(M, M, H, lvl), want, f"rows step, key {kind}, matrix {m}")
            if kind == "identity":
                want = reference(pr, lambda e, c, rk, r: gemv2_rows_compose(e, M, c[0], M, c[1], rk, r), H[:2], lvl, scale)
                assert_words(pr.run(M, M, H[:2], lvl), want, f"rows gemv2, matrix {m}")
    pr.close()


@pytest.mark.parametrize("nmat", [4, 1])
def test_packed_step_on_patterns_under_crafted_keys(oracle, product, nmat):
    """he_hempc_step_packed_batch and he_gemv2_packed_batch on ref, S = 64,
    s = 16, rows 2, with per-loop matrices (nmat = P = 4: the constants
    -1 / q_top, +1 / q_top, 1/2 and a sampled one, a loop each) and a shared
    one, the he_genrk_packed keys overwritten by each key kind; 5 pattern
    ciphertexts.  The same words as the row-folded test, through the packed
    plan's diagonals and fold rotations (multiples of P)."""
    S, s, rows = 64, 16, 2
    pr = PackedPair(oracle, product, "ref", S, s, rows, nmat)
    n, lvl, primes = product.n, product.L, product.primes[:product.L]
    scale, q_top = product.info.delta, primes[product.L - 1]
    rots = packed_rotations(S, s, rows)
    rng = np.random.default_rng(12)
    loop_m = [np.full((rows, s), -1.0 / q_top, dtype=np.complex128), np.full((rows, s), 1.0 / q_top, dtype=np.complex128),
              np.full((rows, s), 0.5, dtype=np.complex128), rng.uniform(-1, 1, (rows, s)) + 1j * rng.uniform(-1, 1, (rows, s))]
    H = step_blocks(oracle, primes, n, "ABCDE")
    for ki, kind in enumerate(X.BATCH_KEY_KINDS):
        craft_rot_keys(pr, kind, rots)
        Ma = np.stack(loop_m) if nmat == 4 else np.stack([loop_m[ki % 4]])
        Mb = np.stack(loop_m[::-1]) if nmat == 4 else np.stack([loop_m[(ki + 1) % 4]])
        want = reference(pr, lambda e, c, rk, r: step_packed_compose(e, Ma, Mb, c[0], c[1], c[2], c[3], rk, s, r, nmat),
                            H, lvl, scale)
        assert_words(pr.run(Ma, Mb, H, lvl), want, f"packed step, key {kind}")
        if kind in ("identity", "qm1"):
            want = reference(pr, lambda e, c, rk, r: gemv2_packed_compose(e, Ma, c[0], Mb, c[1], rk, s, r, nmat), H[:2],
                                lvl, scale)
            assert_words(pr.run(Ma, Mb, H[:2], lvl), want, f"packed gemv2, key {kind}")
    pr.close()


# ==================================================== e. encrypted gains
#: (rotation keys, relinearisation key, gain ciphertexts DA / DB): every X.KEY_KINDS relinearisation key, the
#: identity, zero and genuine rotation keys, every gain pattern
GAIN_PLAN = [("identity", "genuine", "qm1"), ("identity", "qm1", "half_lo|half_hi"), ("zero", "one", "rand_half"),
             ("genuine", "half_lo", "rand_edge"), ("identity", "rand_half", "mixed"), ("genuine", "digit0", "genuine")]
assert {p[1] for p in GAIN_PLAN} == set(X.KEY_KINDS)

# set, rows, plan entries
GAINS = [
    ("i14", 16, (0,)),          # 2 m' = 32 terms; limb 0 the integer sums, the others FP64
    ("i14", 16, (1,)),
    ("i14", 16, (4,)),
    ("f13", 16, (0, 2)),        # 32 terms, all FP64
    ("ref", 2, range(6)),
    ("c1", 2, range(6)),        # 60-bit q0 beside 50-bit limbs
]


def gain_words(pr, spec, mp, lvl, seed):
    """[m'][2 lvl n]: the m' gain ciphertexts placed as patterns (None: genuine)."""
    n, primes = pr.p.n, pr.p.primes[:lvl]
    if spec == "genuine":
        return None
    if spec == "mixed":
        return np.stack([X.mixed(seed + i, primes, n, npolys=2) for i in range(mp)]).reshape(mp, -1)
    return ct_words(pr.o, [spec] * mp, primes, n, seed)  # (the rand_* ones differ by their seeds)


@pytest.mark.parametrize("name,rows,plan", GAINS,
                         ids=["i14-rows16-identity-qm1xqm1-x1-max-32x2(q-1)^2", "i14-rows16-half", "i14-rows16-mixed", "f13-rows16",
                              "ref-rows2", "c1-rows2"])
def test_encgain_on_patterns_under_crafted_keys(oracle, product, name, rows, plan):
    """he_hempc_step_encgain_packed_batch and he_gemv2_encgain_packed_batch at
    S = 64, s = 16, 5 ciphertexts (a partial last group of EG_CG_F64 = 4 and of
    EG_CG_INT = 2), the gain ciphertexts DA / DB placed directly as patterns
    (or genuine), the rotation keys identity / zero / genuine and the
    relinearisation key each of X.KEY_KINDS (GAIN_PLAN), against
    step_encgain_compose / gemv2_encgain_compose on the oracle, whose tensor
    sums are Python integers.
    Aimed at encgain_tensor_kernel's accumulators (encgain_batch.hip:26-76).
    EgAcc<false>, "x1 holds at most 32 products and one residue, 32 (2^61 -
    1)^2 + 2^61 < 2^128", reduced every 16 terms: under the identity key the
    constant (q - 1, q - 1) inputs rotate to themselves, so against constant
    (q - 1, q - 1) gains every one of the 2 m' = 32 terms adds exactly
    2 (q - 1)^2 to x1 and (q - 1)^2 to x0 and x2, on i14's 61-bit limb 0 the
    stated maximum (tests/test_extremes_batch_cpu.py asserts the integers).
    EgAcc<true>, "x1 peaks at 3 q and x0, x2 at 1.75 q, all below 2^53": the
    same words and +-(q - 1)/2 x +-(q - 1)/2 (half_lo|half_hi gains on
    rand_half inputs) on the FP64 limbs of i14 and on f13.  The inputs of the
    gemv2 form are GEMV_CTS, of the step STEP_CTS (its differences exact).
    The relinearisation of (0, X2) and the fold rotations run under the crafted
    keys; behind a non-identity, non-zero key their outputs are not placed."""
    S, s, cnt = 64, 16, 5
    pr = GainPair(oracle, product, name, S, s, rows)
    n, lvl, primes = product.n, product.L, product.primes[:product.L]
    scale, mp = product.info.delta, pow2(rows)
    rots = packed_rotations(S, s, rows)
    Hs = step_blocks(oracle, primes, n, "ABCDE")
    Hg = np.stack([ct_words(oracle, GEMV_CTS, primes, n), ct_words(oracle, GEMV_CTS[::-1], primes, n)])
    rng = np.random.default_rng(4)
    Mg = rng.uniform(-1, 1, (S // s, rows, s)) + 0j
    for pi in plan:
        rk_kind, rlk_kind, spec = GAIN_PLAN[pi]
        craft_rot_keys(pr, rk_kind, rots)
        craft_key(pr, "rlk", pr.O.rlk, pr.P.rlk, rlk_kind)
        DA, DB = gain_words(pr, spec, mp, lvl, 0), gain_words(pr, spec, mp, lvl, 40)
        if DA is None:
            DA, DB = pr.gains(Mg, lvl), pr.gains(Mg[::-1], lvl)
        oa, ob = pr.oracle_gains(DA, lvl), pr.oracle_gains(DB, lvl)
        if pi == 0:  # the maximum: constant (q - 1, q - 1) inputs in the gemv2 form, every ciphertext
            Hmax = np.stack([ct_words(oracle, ["qm1"] * cnt, primes, n)] * 2)
            want = reference(pr, lambda e, c, rk, r: gemv2_encgain_compose(e, oa, c[0], ob, c[1], rk, pr.O.rlk, s, r),
                                Hmax[:, :1], lvl, scale)
            got = pr.run(DA, DB, Hmax, lvl)
            assert_words(got, np.repeat(want, cnt, axis=0), "gemv2, the x1 maximum")
        want = reference(pr, lambda e, c, rk, r: step_encgain_compose(e, oa, ob, c[0], c[1], c[2], c[3], rk, pr.O.rlk, s, r),
                            Hs, lvl, scale)
        assert_words(pr.run(DA, DB, Hs, lvl), want, f"step, {GAIN_PLAN[pi]}")
        if rows == 2:  # (at 32 terms the reference's integer sums take seconds a ciphertext)
            want = reference(pr, lambda e, c, rk, r: gemv2_encgain_compose(e, oa, c[0], ob, c[1], rk, pr.O.rlk, s, r),
                                Hg, lvl, scale)
            assert_words(pr.run(DA, DB, Hg, lvl), want, f"gemv2, {GAIN_PLAN[pi]}")
    pr.close()
