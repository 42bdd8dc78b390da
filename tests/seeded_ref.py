"""The seeded secret-key encryptions of include/gpqhe_ext_seeded_batch.h built
from the calls of include/gpqhe.h and exact integers (a helper, not a test):
  1. he_ecd_ex + he_enc_sk, one ciphertext at a time (tests/sk_ref.py): (c0', c1');
  2. a = ckks_model_rng.sample_uniform under the PUBLIC key and stream;
  3. c0 = (c0' + (c1' - a) s) mod q in Python integers, s the exported secret key.
(c0, a) is the ciphertext the computing side holds after he_expand_seeded_batch;
c0 + a s equals c0' + c1' s word for word, so it decodes double for double like
the plain he_enc_sk ciphertext.  The private streams are those of he_enc_sk.
They run on either engine; the tests run them on the oracle as the reference
for the product's seeded calls.

The reference regulators are the existing ones on a SeededEngine: an engine
whose `encrypt` is that recipe on a running public stream.
"""
import numpy as np

import ckks_model_rng as R
from tests.encgain_ref import RefGainRegulator, gain_diagonals
from tests.packed_ref import deinterleave, interleave, step_packed_compose
from tests.sk_ref import RefSymPackedRegulator, encrypt_sk


def key_words(key):
    """The eight little-endian words of a 32-byte public key (or a PubSeed)."""
    if hasattr(key, "key"):
        return [int(w) for w in key.key]
    if isinstance(key, (bytes, bytearray)):
        return [int(w) for w in np.frombuffer(bytes(key), dtype="<u4")]
    return [int(w) for w in key]


def sample_a(e, key, stream, nl):
    """a [nl][n]: the engine's uniform sample of (key, stream) on the first nl moduli."""
    nmod = e.L + e.K
    return np.stack([R.sample_uniform(key_words(key), stream, e.n, m, e.primes[m], nmod) for m in range(nl)])


def secret_words(e, sk, nl):
    return e.export(sk)[0][:nl].copy()


def reseed(e, words, s_ntt, key, stream):
    """(c0', c1') [2][nl][n] -> (c0, a) [2][nl][n]: c0 = c0' + (c1' - a) s, exact."""
    nl = words.shape[1]
    a = sample_a(e, key, stream, nl)
    out = np.empty_like(words)
    for m in range(nl):
        q = int(e.primes[m])
        c0, c1, s = (v.astype(object) for v in (words[0, m], words[1, m], s_ntt[m]))
        out[0, m] = ((c0 + (c1 - a[m].astype(object)) * s) % q).astype(np.uint64)
        out[1, m] = a[m]
    return out


def encrypt_sk_seeded(e, z, sk, key, stream, slots=None, scale=None, nlimbs=None, s_ntt=None):
    """A new ciphertext (c0, a): encrypt_sk, then reseed with (key, stream), imported."""
    ct = encrypt_sk(e, z, sk, slots, scale, nlimbs)
    nl = ct.nlimbs
    w = reseed(e, e.export(ct), secret_words(e, sk, nl) if s_ntt is None else s_ntt, key, stream)
    e.import_(ct, w, nl, scale=ct.scale, flags=ct.flags)
    return ct


def enc_sk_seeded_words(e, zs, sk, slots, scale, nl, key, stream):
    """Ciphertext i of zs with public stream `stream + i`: (c0 words [cnt][nl n],
    expanded words [cnt][2 nl n], the plain he_enc_sk words [cnt][2 nl n])."""
    s_ntt = secret_words(e, sk, nl)
    plain, full = [], []
    for i, z in enumerate(zs):
        ct = encrypt_sk(e, z, sk, slots, scale, nl)
        assert ct.nlimbs == nl
        w = e.export(ct).copy()
        e.free(ct)
        plain.append(w.ravel())
        full.append(reseed(e, w, s_ntt, key, stream + i).ravel())
    if not zs:
        z0 = np.zeros((0, 2 * nl * e.n), dtype=np.uint64)
        return z0[:, :nl * e.n], z0, z0
    full, plain = np.stack(full), np.stack(plain)
    return full[:, :nl * e.n].copy(), full, plain


def enc_sk_seeded_packed_words(e, zs, sk, scale, nl, key, stream):
    """The same on the interleaved vectors: zs [cnt][P][width], loop-major."""
    return enc_sk_seeded_words(e, [interleave(z, e.slots) for z in zs], sk, e.slots, scale, nl, key, stream)


def enc_gain_sk_seeded_compose(e, M, sk, s, rows, nmat, lvl, key, stream):
    """m' new ciphertexts (c0, a): the extended diagonals E_i at scale q_top, the
    all-zero ones too, public stream `stream + i`."""
    S, s_ntt = e.slots, secret_words(e, sk, lvl)
    return [encrypt_sk_seeded(e, E, sk, key, stream + i, S, float(e.primes[lvl - 1]), lvl, s_ntt)
            for i, E in enumerate(gain_diagonals(M, S, s, rows, nmat))]


class SeededEngine:
    """An engine whose encrypt() ignores the public key it is given: the
    seeded recipe under the secret key of the last keypair(), the public
    stream advancing by one per ciphertext."""

    def __init__(self, e, key, stream=0):
        self._e, self._sk, self._s = e, None, None
        self.pubkey, self.pubstream = key_words(key), stream

    def __getattr__(self, name):
        return getattr(self._e, name)

    def keypair(self, pk, sk):
        self._e.keypair(pk, sk)
        self._sk, self._s = sk, secret_words(self._e, sk, self._e.L)

    def encrypt(self, z, pk, slots=None, scale=None, nlimbs=None):
        nl = nlimbs or self._e.L
        ct = encrypt_sk_seeded(self._e, z, self._sk, self.pubkey, self.pubstream, slots, scale, nlimbs, self._s[:nl])
        self.pubstream += 1
        return ct


class RefSeededGainRegulator(RefGainRegulator):
    """cstr.EncryptedGainRegulator(sym="seeded")'s loop, one ciphertext at a
    time: RefGainRegulator with every encryption (the gains' diagonals, MA's
    first, then the inputs) by the seeded recipe, a imported as c1."""

    def __init__(self, e, problems, slots_total, seed, key, stream=0, **kw):
        super().__init__(SeededEngine(e, key, stream), problems, slots_total, seed, **kw)


class RefSeededPackedRegulator(RefSymPackedRegulator):
    """cstr.PackedEncryptedRegulator(sym="seeded")'s loop written with
    step_packed_compose, one ciphertext at a time."""

    def __init__(self, e, problems, slots_total, seed, key, stream=0, **kw):
        super().__init__(SeededEngine(e, key, stream), problems, slots_total, seed, **kw)

    def __call__(self, xhat, uhat, xr, ur):
        e, cnt, P, w = self.e, self.count, self.P, self.width
        zs = np.zeros((4, cnt * P, w), dtype=np.complex128)
        for b, v in enumerate((xhat, xr, uhat, ur)):
            v = np.asarray(v, dtype=np.float64).reshape(self.nloops, -1)
            zs[b, :self.nloops, :v.shape[1]] = v
        cts = [[e.encrypt(interleave(zs[b, c * P:(c + 1) * P], self.S), None, self.S, self.scale, self.lvl)
                for c in range(cnt)] for b in range(4)]
        out = []
        for c in range(cnt):
            up = step_packed_compose(e, self.MA, self.MB, cts[0][c], cts[1][c], cts[2][c], cts[3][c], self.rk,
                                     self.s, self.rows, P)
            out.append(deinterleave(e.decrypt(up, self.sk, self.S), P, self.rows))
            e.free(up)
        for blk in cts:
            for x in blk:
                e.free(x)
        return np.stack(out).real.reshape(cnt * P, self.rows)[:self.nloops, :self.problems[0].nu].copy()
