"""Generate the committed known-answer vectors.

tests/golden/model_vectors.json comes from the pure-Python model only (no
oracle, no product): prime/root selection rule, NTT by definition, exact
rescale.  tests/golden/chacha_vectors.json holds ChaCha20 keystream blocks
produced by the local `openssl enc -chacha20` (neither the model nor the
engine), for the (key, stream, counter) triples of CHACHA_CASES.
Run: python tests/make_golden.py"""
import json
import os
import random
import shutil
import subprocess

import ckks_model as M
import ckks_model_rng as R

HERE = os.path.dirname(os.path.abspath(__file__))


def pick(bits, two_n, used):
    top = 1 << bits
    c = (top // two_n) * two_n + 1
    while c >= top:
        c -= two_n
    while c > top >> 1:
        if c not in used and M.is_prime(c):
            return c
        c -= two_n
    raise ValueError("no prime")


def psi_of(q, n):
    h = 2
    while True:
        p = pow(h, (q - 1) // (2 * n), q)
        if pow(p, n, q) == q - 1:
            return p
        h += 1


#: (seed or None for the all-zero key, stream, counter)
CHACHA_CASES = [(None, 0, 0), (None, 0, 1), (1, 0, 0), (1, 2, 5), (99, 7, 2 ** 32 - 1), (99, 2 ** 32, 3),
                (2024, 2 ** 32 + 5, 2 ** 31), (0xFFFFFFFFFFFFFFFF, 2 ** 64 - 1, 2 ** 32 - 1)]


def openssl_block(key, stream, counter):
    """64 keystream bytes of block (stream, counter) under the eight key words,
    from `openssl enc -chacha20` over 64 zero bytes."""
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", R.key_bytes(key).hex(), "-iv",
                          R.iv_bytes(stream, counter).hex()], input=bytes(64), stdout=subprocess.PIPE, check=True)
    assert len(out.stdout) == 64
    return out.stdout


def chacha_vectors():
    out = []
    for seed, stream, counter in CHACHA_CASES:
        key = [0] * 8 if seed is None else R.seed_key(seed)
        out.append({"seed": seed, "key": key, "stream": stream, "counter": counter,
                    "keystream": openssl_block(key, stream, counter).hex()})
    return out


def main():
    rnd = random.Random(20261015)
    out = {"ntt": [], "rescale": []}
    for logn, bits in ((4, 40), (6, 40), (8, 50)):
        n = 1 << logn
        q = pick(bits, 2 * n, [])
        psi = psi_of(q, n)
        x = [rnd.randrange(q) for _ in range(n)]
        out["ntt"].append({"logn": logn, "bits": bits, "q": q, "psi": psi, "input": x,
                           "ntt": M.ntt_eval(x, q, psi)})
    logn = 5
    n = 1 << logn
    used = []
    for b in (40, 36, 36):
        used.append(pick(b, 2 * n, used))
    inp, res = [], []
    coef = [[[rnd.randrange(q) for _ in range(n)] for q in used] for _ in range(2)]
    for p in range(2):
        for i in range(3):
            inp.extend(coef[p][i])
    for p in range(2):
        outp = [[0] * n for _ in range(2)]
        for k in range(n):
            X, _ = M.crt([coef[p][i][k] for i in range(3)], used)
            Y = (X - X % used[2]) // used[2]
            for i in range(2):
                outp[i][k] = Y % used[i]
        res.extend(outp[0] + outp[1])
    out["rescale"].append({"logn": logn, "primes": used, "input": inp, "output": res})
    with open(os.path.join(HERE, "golden", "model_vectors.json"), "w") as f:
        json.dump(out, f)
    # last, and only where openssl exists: the pure-model file above needs none
    if shutil.which("openssl") is None:
        print("no openssl on the path: tests/golden/chacha_vectors.json left as it is")
        return
    with open(os.path.join(HERE, "golden", "chacha_vectors.json"), "w") as f:
        json.dump({"source": "openssl enc -chacha20, 64 zero bytes in", "blocks": chacha_vectors()}, f, indent=1)


if __name__ == "__main__":
    main()
