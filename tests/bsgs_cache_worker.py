"""Worker of tests/test_gpu_bsgs.py::test_small_diagonal_cache (a process of its
own: GPQHE_DIAG_MIB is read once per process).  With a 1 MiB cap on `ref` at
32 slots (n = 4096, level 2: 64 KiB per encoded diagonal), each of the three
plan caches sees the same twelve calls over four plans: plan 0 is larger than
the cap, so it is encoded into workspace on every call and never cached; plans
1 to 3 (512 KiB each) rotate through a cache that holds two, so every later
call evicts the least recently used one.
  he_gemv_bsgs, g = 8         a dense matrix (32 diagonals, 2 MiB); three
                              8-diagonal matrices
  he_gemv2_bsgs_batch, g = 8  a dense pair (64 diagonals, 4 MiB); three pairs
                              masked to the diagonals k, k + 8, .. (4 + 4)
  he_gemv2_rows_batch         rows = 16 of a dense pair (16 + 16 extended
                              diagonals, 2 MiB); rows = 4 of three dense pairs
                              (4 + 4)
The three families are interleaved call by call, so an entry that one cache
handed to another kind of call would show as wrong words.  The batch calls run
over two ciphertexts.  Every result must equal the composition on the oracle
(tests/bsgs_ref.py, tests/step_ref.py, tests/rows_ref.py).  Prints one JSON
line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = (0, 0, 1, 2, 3, 1, 2, 3, 0, 3, 2, 1)


def main():
    assert os.environ.get("GPQHE_DIAG_MIB") == "1"
    import torch
    from hectr_amd.gpqhe import Engine
    from tests.bsgs_ref import bsgs_compose, bsgs_keys
    from tests.rows_ref import gemv2_rows_compose, rows_keys
    from tests.step_ref import gemv2_compose
    s, g, cnt = 32, 8, 2
    o, p = Engine.oracle(), Engine.product()
    rng = np.random.default_rng(9)

    def dense():
        return rng.uniform(-1, 1, (s, s)) + 1j * rng.uniform(-1, 1, (s, s))

    z = rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s)
    d = np.add.outer(-np.arange(s), np.arange(s)) % s
    A = dense()
    mats = [A] + [A * np.isin(d, np.arange(k, s, 4)) for k in (0, 1, 2)]
    A, B = dense(), dense()
    pairs = [(A, B)] + [(A * np.isin(d, np.arange(k, s, 8)), B * np.isin(d, np.arange(k, s, 8))) for k in (0, 1, 2)]
    rowed = [(dense(), dense(), 16)] + [(dense(), dense(), 4) for _ in range(3)]
    zs = [rng.uniform(-1, 1, s) + 1j * rng.uniform(-1, 1, s) for _ in range(2 * cnt)]

    side = {}
    for e in (o, p):
        e.init(12, 109, s, 50)
        e.set_seed(31)
        pk, sk = e.pk(), e.sk()
        e.keypair(pk, sk)
        rk, x = bsgs_keys(e, sk, g), e.encrypt(z, pk)
        if e is p:
            rows_rk = e.evks(s)
            e.genrk_rows(rows_rk, sk, 16)
        else:
            rows_rk = rows_keys(e, sk, 16)
        side[e.name] = (rk, x, rows_rk, pk)

    # the batch calls' inputs: the product's encryptions, their exported words
    # the device blocks xa, xb [cnt][2 level n] and, imported, the oracle's
    pk = side["product"][3]
    cts = [p.encrypt(v, pk) for v in zs]
    level, scale = cts[0].nlimbs, cts[0].scale
    assert level == 2 and p.n == 4096
    H = np.stack([p.export(c).ravel().copy() for c in cts])
    imported = []
    for w in H:
        c = o.ct()
        o.import_(c, w, level, scale=scale)
        imported.append(c)

    rk, x, rows_rk, _ = side["oracle"]

    def oracle_words(compose):
        y = compose()
        w = o.export(y).ravel().copy()
        o.free(y)
        return w

    want = [oracle_words(lambda: bsgs_compose(o, M, x, rk, g)) for M in mats]
    want2 = [np.stack([oracle_words(lambda: gemv2_compose(o, Ma, imported[c], Mb, imported[cnt + c], rk, g))
                       for c in range(cnt)]) for Ma, Mb in pairs]
    wantr = [np.stack([oracle_words(lambda: gemv2_rows_compose(o, Ma, imported[c], Mb, imported[cnt + c], rows_rk, r))
                       for c in range(cnt)]) for Ma, Mb, r in rowed]

    rk, x, rows_rk, _ = side["product"]
    ow = 2 * (level - 1) * p.n
    din = torch.from_numpy(H.ravel().view(np.int64)).cuda()
    xa, xb = din.data_ptr(), din.data_ptr() + 8 * cnt * H.shape[1]

    def batch(call):
        dout = torch.zeros(cnt * ow, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        call(dout.data_ptr())
        p.sync()
        return dout.cpu().numpy().view(np.uint64).reshape(cnt, ow)

    calls = {"bsgs": 0, "pair": 0, "rows": 0}
    for n, i in enumerate(ORDER):
        y = p.ct()
        p.gemv_bsgs(y, mats[i], x, rk, g)
        assert np.array_equal(p.export(y).ravel(), want[i]), f"call {n}: matrix {i} differs from the composition"
        p.free(y)
        calls["bsgs"] += 1
        Ma, Mb = pairs[i]
        got = batch(lambda out: p.gemv2_bsgs_batch(out, Ma, xa, Mb, xb, cnt, level, rk, g))
        assert np.array_equal(got, want2[i]), f"call {n}: pair {i} differs from the composition"
        calls["pair"] += 1
        Ma, Mb, r = rowed[i]
        got = batch(lambda out: p.gemv2_rows_batch(out, Ma, xa, Mb, xb, cnt, level, rows_rk, r))
        assert np.array_equal(got, wantr[i]), f"call {n}: row pair {i} differs from the composition"
        calls["rows"] += 1
    assert np.array_equal(din.cpu().numpy().view(np.uint64), H.ravel()), "an input was written"
    for e in (o, p):
        e.exit()
    print(json.dumps({"ok": True, "calls": calls}), flush=True)


if __name__ == "__main__":
    main()
