"""Time the seeded secret-key batch encryptions and their expansion against
he_enc_sk_batch on one MI355X (include/gpqhe_ext_seeded_batch.h).

python scripts/seeded_batch_time.py [--count 64] [--window-s 0.3] > profiles/seeded_batch_time.json
python scripts/seeded_batch_time.py --prof > profiles/seeded_batch_prof.json
One process; per shape the legs alternate over three device-synchronised
rounds, the best window of each is kept (and every window, and the spread
(max - min) / min of each leg's windows), in microseconds per ciphertext at the
top level:
  plain shapes   f13 / 64 slots and bench51 / 16 slots:
    enc_sk      (a) he_enc_sk_batch of COUNT vectors, x [COUNT][2][L][n]
    enc_seeded  (b) he_enc_sk_seeded_batch of the same, c0 [COUNT][L][n]
    expand      (c) he_expand_seeded_batch of that c0 into x
  packed shapes  f13 S = 4096 and bench51 S = 32768, s = 16, width 3: the packed
    forms of (a) and (b), and (c)
  and from them (b) / (a), (c) / (a) and the bytes a ciphertext ships with
  either call.
--prof: the per-class gpqhe_prof_collect table of one warm call of each leg
instead (a run of its own: the events around every launch perturb the
windows).  Fails without a GPU (the product library has no CPU path).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN = [("f13", 64), ("bench51", 16)]
PACKED = [("f13", 16), ("bench51", 16)]  # S = n / 2


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def measure(e, legs, cnt, args):
    """legs {name: call} of cnt ciphertexts each -> the timing or the class tables."""
    for f in legs.values():
        f()
    e.sync()
    if args.prof:
        out = {}
        e.prof_enable(True)
        for k, f in legs.items():
            e.prof_collect()
            f()
            out[k] = kernel_table(e.prof_collect())
        e.prof_enable(False)
        return {"classes_of_one_warm_call": out}
    wins = {k: [] for k in legs}
    for _ in range(3):
        for k, f in legs.items():
            t0, it = time.perf_counter(), 0
            while time.perf_counter() - t0 < args.window_s:
                f()
                e.sync()
                it += 1
            wins[k].append(1e6 * (time.perf_counter() - t0) / it / cnt)
    return {"us_per_ct": {k: {"best": round(min(v), 2), "windows": [round(w, 2) for w in v],
                              "spread": round(max(v) / min(v) - 1, 3)} for k, v in wins.items()}}


def shape(e, np, torch, name, slots, s, args):
    """s = 0: the plain calls at `slots` slots; else the packed ones at S = n / 2."""
    from tests.test_gpu_parity import PARAMS
    kw = PARAMS[name][1]
    S = 1 << (kw["logn"] - 1) if s else slots
    e.init_params(**dict(kw, slots=S))
    e.set_seed(5)
    n, lvl, cnt, scale, width = e.n, e.L, args.count, e.info.delta, 3
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    w = lvl * n
    x = torch.zeros(cnt * 2 * w, dtype=torch.int64, device="cuda")
    c0 = torch.zeros(cnt * w, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ps, seed0 = e.pubseed(bytes(range(32))), e.pubseed(bytes(range(32)))
    if s:
        zs = rng.uniform(-1, 1, (cnt, S // s, width)) + 0j
        legs = {"enc_sk": lambda: e.enc_sk_packed_batch(x.data_ptr(), zs, sk, s, width, scale, lvl),
                "enc_seeded": lambda: e.enc_sk_seeded_packed_batch(c0.data_ptr(), zs, sk, s, width, scale, lvl, ps)}
    else:
        zs = rng.uniform(-1, 1, (cnt, S)) + 1j * rng.uniform(-1, 1, (cnt, S))
        legs = {"enc_sk": lambda: e.enc_sk_batch(x.data_ptr(), zs, sk, S, scale, lvl),
                "enc_seeded": lambda: e.enc_sk_seeded_batch(c0.data_ptr(), zs, sk, S, scale, lvl, ps)}
    legs["expand"] = lambda: e.expand_seeded_batch(x.data_ptr(), c0.data_ptr(), cnt, lvl, seed0)
    out = {"set": name, "n": n, "L": lvl, "slots": S, "count": cnt}
    if s:
        out.update({"s": s, "loops_per_ct": S // s, "width": width})
    out.update(measure(e, legs, cnt, args))
    if not args.prof:
        b = {k: v["best"] for k, v in out["us_per_ct"].items()}
        out["seeded_over_sk"] = round(b["enc_seeded"] / b["enc_sk"], 3)
        out["expand_over_sk"] = round(b["expand"] / b["enc_sk"], 3)
        out["shipped_bytes_per_ct"] = {"enc_sk": 16 * w, "enc_seeded": 8 * w + 40 / cnt}
    e.sync()
    for o in (pk, sk):
        e.free(o)
    e.exit()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from hectr_amd.gpqhe import Engine
    assert torch.cuda.is_available(), "needs an MI355X"
    e = Engine.product()
    res = {"plain": [shape(e, np, torch, name, slots, 0, args) for name, slots in PLAIN],
           "packed": [shape(e, np, torch, name, 0, s, args) for name, s in PACKED]}
    print(json.dumps({"prof" if args.prof else "timing": res}, indent=1))


if __name__ == "__main__":
    main()
