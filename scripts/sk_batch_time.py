"""Time the batch encryptions under the secret key against the public-key ones
on one MI355X (he_enc_sk_batch, he_enc_sk_packed_batch,
include/gpqhe_ext_sk_batch.h).

python scripts/sk_batch_time.py [--count 64] [--window-s 0.3] > profiles/sk_batch_time.json
python scripts/sk_batch_time.py --prof > profiles/sk_batch_prof.json
One process; per shape the legs alternate over three device-synchronised
rounds, the best window of each is kept (and every window), in microseconds
per ciphertext at the top level:
  plain shapes   f13 / 64 slots and bench51 / 16 slots:
    enc_pk  he_enc_pk_batch of COUNT vectors      enc_sk  he_enc_sk_batch of the same
  packed shapes  f13 S = 4096 and bench51 S = 32768, s = 16, width 3:
    enc_pk  he_enc_pk_packed_batch of COUNT loop sets      enc_sk  he_enc_sk_packed_batch
    step    he_hempc_step_packed_batch of COUNT / 4 ciphertexts (rows 2) on those inputs
    dcd     he_dec_dcd_packed_batch of its results
  and from them the packed control step end to end per ciphertext of the
  step: 4 encryptions + step + decode, with either key.
--prof: the per-class gpqhe_prof_collect table of one warm call of each
encryption leg instead (a run of its own: the events around every launch
perturb the windows).  Fails without a GPU (the product library has no CPU
path).
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


def measure(e, legs, per, args):
    """legs {name: call}, per {name: ciphertexts a call handles} -> the timing or the class tables."""
    for f in legs.values():
        f()
    e.sync()
    if args.prof:
        out = {}
        e.prof_enable(True)
        for k, f in legs.items():
            if k.startswith("enc"):
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
            wins[k].append(1e6 * (time.perf_counter() - t0) / it / per[k])
    return {"us_per_ct": {k: {"best": round(min(v), 2), "windows": [round(w, 2) for w in v]} for k, v in wins.items()}}


def plain(e, np, torch, name, slots, args):
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    n, lvl, cnt, scale = e.n, e.L, args.count, e.info.delta
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    zs = rng.uniform(-1, 1, (cnt, slots)) + 1j * rng.uniform(-1, 1, (cnt, slots))
    x = torch.zeros(cnt * 2 * lvl * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    legs = {"enc_pk": lambda: e.enc_pk_batch(x.data_ptr(), zs, pk, slots, scale, lvl),
            "enc_sk": lambda: e.enc_sk_batch(x.data_ptr(), zs, sk, slots, scale, lvl)}
    out = {"set": name, "n": n, "L": lvl, "slots": slots, "count": cnt}
    out.update(measure(e, legs, {k: cnt for k in legs}, args))
    if not args.prof:
        b = {k: v["best"] for k, v in out["us_per_ct"].items()}
        out["sk_over_pk"] = round(b["enc_sk"] / b["enc_pk"], 3)
    e.sync()
    for o in (pk, sk):
        e.free(o)
    e.exit()
    return out


def packed(e, np, torch, name, s, args):
    from tests.test_gpu_parity import PARAMS
    kw = PARAMS[name][1]
    S = 1 << (kw["logn"] - 1)
    e.init_params(**dict(kw, slots=S))
    e.set_seed(5)
    n, lvl, cnt, scale, rows, width = e.n, e.L, args.count, e.info.delta, 2, 3
    P, steps = S // s, max(1, args.count // 4)
    pk, sk, rk = e.pk(), e.sk(), e.evks(S)
    e.keypair(pk, sk)
    e.genrk_packed(rk, sk, s, rows)
    rng = np.random.default_rng(1)
    zs = rng.uniform(-1, 1, (cnt, P, width)) + 0j
    Ma, Mb = (rng.uniform(-1, 1, (P, rows, s)) + 0j for _ in range(2))
    cw, ow = 2 * lvl * n, 2 * (lvl - 1) * n
    x = torch.zeros(max(cnt, 4 * steps) * cw, dtype=torch.int64, device="cuda")
    up = torch.zeros(steps * ow, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    part = [x.data_ptr() + 8 * b * steps * cw for b in range(4)]
    legs = {"enc_pk": lambda: e.enc_pk_packed_batch(x.data_ptr(), zs, pk, s, width, scale, lvl),
            "enc_sk": lambda: e.enc_sk_packed_batch(x.data_ptr(), zs, sk, s, width, scale, lvl),
            "step": lambda: e.hempc_step_packed_batch(up.data_ptr(), Ma, Mb, *part, steps, lvl, rk, s, rows, P),
            "dcd": lambda: e.dec_dcd_packed_batch(up.data_ptr(), steps, lvl - 1, scale, sk, s, rows)}
    per = {"enc_pk": cnt, "enc_sk": cnt, "step": steps, "dcd": steps}
    out = {"set": name, "n": n, "L": lvl, "slots": S, "s": s, "loops_per_ct": P, "width": width, "rows": rows,
           "count": cnt, "step_count": steps}
    out.update(measure(e, legs, per, args))
    if not args.prof:
        b = {k: v["best"] for k, v in out["us_per_ct"].items()}
        out["sk_over_pk"] = round(b["enc_sk"] / b["enc_pk"], 3)
        out["control_step_us_per_ct"] = {k: round(4 * b["enc_" + k] + b["step"] + b["dcd"], 1) for k in ("pk", "sk")}
    e.sync()
    for o in (pk, sk):
        e.free(o)
    e.free_evks(rk)
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
    res = {"plain": [plain(e, np, torch, name, slots, args) for name, slots in PLAIN],
           "packed": [packed(e, np, torch, name, s, args) for name, s in PACKED]}
    print(json.dumps({"prof" if args.prof else "timing": res}, indent=1))


if __name__ == "__main__":
    main()
