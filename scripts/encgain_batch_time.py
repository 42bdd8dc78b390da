"""Time the packed step with encrypted gains on one MI355X
(he_hempc_step_encgain_packed_batch, include/gpqhe_ext_encgain_batch.h).

python scripts/encgain_batch_time.py [--shape bench51:16 --shape f13:16] [--count 16] [--rows 2]
                                     [--window-s 0.3] [--prof] > profiles/encgain_batch_time.json
One process, one context of S = n / 2 slots per shape; the legs alternate over
three device-synchronised rounds, the best window of each is kept (and the
spread), in microseconds per ciphertext at the top level:
  packed    he_hempc_step_packed_batch on the same context: the gains in the
            clear.  encgain / packed is the price of hiding them.
  per_term  the same plaintext from calls the library already had: he_rot_batch
            for the baby rotations and one he_mul_rescale_batch per (rotated
            input, diagonal) pair against replicated diagonals (2 m'
            relinearisations); its sums, fold and tail are left out, in its favour
  encgain   the new step: one tensor pass, one relinearisation
--prof: the per-class gpqhe_prof_collect table of one warm call of the new
step instead (a run of its own: the events around every launch perturb the
windows).  Fails without a GPU (the product library has no CPU path).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def shape(e, np, torch, name, s, args):
    from tests.test_gpu_parity import PARAMS
    kw = PARAMS[name][1]
    S = 1 << (kw["logn"] - 1)
    e.init_params(**dict(kw, slots=S))
    e.set_seed(5)
    n, lvl, cnt, rows = e.n, e.L, args.count, args.rows
    P, mp = S // s, 1 << (rows - 1).bit_length()
    pk, sk, rlk, rk = e.pk(), e.sk(), e.evk(), e.evks(S)
    e.keypair(pk, sk)
    e.genrk_packed(rk, sk, s, rows)
    e.genrlk(rlk, sk)
    rng = np.random.default_rng(1)
    Ma, Mb = (rng.uniform(-1, 1, (P, rows, s)) + 0j for _ in range(2))
    cw, ow = 2 * lvl * n, 2 * (lvl - 1) * n
    x = torch.zeros(4 * cnt * cw, dtype=torch.int64, device="cuda")
    up = torch.zeros(cnt * max(ow, cw), dtype=torch.int64, device="cuda")
    D = torch.zeros(2 * mp * cw, dtype=torch.int64, device="cuda")
    rot = torch.zeros(cnt * cw, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.enc_pk_packed_batch(x.data_ptr(), rng.uniform(-1, 1, (4 * cnt, P, 3)) + 0j, pk, s, 3, e.info.delta, lvl)
    DA, DB = D.data_ptr(), D.data_ptr() + 8 * mp * cw
    e.enc_gain_packed_batch(DA, Ma, pk, s, rows, lvl, P)
    e.enc_gain_packed_batch(DB, Mb, pk, s, rows, lvl, P)
    Drep = D.view(2 * mp, 1, cw).repeat(1, cnt, 1).contiguous()  # every diagonal replicated over the batch
    part = [x.data_ptr() + 8 * b * cnt * cw for b in range(4)]

    def packed():
        e.hempc_step_packed_batch(up.data_ptr(), Ma, Mb, *part, cnt, lvl, rk, s, rows, P)

    def encgain():
        e.hempc_step_encgain_packed_batch(up.data_ptr(), DA, DB, *part, cnt, lvl, rk, rlk, s, rows)

    def per_term():
        for op in (0, 2):
            for i in range(mp):
                src = part[op]
                if i:
                    e.lib.he_rot_batch(rot.data_ptr(), part[op], cnt, lvl, i * P, rk)
                    src = rot.data_ptr()
                d = Drep.data_ptr() + 8 * ((op // 2) * mp + i) * cnt * cw
                e.lib.he_mul_rescale_batch(up.data_ptr(), src, d, cnt, lvl, rlk)

    legs = {"packed": packed, "per_term": per_term, "encgain": encgain}
    out = {"set": name, "n": n, "L": lvl, "slots": S, "s": s, "loops_per_ct": P, "rows": rows, "count": cnt}
    if args.prof:
        encgain()
        e.sync()
        e.prof_enable(True)
        e.prof_collect()
        encgain()
        out["classes_of_one_warm_call"] = kernel_table(e.prof_collect())
        e.prof_enable(False)
    else:
        wins = {k: [] for k in legs}
        for f in legs.values():
            f()
        e.sync()
        for _ in range(3):
            for k, f in legs.items():
                t0, it = time.perf_counter(), 0
                while time.perf_counter() - t0 < args.window_s:
                    f()
                    e.sync()
                    it += 1
                wins[k].append(1e6 * (time.perf_counter() - t0) / it / cnt)
        out["us_per_ct"] = {k: {"best": round(min(v), 2), "windows": [round(w, 2) for w in v]}
                            for k, v in wins.items()}
        b = {k: min(v) for k, v in wins.items()}
        out["encgain_over_packed"] = round(b["encgain"] / b["packed"], 3)
        out["encgain_over_per_term"] = round(b["encgain"] / b["per_term"], 3)
    e.sync()
    for o in (pk, sk, rlk):
        e.free(o)
    e.free_evks(rk)
    e.exit()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append")
    ap.add_argument("--count", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from hectr_amd.gpqhe import Engine
    assert torch.cuda.is_available(), "needs an MI355X"
    e = Engine.product()
    res = [shape(e, np, torch, sh.split(":")[0], int(sh.split(":")[1]), args)
           for sh in (args.shape or ["bench51:16", "f13:16"])]
    print(json.dumps({"prof" if args.prof else "timing": res}, indent=1))


if __name__ == "__main__":
    main()
