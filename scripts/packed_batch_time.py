"""Time many control loops per ciphertext on one MI355X
(he_hempc_step_packed_batch, include/gpqhe_ext_packed_batch.h) against one loop
per ciphertext (he_hempc_step_rows_batch, include/gpqhe_ext_rows_batch.h).

python scripts/packed_batch_time.py --shape bench51:16 --leg rows|packed [--count 16] [--rows 2]
                                    [--window-s 0.3] [--prof]
One leg of one shape per process (the two legs live in contexts of different
slot counts); prints one JSON line holding one device-synchronised window of
each of
  step   the step alone on `count` ciphertexts
  e2e    he_enc_pk*_batch of the 4 count vectors + the step + he_dec_dcd*_batch
  enc    that encryption alone          dec    that decode alone
as microseconds per ciphertext of the step (`count`).  The legs:
  rows    a context of s slots: one loop per ciphertext (the baseline)
  packed  a context of S = n / 2 slots: P = S / s loops per ciphertext, loop p
          its own matrices (nmat = P); vectors of width 3 in, `rows` values out
A driver alternates the legs over three rounds, every process under a time
limit of its own; --assemble takes the best window of each and the spread.
--prof: the per-class gpqhe_prof_collect tables of one warm call of each
instead (a run of its own: the events around every launch perturb the windows).

python scripts/packed_batch_time.py --assemble TIMING.jsonl [PROF.jsonl]
needs no GPU: joins the lines of such runs into the structure of
profiles/packed_batch_time.json, on stdout.
Fails without a GPU otherwise (the product library has no CPU path).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH = 3  # HECTR's nx: the widest vector a loop sends
PARTS = ("step", "e2e", "enc", "dec")


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def run(e, np, name, s, args):
    import torch
    from tests.test_gpu_parity import PARAMS
    kw = PARAMS[name][1]
    packed = args.leg == "packed"
    S = (1 << (kw["logn"] - 1)) if packed else s
    e.init_params(**dict(kw, slots=S))
    e.set_seed(5)
    n, lvl, cnt, rows = e.n, e.L, args.count, args.rows
    P = S // s
    mp = 1 << (rows - 1).bit_length()
    out = {"set": name, "leg": args.leg, "n": n, "L": lvl, "K": e.K, "dnum": e.info.dnum, "slots": S, "s": s,
           "loops_per_ct": P, "level": lvl, "rows": rows, "count": cnt,
           "key_switches_per_ct": 2 * (mp - 1) + int(math.log2(s // mp)),
           "keys": (mp - 1) + int(math.log2(s // mp))}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = e.evks(S)
    rng = np.random.default_rng(1)
    w = min(WIDTH, s)
    if packed:
        e.genrk_packed(rk, sk, s, rows)
        Ma, Mb = (np.ascontiguousarray(rng.uniform(-1, 1, (P, rows, s)) + 0j) for _ in range(2))
        zs = np.ascontiguousarray(rng.uniform(-1, 1, (4 * cnt, P, w)) + 0j)
    else:
        e.genrk_rows(rk, sk, rows)
        Ma, Mb = (np.ascontiguousarray(rng.uniform(-1, 1, (s, s)) + 0j) for _ in range(2))
        zs = np.zeros((4 * cnt, s), dtype=np.complex128)
        zs[:, :w] = rng.uniform(-1, 1, (4 * cnt, w))
    ow, cw = 2 * (lvl - 1) * n, 2 * lvl * n
    din = torch.zeros(4 * cnt * cw, dtype=torch.int64, device="cuda")
    dout = torch.zeros(cnt * ow, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = [din.data_ptr() + 8 * b * cnt * cw for b in range(4)]
    scale = e.info.delta

    if packed:
        def enc():
            e.enc_pk_packed_batch(din.data_ptr(), zs, pk, s, w, scale, lvl)

        def step():
            e.hempc_step_packed_batch(dout.data_ptr(), Ma, Mb, *ptr, cnt, lvl, rk, s, rows, P)

        def dec():
            return e.dec_dcd_packed_batch(dout.data_ptr(), cnt, lvl - 1, scale, sk, s, rows)
    else:
        def enc():
            e.enc_pk_batch(din.data_ptr(), zs, pk, s, scale, lvl)

        def step():
            e.hempc_step_rows_batch(dout.data_ptr(), Ma, Mb, *ptr, cnt, lvl, rk, rows)

        def dec():
            return e.dec_dcd_batch(dout.data_ptr(), cnt, lvl - 1, scale, sk, s)

    def e2e():
        enc()
        step()
        dec()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    enc()  # the step's inputs: real encryptions
    legs = {"step": step, "e2e": e2e, "enc": enc, "dec": dec}
    for k, fn in legs.items():
        out[k] = {"first_call_s": round(wall(fn), 4)}
    # (the result means something: every loop's values are finite and small)
    z = dec()
    assert np.isfinite(z).all() and np.abs(z).max() < 1e3, np.abs(z).max()
    if args.prof:
        for k, fn in legs.items():
            fn()
            e.sync()
            e.prof_enable(True)
            e.prof_collect()
            fn()
            st = e.prof_collect()
            e.prof_enable(False)
            out[k]["kernels"] = kernel_table(st)
            out[k]["kernel_us"] = round(sum(v[1] for v in st.values()), 1)
    else:
        for k, fn in legs.items():
            calls = min(200, max(3, math.ceil(args.window_s / wall(fn))))
            us = wall(lambda: [fn() for _ in range(calls)]) / calls / cnt * 1e6
            out[k].update(calls_per_window=calls, us_per_ct=round(us, 1), us_per_loop=round(us / P, 3))
    for o in (pk, sk):
        e.free(o)
    e.free_evks(rk)
    e.exit()
    return out


def assemble(paths):
    lines = [[json.loads(line) for line in open(p) if line.strip().startswith("{")] for p in paths]
    shapes = {}
    for r in lines[0]:
        sh = shapes.setdefault((r["set"], r["s"]), {})
        leg = sh.setdefault(r["leg"], {k: r[k] for k in ("n", "L", "K", "dnum", "slots", "s", "loops_per_ct", "level",
                                                          "rows", "count", "key_switches_per_ct", "keys")})
        for k in (k for k in PARTS if k in r):  # (lines of a run without the enc / dec windows hold two)
            leg.setdefault(k, {"us_per_ct": [], "first_call_s": []})
            leg[k]["us_per_ct"].append(r[k]["us_per_ct"])
            leg[k]["first_call_s"].append(r[k]["first_call_s"])
    timing = []
    for (name, s), sh in sorted(shapes.items()):
        row = {"set": name, "s": s}
        for legname, leg in sh.items():
            for k in (k for k in PARTS if k in leg):
                v = leg[k]["us_per_ct"]
                best = min(v)
                leg[k].update(us_per_ct_best=best, us_per_ct_worst=max(v), spread=round((max(v) - best) / best, 4),
                              us_per_loop_best=round(best / leg["loops_per_ct"], 3),
                              loops_per_s=round(leg["loops_per_ct"] / best * 1e6))
            row[legname] = leg
        if "rows" in sh and "packed" in sh:
            for k in (k for k in PARTS if k in sh["rows"] and k in sh["packed"]):
                a, b = sh["rows"][k], sh["packed"][k]
                row[k + "_packed_over_rows_per_ct"] = round(b["us_per_ct_best"] / a["us_per_ct_best"], 3)
                row[k + "_loops_per_s_gain"] = round(b["loops_per_s"] / a["loops_per_s"], 1)
            row["predicted_step_packed_over_rows_per_ct"] = 1.0  # equal key-switch counts
        timing.append(row)
    out = {"timing": timing}
    if len(lines) > 1:
        out["one_call_by_kernel_class"] = lines[1]
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assemble", nargs="+", metavar="FILE")
    ap.add_argument("--shape", default="bench51:16")
    ap.add_argument("--leg", choices=("rows", "packed"), default="packed")
    ap.add_argument("--count", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    if args.assemble:
        return assemble(args.assemble)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("packed_batch_time.py needs an MI355X")
    from hectr_amd.gpqhe import Engine
    name, s = args.shape.split(":")
    res = run(Engine.product(), np, name, int(s), args)
    res["prof"] = bool(args.prof)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
