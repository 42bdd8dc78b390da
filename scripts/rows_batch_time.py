"""Time HECTR's encrypted step by row folding over a ciphertext batch on one
MI355X (he_hempc_step_rows_batch, include/gpqhe_ext_rows_batch.h) against the
full step (he_hempc_step_batch, include/gpqhe_ext_step_batch.h).

python scripts/rows_batch_time.py --shape f13:256 [--count 16] [--rows 2] [--windows 3] [--window-s 0.3] [--prof]
One shape per process; prints one JSON line.  The legs alternate in
device-synchronised windows of `calls` calls each (what fills window-s
seconds, between 3 and 200); times are microseconds per ciphertext, with the
range over the windows:
  step_batch       he_hempc_step_batch at g = he_gemv_bsgs_default_g()
  step_rows_batch  he_hempc_step_rows_batch at `rows` leading rows (keys of its own)
`rotations` holds the key switches per ciphertext each form issues and
`predicted_rotation_ratio` their quotient, (2 (m' - 1) + log2(s / m')) /
(2 (g - 1) + G - 1): what row folding leaves of the step's rotation time.
The matrices are dense; the full step reads all of them, the row-folded one
their leading rows.
--prof: the per-class gpqhe_prof_collect tables of one warm call of each leg
instead of the timing (a run of its own: the events around every launch
perturb the windows).

python scripts/rows_batch_time.py --assemble TIMING.jsonl [PROF.jsonl]
needs no GPU: joins the lines of such runs into the structure of
profiles/rows_batch_time.json, on stdout.
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
# the full step's pair plan (2.1 GB of encoded diagonals at 256 slots, N = 2^16,
# L = 8) stays cached beside the row plan
os.environ.setdefault("GPQHE_DIAG_MIB", "8192")


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def run(e, np, name, slots, args):
    import torch
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    n, lvl, s, cnt, rows = e.n, e.L, e.slots, args.count, args.rows
    g = e.bsgs_default_g()
    G = -(-s // g)
    mp = 1 << (rows - 1).bit_length()
    full, folded = 2 * (g - 1) + (G - 1), 2 * (mp - 1) + int(math.log2(s // mp))
    out = {"set": name, "n": n, "L": lvl, "K": e.K, "dnum": e.info.dnum, "slots": s, "level": lvl, "g": g,
           "rows": rows, "count": cnt, "diag_mib": int(os.environ["GPQHE_DIAG_MIB"]),
           "rotations": {"step_batch": full, "step_rows_batch": folded},
           "keys": {"step_batch": (g - 1) + (G - 1), "step_rows_batch": (mp - 1) + int(math.log2(s // mp))},
           "predicted_rotation_ratio": round(folded / full, 3)}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    Ma, Mb = (np.ascontiguousarray((rng.uniform(-1, 1, (s, s)) + 0j).ravel()) for _ in range(2))
    names = ("xhat", "xr", "uhat", "ur")
    host = []
    for k in names:
        for _ in range(cnt):
            x = e.encrypt(rng.uniform(-1, 1, s) + 0j, pk)
            host.append(e.export(x).ravel().copy())
            e.free(x)
    din = torch.from_numpy(np.concatenate(host).view(np.int64)).cuda()
    ow, cw = 2 * (lvl - 1) * n, 2 * lvl * n
    dout = torch.zeros(cnt * ow, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = [din.data_ptr() + 8 * b * cnt * cw for b in range(4)]

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    rk, rkr = e.evks(s), e.evks(s)
    e.genrk_bsgs(rk, sk, g)
    e.genrk_rows(rkr, sk, rows)
    legs = {"step_batch": lambda: e.hempc_step_batch(dout.data_ptr(), Ma, Mb, *ptr, cnt, lvl, rk, g),
            "step_rows_batch": lambda: e.hempc_step_rows_batch(dout.data_ptr(), Ma, Mb, *ptr, cnt, lvl, rkr, rows)}
    for k, fn in legs.items():
        out[k] = {"first_call_s": round(wall(fn), 4)}
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
        calls = {k: min(200, max(3, math.ceil(args.window_s / wall(fn)))) for k, fn in legs.items()}
        us = {k: [] for k in legs}
        for _ in range(args.windows):
            for k, fn in legs.items():  # alternating the legs
                us[k].append(wall(lambda: [fn() for _ in range(calls[k])]) / calls[k] / cnt * 1e6)
        for k in legs:
            out[k].update(calls_per_window=calls[k], us_per_ct=[round(v, 1) for v in us[k]],
                          us_per_ct_best=round(min(us[k]), 1), us_per_ct_worst=round(max(us[k]), 1),
                          spread=round((max(us[k]) - min(us[k])) / min(us[k]), 4))
        out["rows_over_step"] = round(out["step_rows_batch"]["us_per_ct_best"] / out["step_batch"]["us_per_ct_best"], 3)
    for o in (pk, sk):
        e.free(o)
    e.free_evks(rk)
    e.free_evks(rkr)
    e.exit()
    return out


def assemble(paths):
    rows = [[json.loads(line) for line in open(p) if line.strip().startswith("{")] for p in paths]
    out = {"timing": rows[0]}
    if len(rows) > 1:
        out["one_call_by_kernel_class"] = rows[1]
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assemble", nargs="+", metavar="FILE")
    ap.add_argument("--shape", default="f13:256")
    ap.add_argument("--count", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    if args.assemble:
        return assemble(args.assemble)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("rows_batch_time.py needs an MI355X")
    from hectr_amd.gpqhe import Engine
    name, slots = args.shape.split(":")
    res = run(Engine.product(), np, name, int(slots), args)
    res["prof"] = bool(args.prof)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
