"""Time warm he_gemv (full he_genrk key set, fold cached) against warm
he_gemv_bsgs (default g, he_genrk_bsgs keys) on one MI355X.

python scripts/bsgs_time.py [--shapes f13:256,bench51:64,bench51:256,bench51:1024:bsgs]
                            [--windows 3] [--window-s 0.3] [--prof]
Prints one JSON line.  Per shape, in one process, the two legs alternate in
device-synchronised windows of `calls` calls each (calls: what fills window-s
seconds, between 10 and 400); also first-call and key-generation time, and the
bytes of keys and encoded diagonals each leg holds.  Those are not read back
from the engine: the *_formula fields come from the layouts (a key is
2 dnum (L + K) n words, doubled by its Montgomery-form shadow; a folded
diagonal (2 ndig + 1)(lvl + K) n doubles; a BSGS diagonal lvl n words).
A shape marked :bsgs runs the BSGS leg alone and only reports the direct
leg's sizes.  --prof: the per-class gpqhe_prof_collect breakdown of one warm
BSGS call per shape instead of the timing (a run of its own: the events
around every launch perturb the windows).
Fails without a GPU (the product library has no CPU path).

python scripts/bsgs_time.py --assemble TIMING.jsonl PROF.json [UBENCH_MEM.txt]
needs no GPU: it joins the lines of timing runs (one shape per line keeps a
run short), one --prof run and the output of scripts/ubench_mem on the same
box into the structure of profiles/bsgs_time.json, on stdout.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the 1024-slot set of encoded diagonals (4.3 GB at N = 2^16, L = 8) is kept
os.environ.setdefault("GPQHE_DIAG_MIB", "8192")


def shape(e, np, name, slots, direct, args):
    from tests.bsgs_ref import bsgs_rotations
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    info = e.info
    n, L, K, dnum, s = e.n, e.L, e.K, info.dnum, e.slots
    alpha = info.alpha
    lvl = L
    ndig = (lvl + alpha - 1) // alpha
    key_bytes = 2 * dnum * (L + K) * n * 8 * 2
    out = {"set": name, "n": n, "L": L, "K": K, "dnum": dnum, "slots": s, "level": lvl,
           "g": e.bsgs_default_g(), "diag_mib": int(os.environ["GPQHE_DIAG_MIB"])}
    out["direct"] = {"keys": s - 1, "key_bytes_formula": (s - 1) * key_bytes,
                     "diag_bytes_formula": s * (2 * ndig + 1) * (lvl + K) * n * 8}
    out["bsgs"] = {"keys": len(bsgs_rotations(s)), "key_bytes_formula": len(bsgs_rotations(s)) * key_bytes,
                   "diag_bytes_formula": s * lvl * n * 8}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    M = np.ascontiguousarray((rng.uniform(-1, 1, (s, s)) + 0j).ravel())
    x = e.encrypt(rng.uniform(-1, 1, s) + 0j, pk)
    y = e.ct()
    e.sync()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    legs = {}
    rkb = e.evks(s)
    out["bsgs"]["keygen_s"] = wall(lambda: e.genrk_bsgs(rkb, sk))
    legs["bsgs"] = lambda: e.gemv_bsgs(y, M, x, rkb)
    rkd = None
    if direct:
        rkd = e.evks(s)
        out["direct"]["keygen_s"] = wall(lambda: e.genrk(rkd, sk))
        legs["direct"] = lambda: e.gemv(y, M, x, rkd)
    for k, fn in legs.items():
        out[k]["first_call_s"] = wall(fn)
    if args.prof:
        legs["bsgs"]()
        e.sync()
        e.prof_enable(True)
        e.prof_collect()
        legs["bsgs"]()
        st = e.prof_collect()
        e.prof_enable(False)
        out["bsgs"]["kernels"] = {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
                                  for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}
    else:
        calls = {k: min(400, max(10, math.ceil(args.window_s / wall(fn)))) for k, fn in legs.items()}
        us = {k: [] for k in legs}
        for _ in range(args.windows):
            for k, fn in legs.items():  # alternating the legs
                us[k].append(wall(lambda: [fn() for _ in range(calls[k])]) / calls[k] * 1e6)
        for k in legs:
            out[k].update(calls_per_window=calls[k], us_per_call=[round(v, 1) for v in us[k]],
                          us_per_call_best=round(min(us[k]), 1))
        if direct:
            out["faster"] = "bsgs" if out["bsgs"]["us_per_call_best"] < out["direct"]["us_per_call_best"] else "direct"
    for o in (x, y, pk, sk):
        e.free(o)
    e.free_evks(rkb)
    if rkd is not None:
        e.free_evks(rkd)
    e.exit()
    return out


def assemble(paths):
    timing = [sh for line in open(paths[0]) if line.strip() for sh in json.loads(line)["shapes"]]
    out = {"timing": timing, "one_call_by_kernel_class": json.load(open(paths[1]))["shapes"]}
    if len(paths) > 2:
        rows = [line.split() for line in open(paths[2]) if line.strip()]
        out["ubench_mem_GBs"] = {r[0]: float(r[1]) for r in rows}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assemble", nargs="+", metavar="FILE")
    ap.add_argument("--shapes", default="f13:256,bench51:64,bench51:256,bench51:1024:bsgs")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    if args.assemble:
        return assemble(args.assemble)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bsgs_time.py needs an MI355X")
    from hectr_amd.gpqhe import Engine
    e = Engine.product()
    res = []
    for spec in args.shapes.split(","):
        f = spec.split(":")
        res.append(shape(e, np, f[0], int(f[1]), len(f) < 3 or f[2] != "bsgs", args))
    print(json.dumps({"prof": bool(args.prof), "shapes": res}), flush=True)


if __name__ == "__main__":
    main()
