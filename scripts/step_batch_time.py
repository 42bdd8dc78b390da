"""Time HECTR's encrypted step over a ciphertext batch on one MI355X
(he_hempc_step_batch / he_gemv2_bsgs_batch, include/gpqhe_ext_step_batch.h)
against what a caller had before them.

python scripts/step_batch_time.py --shape f13:256 [--count 16] [--windows 3] [--window-s 0.3] [--prof]
One shape per process; prints one JSON line.  The legs alternate in
device-synchronised windows of `calls` calls each (what fills window-s
seconds, between 3 and 200); times are microseconds per ciphertext, with the
range over the windows:
  loop            the step as single calls per ciphertext on he_ct_t objects:
                  he_sub x2, he_gemv_bsgs x2, he_add, he_neg, he_copy_ct,
                  he_moddown, he_add
  gemv_two_batch  two he_gemv_bsgs_batch calls (the products alone, not added)
  gemv2_batch     one he_gemv2_bsgs_batch
  step_batch      he_hempc_step_batch at g = he_gemv_bsgs_default_g()
  step_batch_half_g   ... at half that g (keys of their own)
`rotations` holds the key switches per ciphertext each form issues and
`predicted_rotation_ratio` = (2 (g - 1) + G - 1) / (2 (g - 1) + 2 (G - 1)), what
the shared giant steps leave of gemv_two_batch's rotation time.
--prof: the per-class gpqhe_prof_collect tables of one warm call of
gemv_two_batch, gemv2_batch and step_batch instead of the timing (a run of its
own: the events around every launch perturb the windows).

python scripts/step_batch_time.py --assemble TIMING.jsonl [PROF.jsonl]
needs no GPU: joins the lines of such runs into the structure of
profiles/step_batch_time.json, on stdout.
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
# both pair plans (g and g / 2: 2.1 GB of encoded diagonals each at 256 slots,
# N = 2^16, L = 8) stay cached: alternating legs must not evict one another
os.environ.setdefault("GPQHE_DIAG_MIB", "8192")


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def run(e, np, name, slots, args):
    import torch
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    n, lvl, s, cnt = e.n, e.L, e.slots, args.count
    g = e.bsgs_default_g()
    h = max(1, g // 2)
    G, Gh = -(-s // g), -(-s // h)
    out = {"set": name, "n": n, "L": lvl, "K": e.K, "dnum": e.info.dnum, "slots": s, "level": lvl, "g": g,
           "g_half": h, "count": cnt, "diag_mib": int(os.environ["GPQHE_DIAG_MIB"]),
           "rotations": {"two_products": 2 * (g - 1) + 2 * (G - 1), "shared": 2 * (g - 1) + (G - 1),
                         "shared_half_g": 2 * (h - 1) + (Gh - 1)},
           "predicted_rotation_ratio": round((2 * (g - 1) + G - 1) / (2 * (g - 1) + 2 * (G - 1)), 3)}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    Ma, Mb = (np.ascontiguousarray((rng.uniform(-1, 1, (s, s)) + 0j).ravel()) for _ in range(2))
    names = ("xhat", "xr", "uhat", "ur")
    cts = {k: [e.encrypt(rng.uniform(-1, 1, s) + 0j, pk) for _ in range(cnt)] for k in names}
    tmp = {k: e.ct() for k in ("xd", "ud", "ya", "yb", "du", "c")}
    ups = [e.ct() for _ in range(cnt)]
    host = np.concatenate([e.export(x).ravel() for k in names for x in cts[k]])
    din = torch.from_numpy(host.view(np.int64)).cuda()
    ow, cw = 2 * (lvl - 1) * n, 2 * lvl * n
    dout = torch.zeros(cnt * ow, dtype=torch.int64, device="cuda")
    dout2 = torch.zeros(cnt * ow, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: din.data_ptr() + 8 * b * cnt * cw for b, k in enumerate(names)}

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    rk, rkh = e.evks(s), e.evks(s)
    e.genrk_bsgs(rk, sk, g)
    e.genrk_bsgs(rkh, sk, h)

    def loop():
        t = tmp
        for i in range(cnt):
            e.sub(t["xd"], cts["xhat"][i], cts["xr"][i])
            e.sub(t["ud"], cts["uhat"][i], cts["ur"][i])
            e.gemv_bsgs(t["ya"], Ma, t["xd"], rk, g)
            e.gemv_bsgs(t["yb"], Mb, t["ud"], rk, g)
            e.add(t["du"], t["ya"], t["yb"])
            e.neg(t["du"])
            e.copy_ct(t["c"], cts["uhat"][i])
            e.moddown(t["c"])
            e.add(ups[i], t["c"], t["du"])

    def two():
        e.gemv_bsgs_batch(dout.data_ptr(), Ma, ptr["xhat"], cnt, lvl, rk, g)
        e.gemv_bsgs_batch(dout2.data_ptr(), Mb, ptr["uhat"], cnt, lvl, rk, g)

    def step(keys, gg):
        return lambda: e.hempc_step_batch(dout.data_ptr(), Ma, Mb, ptr["xhat"], ptr["xr"], ptr["uhat"], ptr["ur"], cnt,
                                          lvl, keys, gg)

    legs = {"loop": loop, "gemv_two_batch": two,
            "gemv2_batch": lambda: e.gemv2_bsgs_batch(dout.data_ptr(), Ma, ptr["xhat"], Mb, ptr["uhat"], cnt, lvl, rk, g),
            "step_batch": step(rk, g), "step_batch_half_g": step(rkh, h)}
    if args.prof:
        del legs["loop"], legs["step_batch_half_g"]
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
        best = {k: out[k]["us_per_ct_best"] for k in legs}
        out["gemv2_over_two"] = round(best["gemv2_batch"] / best["gemv_two_batch"], 3)
        out["step_over_loop"] = round(best["step_batch"] / best["loop"], 3)
        out["half_g_over_default_g"] = round(best["step_batch_half_g"] / best["step_batch"], 3)
    for o in [x for k in names for x in cts[k]] + list(tmp.values()) + ups + [pk, sk]:
        e.free(o)
    e.free_evks(rk)
    e.free_evks(rkh)
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
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    if args.assemble:
        return assemble(args.assemble)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("step_batch_time.py needs an MI355X")
    from hectr_amd.gpqhe import Engine
    name, slots = args.shape.split(":")
    res = run(Engine.product(), np, name, int(slots), args)
    res["prof"] = bool(args.prof)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
