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

python scripts/bsgs_time.py --batch COUNT [--shapes f13:256,bench51:64,bench51:256,bench51:1024:bsgs]
                            [--windows 3] [--window-s 0.3] [--prof] [--level LVL]
times COUNT ciphertexts per shape, one process, alternating legs in
device-synchronised windows: (a) "loop", he_gemv_bsgs called once per
ciphertext; (b) "batch", one he_gemv_bsgs_batch; (c) "direct_batch", one
he_gemv_batch with the full key set (not for shapes marked :bsgs).  Times are
per ciphertext.  --prof: the per-class table of one warm batch call, and of it
the share of the baby rotations' time that their ModUps take (classes timed in
a baby-only matrix, g diagonals: the rotation classes are those of the baby
stage alone).

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


#: a rotation's ModUp classes on the windowed path (k_gemv_batch): the split
#: key switch's ModUp (d2_rows, ks_cols*, the forward row passes) or its FP64
#: fallback's conversion.  (The rescale's one forward row pass counts with them:
#: one launch in 3 (g - 1) + 1.)
MODUP_CLASSES = ("d2_rows", "ks_cols", "gemv_fbc", "ntt3_rows_kernel<fwd>")
NOT_ROT = ("bsgs_inner", "bsgs_sum")


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def shape_batch(e, np, name, slots, direct, args):
    import torch
    from tests.bsgs_ref import bsgs_rotations
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    n, L, s, cnt = e.n, e.L, e.slots, args.batch
    lvl = args.level or L
    g = e.bsgs_default_g()
    out = {"set": name, "n": n, "L": L, "K": e.K, "dnum": e.info.dnum, "slots": s, "level": lvl, "g": g,
           "count": cnt, "bsgs_keys": len(bsgs_rotations(s))}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    M = np.ascontiguousarray((rng.uniform(-1, 1, (s, s)) + 0j).ravel())
    xs = [e.encrypt(rng.uniform(-1, 1, s) + 0j, pk, nlimbs=lvl) for _ in range(cnt)]
    ys = [e.ct() for _ in range(cnt)]
    host = np.concatenate([e.export(x).ravel() for x in xs])
    din = torch.from_numpy(host.view(np.int64)).cuda()
    dout = torch.zeros(cnt * 2 * (lvl - 1) * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    rkb = e.evks(s)
    e.genrk_bsgs(rkb, sk)
    legs = {"loop": lambda: [e.gemv_bsgs(ys[i], M, xs[i], rkb) for i in range(cnt)],
            "batch": lambda: e.gemv_bsgs_batch(dout.data_ptr(), M, din.data_ptr(), cnt, lvl, rkb)}
    if args.ab_tb:  # both forms of the inner kernel's baby-slot tile (read per call), same process and windows
        def forced(tb):
            def run():
                os.environ["GPQHE_BSGS_INNER_TB"] = tb
                legs["batch"]()
                del os.environ["GPQHE_BSGS_INNER_TB"]
            return run
        legs["batch_tb8"], legs["batch_tb16"] = forced("8"), forced("16")
    rkd = None
    if direct and not args.prof:
        rkd = e.evks(s)
        e.genrk(rkd, sk)
        legs["direct_batch"] = lambda: e.lib.he_gemv_batch(dout.data_ptr(), M.ctypes.data, din.data_ptr(), cnt, lvl, rkd)
    ow = 2 * (lvl - 1) * n
    for k, fn in legs.items():
        out[k] = {"first_call_s": round(wall(fn), 4)}
        if k == "batch":  # (before the direct leg writes its own result over it)
            got = dout.cpu().numpy().view(np.uint64).reshape(cnt, ow)
            out["batch_equals_loop"] = all(np.array_equal(e.export(ys[i]).ravel(), got[i]) for i in range(cnt))
    if args.prof:
        def prof(fn):
            fn()
            e.sync()
            e.prof_enable(True)
            e.prof_collect()
            fn()
            st = e.prof_collect()
            e.prof_enable(False)
            return st
        out["batch"]["kernels"] = kernel_table(prof(legs["batch"]))
        if args.ab_tb:
            for k in ("batch_tb8", "batch_tb16"):
                out[k]["kernels"] = kernel_table(prof(legs[k]))
        out["loop"]["kernels"] = kernel_table(prof(legs["loop"]))
        # the baby stage alone: a matrix of the diagonals 1 .. g - 1 has no
        # rotated giant step, so every rotation class below is the babies'
        Mb = np.zeros((s, s), dtype=np.complex128)
        idx = np.arange(s)
        for d in range(1, g):
            Mb[idx, (idx + d) % s] = rng.uniform(-1, 1, s)
        Mb = np.ascontiguousarray(Mb.ravel())
        st = prof(lambda: e.gemv_bsgs_batch(dout.data_ptr(), Mb, din.data_ptr(), cnt, lvl, rkb))
        # (the rescale's one ModDown launch stays in: there is no class of its own)
        rot = {k: v[1] for k, v in st.items() if not k.startswith(NOT_ROT)}
        up = sum(v for k, v in rot.items() if k.startswith(MODUP_CLASSES))
        out["batch"]["baby_stage"] = {"kernels": kernel_table(st), "rotation_us": round(sum(rot.values()), 1),
                                      "modup_us": round(up, 1),
                                      "modup_share": round(up / max(sum(rot.values()), 1e-9), 3)}
    else:
        calls = {k: min(200, max(3, math.ceil(args.window_s / wall(fn)))) for k, fn in legs.items()}
        us = {k: [] for k in legs}
        for _ in range(args.windows):
            for k, fn in legs.items():  # alternating the legs
                us[k].append(wall(lambda: [fn() for _ in range(calls[k])]) / calls[k] / cnt * 1e6)
        for k in legs:
            out[k].update(calls_per_window=calls[k], us_per_ct=[round(v, 1) for v in us[k]],
                          us_per_ct_best=round(min(us[k]), 1),
                          spread=round((max(us[k]) - min(us[k])) / min(us[k]), 4))
        out["batch_over_loop"] = round(out["loop"]["us_per_ct_best"] / out["batch"]["us_per_ct_best"], 3)
    for o in xs + ys + [pk, sk]:
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
    ap.add_argument("--batch", type=int, default=0, metavar="COUNT")
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--ab-tb", action="store_true", help="with --batch: legs with GPQHE_BSGS_INNER_TB forced to 8 and to 16")
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
        res.append((shape_batch if args.batch else shape)(e, np, f[0], int(f[1]), len(f) < 3 or f[2] != "bsgs", args))
    print(json.dumps({"prof": bool(args.prof), "batch": args.batch, "shapes": res}), flush=True)


if __name__ == "__main__":
    main()
