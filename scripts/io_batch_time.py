"""Time he_enc_pk_batch and he_dec_dcd_batch against the loops over the public
single calls they replace, on one MI355X.

python scripts/io_batch_time.py [--shapes bench51:16,f13:16] [--counts 16,256] [--rounds 3]
                                [--out profiles/io_batch_time.json]
Per shape and count, in one process, four legs alternate in device-synchronised
rounds (times are per ciphertext, best and all rounds kept):
  enc_batch  one he_enc_pk_batch of COUNT vectors at the top level L into a
             device array [COUNT][2][L][n];
  enc_loop   the cheapest loop over the public single calls that fills the same
             array: he_ecd_ex, he_enc_pk and he_export per ciphertext into one
             host buffer, then one upload through torch;
  dec_batch  one he_dec_dcd_batch of a device array [COUNT][2][L - 1][n] (real
             encryptions at level L - 1, the level he_gemv_batch returns);
  dec_loop   one download of that array, then he_import, he_dec and he_dcd_ex
             per ciphertext.
The single calls are not changed by the batch entry points, so the loops are
what the library offered before them.  Then, outside the timing, the per-class
gpqhe_prof_collect table of one warm call of each batch leg, and of it
dec_fold_kernel's achieved bytes/s beside the read8 / copy8 rates of
scripts/ubench_mem (built beforehand: hipcc --offload-arch=gfx950 -O3
scripts/ubench_mem.hip -o scripts/ubench_mem) run as a child process in the
same job.  Writes one JSON document to --out and prints a one-line summary.
Fails without a GPU (the product library has no CPU path).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_table(st):
    return {k: {"launches": v[0], "us": round(v[1], 1), "GBs": round(v[2] / v[1] / 1e3, 1)}
            for k, v in sorted(st.items(), key=lambda kv: -kv[1][1]) if v[1] > 0}


def shape(e, np, torch, name, slots, cnt, rounds):
    from tests.test_gpu_parity import PARAMS
    e.init_params(**dict(PARAMS[name][1], slots=slots))
    e.set_seed(5)
    n, L, scale = e.n, e.L, e.info.delta
    out = {"set": name, "n": n, "L": L, "slots": slots, "count": cnt, "enc_level": L, "dec_level": L - 1}
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(1)
    zs = rng.uniform(-1, 1, (cnt, slots)) + 1j * rng.uniform(-1, 1, (cnt, slots))
    x = torch.zeros(cnt * 2 * L * n, dtype=torch.int64, device="cuda")
    y = torch.zeros(cnt * 2 * (L - 1) * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.enc_pk_batch(y.data_ptr(), zs, pk, slots, scale, L - 1)
    e.sync()
    host = torch.empty(cnt * 2 * L * n, dtype=torch.int64).pin_memory()
    hview = host.numpy().view(np.uint64).reshape(cnt, -1)
    pt, ct = e.pt(), e.ct()
    res = {}

    def enc_loop():
        from hectr_amd.gpqhe import U64P
        import ctypes as C
        for i in range(cnt):
            e.ecd_ex(pt, zs[i], slots, scale, L)
            e.enc_pk(ct, pt, pk)
            e.lib.he_export(C.byref(ct), hview[i].ctypes.data_as(U64P))
        x.copy_(host, non_blocking=True)
        torch.cuda.synchronize()

    def dec_loop():
        yh = y.cpu().numpy().view(np.uint64).reshape(cnt, -1)
        z = np.empty((cnt, slots), dtype=np.complex128)
        for i in range(cnt):
            e.import_(ct, yh[i], L - 1, scale=scale)
            e.dec(pt, ct, sk)
            z[i] = e.dcd(pt, slots)
        res["dec_loop"] = z

    def dec_batch():
        res["dec_batch"] = e.dec_dcd_batch(y.data_ptr(), cnt, L - 1, scale, sk, slots)

    legs = {"enc_batch": lambda: e.enc_pk_batch(x.data_ptr(), zs, pk, slots, scale, L), "enc_loop": enc_loop,
            "dec_batch": dec_batch, "dec_loop": dec_loop}

    def wall(fn):
        e.sync()
        t0 = time.perf_counter()
        fn()
        e.sync()
        return time.perf_counter() - t0

    for k, fn in legs.items():
        out[k] = {"first_call_s": round(wall(fn), 4)}
    out["dec_batch_equals_loop"] = bool(np.array_equal(res["dec_batch"].view(np.uint64),
                                                       res["dec_loop"].view(np.uint64)))
    out["dec_max_err"] = float(np.abs(res["dec_batch"] - zs).max())
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():  # alternating the legs
            reps = 5 if k.endswith("batch") else 1
            us[k].append(wall(lambda: [fn() for _ in range(reps)]) / reps / cnt * 1e6)
    for k in legs:
        out[k].update(us_per_ct=[round(v, 2) for v in us[k]], us_per_ct_best=round(min(us[k]), 2),
                      spread=round((max(us[k]) - min(us[k])) / min(us[k]), 4))
    for a in ("enc", "dec"):
        out[a + "_loop_over_batch"] = round(out[a + "_loop"]["us_per_ct_best"] / out[a + "_batch"]["us_per_ct_best"], 2)
    # one warm call of each batch leg by kernel class (a pass of its own: the
    # events around every launch perturb the timing)
    e.prof_enable(True)
    for k in ("enc_batch", "dec_batch"):
        e.prof_collect()
        legs[k]()
        out[k]["kernels"] = kernel_table(e.prof_collect())
    e.prof_enable(False)
    for o in (pt, ct, pk, sk):
        e.free(o)
    e.exit()
    return out


def ubench_mem():
    exe = os.path.join(ROOT, "scripts", "ubench_mem")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True)
    rows = [line.split() for line in r.stdout.splitlines() if line.strip()]
    return {f[0]: float(f[1]) for f in rows if len(f) >= 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench51:16,f13:16")
    ap.add_argument("--counts", default="16,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "io_batch_time.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("io_batch_time.py needs an MI355X")
    from hectr_amd.gpqhe import Engine
    e = Engine.product()
    shapes = []
    for spec in args.shapes.split(","):
        name, slots = spec.split(":")
        for cnt in args.counts.split(","):
            shapes.append(shape(e, np, torch, name, int(slots), int(cnt), args.rounds))
    del e
    doc = {"rounds": args.rounds, "shapes": shapes, "ubench_mem_GBs": ubench_mem()}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "shapes": [
        {k: s[k] for k in ("set", "count", "enc_loop_over_batch", "dec_loop_over_batch", "dec_batch_equals_loop")}
        for s in shapes]}), flush=True)


if __name__ == "__main__":
    main()
