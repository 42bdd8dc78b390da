"""Small-N step sequences shared by the GPU parity tests and the switch worker.

Each function drives one engine (product or oracle) through a sequence of
HECTR-style control-step calls and returns every exported object and decoded
vector in call order; the tests compare the two engines' lists bit for bit.
The sequences follow the reference's regulator step: encode + encrypt the
state (src/ctr.c:461-480), he_sub x2, he_gemv x2, he_add / he_neg
(src/hempc.c:253-266), decrypt + decode (src/ctr.c:486-490).

Every sequence takes `params` (hectx_init's arguments; PARAMS_REF, HECTR's own,
by default; PARAMS_RINGS holds the other rings the tests run) and `plain`: a
list that receives, for every decoded vector of the result, its index there and
the value the plaintext step gives.
"""
import numpy as np

PARAMS_REF = dict(logn=12, logq=109, slots=16, log_delta=50)  # src/ctr.c:514-518
# The other rings of the small-N path (every sequence takes `params`): the
# other two rungs of the fused kernels' ring-size ladders, inside the
# speculation gate (10 <= logn <= 12); HECTR's ring with a longer chain (L = 4:
# past the fused kernels' two-limb forms); and logn = 9, just outside the
# gate (the oracle only: the product has no decode below n = 2^10,
# tests/test_gpu_small_rings.py).
PARAMS_RINGS = {
    "n2048": dict(logn=11, logq=109, slots=16, log_delta=50),
    "n1024": dict(logn=10, logq=109, slots=16, log_delta=50),
    "n4096_L4": dict(logn=12, logq=209, slots=16, log_delta=50),
    "n512": dict(logn=9, logq=109, slots=16, log_delta=50),
}
# he_gemv calls an "evict" step of speculative_gemvs adds.  Under a 5 MiB
# diagonal cache: the first is queued (cache at 4.5 MiB), the second runs
# unqueued and clears the cache at its sixth diagonal, the third and fourth are
# queued into freed 1.5 MiB blocks, the fifth runs unqueued again.
EVICT_EXTRAS = 5


def note(plain, res, want):
    """plain (a caller's list, or None) gets (index in res, plaintext value)
    of the decoded vector just appended to res."""
    if plain is not None:
        plain.append((len(res) - 1, want))


def keys(e, rot=True):
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = None
    if rot:
        rk = e.evks(e.slots)
        e.genrk(rk, sk)
    return pk, sk, rk


def speculative_noise(e, seed=1234, rng_seed=9, params=PARAMS_REF, plain=None):
    """Steps of 5 encryptions (HECTR's), then 3 (a prefix of the speculated
    streams), 6 (more than speculated), one with a live plaintext, one at a
    lower level, a reseed between steps (api.cpp SpecNoise)."""
    e.init(**params)
    e.set_seed(seed)
    rng = np.random.default_rng(rng_seed)
    plan = [5, 5, 3, 6, "live", "lvl1", "reseed", 5, 5]
    zs = [[rng.uniform(-1, 1, e.slots) + 0j for _ in range(6)] for _ in plan]
    pk, sk, _ = keys(e, rot=False)
    res = []
    for kind, zz in zip(plan, zs):
        if kind == "reseed":
            e.set_seed(77)
            continue
        cnt = kind if isinstance(kind, int) else 2
        lvl = 1 if kind == "lvl1" else e.L
        pts, cts = [], []
        for z in zz[:cnt]:
            pt = e.pt()
            e.ecd_ex(pt, z, e.slots, e.info.delta, lvl)
            pts.append(pt)
        for pt in pts:
            ct = e.ct()
            e.enc_pk(ct, pt, pk)
            cts.append(ct)
        if kind == "live":
            res.append(e.export(pts[0]))
        for pt in pts:
            e.free(pt)
        d = e.ct()
        e.sub(d, cts[0], cts[1])
        res += [e.export(x) for x in cts + [d]]
        res.append(e.decrypt(d, sk))  # he_dcd: the next step's noise is launched behind it
        note(plain, res, zz[0] - zz[1])
        for x in cts + [d]:
            e.free(x)
    return res


def queued_differences(e, seed=1234, rng_seed=31, params=PARAMS_REF, plain=None):
    """HECTR's regulator step repeated (api.cpp ew_lazy_sub: from the second
    step on the subs stay queued and gemv_inner_kernel forms the differences
    from their operands).  Variants per step: the differences freed unread,
    read back after the gemvs, an operand of a sub overwritten after the
    gemvs, an in-place he_gemv(x, M, x), a gemv whose output is an operand of
    the queued sub, and a non-speculated step (four encryptions)."""
    e.init(**params)
    e.set_seed(seed)
    rng = np.random.default_rng(rng_seed)
    s = e.slots
    M1 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    M2 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    plan = ["free", "free", "read", "free", "clobber", "free", "inplace", "free", "ycts", "free", "four", "free",
            "free"]
    zs = [[rng.uniform(-1, 1, s) + 0j for _ in range(5)] for _ in plan]
    pk, sk, rk = keys(e, rot=True)
    res = []
    for kind, zz in zip(plan, zs):
        cnt = 4 if kind == "four" else 5
        cts = [e.encrypt(z, pk) for z in zz[:cnt]]
        xd, ud = e.ct(), e.ct()
        e.sub(xd, cts[0], cts[1])
        e.sub(ud, cts[2], cts[3])
        if kind == "inplace":  # he_gemv(x, M, x): the output is the queued sub's output
            ya = xd
        elif kind == "ycts":  # the output is an operand of the queued sub
            ya = cts[0]
        else:
            ya = e.ct()
        yb = e.ct()
        e.gemv(ya, M1.ravel(), xd, rk)
        e.gemv(yb, M2.ravel(), ud, rk)
        du = e.ct()
        e.add(du, ya, yb)
        e.neg(du)
        if kind == "read":
            res += [e.export(xd), e.export(ud)]
        if kind == "clobber":
            e.add(cts[0], cts[0], cts[1])  # an operand of the first sub
            res.append(e.export(cts[0]))
        res += [e.export(ya), e.export(yb), e.export(du)]
        for x in (xd, ud, yb) + (() if kind in ("inplace", "ycts") else (ya,)):
            e.free(x)
        res.append(e.decrypt(du, sk))
        note(plain, res, -(M1 @ (zz[0] - zz[1]) + M2 @ (zz[2] - zz[3])))
        for x in cts + [du]:
            e.free(x)
    return res


def rekeyed_steps(e, seed=1234, rng_seed=41, params=PARAMS_REF, plain=None):
    """The regulator step with the public key changing between speculative
    steps (api.cpp SpecModup is keyed on the public key's block): two steps
    on key A; A freed and a new key C generated (its block may be A's); steps
    on C; then keys B and C alternating step by step."""
    e.init(**params)
    e.set_seed(seed)
    rng = np.random.default_rng(rng_seed)
    s = e.slots
    M1 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    M2 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    ks = {"A": keys(e), "B": keys(e)}
    plan = ["A", "A", "newC", "C", "C", "B", "C", "B", "C", "C"]
    zs = [[rng.uniform(-1, 1, s) + 0j for _ in range(5)] for _ in plan]
    res = []
    for kind, zz in zip(plan, zs):
        if kind == "newC":
            pk, sk, rk = ks.pop("A")
            e.free(pk)
            e.free(sk)
            e.free_evks(rk)
            ks["C"] = keys(e)
            kind = "C"
        pk, sk, rk = ks[kind]
        cts = [e.encrypt(z, pk) for z in zz]
        xd, ud, ya, yb, du = e.ct(), e.ct(), e.ct(), e.ct(), e.ct()
        e.sub(xd, cts[0], cts[1])
        e.sub(ud, cts[2], cts[3])
        e.gemv(ya, M1.ravel(), xd, rk)
        e.gemv(yb, M2.ravel(), ud, rk)
        e.add(du, ya, yb)
        e.neg(du)
        res += [e.export(ya), e.export(yb), e.export(du)]
        for x in (xd, ud, ya, yb):
            e.free(x)
        res.append(e.decrypt(du, sk))
        note(plain, res, -(M1 @ (zz[0] - zz[1]) + M2 @ (zz[2] - zz[3])))
        for x in cts + [du]:
            e.free(x)
    return res


def speculative_gemvs(e, seed=1234, rng_seed=53, plan=None, taken=None, params=PARAMS_REF, plain=None):
    """HECTR's step with its own call order (all five encodes, all five
    encryptions, the plaintexts freed: src/ctr.c:461-480, which starts the
    early combine and, from the third step on, the speculated gemvs of the
    last step's pattern, api.cpp SpecGemv), and steps where the speculation
    must not be taken: a gemv matrix that changed, the subtraction's operands
    swapped, an encryption overwritten before its he_sub, the gemvs in the
    other order, the rotation keys regenerated in place, and one gemv only.
    "evict" / "evict_ct": the normal step, then in the same step EVICT_EXTRAS
    more he_gemv calls with fresh dense matrices, on ud / on an encryption (which
    records no speculation pattern), into ciphertexts exported at the end:
    with a small diagonal cache (GPQHE_DIAG_MIB) they clear it and take the
    freed blocks while the next step's speculation records point there.
    taken: a list that gets gpqhe_spec_gemv_taken() after every step."""
    e.init(**params)
    e.set_seed(seed)
    rng = np.random.default_rng(rng_seed)
    s = e.slots
    M1 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    M2 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    M3 = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
    plan = plan or ["same", "same", "same", "newM", "same", "swap", "same", "clobber", "same", "order", "same",
                    "regen", "same", "one", "same", "same"]
    zs = [[rng.uniform(-1, 1, s) + 0j for _ in range(5)] for _ in plan]
    pk, sk, rk = keys(e, rot=True)
    res, keep = [], []
    for kind, zz in zip(plan, zs):
        if kind == "regen":
            e.genrk(rk, sk)
        pts = []
        for z in zz:
            pt = e.pt()
            e.ecd(pt, z)
            pts.append(pt)
        cts = []
        for pt in pts:
            ct = e.ct()
            e.enc_pk(ct, pt, pk)
            cts.append(ct)
        for pt in pts:
            e.free(pt)
        if kind == "clobber":
            e.add(cts[1], cts[1], cts[4])
        xd, ud, ya, yb, du = e.ct(), e.ct(), e.ct(), e.ct(), e.ct()
        if kind == "swap":
            e.sub(xd, cts[2], cts[1])
        else:
            e.sub(xd, cts[1], cts[2])
        e.sub(ud, cts[3], cts[4])
        Ma = M3 if kind == "newM" else M1
        if kind == "order":
            e.gemv(yb, M2.ravel(), ud, rk)
            e.gemv(ya, Ma.ravel(), xd, rk)
        elif kind == "one":
            e.gemv(ya, Ma.ravel(), xd, rk)
            e.copy_ct(yb, ya)
        elif kind == "realias":
            # the speculated result freed and its block (likely) handed to a
            # gemv that is not speculated (another matrix), whose queued launch
            # writes it before the tail reads it (SpecDcd must not replay)
            e.gemv(ya, Ma.ravel(), xd, rk)
            e.gemv(yb, M2.ravel(), ud, rk)
            e.free(ya)
            ya = e.ct()
            e.gemv(ya, M3.ravel(), ud, rk)
        else:
            e.gemv(ya, Ma.ravel(), xd, rk)
            e.gemv(yb, M2.ravel(), ud, rk)
        if kind in ("evict", "evict_ct"):
            for _ in range(EVICT_EXTRAS):
                Me = (rng.uniform(-1, 1, (s, s)) + 0j).astype(np.complex128)
                keep.append(e.ct())
                e.gemv(keep[-1], Me.ravel(), ud if kind == "evict" else cts[0], rk)
        e.add(du, ya, yb)
        e.neg(du)
        e.add(du, du, cts[0])
        # (exported after the last step: an export runs every queue and
        # forgets the speculation records, as any non-queued call does)
        keep += [ya, yb, du]
        for x in (xd, ud):
            e.free(x)
        res.append(e.decrypt(du, sk))
        if plain is not None:
            z1 = zz[1] + zz[4] if kind == "clobber" else zz[1]
            pxd = zz[2] - z1 if kind == "swap" else z1 - zz[2]
            pud = zz[3] - zz[4]
            pya = M3 @ pud if kind == "realias" else Ma @ pxd
            pyb = pya if kind == "one" else M2 @ pud
            note(plain, res, zz[0] - (pya + pyb))
        for x in cts:
            e.free(x)
        if taken is not None and hasattr(e.lib, "gpqhe_spec_gemv_taken"):
            taken.append(int(e.lib.gpqhe_spec_gemv_taken()))
    res += [e.export(x) for x in keep]
    return res


SEQUENCES = {"speculative_noise": speculative_noise, "queued_differences": queued_differences,
             "rekeyed_steps": rekeyed_steps, "speculative_gemvs": speculative_gemvs}


def mismatches(a, b):
    """Indices where two sequence results differ (a length mismatch is one)."""
    if len(a) != len(b):
        return [-1]
    return [i for i, (x, y) in enumerate(zip(a, b)) if not np.array_equal(x, y)]


def cache_evictions(ora, prod):
    """speculative_gemvs with the diagonal cache cleared in the fifth step
    (run with GPQHE_DIAG_MIB=5: a dense 16-slot matrix's diagonals are
    1.5 MiB at PARAMS_REF), once per evict kind: the objects differing from
    the oracle's, and the product's speculated-gemv count after every step."""
    out = {}
    for kind in ("evict", "evict_ct"):
        plan = ["same"] * 4 + [kind] + ["same"] * 6
        taken = []
        want = speculative_gemvs(ora, plan=plan)
        got = speculative_gemvs(prod, plan=plan, taken=taken)
        out[kind] = {"diff": mismatches(want, got), "taken": taken}
    return out
