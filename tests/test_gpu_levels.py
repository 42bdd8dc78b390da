"""Every level of every parameter set through the key-switch kernels, product
(libgpqhe.so on MI355X) vs oracle, word for word.

The host dispatch picks its kernels from the level (tests/level_shapes.py: the
number of digits, the last digit's size, the conversion targets, the dropped
and kept slots and their arithmetic classes), and the other GPU tests pin only
the top of each chain and a few hand-picked levels below it.  Here one test
per parameter set generates the keys once, from one seed, on both engines,
loops over the levels and collects every failing (level, op, shape label); it
asserts once at the end, so a failure shows its pattern across the levels.

  a  he_mul_rescale_batch, levels 2..L, random residues, 3 pairs (the two
     streams' 1 + 2 split; 2 pairs at n = 2^17), and the squaring form (b the
     same pointer as a) at level 2 and at the highest level with a partial
     last digit;
  b  the single calls on imported random-residue ciphertexts: he_mul (1..L),
     he_mul_rescale out of place and in place, he_mul then he_rescale (2..L),
     he_rot by 1 and by slots - 1 (1..L);
  c  he_rot_batch (1..L) and he_gemv_batch (2..L), 16 slots, 2 genuine
     encryptions per level (1 at n = 2^17), the last one decoded against
     np.roll and M @ z, vectors and matrix sized so that a result fits one
     51-bit limb at Delta = 2^50 (level_shapes.sweep_vectors);
     the same matrix and keys walk down the levels and back up: the fold and
     diagonal caches are keyed by level, so the product's second visit of a
     level must give its first visit's bits (which are the oracle's);
  d  the batch families (BSGS, step, rows, packed, encrypted gains) at every
     level 2..L against their compositions on the oracle.

Path switches that only these sweeps reach: c5 at levels <= 8 (8 conversion
targets: ks_cols4_kernel with its own column INTT on a mixed prime set); c1
and bench at levels <= 3 (alpha = 1: from the streaming key switch and the
non-windowed rotation onto the split key switch and the windowed gemv); the
one-digit ksq_kernel forms at n = 2^14, 2^15 and 2^17 (levels <= alpha).

Every output array carries a fill value and guard words behind it that must
stay untouched.  Bits are exact; a decode passes within 1e-6 max(1, |want|)
(the oracle alone stays within 5e-11 at every level, tests/test_levels_cpu.py
bounds it by 1e-8).  he_mul at level 1 is not decoded: its scale exceeds q0.
The 2^17 sets run their levels as two to four tests (the oracle's time there;
level_shapes.PARTS); no level is left out."""
import ctypes

import numpy as np
import pytest

from tests import level_shapes as LS
from tests.test_gpu_parity import PARAMS, init_both, keys, same
from tests.test_gpu_rotations import encrypt_batch, init_slots, rot_keys

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 7


def cases(sweep):
    """(set, "first-last" levels) for every test of a sweep: one per set, the
    2^17 sets in several parts (level_shapes.PARTS)."""
    return [(name, f"{a}-{b}") for name in LS.SWEEPS[sweep][0]
            for a, b in LS.sweep_parts(sweep, name, PARAMS[name][1]["nlimbs"])]


def part_levels(sweep, name, part, L):
    assert L == PARAMS[name][1]["nlimbs"]
    a, b = (int(x) for x in part.split("-"))
    assert (a, b) in LS.sweep_parts(sweep, name, L)
    return list(range(a, b + 1))


def verdict(fails, name):
    assert not fails, f"{name}: {len(fails)} failing (level, op, shape):\n" + "\n".join(
        f"  level {lvl} {op}: {why} [{lab}]" for lvl, op, why, lab in fails)


def diff(got, want):
    """None, or what differs between two word arrays."""
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return None if bad.size == 0 else f"{bad.size} residues differ, first at word {int(bad[0])}"


def guarded(words):
    return np.full(words + GUARD, FILL, dtype=np.uint64)


def split_guard(buf, words):
    """(payload, None or a complaint about the guard words)."""
    ok = np.array_equal(buf[words:], np.full(GUARD, FILL, dtype=np.uint64))
    return buf[:words], None if ok else "guard words written"


def both(oracle, product, fn, ins, out_words, args, ko, kp, run_oracle=True):
    """fn(out, *args, key) on both engines; args name the input arrays of
    `ins` by their index as the strings "0", "1".  Returns (oracle words or
    None, product words, complaint or None); outputs filled and guarded,
    inputs checked unchanged on the device."""
    import torch
    want = None
    if run_oracle:
        buf = guarded(out_words)
        getattr(oracle.lib, fn)(buf.ctypes.data, *[ins[int(a)].ctypes.data if isinstance(a, str) else a for a in args],
                                ko)
        want, why = split_guard(buf, out_words)
        assert why is None, "oracle: " + why
    dins = [torch.from_numpy(x.view(np.int64)).cuda() for x in ins]
    dout = torch.full((out_words + GUARD,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    getattr(product.lib, fn)(dout.data_ptr(), *[dins[int(a)].data_ptr() if isinstance(a, str) else a for a in args], kp)
    product.sync()
    got, why = split_guard(dout.cpu().numpy().view(np.uint64), out_words)
    for d, h in zip(dins, ins):
        if not np.array_equal(d.cpu().numpy().view(np.uint64), h):
            why = why or "an input was written"
    return want, got, why


# --------------------------------------------------------------------------- a. he_mul_rescale_batch
def square_levels(e, levels):
    """Level 2 and the highest level whose last digit is partial (the top
    level where every digit is whole, as with alpha = 1)."""
    alpha = e.info.alpha
    partial = [x for x in levels if x % alpha]
    return {min(levels), max(partial) if partial else max(levels)}


@pytest.mark.parametrize("name,part", cases("mul_rescale_batch"))
def test_mul_rescale_batch_every_level(oracle, product, name, part):
    init_both(oracle, product, name)
    n = product.n
    cnt = 2 if product.info.logn >= 17 else 3
    rlk_o, rlk_p = keys(oracle, rot=False)[3], keys(product, rot=False)[3]
    same(oracle, product, rlk_o, rlk_p)
    levels = part_levels("mul_rescale_batch", name, part, product.L)
    squares = square_levels(product, levels)
    fails = []
    for lvl in levels:
        lab = LS.engine_label(product, lvl)
        a = np.zeros(cnt * 2 * lvl * n, dtype=np.uint64)
        b = np.zeros(cnt * 2 * lvl * n, dtype=np.uint64)
        oracle.lib.poly_fill_uniform(a.ctypes.data, 2 * cnt, lvl, 100 + lvl)
        oracle.lib.poly_fill_uniform(b.ctypes.data, 2 * cnt, lvl, 200 + lvl)
        forms = [("mul_rescale_batch", ("0", "1"))] + ([("square_batch", ("0", "0"))] if lvl in squares else [])
        for op, (ia, ib) in forms:
            want, got, why = both(oracle, product, "he_mul_rescale_batch", [a, b], cnt * 2 * (lvl - 1) * n,
                                  (ia, ib, cnt, lvl), ctypes.byref(rlk_o), ctypes.byref(rlk_p))
            why = why or diff(got, want)
            if why:
                fails.append((lvl, op, why, lab))
    for e, k in ((oracle, rlk_o), (product, rlk_p)):
        e.free(k)
    verdict(fails, name)


# --------------------------------------------------------------------------- b. the single calls
def genrot_keys(e, rots):
    """keypair, relinearisation key and the rotation keys `rots` only."""
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rlk = e.evk()
    e.genrlk(rlk, sk)
    rk = e.evks(e.slots)
    for r in rots:
        e.lib.he_genrot(ctypes.byref(rk[r]), r, ctypes.byref(sk))
    return pk, sk, rk, rlk


def single_ops(e, rk, rlk, wa, wb, lvl, rots):
    """{op: exported words} of the single calls on imports of wa, wb."""
    a, b = e.ct(), e.ct()
    e.import_(a, wa, lvl, scale=e.info.delta)
    e.import_(b, wb, lvl, scale=e.info.delta)
    assert a.nlimbs == lvl and b.nlimbs == lvl
    out = {}

    def keep(op, c, nl):
        assert c.nlimbs == nl, (op, c.nlimbs, nl)
        out[op] = e.export(c).copy()
        e.free(c)

    for r in rots:
        c = e.ct(); e.rot(c, a, r, rk); keep(f"rot{r}", c, lvl)
    c = e.ct(); e.mul(c, a, b, rlk); keep("mul", c, lvl)
    if lvl >= 2:
        c = e.ct(); e.mul_rescale(c, a, b, rlk); keep("mul_rescale", c, lvl - 1)
        c = e.ct(); e.copy_ct(c, a); e.mul_rescale(c, c, b, rlk); keep("mul_rescale_inplace", c, lvl - 1)
        c = e.ct(); e.mul(c, a, b, rlk); e.rescale(c); keep("mul_then_rescale", c, lvl - 1)
    e.free(a)
    e.free(b)
    return out


@pytest.mark.parametrize("name,part", cases("single"))
def test_single_calls_every_level(oracle, product, name, part):
    init_both(oracle, product, name)
    n, s = product.n, product.slots
    rots = (1, s - 1)
    ko, kp = genrot_keys(oracle, rots), genrot_keys(product, rots)
    same(oracle, product, ko[3], kp[3])
    for r in rots:
        same(oracle, product, ko[2][r], kp[2][r])
    fails = []
    for lvl in part_levels("single", name, part, product.L):
        lab = LS.engine_label(product, lvl)
        w = np.zeros(4 * lvl * n, dtype=np.uint64)
        oracle.lib.poly_fill_uniform(w.ctypes.data, 4, lvl, 300 + lvl)
        wa, wb = w[:2 * lvl * n], w[2 * lvl * n:]
        ro = single_ops(oracle, ko[2], ko[3], wa, wb, lvl, rots)
        rp = single_ops(product, kp[2], kp[3], wa, wb, lvl, rots)
        assert list(ro) == list(rp)
        for op in ro:
            why = diff(rp[op], ro[op])
            if why:
                fails.append((lvl, op, why, lab))
    for e, k in ((oracle, ko), (product, kp)):
        for o in (k[0], k[1], k[3]):
            e.free(o)
        e.free_evks(k[2])
    verdict(fails, name)


# --------------------------------------------------------------------------- c. he_rot_batch / he_gemv_batch
@pytest.mark.parametrize("name,part", cases("rot_gemv_batch"))
def test_rot_gemv_batch_every_level(oracle, product, name, part):
    s = 16
    init_slots(oracle, product, name, s, seed=31)
    n = product.n
    cnt = 1 if product.info.logn >= 17 else 2  # (the oracle's time at n = 2^17)
    ko, kp = rot_keys(oracle), rot_keys(product)
    for r in (1, s - 1):
        same(oracle, product, ko[2][r], kp[2][r])
    M = LS.sweep_matrix(s, 9)
    Mc = np.ascontiguousarray(M.ravel(), dtype=np.complex128)
    sk, delta = kp[1], product.info.delta
    levels = part_levels("rot_gemv_batch", name, part, product.L)
    first = {}  # (lvl, op) -> (input words, the first visit's bits)
    fails = []

    def decode(words, nl, lvl, want, op, lab):
        ct = product.ct()
        product.import_(ct, words, nl, scale=delta)
        err = np.abs(product.decrypt(ct, sk) - want).max()
        product.free(ct)
        if not err < 1e-6 * max(1.0, np.abs(want).max()):
            fails.append((lvl, op, f"decodes {err:.3g} away", lab))

    # down the levels against the oracle, then back up: the product alone
    # against what it gave the first time
    for visit, order in ((0, levels[::-1]), (1, levels[1:])):
        for lvl in order:
            lab = LS.engine_label(product, lvl)
            if visit == 0:
                zs = LS.sweep_vectors(cnt, s, 1000 + lvl)
                host = encrypt_batch(product, kp[0], zs, nlimbs=lvl)
            else:
                host, zs = first[lvl, "in"]
            calls = [(f"rot_batch{r}", "he_rot_batch", cnt * 2 * lvl * n, ("0", cnt, lvl, r)) for r in (1, s - 1)]
            if lvl >= 2:
                calls.append(("gemv_batch", "he_gemv_batch", cnt * 2 * (lvl - 1) * n, (Mc.ctypes.data, "0", cnt, lvl)))
            for op, fn, words, args in calls:
                want, got, why = both(oracle, product, fn, [host], words, args, ko[2], kp[2], run_oracle=visit == 0)
                if visit == 0:
                    first[lvl, op] = got
                    first[lvl, "in"] = (host, zs)
                    last = got.reshape(cnt, -1)[cnt - 1]
                    if fn == "he_rot_batch":
                        decode(last, lvl, lvl, np.roll(zs[cnt - 1], -args[3]), op + " decode", lab)
                    else:
                        decode(last, lvl - 1, lvl, M @ zs[cnt - 1], op + " decode", lab)
                else:
                    want, op = first[lvl, op], op + " (second visit)"
                why = why or diff(got, want)
                if why:
                    fails.append((lvl, op, why, lab))
    for e, k in ((oracle, ko), (product, kp)):
        e.free(k[0])
        e.free(k[1])
        e.free_evks(k[2])
    verdict(fails, name)


# --------------------------------------------------------------------------- d. the batch families
# One shape per family, 16-slot loops, 2 ciphertexts, through the families'
# own helpers (keys once per set and family, inputs the product's encryptions
# taken down to the level, the oracle's composition, guard words, decodes).
# Every family has its keys and plans at every level from 2 up: the rotation
# keys are generated over the whole chain and folded per level on demand, the
# row folds run one level down (level 1 at the lowest), and the encrypted
# gains are encrypted at the level of the call.  Level 1 has no product to
# rescale, so none of the calls accepts it.
# The matrices are the helpers' (entries of modulus up to sqrt(2)) over 4 s: a
# step's result up = uhat - (A (xhat - xr) + B (uhat - ur)) on their vectors
# (|z| <= sqrt(2)) then stays below sqrt(2) + 2 = 3.42, inside the 4.0 that one
# limb of f13 holds (q0 / 2 Delta: a coefficient is at most Delta max|z|).
def scaled(M, s):
    return np.asarray(M) / (4 * s)


def family_bsgs(oracle, product, name):
    from tests.test_gpu_bsgs import matrix
    from tests.test_gpu_bsgs_batch import Pair, vectors
    s, g, cnt = 16, 4, 2
    pr = Pair(oracle, product, name, s, g)
    M = scaled(matrix(s, 3 * s + g), s)

    def bsgs(lvl):
        pr.check(("levels", name, lvl), M, vectors(s, cnt, lvl), lvl)

    return pr, [("gemv_bsgs_batch", bsgs)]


def family_step(oracle, product, name):
    from tests.test_gpu_step_batch import StepPair, matrices
    s, g, cnt = 16, 4, 2
    pr = StepPair(oracle, product, name, s, g)
    Ma, Mb = (scaled(m, s) for m in matrices(s, g))

    def step(lvl):
        zs, H, scale = pr.blocks(s, cnt, lvl, lvl)
        pr.check_step(("levels", name, lvl), Ma, Mb, zs, H, lvl, scale)

    return pr, [("hempc_step_batch", step)]


def family_rows(oracle, product, name):
    from tests.test_gpu_rows_batch import RowsPair, matrices
    s, rows, cnt = 16, 2, 2
    pr = RowsPair(oracle, product, name, s, rows)
    Ma, Mb = (scaled(m, s) for m in matrices(s, rows))

    def step(lvl):
        zs, H, scale = pr.blocks(s, cnt, lvl, lvl)
        pr.check_step(("levels", name, lvl), Ma, Mb, zs, H, lvl, scale)

    return pr, [("hempc_step_rows_batch", step)]


def family_packed(oracle, product, name):
    from tests.test_gpu_packed_batch import PackedPair, matrices
    S, s, rows, cnt = 64, 16, 2, 2
    pr = PackedPair(oracle, product, name, S, s, rows)
    Ma, Mb = (scaled(m, s) for m in matrices(S // s, rows, s))

    def step(lvl):
        zs, H, scale = pr.blocks(S, cnt, lvl, lvl)
        pr.check_step(("levels", name, lvl), Ma, Mb, zs, H, lvl, scale)

    return pr, [("hempc_step_packed_batch", step)]


def family_encgain(oracle, product, name):
    from tests.test_gpu_encgain_batch import GainPair
    from tests.test_gpu_packed_batch import matrices
    S, s, rows, cnt = 64, 16, 2, 2
    pr = GainPair(oracle, product, name, S, s, rows)
    Ma, Mb = (scaled(m, s) for m in matrices(S // s, rows, s))

    def step(lvl):
        DA, DB = pr.gains(Ma, lvl), pr.gains(Mb, lvl)  # (encrypted at the level of the call)
        zs, H, scale = pr.blocks(S, cnt, lvl, lvl)
        pr.check(("levels", name, lvl), Ma, Mb, DA, DB, zs, H, lvl, scale)

    return pr, [("hempc_step_encgain_packed_batch", step)]


FAMILIES = {"bsgs": family_bsgs, "step": family_step, "rows": family_rows, "packed": family_packed, "encgain": family_encgain}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", LS.SWEEPS["families"][0])
def test_batch_families_every_level(oracle, product, name, family):
    pr, ops = FAMILIES[family](oracle, product, name)
    fails = []
    for lvl in LS.sweep_levels("families", name, product.L):
        lab = LS.engine_label(product, lvl)
        for op, fn in ops:
            try:
                fn(lvl)
            except AssertionError as ex:
                fails.append((lvl, op, str(ex).splitlines()[0] if str(ex) else "assertion", lab))
    pr.close()
    verdict(fails, name)
