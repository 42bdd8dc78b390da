"""The packed step with encrypted gains (include/gpqhe_ext_encgain_batch.h)
without a GPU: the header, the binding's table, the libraries' exports, and the
yardstick the GPU tests compare against -- tests/encgain_ref on the oracle: it
decodes, loop by loop, to each loop's own (Ma_p za_p + Mb_p zb_p)[:rows] and
the step likewise; encryptions of all-zero diagonals give 0 and uhat; one
loop's matrix moves only that loop; its diagonals are packed_diagonals with the
zero ones kept."""
import re
import subprocess

import numpy as np
import pytest

from hectr_amd import gpqhe
from tests.encgain_ref import (enc_gain_compose, gain_diagonals, gemv2_encgain_compose, gemv2_encgain_per_term,
                               step_encgain_compose)
from tests.packed_ref import deinterleave, expected_packed, packed_diagonals
from tests.rows_ref import pow2
from tests.test_abi import exported
from tests.test_packed_batch_cpu import loop_errors, loop_mats, setup, teardown

ROOT = gpqhe.ROOT
ENCGAIN = ("he_enc_gain_packed_batch", "he_gemv2_encgain_packed_batch", "he_hempc_step_encgain_packed_batch")


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_encgain_header_is_pure_c_and_guarded(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "gpqhe_ext_encgain_batch.h"\n#include "gpqhe_ext_encgain_batch.h"\n#include "gpqhe_ext_batch.h"\n'
        "void (*e)(uint64_t *, const gpqhe_complex_t[], unsigned int, unsigned int, unsigned int, unsigned int,"
        " const he_pk_t *) = he_enc_gain_packed_batch;\n"
        "void (*f)(uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, size_t,"
        " unsigned int, const he_evk_t[], const he_evk_t *, unsigned int, unsigned int)"
        " = he_gemv2_encgain_packed_batch;\n"
        "void (*s)(uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *,"
        " const uint64_t *, const uint64_t *, size_t, unsigned int, const he_evk_t[], const he_evk_t *,"
        " unsigned int, unsigned int) = he_hempc_step_encgain_packed_batch;\n"
        "unsigned int (*g)(void) = he_gemv_bsgs_default_g;\n"  # (it includes gpqhe_ext.h)
        "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Wpedantic", "-Wshadow", "-Werror", "-I",
                    str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_encgain_header_declares_the_binding():
    inc = ROOT / "include"
    batch = (inc / "gpqhe_ext_batch.h").read_text()
    assert '#include "gpqhe_ext_encgain_batch.h"' in batch
    assert batch.index('"gpqhe_ext_packed_batch.h"') < batch.index('"gpqhe_ext_encgain_batch.h"')
    text = re.sub(r"/\*.*?\*/", "", (inc / "gpqhe_ext_encgain_batch.h").read_text(), flags=re.S)
    names = {n for n in re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", text) if n.startswith(("he_", "gpqhe_"))}
    assert names == set(ENCGAIN) == set(gpqhe.PRODUCT_EXT_ENCGAIN_BATCH)
    others = (set(gpqhe.PRODUCT_EXT) | set(gpqhe.PRODUCT_EXT_BATCH) | set(gpqhe.PRODUCT_EXT_IO_BATCH) |
              set(gpqhe.PRODUCT_EXT_STEP_BATCH) | set(gpqhe.PRODUCT_EXT_ROWS_BATCH) |
              set(gpqhe.PRODUCT_EXT_PACKED_BATCH) | set(gpqhe.EXPORTED))
    assert not names & others


def test_product_exports_them_and_the_oracle_does_not():
    assert gpqhe.PRODUCT_LIB.exists(), "product library not built (run __graft_entry__.build())"
    assert set(ENCGAIN) <= exported(gpqhe.PRODUCT_LIB)
    assert not set(ENCGAIN) & exported(gpqhe.ORACLE_LIB)


def test_engine_methods_need_the_symbols():
    e = gpqhe.Engine.oracle()
    with pytest.raises(AttributeError, match="he_enc_gain_packed_batch"):
        e.enc_gain_packed_batch(0, [0j], None, 16, 1, 2)
    with pytest.raises(AttributeError, match="he_gemv2_encgain_packed_batch"):
        e.gemv2_encgain_packed_batch(0, 0, 0, 0, 0, 0, 2, None, None, 16, 1)
    with pytest.raises(AttributeError, match="he_hempc_step_encgain_packed_batch"):
        e.hempc_step_encgain_packed_batch(0, 0, 0, 0, 0, 0, 0, 0, 2, None, None, 16, 1)


def test_reference_diagonals_keep_the_zero_ones():
    S, s, rows, P = 64, 16, 3, 4
    M = loop_mats(P, rows, s, 5)
    for i in range(s):  # E_1 of every loop: entries [r][(k + 1) mod s], k mod m' = r
        if i % 4 < rows:
            M[:, i % 4, (i + 1) % s] = 0
    nz = packed_diagonals(M, S, s, rows, P)
    assert sorted(nz) == [0, 2, 3]
    E = gain_diagonals(M, S, s, rows, P)
    assert E.shape == (pow2(rows), S) and not E[1].any()
    for i, d in nz.items():
        assert np.array_equal(E[i], d)
    assert gain_diagonals(np.zeros_like(M), S, s, rows, P).shape == (4, S)


def with_gains(e, pk, sk, Ma, Mb, s, rows, nmat, lvl):
    rlk = e.evk()
    e.genrlk(rlk, sk)
    return rlk, enc_gain_compose(e, Ma, pk, s, rows, nmat, lvl), enc_gain_compose(e, Mb, pk, s, rows, nmat, lvl)


CASES = [("ref", 64, 16, 2), ("ref", 2048, 16, 3), ("hyb", 128, 32, 2)]


@pytest.mark.parametrize("name,S,s,rows", CASES)
def test_reference_decodes_per_loop(oracle, name, S, s, rows):
    """Random real matrices (one per loop) and vectors in [-1, 1]; the lazy
    form's own error and the per-term form's are printed."""
    e, P = oracle, S // s
    pk, sk, rk, zs, cts = setup(e, name, S, s, rows)
    Ma, Mb = loop_mats(P, rows, s, 7 * S + rows), loop_mats(P, rows, s, 9 * S + rows)
    lvl, scale = cts[0].nlimbs, cts[0].scale
    rlk, DA, DB = with_gains(e, pk, sk, Ma, Mb, s, rows, P, lvl)
    assert len(DA) == len(DB) == pow2(rows) and all(d.nlimbs == lvl for d in DA + DB)
    y = gemv2_encgain_compose(e, DA, cts[0], DB, cts[1], rk, rlk, s, rows)
    assert y.nlimbs == lvl - 1 and np.isclose(y.scale, scale, rtol=1e-12)
    want = expected_packed(Ma, zs[0], Mb, zs[1], s, rows, P)
    got = e.decrypt(y, sk)
    err, scl = loop_errors(got, want, P, rows)
    yt = gemv2_encgain_per_term(e, DA, cts[0], DB, cts[1], rk, rlk, s, rows)
    all_lazy, all_term = np.abs(got - want).max(), np.abs(e.decrypt(yt, sk) - want).max()
    print(f"gemv2_encgain_compose {name} S={S} s={s} rows={rows}: worst loop error {err.max():.3e}, "
          f"all slots lazy {all_lazy:.3e} per-term {all_term:.3e}")
    assert (err < 1e-6 * scl).all()
    assert all_lazy < 1e-6 * max(1.0, np.abs(want).max())  # the periodic copies and zeros too
    up = step_encgain_compose(e, DA, DB, *cts, rk, rlk, s, rows)
    assert up.nlimbs == lvl - 1 and np.isclose(up.scale, scale, rtol=1e-12)
    xhat, xr, uhat, ur = zs
    want = uhat - expected_packed(Ma, xhat - xr, Mb, uhat - ur, s, rows, P)
    err, scl = loop_errors(e.decrypt(up, sk), want, P, rows)
    print(f"step_encgain_compose {name} S={S} s={s} rows={rows}: worst loop error {err.max():.3e}")
    assert (err < 1e-6 * scl).all()
    e.free(rlk)
    teardown(e, pk, sk, rk, cts + [y, yt, up] + DA + DB)


def test_zero_diagonals_and_one_loops_matrix(oracle):
    e, S, s, rows = oracle, 64, 16, 3
    P = S // s
    pk, sk, rk, zs, cts = setup(e, "ref", S, s, rows)
    lvl = cts[0].nlimbs
    Ma, Mb = loop_mats(P, rows, s, 321), loop_mats(P, rows, s, 322)
    rlk, DA, DB = with_gains(e, pk, sk, Ma, Mb, s, rows, P, lvl)
    y = gemv2_encgain_compose(e, DA, cts[0], DB, cts[1], rk, rlk, s, rows)
    # changing one loop's matrix moves only that loop beyond the bound
    Ca = Ma.copy()
    Ca[2] = loop_mats(1, rows, s, 323)[0]
    DC = enc_gain_compose(e, Ca, pk, s, rows, P, lvl)
    y2 = gemv2_encgain_compose(e, DC, cts[0], DB, cts[1], rk, rlk, s, rows)
    d = np.abs(deinterleave(e.decrypt(y2, sk), P, rows) - deinterleave(e.decrypt(y, sk), P, rows)).max(axis=1)
    assert d[2] > 1e-3 and (np.delete(d, 2) < 1e-6).all(), d
    # encryptions of all-zero diagonals: ciphertexts like any other; the product
    # part decodes to 0 and the step to uhat
    Z = np.zeros_like(Ma)
    ZA, ZB = enc_gain_compose(e, Z, pk, s, rows, P, lvl), enc_gain_compose(e, Z, pk, s, rows, P, lvl)
    assert all(e.export(d).any() for d in ZA + ZB)
    y0 = gemv2_encgain_compose(e, ZA, cts[0], ZB, cts[1], rk, rlk, s, rows)
    assert e.export(y0).any() and np.abs(e.decrypt(y0, sk)).max() < 1e-6
    up = step_encgain_compose(e, ZA, ZB, *cts, rk, rlk, s, rows)
    assert np.abs(deinterleave(e.decrypt(up, sk), P, rows) - deinterleave(zs[2], P, rows)).max() < 1e-6
    e.free(rlk)
    teardown(e, pk, sk, rk, cts + [y, y2, y0, up] + DA + DB + DC + ZA + ZB)
