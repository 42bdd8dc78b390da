"""he_genrk_rows / he_gemv2_rows_batch / he_hempc_step_rows_batch without a GPU:
the header (include/gpqhe_ext_rows_batch.h), the binding's table, the
libraries' exports, the rotation lists, and the yardstick the GPU tests compare
against -- tests/rows_ref.gemv2_rows_compose on the oracle: it decodes to the
leading rows of Ma za + Mb zb repeated with period m', with rows = slots it is
bsgs_compose(g = slots) bit for bit, and it reads no row past `rows`."""
import re
import subprocess

import numpy as np
import pytest

from hectr_amd import gpqhe
from tests.bsgs_ref import bsgs_compose
from tests.rows_ref import expected_rows, gemv2_rows_compose, rows_keys, rows_rotations, step_rows_compose
from tests.test_abi import exported
from tests.test_bsgs_cpu import matrix

ROOT = gpqhe.ROOT
ROWS = ("he_genrk_rows", "he_gemv2_rows_batch", "he_hempc_step_rows_batch")


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_rows_header_is_pure_c_and_guarded(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "gpqhe_ext_rows_batch.h"\n#include "gpqhe_ext_rows_batch.h"\n#include "gpqhe_ext_batch.h"\n'
        "void (*k)(he_evk_t[], const poly_mpi_t *, unsigned int) = he_genrk_rows;\n"
        "void (*f)(uint64_t *, const gpqhe_complex_t[], const uint64_t *, const gpqhe_complex_t[], const uint64_t *,"
        " size_t, unsigned int, const he_evk_t[], unsigned int) = he_gemv2_rows_batch;\n"
        "void (*s)(uint64_t *, const gpqhe_complex_t[], const gpqhe_complex_t[], const uint64_t *, const uint64_t *,"
        " const uint64_t *, const uint64_t *, size_t, unsigned int, const he_evk_t[], unsigned int)"
        " = he_hempc_step_rows_batch;\n"
        "unsigned int (*d)(void) = he_gemv_bsgs_default_g;\n"  # (it includes gpqhe_ext.h)
        "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Wpedantic", "-Wshadow", "-Werror", "-I",
                    str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_rows_header_declares_the_binding():
    inc = ROOT / "include"
    assert '#include "gpqhe_ext_rows_batch.h"' in (inc / "gpqhe_ext_batch.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", (inc / "gpqhe_ext_rows_batch.h").read_text(), flags=re.S)
    names = {n for n in re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", text) if n.startswith(("he_", "gpqhe_"))}
    assert names == set(ROWS) == set(gpqhe.PRODUCT_EXT_ROWS_BATCH)
    others = (set(gpqhe.PRODUCT_EXT) | set(gpqhe.PRODUCT_EXT_BATCH) | set(gpqhe.PRODUCT_EXT_IO_BATCH) |
              set(gpqhe.PRODUCT_EXT_STEP_BATCH) | set(gpqhe.EXPORTED))
    assert not names & others


def test_product_exports_them_and_the_oracle_does_not():
    assert gpqhe.PRODUCT_LIB.exists(), "product library not built (run __graft_entry__.build())"
    assert set(ROWS) <= exported(gpqhe.PRODUCT_LIB)
    assert not set(ROWS) & exported(gpqhe.ORACLE_LIB)


def test_engine_methods_need_the_symbols():
    e = gpqhe.Engine.oracle()
    with pytest.raises(AttributeError, match="he_genrk_rows"):
        e.genrk_rows(None, None, 2)
    with pytest.raises(AttributeError, match="he_gemv2_rows_batch"):
        e.gemv2_rows_batch(0, [0j], 0, [0j], 0, 0, 2, None, 1)
    with pytest.raises(AttributeError, match="he_hempc_step_rows_batch"):
        e.hempc_step_rows_batch(0, [0j], [0j], 0, 0, 0, 0, 0, 2, None, 1)


def test_rotation_lists():
    assert len(rows_rotations(256, 2)) == 8
    assert rows_rotations(256, 2) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert rows_rotations(16, 3) == [1, 2, 3, 4, 8]
    assert rows_rotations(16, 16) == list(range(1, 16))
    assert rows_rotations(16, 1) == [1, 2, 4, 8] and rows_rotations(16, 2) == [1, 2, 4, 8]
    assert len(rows_rotations(64, 2)) == 6 and len(rows_rotations(32, 2)) == 5


def setup(e, name, slots, rows, seed=4242):
    if name == "ref":
        e.init(12, 109, slots, 50)
    else:
        e.init_params(logn=13, nlimbs=5, nspecial=2, dnum=3, slots=slots, q0_bits=58, qi_bits=45, p_bits=59)
    e.set_seed(seed)
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rk = rows_keys(e, sk, rows)
    assert [r for r in range(slots) if rk[r].data] == rows_rotations(slots, rows)
    rng = np.random.default_rng(slots + rows)
    zs = [rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots) for _ in range(4)]
    cts = [e.encrypt(z, pk) for z in zs]
    return pk, sk, rk, zs, cts


def teardown(e, pk, sk, rk, cts):
    for o in cts + [pk, sk]:
        e.free(o)
    e.free_evks(rk)


CASES = [("ref", 16, 1), ("ref", 16, 2), ("ref", 16, 3), ("ref", 16, 16), ("ref", 256, 2), ("hyb", 32, 2)]


@pytest.mark.parametrize("name,slots,rows", CASES)
def test_composition_decodes_to_the_periodic_rows(oracle, name, slots, rows):
    e = oracle
    pk, sk, rk, zs, cts = setup(e, name, slots, rows)
    Ma, Mb = matrix(slots, 7 * slots + rows), matrix(slots, 9 * slots + rows)
    lvl, scale = cts[0].nlimbs, cts[0].scale
    y = gemv2_rows_compose(e, Ma, cts[0], Mb, cts[1], rk, rows)
    assert y.nlimbs == lvl - 1 and np.isclose(y.scale, scale, rtol=1e-12)
    want = expected_rows(Ma, zs[0], Mb, zs[1], slots, rows)
    assert np.allclose(want[:rows], (Ma @ zs[0] + Mb @ zs[1])[:rows], rtol=0, atol=1e-12)  # (the helper itself)
    err = np.abs(e.decrypt(y, sk) - want).max()
    print(f"gemv2_rows_compose {name}/{slots}/rows={rows}: error {err:.3e}")
    assert err < 1e-6 * max(1.0, np.abs(want).max())
    # the step around it: the first `rows` slots are the plaintext step's
    up = step_rows_compose(e, Ma, Mb, *cts, rk, rows)
    assert up.nlimbs == lvl - 1 and np.isclose(up.scale, scale, rtol=1e-12)
    xhat, xr, uhat, ur = zs
    want = uhat - expected_rows(Ma, xhat - xr, Mb, uhat - ur, slots, rows)
    assert np.allclose(want[:rows], (uhat - (Ma @ (xhat - xr) + Mb @ (uhat - ur)))[:rows], rtol=0, atol=1e-12)
    err = np.abs(e.decrypt(up, sk) - want).max()
    print(f"step_rows_compose {name}/{slots}/rows={rows}: error {err:.3e}")
    assert err < 1e-6 * max(1.0, np.abs(want).max())
    teardown(e, pk, sk, rk, cts + [y, up])


def test_all_rows_is_the_diagonal_method(oracle):
    """rows = slots, Mb = 0: every E_i is diagonal i and nothing is folded --
    bsgs_compose with one giant step, bit for bit."""
    e, s = oracle, 16
    pk, sk, rk, zs, cts = setup(e, "ref", s, s)
    Ma, Z = matrix(s, 301), np.zeros((s, s))
    y = gemv2_rows_compose(e, Ma, cts[0], Z, cts[1], rk, s)
    yb = bsgs_compose(e, Ma, cts[0], rk, s)
    assert np.array_equal(e.export(y), e.export(yb))
    teardown(e, pk, sk, rk, cts + [y, yb])


def test_zero_matrices_and_unread_rows(oracle):
    e, s, rows = oracle, 16, 3
    pk, sk, rk, zs, cts = setup(e, "ref", s, rows)
    Ma, Mb, Z = matrix(s, 311), matrix(s, 312), np.zeros((s, s))
    lvl = cts[0].nlimbs
    z0 = gemv2_rows_compose(e, Z, cts[0], Z, cts[1], rk, rows)
    assert z0.nlimbs == lvl - 1 and not e.export(z0).any()
    # matrices that are zero in their leading rows only are zero to it
    La, Lb = Ma.copy(), Mb.copy()
    La[:rows] = 0
    Lb[:rows] = 0
    z1 = gemv2_rows_compose(e, La, cts[0], Lb, cts[1], rk, rows)
    assert z1.nlimbs == lvl - 1 and not e.export(z1).any()
    # rows >= `rows` change no bit
    y = gemv2_rows_compose(e, Ma, cts[0], Mb, cts[1], rk, rows)
    Ca, Cb = Ma.copy(), Mb.copy()
    Ca[rows:] = matrix(s, 313)[rows:]
    Cb[rows:] = 0
    y2 = gemv2_rows_compose(e, Ca, cts[0], Cb, cts[1], rk, rows)
    assert np.array_equal(e.export(y), e.export(y2))
    # ... and a leading row does
    Ca[rows - 1, 5] += 0.25
    y3 = gemv2_rows_compose(e, Ca, cts[0], Cb, cts[1], rk, rows)
    assert not np.array_equal(e.export(y), e.export(y3))
    teardown(e, pk, sk, rk, cts + [z0, z1, y, y2, y3])
