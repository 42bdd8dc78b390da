"""he_gemv_bsgs_batch without a GPU: its header (include/gpqhe_ext_batch.h),
the binding's table and the product library's export.  The headers and
tables the earlier tests pin (gpqhe.h, gpqhe_ext.h, PRODUCT_EXT) are not
touched by it."""
import re
import subprocess

from hectr_amd import gpqhe
from tests.test_abi import exported

ROOT = gpqhe.ROOT
EXT_BATCH = ("he_gemv_bsgs_batch",)


def test_batch_header_is_pure_c_and_guarded(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "gpqhe_ext_batch.h"\n#include "gpqhe_ext_batch.h"\n'
        "void (*f)(uint64_t *, const gpqhe_complex_t[], const uint64_t *, size_t, unsigned int,"
        " const he_evk_t[], unsigned int) = he_gemv_bsgs_batch;\n"
        "void (*s)(he_ct_t *, const gpqhe_complex_t[], const he_ct_t *, const he_evk_t[], unsigned int)"
        " = he_gemv_bsgs;\n"  # (it includes gpqhe_ext.h)
        "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Wpedantic", "-Wshadow", "-Werror", "-I",
                    str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_batch_header_declares_the_binding():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gpqhe_ext_batch.h").read_text(), flags=re.S)
    names = {n for n in re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", text) if n.startswith(("he_", "gpqhe_"))}
    assert names == set(EXT_BATCH) == set(gpqhe.PRODUCT_EXT_BATCH)
    assert not set(EXT_BATCH) & (set(gpqhe.PRODUCT_EXT) | set(gpqhe.EXPORTED))


def test_product_exports_it_and_the_oracle_does_not():
    assert gpqhe.PRODUCT_LIB.exists(), "product library not built (run __graft_entry__.build())"
    assert set(EXT_BATCH) <= exported(gpqhe.PRODUCT_LIB)
    assert not set(EXT_BATCH) & exported(gpqhe.ORACLE_LIB)


def test_engine_method_needs_the_symbol():
    e = gpqhe.Engine.oracle()
    assert hasattr(e, "gemv_bsgs_batch")
    try:
        e.gemv_bsgs_batch(0, [0j], 0, 0, 2, None)
    except AttributeError as err:
        assert "he_gemv_bsgs_batch" in str(err)
    else:
        raise AssertionError("the oracle has no he_gemv_bsgs_batch")
