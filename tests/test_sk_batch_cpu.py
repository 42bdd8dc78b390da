"""The batch encryptions under the secret key (include/gpqhe_ext_sk_batch.h)
without a GPU: the header, the binding's table, the libraries' exports, and the
yardstick the GPU tests compare against -- tests/sk_ref on the oracle: a fresh
he_enc_sk ciphertext carries exactly the model's CBD sample as its noise and
the model's uniform sample as c1, from the seed alone; the packed product and
step and their encrypted-gain forms, fed with secret-key encryptions, decode
within the project's bound.  The public-key and secret-key errors are printed
side by side."""
import re
import subprocess

import numpy as np
import pytest

import ckks_model_rng as R
import noise_audit as A
from hectr_amd import gpqhe
from tests.encgain_ref import enc_gain_compose, gemv2_encgain_compose, step_encgain_compose
from tests.packed_ref import expected_packed, gemv2_packed_compose, step_packed_compose
from tests.rows_ref import pow2
from tests.sk_ref import enc_gain_sk_compose, encrypt_sk
from tests.test_abi import exported
from tests.test_packed_batch_cpu import loop_errors, loop_mats, setup, teardown

ROOT = gpqhe.ROOT
SK = ("he_enc_sk_batch", "he_enc_sk_packed_batch", "he_enc_gain_sk_packed_batch")
SEED2 = 97


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_sk_header_is_pure_c_and_guarded(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "gpqhe_ext_sk_batch.h"\n#include "gpqhe_ext_sk_batch.h"\n#include "gpqhe_ext_batch.h"\n'
        "void (*e)(uint64_t *, const gpqhe_complex_t[], size_t, unsigned int, double, unsigned int,"
        " const poly_mpi_t *) = he_enc_sk_batch;\n"
        "void (*p)(uint64_t *, const gpqhe_complex_t[], size_t, unsigned int, unsigned int, double, unsigned int,"
        " const poly_mpi_t *) = he_enc_sk_packed_batch;\n"
        "void (*d)(uint64_t *, const gpqhe_complex_t[], unsigned int, unsigned int, unsigned int, unsigned int,"
        " const poly_mpi_t *) = he_enc_gain_sk_packed_batch;\n"
        "unsigned int (*g)(void) = he_gemv_bsgs_default_g;\n"  # (it includes gpqhe_ext.h)
        "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Wpedantic", "-Wshadow", "-Werror", "-I",
                    str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_sk_header_declares_the_binding():
    inc = ROOT / "include"
    batch = (inc / "gpqhe_ext_batch.h").read_text()
    assert '#include "gpqhe_ext_sk_batch.h"' in batch
    assert batch.index('"gpqhe_ext_encgain_batch.h"') < batch.index('"gpqhe_ext_sk_batch.h"')
    text = re.sub(r"/\*.*?\*/", "", (inc / "gpqhe_ext_sk_batch.h").read_text(), flags=re.S)
    names = {n for n in re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", text) if n.startswith(("he_", "gpqhe_"))}
    assert names == set(SK) == set(gpqhe.PRODUCT_EXT_SK_BATCH)
    others = (set(gpqhe.PRODUCT_EXT) | set(gpqhe.PRODUCT_EXT_BATCH) | set(gpqhe.PRODUCT_EXT_IO_BATCH) |
              set(gpqhe.PRODUCT_EXT_STEP_BATCH) | set(gpqhe.PRODUCT_EXT_ROWS_BATCH) |
              set(gpqhe.PRODUCT_EXT_PACKED_BATCH) | set(gpqhe.PRODUCT_EXT_ENCGAIN_BATCH) | set(gpqhe.EXPORTED))
    assert not names & others


def test_product_exports_them_and_the_oracle_does_not():
    assert gpqhe.PRODUCT_LIB.exists(), "product library not built (run __graft_entry__.build())"
    assert set(SK) <= exported(gpqhe.PRODUCT_LIB)
    assert not set(SK) & exported(gpqhe.ORACLE_LIB)


def test_engine_methods_need_the_symbols():
    e = gpqhe.Engine.oracle()
    with pytest.raises(AttributeError, match="he_enc_sk_batch"):
        e.enc_sk_batch(0, [0j] * 16, None, 16, 1.0, 2)
    with pytest.raises(AttributeError, match="he_enc_sk_packed_batch"):
        e.enc_sk_packed_batch(0, [0j] * 16, None, 16, 16, 1.0, 2)
    with pytest.raises(AttributeError, match="he_enc_gain_sk_packed_batch"):
        e.enc_gain_sk_packed_batch(0, [0j], None, 16, 1, 2)


CASES = [("ref", 64, 16, 2), ("ref", 2048, 16, 3), ("hyb", 128, 32, 2)]


@pytest.mark.parametrize("name,S,s,rows", CASES)
def test_fresh_noise_and_c1_are_the_models_samples(oracle, name, S, s, rows):
    """From gpqhe_set_seed(SEED2), encryption i takes stream 2 i for c1 and
    2 i + 1 for e.  The exact decryption minus the exact plaintext is the CBD
    sample coefficient for coefficient (so |e| <= 21: integers, no tolerance),
    c1 the uniform sample on every limb, at the top level and one below."""
    e = oracle
    pk, sk, rk, zs, cts = setup(e, name, S, s, rows)
    e.set_seed(SEED2)
    st = A.Streams(SEED2)
    n, nmod = e.n, e.L + e.K
    fresh = []
    for i, (z, lvl) in enumerate(zip(zs[:3], (e.L, e.L, e.L - 1))):
        pt, ct = e.pt(), e.ct()
        e.ecd_ex(pt, z, S, e.info.delta, lvl)
        e.enc_sk(ct, pt, sk)
        sa, se = st.take(), st.take()
        assert (sa, se) == (2 * i, 2 * i + 1) and ct.nlimbs == lvl
        noise = A.exact_decrypt(e, ct, sk) - A.exact_plain(e, pt)
        assert np.abs(noise).max() <= R.CBD_ETA
        assert np.array_equal(noise.astype(np.int64), R.sample_cbd(st.key, se, n)), "e is not the model's CBD sample"
        c1 = e.export(ct)[1]
        for m in range(lvl):
            want = R.sample_uniform(st.key, sa, n, m, e.primes[m], nmod)
            assert np.array_equal(c1[m], want), f"c1 limb {m} is not the model's uniform sample"
        fresh.append(np.abs(e.decrypt(ct, sk, S) - z).max())
        e.free(pt)
        e.free(ct)
    pkerr = max(np.abs(e.decrypt(c, sk, S) - z).max() for c, z in zip(cts, zs))
    print(f"fresh {name} S={S}: worst decode error pk {pkerr:.3e} sk {max(fresh[:2]):.3e} "
          f"(ratio {pkerr / max(fresh[:2]):.0f}, sqrt(n + 1) = {np.sqrt(n + 1):.0f})")
    assert max(fresh) < 1e-6
    teardown(e, pk, sk, rk, cts)


@pytest.mark.parametrize("name,S,s,rows", CASES)
def test_pipelines_on_secret_key_encryptions_decode(oracle, name, S, s, rows):
    """The packed product and step with plain gains and with encrypted ones,
    every ciphertext (the gains' diagonals too) a secret-key encryption: each
    loop within 1e-6 max(1, |expected|).  The same compositions on public-key
    encryptions of the same data are run for the printout only."""
    e, P = oracle, S // s
    pk, sk, rk, zs, cpk = setup(e, name, S, s, rows)
    Ma, Mb = loop_mats(P, rows, s, 7 * S + rows), loop_mats(P, rows, s, 9 * S + rows)
    lvl, scale = cpk[0].nlimbs, cpk[0].scale
    rlk = e.evk()
    e.genrlk(rlk, sk)
    csk = [encrypt_sk(e, z, sk) for z in zs]
    assert all(c.nlimbs == lvl and c.scale == scale for c in csk)
    gains = {"pk": (enc_gain_compose(e, Ma, pk, s, rows, P, lvl), enc_gain_compose(e, Mb, pk, s, rows, P, lvl)),
             "sk": (enc_gain_sk_compose(e, Ma, sk, s, rows, P, lvl), enc_gain_sk_compose(e, Mb, sk, s, rows, P, lvl))}
    assert all(len(d) == pow2(rows) and all(x.nlimbs == lvl for x in d) for g in gains.values() for d in g)
    xhat, xr, uhat, ur = zs
    want_g = expected_packed(Ma, zs[0], Mb, zs[1], s, rows, P)
    want_s = uhat - expected_packed(Ma, xhat - xr, Mb, uhat - ur, s, rows, P)
    made, errs = [], {}
    for key, cts in (("pk", cpk), ("sk", csk)):
        DA, DB = gains[key]
        outs = {
            "gemv2 plain gains": (gemv2_packed_compose(e, Ma, cts[0], Mb, cts[1], rk, s, rows, P), want_g),
            "step plain gains": (step_packed_compose(e, Ma, Mb, *cts, rk, s, rows, P), want_s),
            "gemv2 encrypted gains": (gemv2_encgain_compose(e, DA, cts[0], DB, cts[1], rk, rlk, s, rows), want_g),
            "step encrypted gains": (step_encgain_compose(e, DA, DB, *cts, rk, rlk, s, rows), want_s),
        }
        for what, (y, want) in outs.items():
            assert y.nlimbs == lvl - 1 and np.isclose(y.scale, scale, rtol=1e-12)
            err, scl = loop_errors(e.decrypt(y, sk), want, P, rows)
            errs[key, what] = err.max()
            if key == "sk":
                assert (err < 1e-6 * scl).all(), (what, err.max())
            made.append(y)
    for what in ("gemv2 plain gains", "step plain gains", "gemv2 encrypted gains", "step encrypted gains"):
        print(f"{name} {S}/{s}/{rows} {what}: worst loop error pk {errs['pk', what]:.3e} sk {errs['sk', what]:.3e}")
    e.free(rlk)
    teardown(e, pk, sk, rk, cpk + csk + made + [x for g in gains.values() for d in g for x in d])
