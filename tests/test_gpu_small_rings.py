"""The other rings of the small-N path, product (libgpqhe.so on MI355X) vs
oracle, bit for bit.

Every fused small-N kernel is instantiated for n = 2^12, 2^11 and 2^10 behind a
three-way ladder on the ring size (kernels.hip: ntt_small_kernel,
lift_ntt_arg_kernel, inv_dcd_kernel, modup_small_kernel and its halves,
moddown_small_kernel, down_inv / down_fwd_small_kernel), the speculation is
gated on 10 <= logn <= 12 (api.cpp defer_ok, spec_launch), and the fused
decoder takes plaintexts of at most two limbs (k_ew_decode) -- while the other
GPU tests run the small-N path at n = 4096 with HECTR's own chain (L = 2) only.
Here, at the rings of tests/small_n_steps.PARAMS_RINGS:

  n2048, n1024   logn = 11 and 10 at q = 2^109: the other two rungs of every
                 ladder, inside the speculation gate;
  n4096_L4       logn = 12 at q = 2^209: L = 4, K = 1, so a product decodes
                 from three limbs: the generic inverse transform and decoder
                 instead of the fused two-limb one, and the step's speculation
                 records meet levels they were not built for;

the four step sequences of tests/small_n_steps.py (every exported object and
every decoded vector equal element by element), test_gpu_parity's list of
evaluation operations and its keys / encrypt / decrypt comparison.

Not run: n512 (logn = 9, just outside the gate).  he_dcd_ex of a plaintext in
NTT form goes through k_ntt_ex there, which has no transform below n = 2^10
and ends the process (kernels.hip k_ntt_ex), so no step sequence can decode;
INTEGRATION.md states the supported range.  tests/test_levels_cpu.py runs the
oracle alone through all four rings against the plaintext step."""
import pytest

from tests import small_n_steps as S
from tests import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

RINGS = ["n2048", "n1024", "n4096_L4"]  # n512: see above


@pytest.mark.parametrize("seq", list(S.SEQUENCES))
@pytest.mark.parametrize("ring", RINGS)
def test_step_sequences(oracle, product, ring, seq):
    params = S.PARAMS_RINGS[ring]
    want = S.SEQUENCES[seq](oracle, params=params)
    got = S.SEQUENCES[seq](product, params=params)
    taken = product.lib.gpqhe_spec_gemv_taken()  # (counted from the sequence's hectx_init)
    assert (product.n, product.L) == (oracle.n, oracle.L) == (1 << params["logn"], 4 if ring == "n4096_L4" else 2)
    assert S.mismatches(want, got) == []
    print(f"{ring} {seq}: {len(want)} objects, {taken} speculated gemvs")
    if seq == "speculative_gemvs" and ring != "n4096_L4":
        # inside the gate the sequence's repeated steps are served from the
        # speculation (HECTR's ring: test_gpu_parity.test_speculative_gemvs):
        # the ladder rungs of the speculative kernels did run
        assert taken >= 1, taken


@pytest.mark.parametrize("ring", RINGS)
def test_evaluation_ops(oracle, product, ring, monkeypatch):
    """test_gpu_parity.test_evaluation_ops (add, sub, neg, moddown, rot, gemv,
    mul, mul_rescale, mul then rescale and the in-place forms; bits and
    decodes) at the ring."""
    monkeypatch.setitem(parity.PARAMS, ring, ("init", S.PARAMS_RINGS[ring]))
    parity.test_evaluation_ops(oracle, product, ring)


@pytest.mark.parametrize("ring", RINGS)
def test_keys_encrypt_decrypt(oracle, product, ring, monkeypatch):
    """test_gpu_parity.test_keys_encrypt_decrypt (every key, an encryption and
    its decryption; decoded values bit-equal) at the ring."""
    monkeypatch.setitem(parity.PARAMS, ring, ("init", S.PARAMS_RINGS[ring]))
    parity.test_keys_encrypt_decrypt(oracle, product, ring)
