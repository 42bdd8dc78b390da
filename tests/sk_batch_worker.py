"""Child process of tests/test_gpu_sk_batch.py::test_teardown_clean_exit: the
three secret-key batch encryptions (host and GPU encoder) and a batch decode,
hectx_exit, a second context on another parameter set, the same again,
hectx_exit, and a normal interpreter exit.  Prints one JSON line: whether each
context's round trips returned their inputs."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def round_trip(e, slots, cnt):
    import torch
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(slots)
    zs = rng.uniform(-1, 1, (cnt, slots)) + 1j * rng.uniform(-1, 1, (cnt, slots))
    x = torch.zeros(cnt * 2 * e.L * e.n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.enc_sk_batch(x.data_ptr(), zs, sk, slots, e.info.delta, e.L)
    ok = bool(np.abs(e.dec_dcd_batch(x.data_ptr(), cnt, e.L, e.info.delta, sk, slots) - zs).max() < 1e-6)
    # the packed form: loops of 4 slots, width 3
    S, s, w = e.slots, 4, 3
    zp = zs.ravel()[:cnt * (S // s) * w].reshape(cnt, S // s, w)
    e.enc_sk_packed_batch(x.data_ptr(), zp, sk, s, w, e.info.delta, e.L)
    got = e.dec_dcd_packed_batch(x.data_ptr(), cnt, e.L, e.info.delta, sk, s, w)
    ok = ok and bool(np.abs(got - zp).max() < 1e-6)
    # the gains' diagonals: one row, so one diagonal, the matrix's first row in every loop
    M = zs.ravel()[:s].reshape(1, 1, s)
    e.enc_gain_sk_packed_batch(x.data_ptr(), M, sk, s, 1, e.L, 1)
    q_top = float(e.primes[e.L - 1])
    got = e.dec_dcd_packed_batch(x.data_ptr(), 1, e.L, q_top, sk, s, s)
    ok = ok and bool(np.abs(got - M.reshape(1, 1, s)).max() < 1e-6)
    e.free(pk)
    e.free(sk)
    return ok


def main():
    import torch
    from hectr_amd.gpqhe import Engine
    from tests.test_gpu_parity import PARAMS
    assert torch.cuda.is_available()
    e = Engine.product()
    e.init_params(**PARAMS["f13"][1])
    e.set_seed(5)
    first = round_trip(e, 64, 5) and round_trip(e, 2048, 2)
    e.exit()
    e.init(**PARAMS["ref"][1])
    e.set_seed(6)
    second = round_trip(e, 16, 5) and round_trip(e, 2048, 2)
    e.exit()
    print(json.dumps({"first": first, "second": second}))


if __name__ == "__main__":
    main()
