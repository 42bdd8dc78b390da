"""Child process of tests/test_gpu_seeded_batch.py::test_teardown_clean_exit:
the three seeded secret-key batch encryptions (host and GPU encoder), their
expansion and a batch decode, hectx_exit, a second context on another parameter
set, the same again, hectx_exit, and a normal interpreter exit.  Prints one
JSON line: whether each context's round trips returned their inputs."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def round_trip(e, slots, cnt, ps):
    import torch
    from hectr_amd.gpqhe import PubSeed
    pk, sk = e.pk(), e.sk()
    e.keypair(pk, sk)
    rng = np.random.default_rng(slots)
    zs = rng.uniform(-1, 1, (cnt, slots)) + 1j * rng.uniform(-1, 1, (cnt, slots))
    w = e.L * e.n
    c0 = torch.zeros(cnt * w, dtype=torch.int64, device="cuda")
    x = torch.zeros(cnt * 2 * w, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def expanded(count, enc):
        before = PubSeed.from_buffer_copy(ps)
        enc()
        assert ps.stream == before.stream + count
        e.expand_seeded_batch(x.data_ptr(), c0.data_ptr(), count, e.L, before)

    expanded(cnt, lambda: e.enc_sk_seeded_batch(c0.data_ptr(), zs, sk, slots, e.info.delta, e.L, ps))
    ok = bool(np.abs(e.dec_dcd_batch(x.data_ptr(), cnt, e.L, e.info.delta, sk, slots) - zs).max() < 1e-6)
    # the packed form: loops of 4 slots, width 3
    S, s, wd = e.slots, 4, 3
    zp = zs.ravel()[:cnt * (S // s) * wd].reshape(cnt, S // s, wd)
    expanded(cnt, lambda: e.enc_sk_seeded_packed_batch(c0.data_ptr(), zp, sk, s, wd, e.info.delta, e.L, ps))
    got = e.dec_dcd_packed_batch(x.data_ptr(), cnt, e.L, e.info.delta, sk, s, wd)
    ok = ok and bool(np.abs(got - zp).max() < 1e-6)
    # the gains' diagonals: one row, so one diagonal, the matrix's first row in every loop
    M = zs.ravel()[:s].reshape(1, 1, s)
    expanded(1, lambda: e.enc_gain_sk_seeded_packed_batch(c0.data_ptr(), M, sk, s, 1, e.L, ps, 1))
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
    ps = e.pubseed(stream=2 ** 32 - 3)
    e.init_params(**PARAMS["f13"][1])
    e.set_seed(5)
    first = round_trip(e, 64, 5, ps) and round_trip(e, 2048, 2, ps)
    e.exit()
    e.init(**PARAMS["ref"][1])
    e.set_seed(6)
    second = round_trip(e, 16, 5, ps) and round_trip(e, 2048, 2, ps)
    e.exit()
    print(json.dumps({"first": first, "second": second, "streams": ps.stream - (2 ** 32 - 3)}))


if __name__ == "__main__":
    main()
