"""Child process of tests/test_gpu_io_batch.py::test_teardown_clean_exit: both
batch calls (folded and general decoder, host and GPU encoder), hectx_exit, a
second context on another parameter set, both calls again, hectx_exit, and a
normal interpreter exit.  Prints one JSON line: whether each context's batch
round trip returned its inputs."""
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
    e.enc_pk_batch(x.data_ptr(), zs, pk, slots, e.info.delta, e.L)
    ok = True
    for fold in ("1", "0"):
        os.environ["GPQHE_DCD_FOLD"] = fold
        got = e.dec_dcd_batch(x.data_ptr(), cnt, e.L, e.info.delta, sk, slots)
        ok = ok and bool(np.abs(got - zs).max() < 1e-6)
    del os.environ["GPQHE_DCD_FOLD"]
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
