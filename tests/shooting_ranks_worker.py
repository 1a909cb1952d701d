"""Worker of tests/test_gpu_shooting_ranks.py (spawned with RANK / WORLD_SIZE / MASTER_* set): both ranks share cuda:0 through the
host-staged communicator; the spectral flow and the shooting functional refuse a context of more than one rank with their own
message, and the context goes on working."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC for multi-process GPU work (before the HIP runtime loads)

import torch  # noqa: E402,F401
import torch.distributed as dist  # noqa: E402

from bk_amd import hostcomm  # noqa: E402


def main(rank, world):
    from bk_amd import hip, shooting
    from bk_amd._lib import BkHipError
    dims, ls = (16, 12, 20), (2.0, 1.5, 2.5)
    ctx = hip.Context(0, hostcomm.comm_tuple())
    # the only problem kind that exists on several ranks; a cGL problem is refused by the decomposition itself
    prob = hip.SwiftHohenberg(ctx, dims, ls)
    u = np.random.default_rng(1).standard_normal(int(np.prod(dims)))
    U = prob.vec(u)
    before = U.norm()

    def refused(make, pattern):
        try:
            make()
        except BkHipError as e:
            assert pattern in str(e), str(e)
            return
        raise AssertionError(f"no refusal ({pattern})")

    refused(lambda: shooting.Flow(prob, 1), "bk_flow_create: the spectral flow runs on a single rank")
    refused(lambda: shooting.ShootingProblem(prob, 2, 4), "bk_shooting_create: the shooting functional runs on a single rank")
    refused(lambda: hip.CGL2d(ctx, (12, 9), (np.pi, np.pi / 2)), "3-D Swift-Hohenberg problem only")
    # the context is still usable: a global reduction over both ranks gives what it gave before, and the serial value
    after = U.norm()
    assert after == before and abs(after - np.linalg.norm(u)) <= 1e-12 * after, (before, after)
    ctx.close()
    print(f"rank {rank}: shooting rank checks OK", flush=True)


if __name__ == "__main__":
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        main(rank, world)
    finally:
        dist.destroy_process_group()
