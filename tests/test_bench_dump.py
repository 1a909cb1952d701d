"""CPU test of bench.py --dump-outputs: the state sample is the same for every run and every rank layout, stays in bounds and
under the size cap, and the files are float64 .npy."""
import contextvars
import os
import threading
import types

import numpy as np
import torch

import bench


def _prob(dims, slab=None):
    n = int(np.prod(dims))
    lo, hi = slab or (0, dims[-1])
    return types.SimpleNamespace(nglobal=n, nlocal=(hi - lo) * n // dims[-1], slab=(lo, hi), dims=dims)


def test_small_state_is_written_whole():
    dims = (64, 32, 32)
    full = torch.from_numpy(np.random.default_rng(1).standard_normal(int(np.prod(dims))))
    s = bench.state_sample(types.SimpleNamespace(t=full), _prob(dims), 1)
    assert np.array_equal(s, full.numpy())


def test_large_state_sample_is_fixed_sorted_in_bounds_and_capped():
    dims = (512, 512, 512)
    n = int(np.prod(dims))
    vec = types.SimpleNamespace(t=torch.arange(n, dtype=torch.float64))      # value = global index
    s = bench.state_sample(vec, _prob(dims), 1)
    assert s.size == bench.DUMP_STATE_MAX and s.nbytes <= 32 << 20
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < n
    assert np.array_equal(s, bench.state_sample(vec, _prob(dims), 1))


def test_rank_slabs_give_the_same_sample_as_one_rank(monkeypatch):
    """Each rank contributes the sampled values of its own z-slab; gathered in slab order they are the one-rank sample."""
    import torch.distributed as dist
    dims, world = (128, 128, 512), 4
    n = int(np.prod(dims))
    plane = n // dims[-1]
    full = torch.from_numpy(np.random.default_rng(2).standard_normal(n))
    ref = bench.state_sample(types.SimpleNamespace(t=full), _prob(dims), 1)
    slabs = [(r * dims[-1] // world, (r + 1) * dims[-1] // world) for r in range(world)][::-1]   # rank order != slab order
    contrib, meet = [None] * world, threading.Barrier(world)

    def gather(parts, obj):                             # one thread per rank: an all-gather through shared memory
        contrib[slabs.index(rank_slab.get())] = obj
        meet.wait()
        parts[:] = contrib

    monkeypatch.setattr(dist, "all_gather_object", gather)
    rank_slab = contextvars.ContextVar("rank_slab")
    outs = [None] * world

    def rank(r):
        lo, hi = slabs[r]
        rank_slab.set(slabs[r])
        outs[r] = bench.state_sample(types.SimpleNamespace(t=full[lo * plane:hi * plane].clone()), _prob(dims, (lo, hi)), world)

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for out in outs:
        assert np.array_equal(out, ref)


def test_dump_writes_float64_npy(tmp_path):
    d = str(tmp_path / "out")
    shapes = bench.dump_outputs(d, {"u": np.arange(5, dtype=np.float32), "p": [0.1], "itlinear": [24]})
    assert shapes == {"u": [5], "p": [1], "itlinear": [1]}
    for name in shapes:
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float64
