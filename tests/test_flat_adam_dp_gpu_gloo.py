"""FlatAdam's device path under data parallelism: two processes share cuda:0 and gloo carries the exchange (the pattern of
tests/test_dp_gpu_gloo.py).  The ranks see different batches; after `red.finish(); opt.step()` the clipped step must be the same on
both -- the norm is that of the averaged gradient, bit-identical on the two ranks (a deterministic reduction of identical buckets), and
so is every parameter after three steps.  Both ways of averaging: the collective / one division (`average="auto"`) and 1 / world folded
into the optimizer's gradient scale (`average="optimizer"`)."""
import hashlib
import os
import socket
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, average, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import numpy as np
        from tests.test_flat_adam_device_gpu import make_model, make_opt, batch, backward, norm64, bits
        dev = torch.device("cuda:0")
        model = make_model(dev)                                # identical parameters on every rank
        red, opt = make_opt(model, average=average, weight_decay=1e-2, max_grad_norm=1e-3, skip_nonfinite=True)
        scale = 1.0 / world if average == "optimizer" else 1.0
        assert red.grad_scale == scale
        g = torch.Generator().manual_seed(100 + rank)          # different batches
        norms, ok = [], True
        for step in range(3):
            red.begin(sync=True)
            backward(model, batch(g, dev))
            red.finish()
            opt.step()
            want = norm64(opt.params, scale)                   # the buckets hold the averaged gradient (or the sum, scaled in the pass)
            n = float(opt.last_grad_norm.item())
            ok &= want > 0 and abs(n - float(np.float32(want))) <= 2.0 ** -23 * want
            ok &= float(opt.state_block["clip_coef"].item()) < 1.0
            norms.append(int(bits(opt.last_grad_norm).item()))
            red.zero_grad()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for p in model.all_params():
            h.update(p.detach().cpu().numpy().tobytes())
        ok &= int(opt.applied_steps.item()) == 3 and all(bool(torch.isfinite(p).all()) for p in model.all_params())
        out[rank] = (bool(ok), tuple(norms), h.hexdigest())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("average", ["auto", "optimizer"])
def test_clipped_step_is_identical_on_two_ranks(average):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), average, out), nprocs=world, join=False)
    deadline = time.time() + 240                               # the ranks' own time limit: no rank outlives it
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                raise TimeoutError("the two ranks did not finish in 240 s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    res = dict(out)
    assert set(res) == {0, 1} and res[0][0] and res[1][0], res
    assert res[0][1] == res[1][1], res                         # last_grad_norm of every step, bit for bit
    assert res[0][2] == res[1][2], res                         # every parameter, bit for bit
