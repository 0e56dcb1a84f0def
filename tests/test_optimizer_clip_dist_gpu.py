"""Gradient clipping under data parallelism: two ranks with different gradients, set up as tests/test_dist_gpu.py does (RCCL
with one rank per device when two devices show, else gloo with both ranks on cuda:0).  FusedAdamW clips AFTER the
all-reduce -- the norm is that of the averaged gradient, every rank applies the same factor -- whereas
torch.nn.utils.clip_grad_norm_ between backward() and step() would have clipped each rank's local gradient by its own."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

MAX_NORM = 1.0
STEPS = 2


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    if torch.cuda.device_count() >= world:
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        return "nccl"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return "gloo"


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, make_grad, norms64
    flat = cl.FlatParams(Toy(big=False).cuda())
    opt = cl.FusedAdamW(flat, lr=1e-3, max_grad_norm=MAX_NORM, defer_update=defer)
    entries = list(flat.entries)
    checks = []
    for step in range(STEPS):
        local = [make_grad(entries, flat.numel, 500 + 10 * step + r, scale=3.0 + r) for r in range(2)]   # both ranks' draws
        opt.zero_grad()
        flat.grad.copy_(local[rank])
        opt.step()
        st = opt.stats()                                          # applies a deferred update first
        _, avg64 = norms64(entries, (local[0].double() + local[1].double()) / 2)
        _, mine64 = norms64(entries, local[rank])
        checks.append(dict(norm=st["grad_norm"], avg64=avg64, mine64=mine64, coef=st["clip_coef"]))
    theta = cl.get_params_clone(flat.model).flat.clone()
    return theta, checks, opt.stats()["clipped_steps"]


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        th_now, checks, clipped_now = _run(rank, defer=False)
        th_def, checks_def, clipped_def = _run(rank, defer=True)
        both = [torch.empty_like(th_def) for _ in range(world)]
        dist.all_gather(both, th_def)
        q.put((rank, backend, bool(torch.equal(th_now, th_def)), bool(torch.equal(both[0], both[1])), checks, checks_def,
               clipped_now, clipped_def, None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, [], [], 0, 0, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_clip_uses_the_averaged_gradient_on_two_ranks():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, checks, checks_def, clipped_now, clipped_def, err in res:
        assert err is None, err
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert clipped_now == clipped_def == STEPS
        for c in checks + checks_def:
            print(rank, backend, c)
            assert abs(c["norm"] - c["avg64"]) <= 2e-6 * c["avg64"], c
            assert abs(c["coef"] - MAX_NORM / (c["avg64"] + 1e-6)) <= 2e-6 * c["coef"], c
            # the averaged gradient is clipped, and this rank's own gradient would have been clipped by another factor
            assert c["avg64"] > MAX_NORM and c["mine64"] > MAX_NORM
            assert abs(c["mine64"] - c["avg64"]) > 0.1 * c["avg64"], c
    for p in ps:
        assert p.exitcode == 0
