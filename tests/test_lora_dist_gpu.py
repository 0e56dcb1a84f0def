"""LoRA under data parallelism: two ranks with different gradients, set up as tests/test_optimizer_clip_dist_gpu.py does (RCCL with
one rank per device when two devices show, else gloo with both ranks on cuda:0).  The factors are updated where AdamW is applied,
from the averaged gradient every rank holds, and A is drawn from a seed every rank shares, so factors and weights are identical
across ranks without a collective of their own, deferring the update changes nothing, and both equal a single process fed the
averaged gradient."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 2


def _build(defer):
    from indic_cl_asr_amd import cl
    from test_lora_gpu import ADAPTED, FROZEN, GROUP1, Toy
    flat = cl.FlatParams(Toy().cuda())
    lora = cl.LoRA(flat, rank=5, alpha=16.0, adapted=ADAPTED, frozen=FROZEN, seed=1)
    opt = cl.FusedAdamW(flat, lr=1e-3, masks=lora, param_groups=[GROUP1], max_grad_norm=1.0, defer_update=defer)
    lora.begin_language("x", opt)
    return flat, lora, opt


def _draws(flat, step):
    from test_optimizer_clip_gpu import make_grad
    return [make_grad(list(flat.entries), flat.numel, 900 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    flat, lora, opt = _build(defer)
    for step in range(STEPS):
        opt.zero_grad()
        flat.grad.copy_(_draws(flat, step)[rank])
        opt.step()
        cl.flush_pending_updates()                                    # the deferred update consumes flat.grad: apply it first
    theta = cl.get_params_clone(flat.model).flat
    return lora.factors.clone(), lora.factor_exp_avg_sq.clone(), theta, opt.shadow.view(torch.int16).to(torch.int32)


def _single():
    """One process, no process group involved in the step: the averaged gradient, fp32 on the device."""
    flat, lora, opt = _build(defer=False)
    opt.allreduce_grads = lambda: 1.0
    for step in range(STEPS):
        local = _draws(flat, step)
        opt.zero_grad()
        flat.grad.copy_((local[0] + local[1]) * 0.5)
        opt.step()
    return lora.factors.clone(), lora.factor_exp_avg_sq.clone(), flat.theta.clone(), opt.shadow.view(torch.int16).to(torch.int32)


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        now = _run(rank, defer=False)
        deferred = _run(rank, defer=True)
        single = _single()
        same_modes = all(bool(torch.equal(a, b)) for a, b in zip(now, deferred))
        same_single = all(bool(torch.equal(a, b)) for a, b in zip(deferred, single))
        same_ranks = True
        for t in deferred:
            both = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(both, t)
            same_ranks = same_ranks and bool(torch.equal(both[0], both[1]))
        moved = int((deferred[1] != 0).sum())                          # factor elements whose second moment has moved
        q.put((rank, backend, same_modes, same_ranks, same_single, moved, None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, False, 0, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_factors_and_weights_are_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, same_single, moved, err in res:
        assert err is None, err
        print(rank, backend, "factor elements trained:", moved)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert same_single, ("two ranks != one process fed the averaged gradient", rank)
        assert moved > 0
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
