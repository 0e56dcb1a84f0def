"""PackNet under data parallelism: two ranks with different gradients, set up as tests/test_piggyback_dist_gpu.py does (RCCL with
one rank per device when two devices show, else gloo with both ranks on cuda:0).  The step and the pruning run where AdamW is
applied, on the averaged gradient and the weights every rank holds, so owner map, weights and moments are identical across ranks
without a collective of their own, deferring the update changes nothing, and both equal a single process fed the averaged
gradient."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 2          # before the pruning; one more after it


def _build(defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy
    from test_packnet_gpu import FROZEN, PACKED
    flat = cl.FlatParams(Toy(big=False).cuda())
    pn = cl.PackNet(flat, packed=PACKED, frozen=FROZEN, prune=0.5)
    return flat, pn, cl.FusedAdamW(flat, lr=1e-3, masks=pn, defer_update=defer)


def _draws(flat, step):
    from test_optimizer_clip_gpu import make_grad
    return [make_grad(list(flat.entries), flat.numel, 900 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]


def _loop(flat, pn, opt, grad_of):
    from indic_cl_asr_amd import cl
    pn.begin_language("x", opt)
    for step in range(STEPS + 1):
        if step == STEPS:
            pn.prune(opt)                                             # applies a deferred update first
        opt.zero_grad()
        flat.grad.copy_(grad_of(step))
        opt.step()
        cl.flush_pending_updates()                                    # the deferred update consumes flat.grad: apply it first
    theta = cl.get_params_clone(flat.model).flat
    return pn.owner.clone(), theta, opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def _run(rank, defer):
    flat, pn, opt = _build(defer)
    return _loop(flat, pn, opt, lambda step: _draws(flat, step)[rank])


def _single():
    """One process, no process group involved in the step: the averaged gradient, fp32 on the device."""
    flat, pn, opt = _build(defer=False)
    opt.allreduce_grads = lambda: 1.0

    def averaged(step):
        local = _draws(flat, step)
        return (local[0] + local[1]) * 0.5

    return _loop(flat, pn, opt, averaged)


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
        owner = deferred[0]
        q.put((rank, backend, same_modes, same_ranks, same_single, int((owner == 1).sum()), None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, False, 0, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_owner_map_and_weights_are_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, same_single, owned, err in res:
        assert err is None, err
        print(rank, backend, "weights owned after the pruning:", owned)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert same_single, ("two ranks != one process fed the averaged gradient", rank)
        assert owned > 0
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
