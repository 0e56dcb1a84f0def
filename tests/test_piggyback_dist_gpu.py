"""Piggyback masks under data parallelism: two ranks with different gradients, set up as tests/test_optimizer_clip_dist_gpu.py
does (RCCL with one rank per device when two devices show, else gloo with both ranks on cuda:0).  The scores are updated where
AdamW is applied, from the averaged gradient every rank holds, so scores, bits and weights are identical across ranks without a
collective of their own, deferring the update changes nothing, and both equal a single process fed the averaged gradient."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 2


def _build(defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy
    from test_piggyback_gpu import FROZEN, MASKED
    flat = cl.FlatParams(Toy(big=False).cuda())
    pb = cl.Piggyback(flat, masked=MASKED, frozen=FROZEN, threshold=5e-3, init=6e-3)     # two steps from 6e-3 switch bits off
    return flat, pb, cl.FusedAdamW(flat, lr=1e-3, masks=pb, defer_update=defer)


def _draws(flat, step):
    from test_optimizer_clip_gpu import make_grad
    return [make_grad(list(flat.entries), flat.numel, 900 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    flat, pb, opt = _build(defer)
    for step in range(STEPS):
        opt.zero_grad()
        flat.grad.copy_(_draws(flat, step)[rank])
        opt.step()
        cl.flush_pending_updates()                                    # the deferred update consumes flat.grad: apply it first
    theta = cl.get_params_clone(flat.model).flat
    pb.save_language("x")
    return pb.scores.flat.clone(), pb.records["x"]["bits"].clone(), theta


def _single():
    """One process, no process group involved in the step: the averaged gradient, fp32 on the device."""
    flat, pb, opt = _build(defer=False)
    opt.allreduce_grads = lambda: 1.0
    for step in range(STEPS):
        local = _draws(flat, step)
        opt.zero_grad()
        flat.grad.copy_((local[0] + local[1]) * 0.5)
        opt.step()
    pb.save_language("x")
    return pb.scores.flat.clone(), pb.records["x"]["bits"].clone(), flat.theta.clone()


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
        bits_off = int((deferred[0] < 5e-3).sum() - (deferred[0] == 0).sum())
        q.put((rank, backend, same_modes, same_ranks, same_single, bits_off, None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, False, 0, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_scores_and_bits_are_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, same_single, bits_off, err in res:
        assert err is None, err
        print(rank, backend, "masked elements off:", bits_off)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert same_single, ("two ranks != one process fed the averaged gradient", rank)
        assert bits_off > 0
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
