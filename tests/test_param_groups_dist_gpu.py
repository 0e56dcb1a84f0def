"""Parameter groups with a scheduler under data parallelism: two ranks with different gradients, set up as
tests/test_optimizer_clip_dist_gpu.py does (RCCL with one rank per device when two devices show, else gloo with both ranks on
cuda:0).  The scheduler is stepped right after opt.step(), as every torch training loop does; with `defer_update` the AdamW
launch happens later, at flush(), and must still use the learning rates its step() saw -- the deferred run has to end in
the bits of the immediate one.  It would not if flush() read the live param_groups."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 4


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, make_grad
    flat = cl.FlatParams(Toy(big=False).cuda())
    opt = cl.FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, defer_update=defer, param_groups=[
        dict(params=["v5", "v6", "v7", "v8", "v9", "idle"], lr=1e-4, weight_decay=0.0),
        dict(match="^mat$", lr=3e-3, weight_decay=0.2)])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 1.0 / (1 + e), lambda e: 0.5 ** e, lambda e: 1.0 + 0.5 * e])
    entries = list(flat.entries)
    seen = []
    for step in range(STEPS):
        opt.zero_grad()
        flat.grad.copy_(make_grad(entries, flat.numel, 800 + 10 * step + rank, scale=3.0 + rank).cuda())
        seen.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()                                  # moves every group's lr before a deferred update has been applied
        cl.flush_pending_updates()                    # what the next forward does
    return [flat.theta.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.shadow.clone()], seen


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        now, seen_now = _run(rank, defer=False)
        deferred, seen_def = _run(rank, defer=True)
        same_modes = [bool(torch.equal(a, b)) for a, b in zip(now, deferred)]
        same_ranks = []
        for t in deferred:
            both = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(both, t)
            same_ranks.append(bool(torch.equal(both[0], both[1])))
        q.put((rank, backend, same_modes, same_ranks, seen_now, seen_def, None))
    except Exception:
        import traceback
        q.put((rank, "?", [], [], [], [], traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_deferred_update_uses_the_learning_rates_of_its_step():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, seen_now, seen_def, err in res:
        assert err is None, err
        print(rank, backend, same_modes, same_ranks)
        assert same_modes == [True] * 4, ("deferred != immediate (theta, exp_avg, exp_avg_sq, shadow)", rank, same_modes)
        assert same_ranks == [True] * 4, ("ranks diverged", rank, same_ranks)
        assert seen_now == seen_def and len(seen_now) == STEPS
        for k in range(3):                            # every group's lr changed at every step
            assert len({lrs[k] for lrs in seen_now}) == STEPS, (k, seen_now)
    for p in ps:
        assert p.exitcode == 0
