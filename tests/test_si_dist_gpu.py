"""Synaptic Intelligence under data parallelism: two ranks with different gradients, set up as
tests/test_optimizer_clip_dist_gpu.py does (RCCL with one rank per device when two devices show, else gloo with both ranks on
cuda:0).  The path integral is updated where AdamW is applied, from the averaged gradient every rank holds, so w, omega and the
weights are identical across ranks without a collective of their own, and deferring the update changes nothing."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, make_grad
    flat = cl.FlatParams(Toy(big=False).cuda())
    si = cl.SynapticIntelligence(flat, si_c=0.5)
    opt = cl.FusedAdamW(flat, lr=1e-3, path_integral=si, defer_update=defer)
    entries = list(flat.entries)
    rule_holds = []
    for step in range(3):                                             # two steps, consolidate, one penalised step
        if step == 2:
            si.consolidate()
        local = [make_grad(entries, flat.numel, 700 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]   # both ranks' draws
        before, w_prev = flat.theta.clone(), si.w.flat.clone()
        opt.zero_grad()
        flat.grad.copy_(local[rank])
        opt.step()
        after = cl.get_params_clone(flat.model).flat                  # applies a deferred update first
        ge = (local[0] + local[1]) * 0.5                              # the averaged gradient, fp32 on the device
        moved = after - before
        prod = ge * moved
        rule_holds.append(bool(torch.equal(si.w.flat, w_prev - prod)) and bool(si.w.flat.ne(0).any()))
    return after, si.w.flat.clone(), si.omega.flat.clone(), rule_holds, si.tasks_consolidated


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        now = _run(rank, defer=False)
        deferred = _run(rank, defer=True)
        same_modes = all(bool(torch.equal(a, b)) for a, b in zip(now[:3], deferred[:3]))
        same_ranks = True
        for t in deferred[:3]:
            both = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(both, t)
            same_ranks = same_ranks and bool(torch.equal(both[0], both[1]))
        q.put((rank, backend, same_modes, same_ranks, now[3], deferred[3], bool(deferred[2].gt(0).any()),
               now[4] == deferred[4] == 1, None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, [], [], False, False, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_path_integral_is_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, rule_now, rule_deferred, omega_positive, consolidated_once, err in res:
        assert err is None, err
        print(rank, backend, rule_now, rule_deferred)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert rule_now == rule_deferred == [True, True, True], rank
        assert omega_positive and consolidated_once
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
