"""Averaged GEM under data parallelism: two ranks with different task gradients and different memory gradients, set up as
tests/test_optimizer_clip_dist_gpu.py does (RCCL with one rank per device when two devices show, else gloo with both ranks on
cuda:0).  store_reference() averages the reference over the optimizer's group and the projection runs where AdamW is applied,
on the averaged task gradient every rank holds: both ranks take the same decision with the same alpha, the weights stay
identical without a collective of their own, and deferring the update changes nothing.  The rule is checked bit for bit: a plain
optimizer on the same ranks is fed (g0 + g1) * 0.5 - alpha * ((r0 + r1) * 0.5), one fp32 torch op per rounding (its own exchange
doubles and halves that gradient, which is exact)."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 3


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, assert_same, make_grad
    flat, flat_b = cl.FlatParams(Toy(big=False).cuda()), cl.FlatParams(Toy(big=False).cuda())
    agem = cl.AveragedGEM(flat)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=agem, defer_update=defer)
    twin = cl.FusedAdamW(flat_b, lr=1e-3, defer_update=False)
    entries = list(flat.entries)
    rule_holds, alphas = [], []
    for step in range(STEPS):
        # both ranks' draws: rank r's reference opposes rank r's gradient, so the averages oppose each other too
        gs = [make_grad(entries, flat.numel, 800 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]
        rs = [make_grad(entries, flat.numel, 900 + 10 * step + r, scale=3.0 + r).cuda() - 0.5 * gs[r] for r in range(2)]
        opt.zero_grad()
        flat.grad.copy_(rs[rank])
        agem.store_reference(opt)
        ref = (rs[0] + rs[1]) * 0.5                                   # fp32 on the device
        ref_ok = bool(torch.equal(agem.ref.flat, ref)) and not bool(flat.grad.any())
        flat.grad.copy_(gs[rank])
        opt.step()
        st = agem.stats()                                             # applies a deferred update first
        ge = (gs[0] + gs[1]) * 0.5
        ar = torch.tensor(st["alpha"], dtype=torch.float32, device="cuda") * ref
        twin.zero_grad()
        flat_b.grad.copy_(ge - ar)
        twin.step()
        try:
            assert_same(opt, twin, step)
            same = True
        except AssertionError:
            same = False
        rule_holds.append(ref_ok and same and st["projected"] == 1)
        alphas.append(st["alpha"])
    return flat.theta.clone(), torch.tensor(alphas, device="cuda"), rule_holds, agem.stats()["projected_steps"]


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        now = _run(rank, defer=False)
        deferred = _run(rank, defer=True)
        same_modes = all(bool(torch.equal(a, b)) for a, b in zip(now[:2], deferred[:2]))
        same_ranks = True
        for t in deferred[:2]:
            both = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(both, t)
            same_ranks = same_ranks and bool(torch.equal(both[0], both[1]))
        q.put((rank, backend, same_modes, same_ranks, now[2], deferred[2], now[3], deferred[3], None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, [], [], 0, 0, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_projection_is_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, rule_now, rule_deferred, projected_now, projected_deferred, err in res:
        assert err is None, err
        print(rank, backend, rule_now, rule_deferred)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert rule_now == rule_deferred == [True] * STEPS, rank
        assert projected_now == projected_deferred == STEPS
    for p in ps:
        assert p.exitcode == 0
