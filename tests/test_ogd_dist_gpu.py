"""OGD under data parallelism: two ranks with different gradients, set up as tests/test_gem_dist_gpu.py does (RCCL with one rank
per device when two devices show, else gloo with both ranks on cuda:0).  add_direction() averages the candidate over the
optimizer's group, and the dots and the projection run where AdamW is applied, on the averaged gradient every rank holds: both
ranks keep the same basis and the same weights without a collective of their own, and deferring the update changes nothing.
Those bits equal a single process fed the averaged gradients: on the same ranks a second OGD is handed (r0_k + r1_k) * 0.5 without
an optimizer (no averaging of its own), and its optimizer is fed (g0 + g1) * 0.5 (its exchange doubles and halves that gradient,
which is exact, as is the projection of a gradient scaled by two)."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

DIRECTIONS = 3
OUT = ("v3", "v8")


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, assert_same, make_grad
    flat, flat_b = cl.FlatParams(Toy(big=False).cuda()), cl.FlatParams(Toy(big=False).cuda())
    scope = [n for n in flat.names if n not in OUT]
    ogd, single = cl.OGD(flat, DIRECTIONS, scope=scope), cl.OGD(flat_b, DIRECTIONS, scope=scope)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=ogd, defer_update=defer)
    twin = cl.FusedAdamW(flat_b, lr=1e-3, projection=single, defer_update=False)
    entries = list(flat.entries)
    ok = True
    for k in range(DIRECTIONS):
        rs = [make_grad(entries, flat.numel, 900 + 10 * k + r, scale=3.0 + r).cuda() for r in range(2)]
        opt.zero_grad()
        flat.grad.copy_(rs[rank])
        ok = ok and ogd.add_direction(opt) and not bool(flat.grad.any())
        flat_b.grad.copy_((rs[0] + rs[1]) * 0.5)                      # fp32 on the device
        ok = ok and single.add_direction() and not bool(flat_b.grad.any())
    ok = ok and ogd.directions == single.directions == DIRECTIONS and bool(torch.equal(ogd.basis, single.basis))
    gs = [make_grad(entries, flat.numel, 800 + r, scale=3.0 + r).cuda() for r in range(2)]
    flat.grad.copy_(gs[rank])
    opt.step()
    st = ogd.stats()                                                  # applies a deferred update first
    twin.zero_grad()
    flat_b.grad.copy_((gs[0] + gs[1]) * 0.5)
    twin.step()
    try:
        assert_same(opt, twin, "one step")
        same = True
    except AssertionError:
        same = False
    ok = ok and same and 0.0 < st["removed_fraction"] < 1.0 and st["directions"] == DIRECTIONS
    return flat.theta.clone(), ogd.basis.clone(), ok


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
        q.put((rank, backend, same_modes, same_ranks, now[2], deferred[2], None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, False, False, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_basis_and_step_are_rank_identical_and_equal_a_single_process():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for rank, backend, same_modes, same_ranks, ok_now, ok_deferred, err in res:
        assert err is None, err
        print(rank, backend, ok_now, ok_deferred)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert ok_now and ok_deferred, rank
    for p in ps:
        assert p.exitcode == 0
