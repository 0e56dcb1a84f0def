"""GEM under data parallelism: two ranks with different task gradients and different memory gradients, set up as
tests/test_agem_dist_gpu.py does (RCCL with one rank per device when two devices show, else gloo with both ranks on cuda:0).
store_reference() averages each task's reference over the optimizer's group, and the dots, the program and the projection run
where AdamW is applied, on the averaged task gradient every rank holds: both ranks solve the same program to the same v, the
weights stay identical without a collective of their own, and deferring the update changes nothing.  The rule is checked bit for
bit: a plain optimizer on the same ranks is fed (g0 + g1) * 0.5 + sum_k v_k * ((r0_k + r1_k) * 0.5), one fp32 torch op per
rounding (its own exchange doubles and halves that gradient, which is exact)."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

STEPS = 3
SIGNS = (-1.0, +1.0, -1.0)      # per task: the reference opposes / agrees with the rank's gradient
GAMMA = 0.1                     # below the free minimiser of an opposing row (tests/test_gem_gpu.py): both kinds of v_k occur


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, assert_same, make_grad
    flat, flat_b = cl.FlatParams(Toy(big=False).cuda()), cl.FlatParams(Toy(big=False).cuda())
    gem = cl.GEM(flat, max_tasks=len(SIGNS), memory_strength=GAMMA)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=gem, defer_update=defer)
    twin = cl.FusedAdamW(flat_b, lr=1e-3, defer_update=False)
    entries = list(flat.entries)
    rule_holds, vs = [], []
    for step in range(STEPS):
        # both ranks' draws: task k's reference on rank r is noise -/+ half of rank r's gradient, so the averages relate alike
        gs = [make_grad(entries, flat.numel, 800 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]
        rs = [[make_grad(entries, flat.numel, 900 + 100 * k + 10 * step + r, scale=3.0 + r).cuda() + 0.5 * s * gs[r]
               for r in range(2)] for k, s in enumerate(SIGNS)]
        opt.zero_grad()
        refs, ref_ok = [], True
        for k in range(len(SIGNS)):
            flat.grad.copy_(rs[k][rank])
            gem.store_reference(f"task{k}", opt)
            refs.append((rs[k][0] + rs[k][1]) * 0.5)                  # fp32 on the device
            ref_ok = ref_ok and bool(torch.equal(gem.refs[k, :flat.numel], refs[k])) and not bool(flat.grad.any())
        flat.grad.copy_(gs[rank])
        opt.step()
        st = gem.stats()                                              # applies a deferred update first
        G = (gs[0] + gs[1]) * 0.5
        for vk, r in zip(st["v"], refs):
            if vk != 0.0:
                G = G + torch.tensor(vk, dtype=torch.float32, device="cuda") * r
        twin.zero_grad()
        flat_b.grad.copy_(G)
        twin.step()
        try:
            assert_same(opt, twin, step)
            same = True
        except AssertionError:
            same = False
        mixed = max(st["v"]) > min(st["v"]) == float(torch.tensor(GAMMA, dtype=torch.float32))
        rule_holds.append(ref_ok and same and mixed and st["projected"] == 1 and st["unsolved_steps"] == 0)
        vs.append(st["v"])
    return flat.theta.clone(), torch.tensor(vs, device="cuda"), rule_holds, gem.stats()["projected_steps"]


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
