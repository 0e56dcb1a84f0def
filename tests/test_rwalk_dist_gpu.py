"""Riemannian Walk under data parallelism: two ranks with different gradients, set up as tests/test_si_dist_gpu.py does (RCCL
with one rank per device when two devices show, else gloo with both ranks on cuda:0).  The Fisher, the path integral and the
score are updated where AdamW is applied, from the averaged gradient every rank holds, so all buffers and the weights are
identical across ranks without a collective of their own, and deferring the update changes nothing -- a deferred update folds
according to the count at the time it is applied."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optimizer_clip_dist_gpu import _free_port, _init

pytestmark = pytest.mark.gpu

BUFFERS = ("fisher", "importance", "theta_star", "w", "anchor", "score", "score_acc")


def _run(rank, defer):
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy, make_grad
    from test_rwalk_gpu import fisher_rule
    from test_si_gpu import w_rule
    flat = cl.FlatParams(Toy(big=False).cuda())
    rw = cl.RWalk(flat, rw_lambda=0.5, alpha=0.9, eps=1e-3, interval=2)
    opt = cl.FusedAdamW(flat, lr=1e-3, path_integral=rw, defer_update=defer)
    entries = list(flat.entries)
    rule_holds, folded = [], []
    for step in range(4):                                             # three steps (a fold at the second), consolidate, one penalised step
        if step == 3:
            rw.consolidate()
        local = [make_grad(entries, flat.numel, 800 + 10 * step + r, scale=3.0 + r).cuda() for r in range(2)]   # both ranks' draws
        before, F_prev, w_prev = flat.theta.clone(), rw.fisher.flat.clone(), rw.w.flat.clone()
        opt.zero_grad()
        flat.grad.copy_(local[rank])
        opt.step()
        after = cl.get_params_clone(flat.model).flat                  # applies a deferred update first
        ge = (local[0] + local[1]) * 0.5                              # the averaged gradient, fp32 on the device
        fold = rw.calls % 2 == 0
        ok = bool(torch.equal(rw.fisher.flat, fisher_rule(F_prev, ge)))
        if fold:
            ok = ok and not bool(rw.w.flat.any()) and bool(torch.equal(rw.anchor.flat, after))
        else:
            ok = ok and bool(torch.equal(rw.w.flat, w_rule(w_prev, ge, after, before))) and bool(rw.w.flat.ne(0).any())
        rule_holds.append(ok)
        folded.append(fold)
    tensors = [after] + [getattr(rw, k).flat.clone() for k in BUFFERS] + [rw.last_maxima.clone()]
    return tensors, rule_holds, folded, (rw.tasks_consolidated, rw.calls)


def _worker(rank, world, port, q):
    try:
        backend = _init(rank, world, port)
        now = _run(rank, defer=False)
        deferred = _run(rank, defer=True)
        same_modes = all(bool(torch.equal(a, b)) for a, b in zip(now[0], deferred[0]))
        same_ranks = True
        for t in deferred[0]:
            both = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(both, t)
            same_ranks = same_ranks and bool(torch.equal(both[0], both[1]))
        importance, score = deferred[0][2], deferred[0][6]
        q.put((rank, backend, same_modes, same_ranks, now[1], deferred[1], now[2], deferred[2], bool(importance.gt(0).any()),
               bool(score.gt(0).any()), now[3] == deferred[3] == (1, 4), None))
    except Exception:
        import traceback
        q.put((rank, "?", False, False, [], [], [], [], False, False, False, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_buffers_are_rank_identical_and_deferral_changes_nothing():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
    for (rank, backend, same_modes, same_ranks, rule_now, rule_deferred, fold_now, fold_deferred, importance_positive,
         score_positive, counted, err) in res:
        assert err is None, err
        print(rank, backend, rule_now, rule_deferred, fold_now)
        assert same_modes, ("deferred != immediate", rank)
        assert same_ranks, ("ranks diverged", rank)
        assert rule_now == rule_deferred == [True] * 4, rank
        assert fold_now == fold_deferred == [False, True, False, True], rank
        assert importance_positive and score_positive and counted       # the penalised step folded into the new language's score
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
