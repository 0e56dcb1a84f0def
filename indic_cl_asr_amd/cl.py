"""Continual-learning state and arithmetic on flat device buffers (EWC / MAS / LwF + AdamW + DP exchange).

Reference call sites restated here (R/ = reference repo root):
  get_params / get_params_clone / get_zero_params / get_grads / set_grads ... R/utils.py:273-321
  get_penalty_grads (EWC) ............................................... R/cl_baseline_ewc.py:69-81
  Fisher epoch ........................................................... R/cl_baseline_ewc.py:245-282
  penalty (MAS) + importance epoch ...................................... R/cl_baseline_mas.py:70-75,212-288
  LwF distillation ....................................................... R/cl_baseline_lwf.py:212-264
  AdamW(lr) / zero_grad / step ........................................... R/cl_baseline.py:137,187-196

MI355X design: every trainable parameter lives in ONE flat fp32 buffer (`FlatParams.theta`), `.grad`s are views
of ONE flat gradient buffer, so the penalty, Fisher/omega accumulation, AdamW and the RCCL all-reduce are each
a single launch / a single collective over ~N*4 bytes instead of ~300 per-tensor kernels.
The dict-of-tensors API of the reference is kept: the dicts handed out are `FlatDict`s (name -> view).
"""
import ctypes
import math
import re
import weakref
from contextlib import contextmanager
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _lib

_ALIGN = 64  # floats: every tensor starts on a 256-byte boundary inside the flat buffers


class FlatDict(dict):
    """name -> view into `.flat` (a 1-D fp32 device tensor laid out by `.layout`)."""

    def __init__(self, layout: "FlatParams", flat: torch.Tensor):
        super().__init__()
        self.layout, self.flat = layout, flat
        for name, off, numel, shape in layout.entries:
            self[name] = flat[off:off + numel].view(shape)


class FlatParams:
    def __init__(self, model: torch.nn.Module):
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("model has no trainable parameters")
        named = _qkv_adjacent(named)
        dev = named[0][1].device
        self.model = model
        self.entries, off = [], 0
        for n, p in named:
            if p.dtype != torch.float32:
                raise TypeError(f"{n}: master parameters must be float32")
            self.entries.append((n, off, p.numel(), tuple(p.shape)))
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self.params = [p for _, p in named]
        self.names = [n for n, _ in named]
        self.theta = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self._theta_views = FlatDict(self, self.theta)
        self._grad_views = FlatDict(self, self.grad)
        with torch.no_grad():
            for (n, o, k, shape), p in zip(self.entries, self.params):
                self._theta_views[n].copy_(p.data)
                p.data = self._theta_views[n]
                p.grad = self._grad_views[n]
        # chunk table for ia_cl_penalty (chunks never straddle tensors)
        ch = _lib.lib().ia_cl_chunk_elems() if dev.type == "cuda" else 4096
        rows = []
        for seg, (n, o, k, shape) in enumerate(self.entries):
            for c0 in range(0, k, ch):
                rows.append((o + c0, min(ch, k - c0), seg, 0))
        self.chunk_table = torch.tensor(rows, dtype=torch.int32, device=dev)
        # chunks of tensor k are rows [seg_chunk_begin[k], seg_chunk_begin[k+1]) of the table (ia_grad_norm's per-tensor sums)
        begin = [0]
        for n, o, k, shape in self.entries:
            begin.append(begin[-1] + (k + ch - 1) // ch)
        self.seg_chunk_begin = torch.tensor(begin, dtype=torch.int32, device=dev)
        self.seg_inv_numel = torch.tensor([1.0 / e[2] for e in self.entries], dtype=torch.float32, device=dev)
        # True once something gave EVERY trainable tensor a gradient since the last zero_grad (a pre-loaded EWC penalty /
        # the MAS penalty: R/utils.py:316-321, R/cl_baseline_mas.py:231-234) -- torch.optim.AdamW then updates them all
        self.all_grads_live = False
        model._ia_flat = self

    # -- buffers ---------------------------------------------------------------------------------
    def zeros(self) -> FlatDict:
        return FlatDict(self, torch.zeros_like(self.theta))

    def clone_theta(self) -> FlatDict:
        flush_pending_updates()
        return FlatDict(self, self.theta.clone())

    def params_dict(self) -> FlatDict:
        flush_pending_updates()
        return self._theta_views

    def grads_dict(self) -> FlatDict:
        return self._grad_views

    def attach_grads(self):
        for n, p in zip(self.names, self.params):
            p.grad = self._grad_views[n]

    def zero_grad(self):
        self.grad.zero_()
        self.all_grads_live = False
        self.attach_grads()

    @contextmanager
    def weights(self, other: FlatDict):
        """Run with the parameters temporarily pointing at another flat buffer (LwF teacher forward) -- no
        torch.save/torch.load ping-pong and no barriers (R/cl_baseline_lwf.py:220-234 does both per batch)."""
        from .ops import fast
        flush_pending_updates()
        try:
            for n, p in zip(self.names, self.params):
                p.data = other[n]
            fast.bump_weight_epoch()
            yield
        finally:
            for n, p in zip(self.names, self.params):
                p.data = self._theta_views[n]
            fast.bump_weight_epoch()


def _qkv_adjacent(named):
    """Layout order of the flat buffers: as named_parameters(), except that each attention module's linear_q | linear_k | linear_v
    weights (and then their biases) are placed back to back, so the [3d, d] operand of the fused Q/K/V projection and its bias
    are VIEWS of the flat weight / bf16 shadow buffers (ops/fast.bf16_shadow, f32_cat) instead of three-way concatenations
    rebuilt after every optimizer step.  The dict-of-names surface (FlatDict) does not depend on the order."""
    by_name = dict(named)
    order, done = [], set()
    for n, p in named:
        if n in done:
            continue
        if n.endswith("linear_q.weight") or n.endswith("linear_q.bias"):
            kind = n.rsplit(".", 1)[1]
            stem = n[: -len("linear_q." + kind)]
            group = [stem + f"linear_{x}.{kind}" for x in ("q", "k", "v")]
            if all(g in by_name for g in group):
                for g in group:
                    order.append((g, by_name[g])); done.add(g)
                continue
        order.append((n, p)); done.add(n)
    return order


def flat_of(model) -> FlatParams:
    m = getattr(model, "module", model)
    f = getattr(m, "_ia_flat", None)
    if f is None:
        f = FlatParams(m)
    return f


# ----------------------------------------------------------------------------- R/utils.py:273-321 drop-ins
def get_params(model) -> FlatDict:
    return flat_of(model).params_dict()


def get_params_clone(model) -> FlatDict:
    return flat_of(model).clone_theta()


def get_zero_params(model, device=None) -> FlatDict:
    return flat_of(model).zeros()


def get_grads(model) -> FlatDict:
    return flat_of(model).grads_dict()


def set_grads(model, grad_dict):
    """R/utils.py:316-321.  A FlatDict produced by get_penalty_grads already IS the flat gradient buffer."""
    flush_pending_updates()
    flush_pending_updates()
    f = flat_of(model)
    if isinstance(grad_dict, FlatDict) and grad_dict.flat.data_ptr() != f.grad.data_ptr():
        f.grad.copy_(grad_dict.flat)
        grad_dict = f.grads_dict()
    f.all_grads_live = True
    for name, p in getattr(model, "module", model).named_parameters():
        p.grad = grad_dict[name] if name in grad_dict else None


def save_model(model, path):
    """R/utils.py:265-271: trainable-only state dict (same interchange format)."""
    flush_pending_updates()
    torch.save({n: p.data.clone() for n, p in getattr(model, "module", model).named_parameters() if p.requires_grad}, path)


# ----------------------------------------------------------------------------- EWC
def ewc_penalty_into_grads(flat: FlatParams, fisher: FlatDict, checkpoint: FlatDict, e_lambda: float,
                           monitor_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad <- 2*lambda*F*(theta-theta*) (pre-load, autograd accumulates on top: R/cl_baseline_ewc.py:228-231);
    returns a 0-dim device tensor = mean_k mean|penalty_k| (the 'ewc_penalty' monitor, :74-80)."""
    flush_pending_updates()
    L = _lib.lib()
    seg = torch.zeros(len(flat.entries), dtype=torch.float32, device=flat.theta.device)
    st = L.ia_cl_penalty(_lib.ptr(flat.theta), _lib.ptr(checkpoint.flat), _lib.ptr(fisher.flat), 2.0 * float(e_lambda),
                         _lib.ptr(flat.grad), 0, _lib.ptr(flat.chunk_table), flat.chunk_table.shape[0],
                         _lib.ptr(flat.seg_inv_numel), _lib.ptr(seg), None, _lib.stream_ptr())
    _lib.check(st, "ia_cl_penalty")
    flat.attach_grads()
    flat.all_grads_live = True
    return seg.mean()


def get_penalty_grads(config, fish: FlatDict, curr_checkpoint: FlatDict, checkpoint: FlatDict):
    """Signature of R/cl_baseline_ewc.py:69: returns (grad dict, python float)."""
    flat = fish.layout
    avg = ewc_penalty_into_grads(flat, fish, checkpoint, config.cl_config.e_lambda)
    return flat.grads_dict(), avg.item()


def fisher_accumulate(flat: FlatParams, fish: FlatDict, loss: torch.Tensor):
    """fish += mean(loss) * grad**2 (R/cl_baseline_ewc.py:245-255), loss stays on the device."""
    s = loss.detach().float().mean().reshape(1).contiguous()
    st = _lib.lib().ia_cl_fisher_accumulate(_lib.ptr(fish.flat), _lib.ptr(flat.grad), _lib.ptr(s), flat.numel,
                                            _lib.stream_ptr())
    _lib.check(st, "ia_cl_fisher_accumulate")


def fisher_finish(main_fish: Optional[FlatDict], fish: FlatDict, total_ds: int, e_gamma: float,
                  group=None) -> FlatDict:
    """fish /= N; main = gamma*main + fish (R/cl_baseline_ewc.py:267-280).  Under DP the rank-local Fisher sums and
    sample counts are all-reduced first (one RCCL collective over the flat buffer) so the result equals the
    1-GPU Fisher over the union of the shards (the reference keeps rank-local dicts)."""
    n = torch.tensor([float(total_ds)], device=fish.flat.device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(fish.flat, group=group)
        dist.all_reduce(n, group=group)
    fish.flat.div_(n)
    if main_fish is None:
        return fish
    main_fish.flat.mul_(e_gamma).add_(fish.flat)
    return main_fish


# ----------------------------------------------------------------------------- MAS
def mas_penalty_add_grads(flat: FlatParams, importance: FlatDict, checkpoint: FlatDict, mas_lambda: float):
    """Adds d/dtheta [mas_lambda * sum omega (theta-theta*)^2] to the flat gradient buffer and returns the
    un-weighted penalty value as a 0-dim device tensor ('mass_loss', R/cl_baseline_mas.py:70-75,231-234).
    The reference obtains the same gradient through autograd on `loss + mass_loss*mas_lambda`."""
    flush_pending_updates()
    val = torch.zeros(1, dtype=torch.float32, device=flat.theta.device)
    st = _lib.lib().ia_cl_penalty(_lib.ptr(flat.theta), _lib.ptr(checkpoint.flat), _lib.ptr(importance.flat),
                                  2.0 * float(mas_lambda), _lib.ptr(flat.grad), 1, _lib.ptr(flat.chunk_table),
                                  flat.chunk_table.shape[0], None, None, _lib.ptr(val), _lib.stream_ptr())
    _lib.check(st, "ia_cl_penalty")
    flat.all_grads_live = True
    return val[0]


def penalty(model, main_importance: FlatDict, prev_params: FlatDict):
    """Signature of R/cl_baseline_mas.py:70.  Returns the penalty VALUE (no autograd graph); pair it with
    mas_penalty_add_grads() after backward, or use MASRegulariser which does both."""
    flush_pending_updates()
    flat = flat_of(model)
    val = torch.zeros(1, dtype=torch.float32, device=flat.theta.device)
    st = _lib.lib().ia_cl_penalty(_lib.ptr(flat.theta), _lib.ptr(prev_params.flat), _lib.ptr(main_importance.flat), 0.0,
                                  None, 0, _lib.ptr(flat.chunk_table), flat.chunk_table.shape[0], None, None,
                                  _lib.ptr(val), _lib.stream_ptr())
    _lib.check(st, "ia_cl_penalty")
    return val[0]


def mas_importance_loss(model, mas_ctx: float):
    """R/cl_baseline_mas.py:258-265 on the stashed raw logits (joint.store_list, ctc_decoder.decoder_logits)."""
    m = getattr(model, "module", model)
    from .ops.joint import LatticeStash, lattice_sumsq_term
    decoder_logits = (m.ctc_decoder.decoder_logits.flatten(end_dim=-2).float() ** 2).sum(dim=-1).mean()
    if isinstance(m.joint.store_list, LatticeStash):   # fused joint: one streaming pass over the f16 lattice
        rnn_logits = lattice_sumsq_term(m.joint.store_list)
    else:
        rnn_logits = 0
        for i in m.joint.store_list:
            rnn_logits = rnn_logits + (i.flatten(end_dim=-2).float() ** 2).sum(dim=-1).mean()
        rnn_logits = rnn_logits / len(m.joint.store_list)
    return rnn_logits * (1 - mas_ctx) + decoder_logits * mas_ctx


def importance_accumulate(flat: FlatParams, importance: FlatDict):
    st = _lib.lib().ia_cl_abs_accumulate(_lib.ptr(importance.flat), _lib.ptr(flat.grad), flat.numel, _lib.stream_ptr())
    _lib.check(st, "ia_cl_abs_accumulate")


def importance_finish(importance: FlatDict, n_batches: int, group=None) -> FlatDict:
    """omega /= #batches (R/cl_baseline_mas.py:284-287; overwrites the previous task's omega as the reference
    does).  Under DP: all-reduce(SUM) of omega and of the batch counts first."""
    n = torch.tensor([float(n_batches)], device=importance.flat.device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(importance.flat, group=group)
        dist.all_reduce(n, group=group)
    importance.flat.div_(n)
    return importance


# ----------------------------------------------------------------------------- SI
class SynapticIntelligence:
    """Synaptic Intelligence (Zenke, Poole, Ganguli 2017): importance integrated online, inside the optimizer step, from the
    task gradient and the parameter's own movement -- no Fisher / importance epoch after the task.

    Three flat fp32 buffers over the layout (12 B per parameter): `w` the running path integral of the current task, `omega`
    the consolidated importance of the earlier tasks, `theta_star` the weights at the end of the previous task (= at the start
    of this one; initialised to the current weights).  Attach it with `FusedAdamW(..., path_integral=si)`: each step then
    updates `w -= ge * (theta' - theta)` with ge the (data-parallel averaged) task gradient, and from the second task on adds
    the surrogate's gradient `2 * si_c * omega * (theta - theta_star)` to what AdamW consumes.  `consolidate()` at the end of
    a task: `omega += max(0, w / ((theta - theta_star)^2 + xi))`, `w = 0`, `theta_star = theta` (negative contributions are
    dropped so that the surrogate stays convex).

    Clip order: with `max_grad_norm` the norm and the coefficient are those of the task gradient and the surrogate's gradient
    is added AFTER clipping -- not `clip_grad_norm_` of the total gradient (for that, add the penalty to `.grad` with
    `mas_penalty_add_grads(flat, si.omega, si.theta_star, si.si_c)`; `w` would then integrate the penalised gradient)."""

    def __init__(self, model_or_flat, si_c=1.0, xi=1e-3):
        if not float(xi) > 0.0:
            raise ValueError(f"SynapticIntelligence: xi must be > 0 (got {xi})")
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        self.si_c, self.xi = float(si_c), float(xi)
        flush_pending_updates()
        self.w = self.flat.zeros()
        self.omega = self.flat.zeros()
        self.theta_star = FlatDict(self.flat, self.flat.theta.clone())
        self.tasks_consolidated = 0

    @classmethod
    def from_config(cls, model_or_flat, config):
        """`cl_config.si_c` / `cl_config.si_xi` when the config has them (the reference's config.yaml has neither key)."""
        cc = getattr(config, "cl_config", None) or {}
        return cls(model_or_flat, si_c=cc.get("si_c", 1.0), xi=cc.get("si_xi", 1e-3))

    def penalty_value(self) -> torch.Tensor:
        """Sum omega * (theta - theta_star)^2 as a 0-dim device tensor (the 'si_penalty' monitor; un-weighted, as 'mass_loss').
        One pass over three flat buffers: call it only when the value is logged."""
        flush_pending_updates()
        f = self.flat
        val = torch.zeros(1, dtype=torch.float32, device=f.theta.device)
        st = _lib.lib().ia_cl_penalty(_lib.ptr(f.theta), _lib.ptr(self.theta_star.flat), _lib.ptr(self.omega.flat), 0.0, None, 0,
                                      _lib.ptr(f.chunk_table), f.chunk_table.shape[0], None, None, _lib.ptr(val),
                                      _lib.stream_ptr())
        _lib.check(st, "ia_cl_penalty")
        return val[0]

    def consolidate(self):
        """End of a task (one launch).  Under data parallelism every rank holds the same w, theta and theta_star, so no
        collective is needed."""
        flush_pending_updates()
        f = self.flat
        st = _lib.lib().ia_si_consolidate(_lib.ptr(f.theta), _lib.ptr(self.theta_star.flat), _lib.ptr(self.w.flat),
                                          _lib.ptr(self.omega.flat), self.xi, f.numel, _lib.stream_ptr())
        _lib.check(st, "ia_si_consolidate")
        self.tasks_consolidated += 1

    def flat_dicts(self) -> Dict[str, FlatDict]:
        """For `checkpoint.save_cl_state(path, **si.flat_dicts())`; `load_flat_dicts(checkpoint.load_cl_state(path, flat))`
        is the way back."""
        flush_pending_updates()
        return {"si_w": self.w, "si_omega": self.omega, "si_theta_star": self.theta_star}

    def load_flat_dicts(self, dicts, tasks_consolidated=None):
        """Copies the three buffers in place (an attached optimizer keeps pointing at them).  The file carries no task count:
        unless given, the penalty counts as attached (tasks_consolidated = 1) when the loaded omega has a non-zero entry."""
        flush_pending_updates()
        for key, mine in self.flat_dicts().items():
            if dicts[key].layout.entries != self.flat.entries:
                raise ValueError(f"'{key}' was saved for a different set of trainable tensors")
            mine.flat.copy_(dicts[key].flat)
        if tasks_consolidated is None:
            tasks_consolidated = int(bool(self.omega.flat.any()))
        self.tasks_consolidated = int(tasks_consolidated)

    def state_dict(self) -> dict:
        flush_pending_updates()
        return {"entries": list(self.flat.entries), "w": self.w.flat.detach().to("cpu", copy=True),
                "omega": self.omega.flat.detach().to("cpu", copy=True),
                "theta_star": self.theta_star.flat.detach().to("cpu", copy=True), "si_c": self.si_c, "xi": self.xi,
                "tasks_consolidated": self.tasks_consolidated}

    def load_state_dict(self, sd: dict, source="state dict"):
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'si' was saved for a different set of trainable tensors")
        if not float(sd["xi"]) > 0.0:
            raise ValueError(f"{source}: xi must be > 0")
        flush_pending_updates()
        self.w.flat.copy_(sd["w"])
        self.omega.flat.copy_(sd["omega"])
        self.theta_star.flat.copy_(sd["theta_star"])
        self.si_c, self.xi = float(sd["si_c"]), float(sd["xi"])
        self.tasks_consolidated = int(sd["tasks_consolidated"])


# ----------------------------------------------------------------------------- Riemannian Walk
class RWalk:
    """Riemannian Walk (Chaudhry, Dokania, Ajanthan, Torr, ECCV 2018): EWC with a Fisher that is maintained online, as a moving
    average of the squared task gradient inside the optimizer step (the paper's EWC++: no Fisher epoch after a language), joined
    with a path score -- SI's path integral measured in that Fisher's metric.  The two are normalised by their maxima and summed
    into one importance.

    Flat fp32 buffers over the layout: `fisher` F (carried across languages, never reset), `importance` (what the penalty
    uses) and `theta_star` (the weights at the end of the previous language); with `scores=True` also `w` (the path integral of
    the current interval), `anchor` (the weights at the last fold), `score` (of the current language) and `score_acc` (the mean
    normalised score of the finished languages): 28 B per parameter, 12 with `scores=False` (EWC++ alone).  Attach it with
    `FusedAdamW(..., path_integral=rw)`.  Every applied update then does, per element of a tensor that received a gradient, with
    ge the (data-parallel averaged) task gradient:
        F += alpha * (ge * ge - F);   w -= ge * (theta' - theta)
    and every `interval`-th applied update (`calls % interval == 0`, deferred updates counted when they are applied) folds:
        score += max(0, w) / (0.5 * F * (theta' - anchor)^2 + eps);   w = 0;   anchor = theta'
    Once a language is consolidated the step adds `2 * rw_lambda * importance * (theta - theta_star)` to what AdamW consumes --
    AFTER the clip, as for SynapticIntelligence, and every tensor is live then.  A step skipped as non-finite changes no buffer
    and drops a fold that was due: `w` waits for the next one.

    `consolidate()` at the end of a language, on the device with nothing read back: one more fold; maxF = max F and maxS = max
    score; a = F / maxF and b = score / maxS (0 where the maximum is 0; F and score themselves with `normalize=False`);
    `score_acc = b` for the first language, else `0.5 * (score_acc + b)`; `importance = a + score_acc` (a alone without
    scores); `score = 0`, `w = 0`, `theta_star = anchor = theta`.  The maxima stay on the device in `last_maxima`.  Non-finite
    maxima are not guarded: `skip_nonfinite` on the optimizer is what keeps inf and NaN out of F and w.

    `importance` and `fisher` are FlatDicts: `TaskVectors.store(lang, opt, importance=rw.importance)` and the EWC helpers take
    them as they take an epoch's Fisher."""

    _BUFFERS = ("fisher", "importance", "theta_star", "w", "anchor", "score", "score_acc")

    def __init__(self, model_or_flat, rw_lambda=1.0, alpha=0.9, interval=50, eps=1e-3, scores=True, normalize=True):
        self._check(alpha, interval, eps, "RWalk")
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        self.rw_lambda, self.alpha, self.interval, self.eps = float(rw_lambda), float(alpha), int(interval), float(eps)
        self.scores, self.normalize = bool(scores), bool(normalize)
        flush_pending_updates()
        self.fisher = self.flat.zeros()
        self.importance = self.flat.zeros()
        self.theta_star = FlatDict(self.flat, self.flat.theta.clone())
        self.w = self.flat.zeros() if self.scores else None
        self.anchor = FlatDict(self.flat, self.flat.theta.clone()) if self.scores else None
        self.score = self.flat.zeros() if self.scores else None
        self.score_acc = self.flat.zeros() if self.scores else None
        self.last_maxima = torch.zeros(2, dtype=torch.float32, device=self.flat.theta.device)    # {maxF, maxS}
        self._ws = None
        self.calls = 0                      # updates applied by the attached optimizer
        self.tasks_consolidated = 0

    @staticmethod
    def _check(alpha, interval, eps, who):
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError(f"{who}: alpha must be in (0, 1] (got {alpha})")
        if not float(eps) > 0.0:
            raise ValueError(f"{who}: eps must be > 0 (got {eps})")
        if int(interval) != interval or int(interval) < 1:
            raise ValueError(f"{who}: interval must be an integer >= 1 (got {interval})")

    @classmethod
    def from_config(cls, model_or_flat, config, **kw):
        """`cl_config.rwalk_lambda` / `rwalk_alpha` / `rwalk_interval` / `rwalk_eps` when the config has them (the reference's
        config.yaml has none of these keys)."""
        cc = getattr(config, "cl_config", None) or {}
        return cls(model_or_flat, rw_lambda=cc.get("rwalk_lambda", 1.0), alpha=cc.get("rwalk_alpha", 0.9),
                   interval=cc.get("rwalk_interval", 50), eps=cc.get("rwalk_eps", 1e-3), **kw)

    def _buffers(self) -> Dict[str, FlatDict]:
        return {k: getattr(self, k) for k in self._BUFFERS if getattr(self, k) is not None}

    def _next_fold(self) -> int:
        """Called by the optimizer once per applied update: counts it and says whether this one folds."""
        self.calls += 1
        return int(self.scores and self.calls % self.interval == 0)

    def penalty_value(self) -> torch.Tensor:
        """Sum importance * (theta - theta_star)^2 as a 0-dim device tensor (un-weighted, as 'mass_loss').  One pass over three
        flat buffers: call it only when the value is logged."""
        flush_pending_updates()
        f = self.flat
        val = torch.zeros(1, dtype=torch.float32, device=f.theta.device)
        st = _lib.lib().ia_cl_penalty(_lib.ptr(f.theta), _lib.ptr(self.theta_star.flat), _lib.ptr(self.importance.flat), 0.0, None,
                                      0, _lib.ptr(f.chunk_table), f.chunk_table.shape[0], None, None, _lib.ptr(val),
                                      _lib.stream_ptr())
        _lib.check(st, "ia_cl_penalty")
        return val[0]

    def consolidate(self):
        """End of a language (three launches, no host read).  Under data parallelism every rank holds the same buffers, so no
        collective is needed."""
        flush_pending_updates()
        f, L, ptr = self.flat, _lib.lib(), _lib.ptr
        nchunks = f.chunk_table.shape[0]
        if self._ws is None:
            self._ws = torch.empty(L.ia_rwalk_workspace_bytes(nchunks), dtype=torch.uint8, device=f.theta.device)
        fp = lambda d: ptr(d.flat) if d is not None else None      # the score buffers are absent with scores=False
        st = L.ia_rwalk_consolidate(ptr(f.theta), ptr(self.theta_star.flat), ptr(self.fisher.flat), fp(self.w), fp(self.anchor),
                                    fp(self.score), fp(self.score_acc), ptr(self.importance.flat), ptr(self.last_maxima),
                                    self.eps, int(self.normalize), int(self.tasks_consolidated == 0), f.numel,
                                    ptr(f.chunk_table), nchunks, ptr(self._ws), self._ws.numel(), _lib.stream_ptr())
        _lib.check(st, "ia_rwalk_consolidate")
        self.tasks_consolidated += 1

    def flat_dicts(self) -> Dict[str, FlatDict]:
        """For `checkpoint.save_cl_state(path, **rw.flat_dicts())`; `load_flat_dicts(checkpoint.load_cl_state(path, flat))` is
        the way back."""
        flush_pending_updates()
        return {"rw_" + k: d for k, d in self._buffers().items()}

    def load_flat_dicts(self, dicts, tasks_consolidated=None, calls=0):
        """Copies the buffers in place (an attached optimizer keeps pointing at them).  The file carries neither count: unless
        given, the penalty counts as attached (tasks_consolidated = 1) when the loaded importance has a non-zero entry."""
        flush_pending_updates()
        mine = self.flat_dicts()
        for key in mine:
            if key not in dicts:
                raise ValueError(f"'{key}' is missing (saved with scores={not self.scores}?)")
            if dicts[key].layout.entries != self.flat.entries:
                raise ValueError(f"'{key}' was saved for a different set of trainable tensors")
        for key, d in mine.items():
            d.flat.copy_(dicts[key].flat)
        if tasks_consolidated is None:
            tasks_consolidated = int(bool(self.importance.flat.any()))
        self.tasks_consolidated, self.calls = int(tasks_consolidated), int(calls)

    def state_dict(self) -> dict:
        flush_pending_updates()
        sd = {"entries": list(self.flat.entries), "rw_lambda": self.rw_lambda, "alpha": self.alpha, "interval": self.interval,
              "eps": self.eps, "scores": self.scores, "normalize": self.normalize, "calls": self.calls,
              "tasks_consolidated": self.tasks_consolidated}
        for k, d in self._buffers().items():
            sd[k] = d.flat.detach().to("cpu", copy=True)
        return sd

    def load_state_dict(self, sd: dict, source="state dict"):
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'rwalk' was saved for a different set of trainable tensors")
        if bool(sd["scores"]) != self.scores:
            raise ValueError(f"{source}: 'rwalk' was saved with scores={bool(sd['scores'])}, this one has scores={self.scores}")
        self._check(sd["alpha"], sd["interval"], sd["eps"], source)
        flush_pending_updates()
        for k, d in self._buffers().items():
            d.flat.copy_(sd[k])
        self.rw_lambda, self.alpha, self.interval, self.eps = (float(sd["rw_lambda"]), float(sd["alpha"]), int(sd["interval"]),
                                                               float(sd["eps"]))
        self.normalize = bool(sd["normalize"])
        self.calls, self.tasks_consolidated = int(sd["calls"]), int(sd["tasks_consolidated"])


# ----------------------------------------------------------------------------- A-GEM
class AveragedGEM:
    """Averaged GEM (Chaudhry, Ranzato, Rohrbach, Elhoseiny, ICLR 2019): the gradient `ref` of a batch drawn from an episodic
    memory of earlier tasks constrains the task gradient g.  When they point against each other (g.ref < 0) the step consumes
    g - (g.ref / ref.ref) * ref, whose product with ref is zero: to first order the step no longer raises the memory's loss.

    One flat fp32 buffer over the layout (4 B per parameter) plus {dot, ref_sq, alpha, violated} and a counter on the device.
    Attach it with `FusedAdamW(..., projection=agem)`; per step: memory batch -> backward -> `agem.store_reference(opt)`, then
    task batch -> backward -> `opt.step()`.  The two dots, the decision and the projection run inside the step, after the
    data-parallel all-reduce; nothing is read back unless `stats()` is called.  With `max_grad_norm` the order is project, then
    clip -- what `clip_grad_norm_` after a torch projection gives.  Liveness is that of the task gradient: a tensor that received
    no task gradient (another language's heads) is untouched even where `ref` is non-zero, as the usual torch implementations
    leave a `.grad` of None alone; ref.ref still runs over the whole buffer."""

    def __init__(self, model_or_flat):
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        self.ref = self.flat.zeros()
        # {dot, ref_sq, alpha, violated} as fp32 + {projected steps} as int32 in ONE device buffer (stats() reads it in one copy)
        self._buf = torch.zeros(5, dtype=torch.int32, device=self.flat.theta.device)
        self.proj_state = self._buf[:4].view(torch.float32)
        self.proj_counters = self._buf[4:]
        self._ws = None
        self.has_reference = False

    def store_reference(self, optimizer: Optional["FusedAdamW"] = None):
        """The flat gradient (of the memory batch just back-propagated) becomes `ref`; the flat gradient is then zeroed, ready
        for the task batch.  Under data parallelism `ref` is averaged over `optimizer`'s group first: a synchronous fp32
        all-reduce, then times 1/world, so every rank projects onto the same reference."""
        flush_pending_updates()
        self.ref.flat.copy_(self.flat.grad)
        if optimizer is not None:
            ws = optimizer._world()
            if ws > 1:
                dist.all_reduce(self.ref.flat, group=optimizer.group)
                self.ref.flat.mul_(1.0 / ws)
        self.flat.zero_grad()
        self.has_reference = True

    def clear(self):
        """Forget the reference: the following steps are plain steps until the next store_reference() (a deferred update
        that was issued with the reference is applied with it first)."""
        flush_pending_updates()
        self.has_reference = False

    def workspace(self, nchunks):
        if self._ws is None:
            self._ws = torch.empty(_lib.lib().ia_agem_workspace_bytes(nchunks), dtype=torch.uint8, device=self.flat.theta.device)
        return self._ws

    def stats(self) -> dict:
        """One small device-to-host read: the latest step's dot (g.ref, of the averaged gradient), ref.ref, alpha and whether it
        projected, and how many steps have projected so far."""
        flush_pending_updates()
        host = self._buf.cpu()
        dot, ref_sq, alpha, violated = host[:4].view(torch.float32).tolist()
        return {"dot": dot, "ref_sq": ref_sq, "alpha": alpha, "projected": int(violated != 0.0), "projected_steps": int(host[4])}


GEM_MAX_TASKS = 16         # IA_GEM_MAX_TASKS of include/indicasr.h
_GEM_STATE = 20            # IA_GEM_STATE_FLOATS: v[16], violated, active, iterations, solved
_GEM_SUMS = 272            # IA_GEM_SUMS_DOUBLES: d[16], Gram matrix [16, 16]


class GEM:
    """GEM (Lopez-Paz and Ranzato, NeurIPS 2017): one reference gradient r_k per earlier task, each from a batch of that task
    drawn from an episodic memory, and one constraint per task.  With d_k = <g, r_k> for the (data-parallel averaged) task
    gradient g: when no d_k is negative the step is the plain step; otherwise it consumes g + sum_k v_k r_k with
    v = argmin 1/2 v'Pv + d'v subject to v_k >= memory_strength, P = R R' + eps I -- the program the paper's code hands to
    quadprog -- so that to first order the step raises none of the earlier tasks' losses.  AveragedGEM is the cheap member of
    the family: it can agree with the mean memory gradient and still raise the loss of one task.

    Cost: the reference buffer `refs` [max_tasks, numel] is allocated here, 4 B * trainable parameters * max_tasks (1.76 GB for
    40 M parameters and 11 earlier languages), plus a few hundred bytes of solver state.  Attach it with
    `FusedAdamW(..., projection=gem)`; per step, for each earlier task: memory batch of that task
    (`EpisodicMemory.sample(n, device, language=task)`) -> backward -> `gem.store_reference(task, opt)`; then task batch ->
    backward -> `opt.step()`.  The K dots, the program and the projected step run on the device after the data-parallel
    all-reduce (ia_gem_dots, ia_gem_solve, ia_grad_norm_gem, ia_adamw_step_segmented_gem); nothing is read back unless `stats()`
    is called.  With `max_grad_norm` the order is project, then clip.  Liveness is the task gradient's, as for AveragedGEM: a
    tensor that received no task gradient stays untouched whatever the references hold there.  A non-finite reference, or a
    program the solver cannot finish, never projects: that step is the plain step and counts in `unsolved_steps`.

    Nothing of this goes into a checkpoint: the references are gradients at the current weights and are recomputed from the
    memory (which `checkpoint.py` does save) at every step."""

    def __init__(self, model_or_flat, max_tasks=11, memory_strength=0.5, eps=1e-3):
        if not 1 <= int(max_tasks) <= GEM_MAX_TASKS:
            raise ValueError(f"GEM: max_tasks must be in 1..{GEM_MAX_TASKS} (got {max_tasks})")
        if not (float(memory_strength) >= 0.0 and math.isfinite(memory_strength)):
            raise ValueError(f"GEM: memory_strength must be >= 0 (got {memory_strength})")
        if not (float(eps) >= 0.0 and math.isfinite(eps)):
            raise ValueError(f"GEM: eps must be >= 0 (got {eps})")
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        self.max_tasks, self.memory_strength, self.eps = int(max_tasks), float(memory_strength), float(eps)
        dev = self.flat.theta.device
        self.stride = (self.flat.numel + 3) // 4 * 4           # float4 loads of every row stay aligned
        self.refs = torch.zeros(self.max_tasks, self.stride, dtype=torch.float32, device=dev)
        # d[16] and the Gram matrix [16, 16] as fp64, then v[16], {violated, active, iterations, solved} as fp32 and {projected
        # steps, unsolved steps} as int32, in ONE device buffer (stats() reads it in one copy)
        self._buf = torch.zeros(2 * _GEM_SUMS + _GEM_STATE + 2, dtype=torch.int32, device=dev)
        self.sums = self._buf[:2 * _GEM_SUMS].view(torch.float64)
        self.state = self._buf[2 * _GEM_SUMS:2 * _GEM_SUMS + _GEM_STATE].view(torch.float32)
        self.counters = self._buf[2 * _GEM_SUMS + _GEM_STATE:]
        self._ws = None
        self._rows: Dict[object, int] = {}                      # task -> row of refs, in order of first use

    @property
    def has_reference(self) -> bool:
        return bool(self._rows)

    def tasks(self) -> list:
        """The tasks that hold a reference, in row order."""
        return list(self._rows)

    def workspace(self, nchunks):
        if self._ws is None:
            self._ws = torch.empty(_lib.lib().ia_gem_workspace_bytes(nchunks, self.max_tasks), dtype=torch.uint8,
                                   device=self.flat.theta.device)
        return self._ws

    def store_reference(self, task, optimizer: Optional["FusedAdamW"] = None):
        """The flat gradient (of the memory batch of `task` just back-propagated) becomes the task's row; `task` is a language
        name or any hashable and gets the next free row on first use.  Under data parallelism the row is averaged over
        `optimizer`'s group first (a synchronous fp32 all-reduce, then times 1/world), so every rank solves the same program.
        The row's dots with every stored row refresh row and column of the Gram matrix (one ia_gem_dots), and the flat
        gradient is zeroed, ready for the next batch."""
        if task not in self._rows and len(self._rows) >= self.max_tasks:
            raise ValueError(f"GEM: max_tasks = {self.max_tasks} references are stored already; '{task}' would be one more")
        flush_pending_updates()
        f = self.flat
        row = self._rows.setdefault(task, len(self._rows))
        ref = self.refs[row]
        ref[:f.numel].copy_(f.grad)
        if optimizer is not None:
            ws = optimizer._world()
            if ws > 1:
                dist.all_reduce(ref, group=optimizer.group)
                ref.mul_(1.0 / ws)
        nchunks = f.chunk_table.shape[0]
        wsp = self.workspace(nchunks)
        st = _lib.lib().ia_gem_dots(_lib.ptr(ref), _lib.ptr(self.refs), self.stride, len(self._rows), _lib.ptr(f.chunk_table),
                                    nchunks, len(f.entries), 1.0, None, row, _lib.ptr(self.sums), _lib.ptr(wsp), wsp.numel(),
                                    _lib.stream_ptr())
        _lib.check(st, "ia_gem_dots")
        f.zero_grad()

    def clear(self):
        """Forget every reference: the following steps are plain steps until the next store_reference() (a deferred update
        that was issued with the references is applied with them first).  The step counters stay."""
        flush_pending_updates()
        self._rows = {}
        self.state.zero_()
        self.sums[:GEM_MAX_TASKS].zero_()

    def gram_matrix(self) -> torch.Tensor:
        """The K x K Gram matrix R R' of the stored references as the solver reads it (fp64, on the host; eps not added)."""
        flush_pending_updates()
        k = len(self._rows)
        return self.sums[GEM_MAX_TASKS:].view(GEM_MAX_TASKS, GEM_MAX_TASKS)[:k, :k].cpu()

    def stats(self) -> dict:
        """One small device-to-host read.  Of the latest step: `dots` (d_k of the averaged gradient), `v`, both one entry per
        stored task in row order, whether it `projected`, how many v_k lie above memory_strength (`active`) and how many linear
        systems the solver factored (`qp_iterations`); and how many steps have projected / could not be solved so far."""
        flush_pending_updates()
        host = self._buf.cpu()
        k, c = len(self._rows), 2 * _GEM_SUMS + _GEM_STATE
        s = host[2 * _GEM_SUMS:c].view(torch.float32).tolist()
        return {"dots": host[:2 * k].view(torch.float64).tolist(), "v": s[:k], "projected": int(s[16] != 0.0),
                "active": int(s[17]), "qp_iterations": int(s[18]), "projected_steps": int(host[c]),
                "unsolved_steps": int(host[c + 1])}


OGD_MAX_DIRECTIONS = 4096   # IA_OGD_MAX_ROWS of include/indicasr.h


class OGD:
    """Orthogonal Gradient Descent (Farajtabar, Azizan, Mott, Li, AISTATS 2020): the member of the gradient-projection family
    that keeps no audio.  When a language is finished, a number of its loss gradients are orthonormalised and kept as the rows
    v_k of `basis`; every later step consumes g - sum_k <g, v_k> v_k for the (data-parallel averaged) gradient g, so to first
    order it does not move what those directions measured.  Use it where the earlier languages' recordings may not be retained;
    `GEM` / `AveragedGEM` need them at every step.

    Cost: `basis` [max_directions, numel] is allocated here, 4 B * trainable parameters * max_directions (69 MB per direction at
    17.3 M trainable parameters: 4.4 GB for 64 directions, 35 GB for 512), plus (max_directions + 1) floats per 4096-element chunk
    of workspace, allocated at first use.  `scope` selects the tensors that are projected, by a list of names or one regular
    expression (re.search on the name); None: every trainable tensor.  Exclude the per-language heads: a later language cannot
    move them anyway, and their part of a stored gradient would only spend the direction's norm.  Rows are zero outside the scope.

    At the end of a language, for n batches: `opt.zero_grad()` -> `training_step` -> `backward()` -> `ogd.add_direction(opt)`.
    Afterwards train as usual with `FusedAdamW(..., projection=ogd)`: once a row is stored the step runs ia_ogd_dots and
    ia_ogd_project on the flat gradient after the data-parallel all-reduce, then the norm (if measured) and the usual step: project,
    then clip.  Liveness is that of the unprojected gradient: a tensor whose projected gradient is exactly zero still takes its
    AdamW step (counter, weight decay), as torch.optim.AdamW does with a zero `.grad`.  Nothing is read back unless `stats()` is
    called.  The basis cannot be recomputed without the earlier languages' data, so unlike GEM's references it belongs in the
    checkpoint: `state_dict()` / `checkpoint.save_projection`.  Not here: a bf16 basis, a compressed basis (PCA-OGD), per-logit
    gradients (OGD-ALL) and OGD combined with GEM."""

    def __init__(self, model_or_flat, max_directions, scope=None, tol=1e-3):
        if not 1 <= int(max_directions) <= OGD_MAX_DIRECTIONS:
            raise ValueError(f"OGD: max_directions must be in 1..{OGD_MAX_DIRECTIONS} (got {max_directions})")
        if not (float(tol) > 0.0 and float(tol) < 1.0):
            raise ValueError(f"OGD: tol must be in (0, 1) (got {tol})")
        self.flat = f = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        self.max_directions, self.tol = int(max_directions), float(tol)
        self.scope_names = list(f.names) if scope is None else _select_names(f, scope, "scope=", "OGD")
        in_scope = set(self.scope_names)
        self.scope_names = [n for n in f.names if n in in_scope]          # layout order, each name once
        dev = f.theta.device
        self.seg_scope = torch.tensor([int(n in in_scope) for n in f.names], dtype=torch.int32, device=dev)
        self.stride = (f.numel + 3) // 4 * 4                                # float4 loads of every row stay aligned
        self.basis = torch.zeros(self.max_directions, self.stride, dtype=torch.float32, device=dev)
        # <g, v_k> of the latest step and <g, g> over the scope behind them, as fp64 and as fp32 (what ia_ogd_project reads);
        # the same for the gradient being inserted
        self.dots64 = torch.zeros(self.max_directions + 1, dtype=torch.float64, device=dev)
        self.dots32 = torch.zeros(self.max_directions + 1, dtype=torch.float32, device=dev)
        self._ins64, self._ins32 = torch.zeros_like(self.dots64), torch.zeros_like(self.dots32)
        self._ws = None
        self._rows = 0              # rows in use
        self._stat_rows = 0         # rows the latest step projected off: the valid entries of dots64
        self.dependent = self.nonfinite = 0

    @property
    def directions(self) -> int:
        return self._rows

    @property
    def has_reference(self) -> bool:
        return self._rows > 0

    def _device_only(self, what):
        if not self.flat.theta.is_cuda:
            raise RuntimeError(f"OGD.{what} runs on the HIP kernels: the parameters are not on the device")

    def workspace(self, nchunks):
        if self._ws is None:
            self._ws = torch.empty(_lib.lib().ia_ogd_workspace_bytes(nchunks, self.max_directions), dtype=torch.uint8,
                                   device=self.flat.theta.device)
        return self._ws

    def _dots(self, x, rows, nrows, live, out64, out32, with_sq=True):
        f = self.flat
        nchunks = f.chunk_table.shape[0]
        ws = self.workspace(nchunks)
        st = _lib.lib().ia_ogd_dots(_lib.ptr(x), _lib.ptr(rows), self.stride, f.numel, nrows, _lib.ptr(f.chunk_table), nchunks,
                                    len(f.entries), _lib.ptr(self.seg_scope), live, int(with_sq), _lib.ptr(out64),
                                    _lib.ptr(out32), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(st, "ia_ogd_dots")

    def _project(self, x, nrows, coef, live, dst, alpha=1.0):
        f = self.flat
        st = _lib.lib().ia_ogd_project(_lib.ptr(x), _lib.ptr(self.basis), self.stride, f.numel, nrows, _lib.ptr(coef),
                                       float(alpha), _lib.ptr(f.chunk_table), f.chunk_table.shape[0], len(f.entries),
                                       _lib.ptr(self.seg_scope), live, _lib.ptr(dst), _lib.stream_ptr())
        _lib.check(st, "ia_ogd_project")

    def project_step(self, live):
        """The step's part (FusedAdamW._apply): the dots of the flat gradient with every row, which also set the liveness
        flags, and the projection in place."""
        g = self.flat.grad
        self._dots(g, self.basis, self._rows, live, self.dots64, self.dots32)
        self._project(g, self._rows, self.dots32, live, g)
        self._stat_rows = self._rows

    def add_direction(self, optimizer: Optional["FusedAdamW"] = None) -> bool:
        """The flat gradient (of the batch just back-propagated) becomes a candidate direction.  Under data parallelism it is
        averaged over `optimizer`'s group first (a synchronous fp32 all-reduce, then times 1/world), so every rank keeps the
        same basis.  It is orthogonalised against the stored rows by classical Gram-Schmidt applied twice (dots, project, dots,
        project), and its residual r is kept, normalised, as the next row when |r| > tol * |g| (norms over the scope): True.
        Otherwise it is dropped and counted in `dependent` (a non-finite gradient: in `nonfinite`): False.  One small host read;
        the flat gradient is zeroed afterwards.  A full basis raises ValueError."""
        self._device_only("add_direction")
        if self._rows >= self.max_directions:
            raise ValueError(f"OGD: max_directions = {self.max_directions} directions are stored already")
        flush_pending_updates()
        f, n = self.flat, self._rows
        g, cand = f.grad, self.basis[n]
        if optimizer is not None:
            ws = optimizer._world()
            if ws > 1:
                dist.all_reduce(g, group=optimizer.group)
                g.mul_(1.0 / ws)
        if n == 0:
            cand[:f.numel].copy_(g)
            for (name, off, k, _), s in zip(f.entries, self.seg_scope.tolist()):
                if not s:
                    cand[off:off + k].zero_()
        else:
            self._dots(g, self.basis, n, None, self._ins64, self._ins32)              # entry n: <g, g> over the scope
            g_sq = self._ins64[n].clone()
            self._project(g, n, self._ins32, None, cand)
            self._dots(cand, self.basis, n, None, self._ins64, self._ins32, with_sq=False)
            self._project(cand, n, self._ins32, None, cand)
        self._dots(cand, cand, 1, None, self._ins64, self._ins32)                      # entries 0 and 1: <r, r>
        r_sq = self._ins64[1]
        g_sq, r_sq = torch.stack([r_sq if n == 0 else g_sq, r_sq]).tolist()            # the insert's one host read
        f.zero_grad()
        if not (math.isfinite(g_sq) and math.isfinite(r_sq)):
            self.nonfinite += 1
            return False
        if not math.sqrt(r_sq) > self.tol * math.sqrt(g_sq):
            self.dependent += 1
            return False
        # a true division by the norm (the root in fp64, rounded once to fp32): a one-element residual becomes exactly +-1
        cand.div_(torch.tensor(math.sqrt(r_sq), dtype=torch.float32, device=cand.device))
        self._rows = n + 1
        return True

    def clear(self):
        """Forget every direction: the following steps are plain steps until the next add_direction() (a deferred update that
        was issued with the basis is applied with it first).  The counters stay."""
        flush_pending_updates()
        self._rows = self._stat_rows = 0

    def stats(self) -> dict:
        """One small device-to-host read: `directions`; of the latest projected step `removed_fraction` = sum_k c_k^2 / |g|^2
        over the scope (the share of the averaged gradient's energy that lay along stored directions; NaN before the first
        projected step); and how many candidates were dropped as `dependent` / `nonfinite`."""
        flush_pending_updates()
        k = self._stat_rows
        frac = float("nan")
        if k:
            host = self.dots64[:k + 1].cpu()
            c, g_sq = host[:k], float(host[k])
            frac = float((c * c).sum()) / g_sq if g_sq > 0.0 else float("nan")
        return {"directions": self._rows, "removed_fraction": frac, "dependent": self.dependent, "nonfinite": self.nonfinite}

    def coefficients(self) -> torch.Tensor:
        """<g, v_k> of the latest projected step as the projection consumed them (fp32, on the host), one per row used."""
        flush_pending_updates()
        return self.dots32[:self._stat_rows].cpu()

    def state_dict(self) -> dict:
        """The rows in use (CPU), the scope, the flat layout they belong to and the counters."""
        flush_pending_updates()
        return {"entries": list(self.flat.entries), "scope": list(self.scope_names), "max_directions": self.max_directions,
                "tol": self.tol, "basis": self.basis[:self._rows, :self.flat.numel].to("cpu", copy=True),
                "dependent": self.dependent, "nonfinite": self.nonfinite}

    def load_state_dict(self, sd: dict, source="state dict"):
        """Inverse of state_dict(); refuses a state saved for another set of trainable tensors, another scope or more rows than
        this object holds."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'projection' was saved for a different set of trainable tensors")
        if list(sd["scope"]) != self.scope_names:
            raise ValueError(f"{source}: 'projection' was saved for a different scope ({len(sd['scope'])} tensors saved, "
                             f"{len(self.scope_names)} here, compared by names and order)")
        rows = sd["basis"]
        if rows.dim() != 2 or rows.shape[1] != self.flat.numel or rows.dtype != torch.float32:
            raise ValueError(f"{source}: 'projection' holds a basis of shape {tuple(rows.shape)} and dtype {rows.dtype}; "
                             f"expected [rows, {self.flat.numel}] float32")
        if rows.shape[0] > self.max_directions:
            raise ValueError(f"{source}: 'projection' holds {rows.shape[0]} directions, max_directions here is "
                             f"{self.max_directions}")
        flush_pending_updates()
        self._rows, self._stat_rows = rows.shape[0], 0
        self.basis[:self._rows, :self.flat.numel].copy_(rows)
        self.dependent, self.nonfinite = int(sd["dependent"]), int(sd["nonfinite"])


class EpisodicMemory:
    """Host-side episodic memory for replay methods: up to `per_language` utterances of every language seen, chosen by reservoir
    sampling (Vitter's algorithm R), so that each utterance of a language's stream is kept with equal probability.  Utterances
    are stored trimmed to their lengths on the CPU; `sample` re-pads them with data.speech_collate.  Every draw comes from the
    memory's own seeded generator, whose state is part of state_dict()."""

    def __init__(self, per_language: int, seed: int = 0):
        if int(per_language) < 1:
            raise ValueError(f"EpisodicMemory: per_language must be >= 1 (got {per_language})")
        self.per_language = int(per_language)
        self.gen = torch.Generator().manual_seed(int(seed))
        self.items: Dict[str, List[tuple]] = {}    # language -> [(signal [n] f32, tokens [m] i64)]
        self.seen: Dict[str, int] = {}             # language -> utterances offered so far

    def __len__(self):
        return sum(len(v) for v in self.items.values())

    def languages(self) -> List[str]:
        return list(self.items)

    def add(self, batch, lang_ids):
        """batch = (signal [B, L], signal lengths [B], tokens [B, U], token lengths [B]) on any device; lang_ids: B names."""
        sig, sig_len, tok, tok_len = (t.detach().cpu() for t in batch)
        if len(lang_ids) != sig.shape[0]:
            raise ValueError("EpisodicMemory.add: one language id per utterance")
        for i, lang in enumerate(lang_ids):
            n, m = int(sig_len[i]), int(tok_len[i])
            item = (sig[i, :n].to(torch.float32).clone(), tok[i, :m].to(torch.long).clone())
            kept = self.items.setdefault(lang, [])
            seen = self.seen.get(lang, 0)
            if len(kept) < self.per_language:
                kept.append(item)
            else:
                j = int(torch.randint(0, seen + 1, (1,), generator=self.gen))
                if j < self.per_language:
                    kept[j] = item
            self.seen[lang] = seen + 1

    def sample(self, n: int, device=None, language=None):
        """-> ((signal, signal lengths, tokens, token lengths), lang_ids): n utterances drawn uniformly (with replacement) over
        everything stored, languages mixed, collated as a training batch and moved to `device` (None: left on the host).
        `language`: draw from that language's utterances only (GEM's one batch per earlier task)."""
        from . import data
        if language is not None and not self.items.get(language):
            raise ValueError(f"EpisodicMemory.sample: nothing is stored for language '{language}'")
        pool = [(lang, it) for lang, kept in self.items.items() for it in kept if language is None or lang == language]
        if not pool:
            raise ValueError("EpisodicMemory.sample: the memory is empty")
        picks = torch.randint(0, len(pool), (int(n),), generator=self.gen).tolist()
        samples = [(pool[j][1][0], torch.tensor(pool[j][1][0].shape[0], dtype=torch.long), pool[j][1][1],
                    torch.tensor(pool[j][1][1].shape[0], dtype=torch.long)) for j in picks]
        batch = data.speech_collate(samples)
        if device is not None:
            batch = data.move_to_device(batch, device)
        return batch, [pool[j][0] for j in picks]

    def state_dict(self) -> dict:
        return {"per_language": self.per_language, "generator": self.gen.get_state(), "seen": dict(self.seen),
                "items": {lang: [(x.clone(), t.clone()) for x, t in kept] for lang, kept in self.items.items()}}

    def load_state_dict(self, sd: dict):
        self.per_language = int(sd["per_language"])
        self.gen.set_state(sd["generator"])
        self.seen = {k: int(v) for k, v in sd["seen"].items()}
        self.items = {lang: [(x.clone(), t.clone()) for x, t in kept] for lang, kept in sd["items"].items()}


# ----------------------------------------------------------------------------- Piggyback
MASK_FREE, MASK_MASKED, MASK_FROZEN = 0, 1, 2      # IA_MASK_* of include/indicasr.h
_KIND_NAMES = ("free", "masked", "frozen")
_HEAD_RE = re.compile(r"^(joint\.joint_net\.[^.]+\.[^.]+\.[^.]+|ctc_decoder\.decoder_layers\.0\.(weight|bias))$")


def _select_names(flat: FlatParams, spec, what: str, who: str = "Piggyback") -> List[str]:
    """`spec` is a list of parameter names or one regular expression (re.search on the name, as "match" of param_groups)."""
    if isinstance(spec, str):
        names = [n for n in flat.names if re.search(spec, n)]
        if not names:
            raise ValueError(f"{who}: {what} '{spec}' matches no trainable tensor")
        return names
    names, known = list(spec), set(flat.names)
    for n in names:
        if n not in known:
            raise ValueError(f"{who}: {what}: '{n}' is not a trainable tensor of this FlatParams")
    return names


def _select_kinds(flat: FlatParams, special, frozen, who: str, special_name: str) -> List[int]:
    """The kind of every trainable tensor, for Piggyback (`special` is masked=) and PackNet (packed=).  Defaults: special = tensors
    with dim() >= 2 that are not heads, free = the per-language heads, frozen = everything else.  `special` / `frozen` replace the
    default sets; a tensor named by one of them leaves the other's default set; one both name raises; what neither holds is free."""
    f = flat
    heads = {n for n in f.names if _HEAD_RE.search(n)}
    default_special = [n for n, p in zip(f.names, f.params) if p.dim() >= 2 and n not in heads]
    given_s = None if special is None else _select_names(f, special, f"{special_name}=", who)
    given_f = None if frozen is None else _select_names(f, frozen, "frozen=", who)
    both = sorted(set(given_s or ()) & set(given_f or ()))
    if both:
        raise ValueError(f"{who}: '{both[0]}' is claimed by {special_name}= and by frozen=")
    s_set = set(default_special if given_s is None else given_s) - set(given_f or ())
    f_set = (set(f.names) - heads - set(default_special) if given_f is None else set(given_f)) - s_set
    return [MASK_MASKED if n in s_set else MASK_FROZEN if n in f_set else MASK_FREE for n in f.names]


class Piggyback:
    """Piggyback (Mallya, Davis, Lazebnik, ECCV 2018): parameter isolation.  One fixed backbone `base` and, per language, a binary
    mask over its weights, trained through real-valued `scores` with the straight-through estimator: the network sees
    `base * 1[score >= threshold]`.  Nothing a language learns touches what another language uses, so forgetting is exactly zero
    and the order of the languages does not matter; a language costs 1 bit per trainable weight plus its own heads.

    Every trainable tensor has a kind, fixed here:
      masked  `flat.theta` holds base * mask; the optimizer trains the scores.  Default: tensors with dim() >= 2 that are not heads.
      free    plain AdamW as without masks, snapshotted per language.  Default: the per-language heads `joint.joint_net.*.<lang>.*`
              and the CTC head `ctc_decoder.decoder_layers.0.{weight,bias}` (one tensor with every language's rows: the
              per-language snapshot is what keeps weight decay from eroding the other languages' rows).
      frozen  never written.  Default: everything else (biases, LayerNorm / BatchNorm affine parameters).
    `masked=` / `frozen=` replace the default sets: a list of parameter names or one regular expression.  A tensor named by one
    of them leaves the other's default set; a tensor both name raises ValueError; what neither holds is free.

    Attach it with `FusedAdamW(..., masks=pb)`: the step is then ia_adamw_step_segmented_masked, one launch.  Two flat fp32 buffers
    over the layout (8 B per parameter) while training; per saved language numel / 8 bytes of bits, the free tensors and the
    module buffers (BatchNorm running statistics: frozen layers still update them in train mode).

    Limits: one language is active at a time -- `flat.theta`, `get_params`, `save_trainable` and the bf16 images show the ACTIVE
    language's masked weights, and a batch that mixes languages is out of scope.  `activate` is for evaluation: it restores the
    bits, not the scores, so training continues only after `begin_language`."""

    def __init__(self, model_or_flat, masked=None, frozen=None, threshold=5e-3, init=1e-2):
        self.flat = _as_flat(model_or_flat)
        self.threshold, self.init = float(threshold), float(init)
        if not self.init >= self.threshold:
            raise ValueError(f"Piggyback: init ({init}) must be >= threshold ({threshold}): a new language starts with every bit on")
        f = self.flat
        self._kinds = _select_kinds(f, masked, frozen, "Piggyback", "masked")
        dev = f.theta.device
        self.seg_kind = torch.tensor(self._kinds, dtype=torch.int32, device=dev)
        flush_pending_updates()
        self.base = FlatDict(f, f.theta.clone())
        self.scores = f.zeros()
        self._fill_scores()
        self.current: Optional[str] = None
        self.records: Dict[str, dict] = {}    # lang -> {"bits": int64 [numel / 64], "free": {name: tensor}, "buffers": {name: tensor}}
        self._scores_lang: Optional[str] = None    # the language the scores describe (None: nobody's yet)
        self._stale = False                    # True while theta shows a language the scores do not describe
        self._optimizer = None                 # weak reference to the FusedAdamW that holds the bf16 shadow
        self._scratch = None

    # -- kinds -----------------------------------------------------------------------------------------------------
    def kinds(self) -> Dict[str, str]:
        return {n: _KIND_NAMES[k] for n, k in zip(self.flat.names, self._kinds)}

    def _names_of(self, kind):
        return [n for n, k in zip(self.flat.names, self._kinds) if k == kind]

    def languages(self) -> List[str]:
        return list(self.records)

    def _fill_scores(self):
        for n in self._names_of(MASK_MASKED):
            self.scores[n].fill_(self.init)

    def _shadow(self):
        opt = self._optimizer() if self._optimizer is not None else None
        return opt, (opt.shadow if opt is not None else None)

    # -- bits <-> weights ------------------------------------------------------------------------------------------
    def _pack(self, out=None, kept=None) -> torch.Tensor:
        f = self.flat
        if out is None:
            out = torch.empty(f.numel // 64, dtype=torch.int64, device=f.theta.device)
        st = _lib.lib().ia_mask_pack(_lib.ptr(self.scores.flat), _lib.ptr(f.chunk_table), f.chunk_table.shape[0],
                                     _lib.ptr(self.seg_kind), len(f.entries), self.threshold, _lib.ptr(out), out.numel(),
                                     _lib.ptr(kept), _lib.stream_ptr())
        _lib.check(st, "ia_mask_pack")
        return out

    def _apply_bits(self, bits):
        """theta = bit ? base : 0 on masked tensors and the bf16 image of every tensor, one launch; then what
        FusedAdamW._after_update does: the weight epoch moves and the flat shadow views are handed to the shadow cache."""
        f = self.flat
        opt, shadow = self._shadow()
        st = _lib.lib().ia_mask_apply(_lib.ptr(f.theta), _lib.ptr(self.base.flat), _lib.ptr(bits), bits.numel(),
                                      _lib.ptr(f.chunk_table), f.chunk_table.shape[0], _lib.ptr(self.seg_kind), len(f.entries),
                                      _lib.ptr(shadow), _lib.stream_ptr())
        _lib.check(st, "ia_mask_apply")
        if opt is not None:
            opt._after_update()
        else:
            from .ops import fast
            fast.bump_weight_epoch()

    # -- the per-language loop ---------------------------------------------------------------------------------------
    def save_language(self, lang: Optional[str] = None):
        """Record `lang` (default: the current language): the bits of the scores, the free tensors and every module buffer.
        Before any masked training every bit is on: this is how the language the backbone was trained on is recorded."""
        lang = self.current if lang is None else lang
        if lang is None:
            raise ValueError("Piggyback.save_language: no language is current; name one")
        if self._stale:
            raise RuntimeError(f"Piggyback.save_language: the weights show '{self.current}' as activate() restored it, but the "
                               "scores belong to another language; call begin_language() before training and saving")
        flush_pending_updates()
        f = self.flat
        self.records[lang] = {
            "bits": self._pack(),
            "free": {n: f._theta_views[n].detach().clone() for n in self._names_of(MASK_FREE)},
            "buffers": {n: b.detach().clone() for n, b in f.model.named_buffers()}}
        self.current = self._scores_lang = lang

    def begin_language(self, lang: str, optimizer: Optional["FusedAdamW"] = None):
        """Start training `lang`: scores = init, so every bit is on and theta equals base on the masked tensors; the free tensors
        and buffers continue from where they are.  With an optimizer, the moments and step counters of every tensor that is not
        frozen are zeroed (a frozen tensor's are never read)."""
        flush_pending_updates()
        self._fill_scores()
        if optimizer is not None:
            if optimizer.flat is not self.flat:
                raise ValueError("optimizer belongs to another FlatParams")
            for k, (n, o, cnt, shape) in enumerate(self.flat.entries):
                if self._kinds[k] != MASK_FROZEN:
                    optimizer.exp_avg[o:o + cnt].zero_()
                    optimizer.exp_avg_sq[o:o + cnt].zero_()
            optimizer.seg_step.mul_((self.seg_kind == MASK_FROZEN).to(torch.int32))
        self._apply_bits(self._pack())
        self.current, self._scores_lang, self._stale = lang, lang, False

    def activate(self, lang: str):
        """Show `lang` to the network: its free tensors and buffers come back, then one launch rewrites the masked weights from
        its bits and the whole bf16 image; every cached derived weight image is re-made on its next use.  Progress of the
        current language that save_language() has not recorded is lost (its heads are overwritten); after save_language(x),
        activate(other), ..., activate(x) training x continues where it was."""
        if lang not in self.records:
            raise ValueError(f"Piggyback.activate: unknown language '{lang}' (saved: {', '.join(self.records) or 'none'})")
        flush_pending_updates()
        rec, f = self.records[lang], self.flat
        with torch.no_grad():
            for n, t in rec["free"].items():
                f._theta_views[n].copy_(t)
            buffers = dict(f.model.named_buffers())
            for n, t in rec["buffers"].items():
                buffers[n].copy_(t)
        self._apply_bits(rec["bits"])
        self.current, self._stale = lang, lang != self._scores_lang

    # -- reports ---------------------------------------------------------------------------------------------------
    def sparsity(self) -> Dict[str, float]:
        """name -> fraction of bits ON, for the masked tensors, from the scores as they are now: one pack into scratch and one
        small device-to-host read."""
        flush_pending_updates()
        f = self.flat
        if self._scratch is None:
            self._scratch = (torch.empty(f.numel // 64, dtype=torch.int64, device=f.theta.device),
                             torch.zeros(len(f.entries), dtype=torch.int32, device=f.theta.device))
        self._pack(*self._scratch)
        kept = self._scratch[1].tolist()
        return {e[0]: kept[k] / e[2] for k, e in enumerate(f.entries) if self._kinds[k] == MASK_MASKED}

    def bytes_per_language(self) -> dict:
        """Bytes one saved language holds: the bits (1 per flat element), the free tensors and the module buffers."""
        f = self.flat
        free = sum(e[2] * 4 for k, e in enumerate(f.entries) if self._kinds[k] == MASK_FREE)
        buffers = sum(b.numel() * b.element_size() for b in f.model.buffers())
        mask = f.numel // 64 * 8
        return {"mask": mask, "free": free, "buffers": buffers, "total": mask + free + buffers}

    # -- resumable state -------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        flush_pending_updates()
        cpu = lambda t: t.detach().to("cpu", copy=True)
        return {"entries": list(self.flat.entries), "kinds": [_KIND_NAMES[k] for k in self._kinds], "threshold": self.threshold,
                "init": self.init, "base": cpu(self.base.flat), "scores": cpu(self.scores.flat), "current": self.current,
                "scores_language": self._scores_lang,
                "languages": {lang: {"bits": cpu(r["bits"]), "free": {n: cpu(t) for n, t in r["free"].items()},
                                     "buffers": {n: cpu(t) for n, t in r["buffers"].items()}}
                              for lang, r in self.records.items()}}

    def load_state_dict(self, sd: dict, source="state dict"):
        """In place: base, scores and the kind table keep their addresses (an attached optimizer keeps pointing at them).  The
        weights are not part of this state: `activate(lang)` or `begin_language(lang)` puts them in step with it."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'masks' was saved for a different set of trainable tensors")
        kinds = [_KIND_NAMES.index(k) for k in sd["kinds"]]
        if not float(sd["init"]) >= float(sd["threshold"]):
            raise ValueError(f"{source}: init must be >= threshold")
        flush_pending_updates()
        dev = self.flat.theta.device
        self.base.flat.copy_(sd["base"])
        self.scores.flat.copy_(sd["scores"])
        self._kinds = kinds
        self.seg_kind.copy_(torch.tensor(kinds, dtype=torch.int32))
        self.threshold, self.init = float(sd["threshold"]), float(sd["init"])
        self.current, self._scores_lang = sd["current"], sd["scores_language"]
        self._stale = False                    # the weights are the caller's to restore
        self.records = {lang: {"bits": r["bits"].to(dev), "free": {n: t.to(dev) for n, t in r["free"].items()},
                               "buffers": {n: t.to(dev) for n, t in r["buffers"].items()}}
                        for lang, r in sd["languages"].items()}


# ----------------------------------------------------------------------------- PackNet
_PACK_KIND_NAMES = ("free", "packed", "frozen")       # the numbering of _KIND_NAMES, `packed` in the masked slot
_PACK_PHASES = (None, "train", "retrain", "finished")


class PackNet:
    """PackNet (Mallya, Lazebnik, CVPR 2018): parameter isolation by weight ownership.  All languages share `flat.theta`; one byte
    per weight (`owner`) says whose it is: 0 free, t >= 1 the t-th language's.  A language trains the free weights beside
    everything the earlier languages own, then `prune` releases the smallest-magnitude fraction of the weights it used (they are
    set to +0 and stay free) and the rest become its property; a short retraining moves only those.  Nothing a later language
    does touches an owned weight, so forgetting is exactly zero; unlike Piggyback every language trains weights of its own.

    The kinds are Piggyback's, with the same defaults and overrides (`packed=` in the place of `masked=`):
      packed  the owner map decides per element.  Default: tensors with dim() >= 2 that are not heads.
      free    plain AdamW, snapshotted per language.  Default: the per-language heads.
      frozen  never written.  Default: everything else.

        pn  = PackNet(model_or_flat, prune=0.5)
        opt = FusedAdamW(flat, ..., masks=pn)     # the step is ia_adamw_step_segmented_packed, one launch
        pn.begin_language("hi", opt)              # task t = number of languages + 1; train_owner = 0
        ...train...
        pn.prune(opt)                             # ia_pack_prune on the device; train_owner = t
        ...retrain...                             # only language t's weights move; the released ones stay +0
        pn.finish_language()                      # base <- theta, heads and module buffers recorded; train_owner = -1
        pn.activate("hi")                         # theta = 1 <= owner <= task("hi") ? base : 0, heads and buffers restored

    State: the owner map (1 B per flat element) and `base`, the weights as the latest finished language left them (4 B), against
    Piggyback's two fp32 buffers (8 B) while training; per language only its free tensors and the module buffers.  While no
    language is open train_owner is -1 and a step moves no packed weight.

    Limits: one language is active at a time, as with Piggyback; a language sees the weights of the languages before it, so the
    order matters; at most 255 languages."""

    def __init__(self, model_or_flat, packed=None, frozen=None, prune=0.5):
        self.flat = _as_flat(model_or_flat)
        self.prune_fraction = self._checked_fraction(prune)
        f = self.flat
        self._kinds = _select_kinds(f, packed, frozen, "PackNet", "packed")
        dev = f.theta.device
        self.seg_kind = torch.tensor(self._kinds, dtype=torch.int32, device=dev)
        flush_pending_updates()
        self.base = FlatDict(f, f.theta.clone())
        self.owner = torch.zeros(f.numel, dtype=torch.uint8, device=dev)
        self.seg_counts = torch.zeros(len(f.entries), 2, dtype=torch.int32, device=dev)    # {released, newly owned} of the last prune
        self.current: Optional[str] = None
        self.phase: Optional[str] = None       # None | "train" | "retrain" | "finished"
        self.train_owner = -1
        self.tasks: Dict[str, int] = {}        # lang -> task index, in language order (the open language included)
        self.records: Dict[str, dict] = {}     # finished lang -> {"task": int, "free": {name: tensor}, "buffers": {name: tensor}}
        self._optimizer = None                 # weak reference to the FusedAdamW that holds the moments and the bf16 shadow
        self._workspace = None

    @staticmethod
    def _checked_fraction(fraction) -> float:
        fraction = float(fraction)
        if not 0.0 <= fraction < 1.0:
            raise ValueError(f"PackNet: prune fraction {fraction} is outside [0, 1)")
        return fraction

    # -- kinds -----------------------------------------------------------------------------------------------------
    def kinds(self) -> Dict[str, str]:
        return {n: _PACK_KIND_NAMES[k] for n, k in zip(self.flat.names, self._kinds)}

    def _names_of(self, kind):
        return [n for n, k in zip(self.flat.names, self._kinds) if k == kind]

    def _packed_entries(self):
        return [e for k, e in enumerate(self.flat.entries) if self._kinds[k] == MASK_MASKED]

    def languages(self) -> List[str]:
        return list(self.records)

    def _attached(self, optimizer=None):
        opt = optimizer if optimizer is not None else (self._optimizer() if self._optimizer is not None else None)
        if opt is not None and opt.flat is not self.flat:
            raise ValueError("optimizer belongs to another FlatParams")
        return opt

    def _weights_changed(self, opt):
        """What FusedAdamW._after_update does: the weight epoch moves and the flat shadow views go to the shadow cache."""
        if opt is not None:
            opt._after_update()
        else:
            from .ops import fast
            fast.bump_weight_epoch()

    def _apply_owners(self, lo, hi):
        """theta = lo <= owner <= hi ? base : +0 on packed tensors and the bf16 image of every tensor, one launch."""
        f, opt = self.flat, self._attached()
        st = _lib.lib().ia_pack_apply(_lib.ptr(f.theta), _lib.ptr(self.base.flat), _lib.ptr(self.owner), _lib.ptr(f.chunk_table),
                                      f.chunk_table.shape[0], _lib.ptr(self.seg_kind), len(f.entries), int(lo), int(hi),
                                      _lib.ptr(opt.shadow if opt is not None else None), _lib.stream_ptr())
        _lib.check(st, "ia_pack_apply")
        self._weights_changed(opt)

    # -- the per-language loop ---------------------------------------------------------------------------------------
    def begin_language(self, lang: str, optimizer: Optional["FusedAdamW"] = None):
        """Open `lang` as task number of languages + 1 and train the free weights (train_owner = 0).  The first language keeps
        theta as it is: it prunes the pretrained network.  Later ones start from `owner >= 1 ? base : +0`.  With an optimizer
        (given, or attached through masks=) the moments and step counters of every tensor that is not frozen are zeroed."""
        if self.phase in ("train", "retrain"):
            raise RuntimeError(f"PackNet.begin_language: '{self.current}' is still open (phase '{self.phase}'); prune() and "
                               "finish_language() first")
        if lang in self.tasks:
            raise ValueError(f"PackNet.begin_language: '{lang}' has been trained already; activate() shows it")
        task = len(self.records) + 1
        if task > 255:
            raise ValueError("PackNet: the owner map holds at most 255 languages")
        opt = self._attached(optimizer)
        flush_pending_updates()
        packed = self._packed_entries()
        free = torch.stack([(self.owner[o:o + k] == 0).sum() for _, o, k, _ in packed]).sum() if packed else None
        if free is None or int(free) == 0:          # one small device read per language
            raise RuntimeError(f"PackNet.begin_language: no packed tensor has a free weight left for '{lang}'")
        if optimizer is not None:
            self._optimizer = weakref.ref(optimizer)
        if self.records:
            self._apply_owners(1, 255)
        if opt is not None:
            for k, (n, o, cnt, shape) in enumerate(self.flat.entries):
                if self._kinds[k] != MASK_FROZEN:
                    opt.exp_avg[o:o + cnt].zero_()
                    opt.exp_avg_sq[o:o + cnt].zero_()
            opt.seg_step.mul_((self.seg_kind == MASK_FROZEN).to(torch.int32))
        self.tasks[lang] = task
        self.current, self.phase, self.train_owner = lang, "train", 0

    def prune(self, optimizer: Optional["FusedAdamW"] = None, fraction: Optional[float] = None):
        """Per packed tensor, release the `fraction` (default: the constructor's) of its free weights with the smallest magnitude
        and give the rest to the open language; the moments of the packed tensors are zeroed and their step counters with them.
        From here on only the language's own weights move (train_owner = its task).  No host synchronisation."""
        if self.phase != "train":
            raise RuntimeError("PackNet.prune: " + ("no language is open; call begin_language() first" if self.phase != "retrain"
                                                    else f"'{self.current}' has been pruned already"))
        fraction = self.prune_fraction if fraction is None else self._checked_fraction(fraction)
        opt = self._attached(optimizer)
        if opt is None:
            raise RuntimeError("PackNet.prune: no optimizer is attached (FusedAdamW(..., masks=pn)) and none was given: the "
                               "pruning resets its moments")
        flush_pending_updates()
        f, L, task = self.flat, _lib.lib(), self.tasks[self.current]
        nseg = len(f.entries)
        if self._workspace is None:
            self._workspace = torch.empty(L.ia_pack_prune_workspace_bytes(nseg), dtype=torch.uint8, device=f.theta.device)
        st = L.ia_pack_prune(_lib.ptr(f.theta), _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq), _lib.ptr(self.owner),
                             _lib.ptr(f.chunk_table), f.chunk_table.shape[0], _lib.ptr(self.seg_kind), nseg, fraction, task,
                             _lib.ptr(opt.shadow), _lib.ptr(self.seg_counts), _lib.ptr(self._workspace), self._workspace.numel(),
                             _lib.stream_ptr())
        _lib.check(st, "ia_pack_prune")
        opt.seg_step.mul_((self.seg_kind != MASK_MASKED).to(torch.int32))
        self._weights_changed(opt)
        self.phase, self.train_owner = "retrain", task

    def finish_language(self):
        """Close the open language after its retraining: base <- theta, its free tensors and every module buffer are recorded, and
        train_owner = -1, so that no packed weight moves until the next begin_language()."""
        if self.phase != "retrain":
            raise RuntimeError("PackNet.finish_language: " + (f"'{self.current}' has not been pruned; call prune() first"
                                                              if self.phase == "train" else "no language is open"))
        flush_pending_updates()
        f = self.flat
        self.base.flat.copy_(f.theta)
        self.records[self.current] = {
            "task": self.tasks[self.current],
            "free": {n: f._theta_views[n].detach().clone() for n in self._names_of(MASK_FREE)},
            "buffers": {n: b.detach().clone() for n, b in f.model.named_buffers()}}
        self.phase, self.train_owner = "finished", -1

    def activate(self, lang: str):
        """Show finished language `lang` to the network: its free tensors and buffers come back, then one launch rewrites the
        packed weights as `1 <= owner <= task(lang) ? base : +0` and the whole bf16 image."""
        if lang not in self.records:
            raise ValueError(f"PackNet.activate: unknown language '{lang}' (finished: {', '.join(self.records) or 'none'})")
        if self.phase in ("train", "retrain"):
            raise RuntimeError(f"PackNet.activate: '{self.current}' is still open; finish_language() first")
        flush_pending_updates()
        rec, f = self.records[lang], self.flat
        with torch.no_grad():
            for n, t in rec["free"].items():
                f._theta_views[n].copy_(t)
            buffers = dict(f.model.named_buffers())
            for n, t in rec["buffers"].items():
                buffers[n].copy_(t)
        self._apply_owners(1, rec["task"])
        self.current = lang

    # -- reports ---------------------------------------------------------------------------------------------------
    def usage(self) -> Dict[str, dict]:
        """name -> {"owned": {language: fraction of the tensor it owns, in language order}, "free": fraction still free} for the
        packed tensors: plain torch ops and one device-to-host read."""
        flush_pending_updates()
        packed = self._packed_entries()
        if not packed:
            return {}
        counts = torch.stack([torch.bincount(self.owner[o:o + k].to(torch.int64), minlength=256) for _, o, k, _ in packed]).tolist()
        return {n: {"owned": {lang: row[t] / k for lang, t in self.tasks.items()}, "free": row[0] / k}
                for (n, o, k, _), row in zip(packed, counts)}

    def free_fraction(self) -> float:
        """Fraction of all packed weights that no language owns."""
        flush_pending_updates()
        packed = self._packed_entries()
        total = sum(e[2] for e in packed)
        return float(torch.stack([(self.owner[o:o + k] == 0).sum() for _, o, k, _ in packed]).sum()) / total if total else 0.0

    def bytes_per_language(self) -> dict:
        """Bytes one finished language holds (its free tensors and the module buffers), beside what all languages share: the
        owner map (1 B per flat element) and base (4 B)."""
        f = self.flat
        free = sum(e[2] * 4 for k, e in enumerate(f.entries) if self._kinds[k] == MASK_FREE)
        buffers = sum(b.numel() * b.element_size() for b in f.model.buffers())
        return {"free": free, "buffers": buffers, "total": free + buffers, "shared_owner_map": f.numel, "shared_base": 4 * f.numel}

    # -- resumable state -------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        flush_pending_updates()
        cpu = lambda t: t.detach().to("cpu", copy=True)
        return {"entries": list(self.flat.entries), "kinds": [_PACK_KIND_NAMES[k] for k in self._kinds],
                "prune": self.prune_fraction, "owner": cpu(self.owner), "base": cpu(self.base.flat), "current": self.current,
                "phase": self.phase, "tasks": dict(self.tasks),
                "languages": {lang: {"task": r["task"], "free": {n: cpu(t) for n, t in r["free"].items()},
                                     "buffers": {n: cpu(t) for n, t in r["buffers"].items()}}
                              for lang, r in self.records.items()}}

    def load_state_dict(self, sd: dict, source="state dict"):
        """In place: owner map, base and the kind table keep their addresses (an attached optimizer keeps pointing at them).  The
        weights are not part of this state: `activate(lang)` puts them in step with it, or the weights of a checkpoint taken at
        the same moment when a language was open."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'masks' was saved for a different set of trainable tensors")
        if "owner" not in sd:
            raise ValueError(f"{source}: 'masks' does not hold a PackNet owner map")
        kinds = [_PACK_KIND_NAMES.index(k) for k in sd["kinds"]]
        fraction = self._checked_fraction(sd["prune"])
        if sd["phase"] not in _PACK_PHASES:
            raise ValueError(f"{source}: unknown phase '{sd['phase']}'")
        flush_pending_updates()
        dev = self.flat.theta.device
        self.owner.copy_(sd["owner"])
        self.base.flat.copy_(sd["base"])
        self._kinds = kinds
        self.seg_kind.copy_(torch.tensor(kinds, dtype=torch.int32))
        self.prune_fraction = fraction
        self.current, self.phase, self.tasks = sd["current"], sd["phase"], {k: int(v) for k, v in sd["tasks"].items()}
        self.train_owner = {"train": 0, "retrain": self.tasks.get(self.current, -1)}.get(self.phase, -1)
        self.records = {lang: {"task": int(r["task"]), "free": {n: t.to(dev) for n, t in r["free"].items()},
                               "buffers": {n: t.to(dev) for n, t in r["buffers"].items()}}
                        for lang, r in sd["languages"].items()}


# ----------------------------------------------------------------------------- LoRA
_LORA_KIND_NAMES = ("free", "adapted", "frozen")      # the numbering of _KIND_NAMES, `adapted` in the masked slot
LORA_MAX_RANK = 64         # IA_LORA_MAX_RANK of include/indicasr.h


class LoRA:
    """LoRA (Hu et al. 2021): low-rank adaptation, one pair of thin factors per adapted matrix and language.  One fixed backbone
    `base` is kept; adapted tensor W, viewed as [m, n] with m = shape[0] and n = numel / m (the view the bf16 shadow has), reads
    `base + s * B @ A` with B [m, r], A [r, n] and s = alpha / r.  A language costs r * (m + n) numbers per matrix instead of
    m * n, forgetting is exactly zero, and inference costs nothing: the factors are folded into `flat.theta` and its bf16 image.

    The route is Piggyback's and PackNet's: forward and backward are left alone, the existing backward produces the full dW, and
    the optimizer step turns it into factor gradients (ia_lora_grad), trains the factors with the shared AdamW rule and rewrites
    the weights and the shadow (ia_lora_apply).  So LoRA's storage, zero-forgetting and zero-inference-cost properties are kept;
    its training-FLOP saving is NOT: dW is still computed in full.

    Every trainable tensor has a kind, fixed here (the vocabulary and numbering of Piggyback's `seg_kind`):
      adapted  theta = base + s * B @ A; the optimizer trains B and A.  Default: tensors with dim() >= 2 that are not heads and
               have min(m, n) >= 2 * rank.
      free     plain AdamW, snapshotted per language.  Default: the per-language heads, as for Piggyback.
      frozen   never written.  Default: everything else -- biases and norm parameters, and every dim() >= 2 tensor that is not a
               head and is too small for the rank (the depthwise kernels [d, 1, k]).
    `adapted=` / `frozen=` replace the default sets as `masked=` / `frozen=` do for Piggyback; an explicitly adapted tensor with
    min(m, n) < rank raises ValueError.

        lora = LoRA(model_or_flat, rank=8, alpha=16.0)
        opt  = FusedAdamW(flat, ..., masks=lora)
        lora.begin_language("hi", opt)      # B = 0, A ~ U(-1/sqrt(n), 1/sqrt(n)) (peft's kaiming_uniform_(a=sqrt(5))); theta = base
        ...train...
        lora.save_language()                # factors, free tensors and module buffers
        lora.activate("hi")                 # theta = base + s * B @ A of "hi", heads and buffers restored

    A is drawn on the CPU from a generator seeded by (seed, crc32(lang), tensor index): every rank draws the same values.

    Limits: one language is active at a time, as with Piggyback.  There is no `lora_dropout`: the factors are folded into the
    weights before the forward, so there is no separate low-rank branch whose input could be dropped.  Adapted tensors must be in
    the flat layout, which holds trainable tensors only (requires_grad=True on the backbone matrices that are adapted).  The
    optimizer's full-size moments of adapted tensors stay allocated and unused."""

    def __init__(self, model_or_flat, rank=8, alpha=16.0, adapted=None, frozen=None, seed=0):
        self.flat = _as_flat(model_or_flat)
        f = self.flat
        if int(rank) != rank or not 1 <= int(rank) <= LORA_MAX_RANK:
            raise ValueError(f"LoRA: rank {rank} is outside 1..{LORA_MAX_RANK}")
        self.rank, self.alpha, self.seed = int(rank), float(alpha), int(seed)
        self.scale = ctypes.c_float(self.alpha / self.rank).value       # s as the kernels take it
        kinds = _select_kinds(f, adapted, frozen, "LoRA", "adapted")
        for k, (n, o, numel, shape) in enumerate(f.entries):
            if kinds[k] != MASK_MASKED:
                continue
            small = min(shape[0], numel // shape[0])
            if adapted is None:
                if small < 2 * self.rank:
                    kinds[k] = MASK_FROZEN
            elif small < self.rank:
                raise ValueError(f"LoRA: '{n}' viewed as [{shape[0]}, {numel // shape[0]}] is too small for rank {self.rank}")
        self._kinds = kinds
        if MASK_MASKED not in kinds:
            raise ValueError(f"LoRA: no trainable tensor is adapted at rank {self.rank}")
        dev = f.theta.device
        self.seg_kind = torch.tensor(kinds, dtype=torch.int32, device=dev)
        # what the plain step sees: an adapted tensor is not its to write
        self.step_kind = torch.tensor([MASK_FREE if k == MASK_FREE else MASK_FROZEN for k in kinds], dtype=torch.int32, device=dev)
        self._build_layout()
        flush_pending_updates()
        self.base = FlatDict(f, f.theta.clone())
        nf = self.factor_numel
        self.factors = torch.zeros(nf, dtype=torch.float32, device=dev)
        self.factor_grad = torch.zeros(nf, dtype=torch.float32, device=dev)
        self.factor_exp_avg = torch.zeros(nf, dtype=torch.float32, device=dev)
        self.factor_exp_avg_sq = torch.zeros(nf, dtype=torch.float32, device=dev)
        self.factor_step = torch.zeros(2 * len(self.adapted), dtype=torch.int32, device=dev)
        self.factor_active = torch.zeros(2 * len(self.adapted), dtype=torch.int32, device=dev)
        self.current: Optional[str] = None
        self.records: Dict[str, dict] = {}    # lang -> {"factors": fp32 [factor_numel], "free": {name: tensor}, "buffers": {...}}
        self._factors_lang: Optional[str] = None   # the language the live factors describe (None: nobody's yet)
        self._stale = False                    # True while theta shows a language the live factors do not describe
        self._optimizer = None                 # weak reference to the FusedAdamW that holds the bf16 shadow
        self._workspace = None
        self._factor_group = None              # (optimizer id, int32 [2 * adapted]): the parameter group of every factor's parent

    def _build_layout(self):
        """The factor buffer (per adapted tensor B [m, r] then A [r, n], each on a 64-float boundary), its chunk table, the tile
        list of ia_lora_grad and where every tensor's partial sums lie in the workspace."""
        f, r, L = self.flat, self.rank, _lib.lib()
        rows_per, cols_per = L.ia_lora_tile_rows(), L.ia_lora_tile_cols()
        up = lambda x: (x + _ALIGN - 1) // _ALIGN * _ALIGN
        self.adapted = []                      # (name, index in the flat layout, m, n, offset of B, offset of A)
        desc, tiles, chunks, seg_tensor = [], [], [], [-1] * len(f.entries)
        off = ws = 0
        for k, (name, o, numel, shape) in enumerate(f.entries):
            if self._kinds[k] != MASK_MASKED:
                continue
            t, m = len(self.adapted), shape[0]
            n = numel // m
            b_off, a_off = off, off + up(m * r)
            off = a_off + up(r * n)
            nrt, nct = (m + rows_per - 1) // rows_per, (n + cols_per - 1) // cols_per
            nbytes = L.ia_lora_workspace_bytes(m, n, r)
            if nbytes < 4 * r * (nct * m + nrt * n) or nbytes % 4:
                raise RuntimeError(f"ia_lora_workspace_bytes({m}, {n}, {r}) returned {nbytes}")
            desc.append((o, m, n, b_off, a_off, ws, ws + nct * m * r, k))
            ws += nbytes // 4
            tiles += [(t, rt, ct, 0) for rt in range(nrt) for ct in range(nct)]
            for which, (start, cnt) in enumerate(((b_off, m * r), (a_off, r * n))):
                chunks += [(start + c0, min(4096, cnt - c0), 2 * t + which, t) for c0 in range(0, cnt, 4096)]
            seg_tensor[k] = t
            self.adapted.append((name, k, m, n, b_off, a_off))
        dev = f.theta.device
        self.factor_numel, self.workspace_bytes = off, 4 * ws
        self.tensor_table = torch.tensor(desc, dtype=torch.int64, device=dev)
        self.tile_table = torch.tensor(tiles, dtype=torch.int32, device=dev)
        self.factor_table = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self.seg_tensor = torch.tensor(seg_tensor, dtype=torch.int32, device=dev)

    # -- kinds -----------------------------------------------------------------------------------------------------
    def kinds(self) -> Dict[str, str]:
        return {n: _LORA_KIND_NAMES[k] for n, k in zip(self.flat.names, self._kinds)}

    def _names_of(self, kind):
        return [n for n, k in zip(self.flat.names, self._kinds) if k == kind]

    def languages(self) -> List[str]:
        return list(self.records)

    def _shadow(self):
        opt = self._optimizer() if self._optimizer is not None else None
        return opt, (opt.shadow if opt is not None else None)

    def factor_views(self, factors: Optional[torch.Tensor] = None) -> Dict[str, dict]:
        """name -> {"lora_A": view [r, n], "lora_B": view [m, r]} into a factor buffer (default: the live one)."""
        fb = self.factors if factors is None else factors
        return {name: {"lora_A": fb[a:a + self.rank * n].view(self.rank, n), "lora_B": fb[b:b + m * self.rank].view(m, self.rank)}
                for name, k, m, n, b, a in self.adapted}

    # -- factors -> weights ------------------------------------------------------------------------------------------
    def _materialise(self, factors, theta=None, base=None, shadow=None, norm_state=None, skip=False):
        f = self.flat
        st = _lib.lib().ia_lora_apply(_lib.ptr(f.theta if theta is None else theta), _lib.ptr(self.base.flat if base is None else base),
                                      _lib.ptr(factors), _lib.ptr(self.tensor_table), len(self.adapted), _lib.ptr(self.seg_tensor),
                                      _lib.ptr(f.chunk_table), f.chunk_table.shape[0], len(f.entries), self.rank, self.scale,
                                      _lib.ptr(shadow), _lib.ptr(norm_state), int(skip), _lib.stream_ptr())
        _lib.check(st, "ia_lora_apply")

    def _apply_factors(self, factors):
        """theta = base + s * B @ A on adapted tensors and the bf16 image of every tensor, one launch; then what
        FusedAdamW._after_update does: the weight epoch moves and the flat shadow views are handed to the shadow cache."""
        opt, shadow = self._shadow()
        self._materialise(factors, shadow=shadow)
        if opt is not None:
            opt._after_update()
        else:
            from .ops import fast
            fast.bump_weight_epoch()

    def _seed_of(self, lang: str, index: int) -> int:
        import zlib
        x = self.seed & 0x7FFFFFFFFFFFFFFF
        for v in (zlib.crc32(lang.encode("utf-8")), index):
            x = (x * 6364136223846793005 + v + 1442695040888963407) & 0x7FFFFFFFFFFFFFFF
        return x

    # -- the per-language loop ---------------------------------------------------------------------------------------
    def save_language(self, lang: Optional[str] = None):
        """Record `lang` (default: the current language): its factors, the free tensors and every module buffer."""
        lang = self.current if lang is None else lang
        if lang is None:
            raise ValueError("LoRA.save_language: no language is current; name one")
        if self._stale:
            raise RuntimeError(f"LoRA.save_language: the weights show '{self.current}' as activate() restored it, but the "
                               "live factors belong to another language; call begin_language() before training and saving")
        flush_pending_updates()
        f = self.flat
        self.records[lang] = {
            "factors": self.factors.detach().clone(),
            "free": {n: f._theta_views[n].detach().clone() for n in self._names_of(MASK_FREE)},
            "buffers": {n: b.detach().clone() for n, b in f.model.named_buffers()}}
        self.current = self._factors_lang = lang

    def begin_language(self, lang: str, optimizer: Optional["FusedAdamW"] = None):
        """Start training `lang`: B = 0 and A ~ U(-1/sqrt(n), 1/sqrt(n)), so theta equals base on the adapted tensors; the factor
        moments and step counters are zeroed; the free tensors and buffers continue from where they are.  With an optimizer, its
        moments and step counters of every tensor that is not frozen are zeroed too, as Piggyback does."""
        flush_pending_updates()
        if optimizer is not None and optimizer.flat is not self.flat:
            raise ValueError("optimizer belongs to another FlatParams")
        with torch.no_grad():
            self.factors.zero_()
            views = self.factor_views()
            for name, k, m, n, b, a in self.adapted:
                gen = torch.Generator().manual_seed(self._seed_of(lang, k))
                bound = 1.0 / math.sqrt(n)
                views[name]["lora_A"].copy_(torch.empty(self.rank, n, dtype=torch.float32).uniform_(-bound, bound, generator=gen))
            self.factor_exp_avg.zero_()
            self.factor_exp_avg_sq.zero_()
            self.factor_step.zero_()
            self.factor_active.zero_()
        if optimizer is not None:
            for k, (n, o, cnt, shape) in enumerate(self.flat.entries):
                if self._kinds[k] != MASK_FROZEN:
                    optimizer.exp_avg[o:o + cnt].zero_()
                    optimizer.exp_avg_sq[o:o + cnt].zero_()
            optimizer.seg_step.mul_((self.seg_kind == MASK_FROZEN).to(torch.int32))
        self._apply_factors(self.factors)
        self.current, self._factors_lang, self._stale = lang, lang, False

    def activate(self, lang: str):
        """Show `lang` to the network: its free tensors and buffers come back, then one launch rewrites the adapted weights from
        its factors and the whole bf16 image.  The live factors and their moments are left alone: after save_language(x),
        activate(other), ..., activate(x) training x continues where it was; progress that save_language() has not recorded is
        lost for the heads, as with Piggyback."""
        if lang not in self.records:
            raise ValueError(f"LoRA.activate: unknown language '{lang}' (saved: {', '.join(self.records) or 'none'})")
        flush_pending_updates()
        rec, f = self.records[lang], self.flat
        with torch.no_grad():
            for n, t in rec["free"].items():
                f._theta_views[n].copy_(t)
            buffers = dict(f.model.named_buffers())
            for n, t in rec["buffers"].items():
                buffers[n].copy_(t)
        self._apply_factors(rec["factors"])
        self.current, self._stale = lang, lang != self._factors_lang

    # -- the step (FusedAdamW._apply) ----------------------------------------------------------------------------------
    def _groups_of_factors(self, opt) -> torch.Tensor:
        if self._factor_group is None or self._factor_group[0] != id(opt):
            parents = torch.tensor([k for _, k, *_ in self.adapted], dtype=torch.int64, device=opt.seg_group.device)
            self._factor_group = (id(opt), opt.seg_group[parents].repeat_interleave(2).contiguous())
        return self._factor_group[1]

    def _step(self, opt, common, measured, skip, all_live, stream):
        """ia_lora_grad (factor gradients from the task gradient, clipped as the free tensors' is), the plain step on the free
        tensors, the shared AdamW rule on the factor buffer, ia_lora_apply.  `common` is what every segmented step takes."""
        L, ptr, f = _lib.lib(), _lib.ptr, self.flat
        norm_state = ptr(opt._norm_state) if measured else None
        if self._workspace is None:
            self._workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=f.theta.device)
        nt, scale = len(self.adapted), common[13]
        _lib.check(L.ia_lora_grad(ptr(f.grad), ptr(self.factors), ptr(self.factor_grad), ptr(self.tensor_table), nt,
                                  ptr(self.tile_table), self.tile_table.shape[0], ptr(self.factor_table), self.factor_table.shape[0],
                                  self.rank, self.scale, scale, norm_state, int(skip), int(all_live), ptr(self.factor_active),
                                  ptr(self._workspace), self._workspace.numel(), self.workspace_bytes, stream), "ia_lora_grad")
        # free tensors: the plain step; the shadow is left to ia_lora_apply, which writes every tensor's
        _lib.check(L.ia_adamw_step_segmented_kinds(*common[:14], None, *common[15:], ptr(self.step_kind), 0, stream),
                   "ia_adamw_step_segmented_kinds")
        # the factors: liveness is the parent's (set by ia_lora_grad), lr / weight_decay its group's, G already carries scale and coef
        _lib.check(L.ia_adamw_step_segmented_kinds(
            ptr(self.factors), ptr(self.factor_grad), ptr(self.factor_exp_avg), ptr(self.factor_exp_avg_sq), ptr(self.factor_table),
            self.factor_table.shape[0], ptr(self.factor_active), ptr(self.factor_step), 2 * nt, 0, *common[10:13], 1.0, None,
            ptr(self._groups_of_factors(opt)), *common[16:19], None, 0, None, None, 1, stream), "ia_adamw_step_segmented_kinds")
        self._materialise(self.factors, shadow=opt.shadow, norm_state=opt._norm_state if measured else None, skip=skip)

    # -- reports ---------------------------------------------------------------------------------------------------
    def delta(self, lang: Optional[str] = None) -> FlatDict:
        """s * B @ A of `lang` (default: the live factors) as a FlatDict: +0 outside the adapted tensors.  The arithmetic is
        ia_lora_apply's on a base of zeros."""
        if lang is not None and lang not in self.records:
            raise ValueError(f"LoRA.delta: unknown language '{lang}' (saved: {', '.join(self.records) or 'none'})")
        flush_pending_updates()
        out = self.flat.zeros()
        self._materialise(self.factors if lang is None else self.records[lang]["factors"], theta=out.flat,
                          base=torch.zeros_like(out.flat))
        return out

    def export(self, lang: Optional[str] = None) -> dict:
        """A plain dict for interchange: {name: {"lora_A": A [r, n], "lora_B": B [m, r]}, ..., "r": rank, "alpha": alpha} with
        copies of the factors of `lang` (default: the live ones).  W = base + (alpha / r) * lora_B @ lora_A viewed as [m, n]."""
        if lang is not None and lang not in self.records:
            raise ValueError(f"LoRA.export: unknown language '{lang}' (saved: {', '.join(self.records) or 'none'})")
        flush_pending_updates()
        views = self.factor_views(None if lang is None else self.records[lang]["factors"])
        out = {name: {key: t.detach().clone() for key, t in fac.items()} for name, fac in views.items()}
        out["r"], out["alpha"] = self.rank, self.alpha
        return out

    def bytes_per_language(self) -> dict:
        """Bytes one saved language holds: the factors (r * (m + n) floats per adapted tensor; the record keeps them in the padded
        factor buffer, `factors_padded`), the free tensors and the module buffers."""
        f = self.flat
        factors = sum(4 * self.rank * (m + n) for _, _, m, n, _, _ in self.adapted)
        free = sum(e[2] * 4 for k, e in enumerate(f.entries) if self._kinds[k] == MASK_FREE)
        buffers = sum(b.numel() * b.element_size() for b in f.model.buffers())
        return {"factors": factors, "factors_padded": 4 * self.factor_numel, "free": free, "buffers": buffers,
                "total": 4 * self.factor_numel + free + buffers}

    # -- resumable state -------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        flush_pending_updates()
        cpu = lambda t: t.detach().to("cpu", copy=True)
        return {"entries": list(self.flat.entries), "kinds": [_LORA_KIND_NAMES[k] for k in self._kinds], "rank": self.rank,
                "alpha": self.alpha, "seed": self.seed, "base": cpu(self.base.flat), "factors": cpu(self.factors),
                "factor_exp_avg": cpu(self.factor_exp_avg), "factor_exp_avg_sq": cpu(self.factor_exp_avg_sq),
                "factor_step": cpu(self.factor_step), "current": self.current, "factors_language": self._factors_lang,
                "languages": {lang: {"factors": cpu(r["factors"]), "free": {n: cpu(t) for n, t in r["free"].items()},
                                     "buffers": {n: cpu(t) for n, t in r["buffers"].items()}}
                              for lang, r in self.records.items()}}

    def load_state_dict(self, sd: dict, source="state dict"):
        """In place: base, the factors, their moments and the tables keep their addresses (an attached optimizer keeps pointing at
        them).  The factor layout follows from the kinds and the rank, so a state saved with other kinds or another rank is
        refused.  The weights are not part of this state: `activate(lang)` or `begin_language(lang)` puts them in step with it."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'masks' was saved for a different set of trainable tensors")
        if "factors" not in sd:
            raise ValueError(f"{source}: 'masks' does not hold LoRA factors")
        kinds = [_LORA_KIND_NAMES.index(k) for k in sd["kinds"]]
        if kinds != self._kinds or int(sd["rank"]) != self.rank or sd["factors"].numel() != self.factor_numel:
            raise ValueError(f"{source}: 'masks' was saved for another factor layout (rank {sd['rank']}, "
                             f"{sum(k == MASK_MASKED for k in kinds)} adapted tensors; here rank {self.rank}, {len(self.adapted)})")
        for lang, r in sd["languages"].items():
            if r["factors"].numel() != self.factor_numel:
                raise ValueError(f"{source}: the factors of '{lang}' do not fit this factor layout")
        flush_pending_updates()
        dev = self.flat.theta.device
        self.base.flat.copy_(sd["base"])
        self.factors.copy_(sd["factors"])
        self.factor_exp_avg.copy_(sd["factor_exp_avg"])
        self.factor_exp_avg_sq.copy_(sd["factor_exp_avg_sq"])
        self.factor_step.copy_(sd["factor_step"])
        self.alpha, self.seed = float(sd["alpha"]), int(sd["seed"])
        self.scale = ctypes.c_float(self.alpha / self.rank).value
        self.current, self._factors_lang = sd["current"], sd["factors_language"]
        self._stale = False                    # the weights are the caller's to restore
        self.records = {lang: {"factors": r["factors"].to(dev), "free": {n: t.to(dev) for n, t in r["free"].items()},
                               "buffers": {n: t.to(dev) for n, t in r["buffers"].items()}}
                        for lang, r in sd["languages"].items()}


# ----------------------------------------------------------------------------- LwF
MERGE_MAX_TASKS = 32      # IA_MERGE_MAX_TASKS of include/indicasr.h
MERGE_METHODS = ("task_arithmetic", "average", "ties", "fisher", "dare_linear", "dare_ties")
MERGE_WEIGHTED = ("task_arithmetic", "fisher", "dare_linear")      # the methods that take `weights`
MERGE_SCOPES = ("tensor", "model")


def density_to_trim(density) -> float:
    """TIES keeps the `density` largest-magnitude fraction of a task vector; the kernels take the trimmed fraction as a float:
    trim = float32(1.0 - density), the difference formed in double.  ValueError unless 0 < density <= 1 and trim < 1."""
    density = float(density)
    if not 0.0 < density <= 1.0:
        raise ValueError(f"TaskVectors: density {density} is outside (0, 1]")
    trim = ctypes.c_float(1.0 - density).value
    if not 0.0 <= trim < 1.0:
        raise ValueError(f"TaskVectors: density {density} is too small: 1 - density rounds to 1 in fp32")
    return trim


def density_to_keep(density, rescale=True):
    """DARE keeps every task-vector entry with probability `density` and divides the kept ones by it.  The kernels compare a
    32-bit hash with keep_threshold = min(floor(density * 2^32), 2^32 - 1), formed in double, and divide by
    keep_prob = float32(density) (1.0 without `rescale`).  -> (keep_threshold, keep_prob).  ValueError unless 0 < density <= 1
    and the threshold is at least 1 (density >= 2^-32)."""
    density = float(density)
    if not 0.0 < density <= 1.0:
        raise ValueError(f"TaskVectors: density {density} is outside (0, 1]")
    threshold = min(math.floor(density * 4294967296.0), 0xFFFFFFFF)
    if threshold < 1:
        raise ValueError(f"TaskVectors: density {density} is too small: below 2^-32 no entry would be kept")
    return threshold, (ctypes.c_float(density).value if rescale else 1.0)


class TaskVectors:
    """Model merging, the fourth continual-learning family beside regularisation, replay and parameter isolation: one copy of
    the model is fine-tuned per language from the same start, and the weight deltas ("task vectors", tau = theta - base) are
    combined afterwards.  No importance epoch, no memory of old audio, no per-language mask at inference, and the languages can
    be trained independently, on different nodes, and joined later.

        tv = TaskVectors(model_or_flat)
        tv.set_base(opt)                          # theta and the module buffers as they are now
        for lang in languages:
            ...fine-tune on lang...
            tv.store(lang, opt)                   # row k of `vectors` <- theta - base; the language's buffers are kept
            tv.restore_base(opt)                  # the next language starts from the same weights
        tv.merge("ties", density=0.2, optimizer=opt)

    `merge` writes the merged weights into `flat.theta` in place, refreshes every bf16 image and moves the weight epoch:
      "task_arithmetic"  theta = base + scale * sum_k w_k tau_k (Ilharco et al., ICLR 2023); `weights` defaults to 1 each.
      "average"          the same rule with w_k = 1 / K and scale = 1: the mean of the fine-tuned models.  The weight averaging of
                         Vander Eeckt and Van hamme (ICASSP 2023) is its K = 2 case with base = the previous model: store the
                         previous model itself (a zero task vector) and the newly adapted one.
      "ties"             trim, elect sign, disjoint mean (Yadav et al., NeurIPS 2023): per language only the `density` fraction of
                         largest magnitude stays (ties at the cutoff all stay); per weight the sign of the summed survivors is
                         elected and the survivors that carry it are averaged; theta = base + scale * that mean.  scope="tensor"
                         selects per tensor, scope="model" over the whole task vector, as the authors' code does.  Where the
                         survivors cancel to exactly zero no sign is elected and the weight takes its base value (the authors'
                         code gives such weights the majority sign of the whole model).
      "fisher"           the importance-weighted mean sum_k w_k F_k theta_k / sum_k w_k F_k (Matena & Raffel, NeurIPS 2022), as
                         theta = base + scale * sum_k w_k F_k tau_k / sum_k w_k F_k.  F_k is the importance stored with the
                         language: `store(lang, opt, importance=fish)` or `set_importance(lang, fish)` with the language's own
                         diagonal Fisher (`fisher_finish(None, fish, N, 1.0)`), MAS's omega or SI's importance.  An importance
                         that is not above `fisher_floor` counts as the floor (a select, so a NaN or negative one does too);
                         where the denominator is zero (floor 0 and no importance anywhere) the weight takes its base value.
                         `weights` are the lambda_k: > 0, 1 each by default.
      "dare_linear"      drop and rescale (Yu et al., ICML 2024), then the task-arithmetic rule: every entry of every task
                         vector is kept with probability `density` and divided by it (`rescale=False`: kept as it is), or
                         becomes +0.  The mask is a hash of (`seed`, the language's position in `languages`, the element's
                         flat index), never stored: the same seed gives the same merge, on every rank.
      "dare_ties"        the same drop and rescale in place of TIES' magnitude trim, then its sign election and disjoint mean.
    Floating-point module buffers (the BatchNorm running statistics) become the arithmetic mean of the merged languages' buffers,
    integer buffers are those of the last listed language.  The arithmetic is ia_merge_linear / ia_merge_trim / ia_merge_ties /
    ia_merge_fisher / ia_merge_linear_dare / ia_merge_ties_dare:
    every operation rounded on its own in the order of `languages`, so the result is reproducible bit for bit, and every rank
    of a distributed run performs the same merge on its own (no collective).

    Cost: `vectors` is [rows in use, flat.numel] fp32 on the device, grown on demand up to `max_tasks` rows (4 B * trainable
    parameters per language), plus `base`; `importances` is a second buffer of that shape, allocated when the first importance
    is stored.  An optimizer given to any call (or none: the weight caches are invalidated instead)
    has its bf16 shadow rewritten; `restore_base` and `merge` also zero its moments and step counters, as PackNet does when the
    weights change under it: the moments belong to a trajectory the new weights are not on."""

    def __init__(self, model_or_flat, max_tasks=MERGE_MAX_TASKS):
        if not 1 <= int(max_tasks) <= MERGE_MAX_TASKS:
            raise ValueError(f"TaskVectors: max_tasks must be in 1..{MERGE_MAX_TASKS} (got {max_tasks})")
        self.flat = _as_flat(model_or_flat)
        self.max_tasks = int(max_tasks)
        self.stride = (self.flat.numel + 3) // 4 * 4           # GEM's row convention: float4 loads of every row stay aligned
        self.base: Optional[FlatDict] = None
        self.base_buffers: Dict[str, torch.Tensor] = {}
        self.vectors: Optional[torch.Tensor] = None             # [capacity, stride]; rows 0 .. len(_rows)-1 are in use
        self._rows: Dict[str, int] = {}                         # language -> row, in order of first store
        self.buffers: Dict[str, Dict[str, torch.Tensor]] = {}   # language -> its module buffers
        self.importances: Optional[torch.Tensor] = None         # [capacity, stride], row-parallel to `vectors`; on first use
        self._important: set = set()                            # the languages whose row of `importances` is filled
        self._inside: Optional[torch.Tensor] = None             # bool [flat.numel]: inside a tensor (not an alignment gap)
        self._fisher_counts = None
        self._optimizer = None
        self._scopes: Dict[str, torch.Tensor] = {}
        self._trim_ws = self._cutoffs = self._seg_counts = None
        self.last_merge: Optional[dict] = None

    # -- bookkeeping -----------------------------------------------------------------------------------------------
    def languages(self) -> List[str]:
        """The stored languages, in row order."""
        return list(self._rows)

    def _attached(self, optimizer=None):
        if optimizer is not None:
            if optimizer.flat is not self.flat:
                raise ValueError("optimizer belongs to another FlatParams")
            self._optimizer = weakref.ref(optimizer)
        return self._optimizer() if self._optimizer is not None else None

    def _weights_changed(self, opt, reset_moments=True):
        """PackNet's convention: fresh moments and step counters, the weight epoch moves, the flat shadow views are registered."""
        if opt is not None:
            if reset_moments:
                opt.exp_avg.zero_()
                opt.exp_avg_sq.zero_()
                opt.seg_step.zero_()
            opt._after_update()
        else:
            from .ops import fast
            fast.bump_weight_epoch()

    def _snapshot_buffers(self) -> Dict[str, torch.Tensor]:
        return {n: b.detach().clone() for n, b in self.flat.model.named_buffers()}

    def _load_buffers(self, saved: Dict[str, torch.Tensor]):
        live = dict(self.flat.model.named_buffers())
        with torch.no_grad():
            for n, t in saved.items():
                live[n].copy_(t)

    def _row_storage(self, rows: int) -> torch.Tensor:
        """`vectors` with room for `rows` rows: grown by doubling, never beyond max_tasks; rows in use keep their contents."""
        have = 0 if self.vectors is None else self.vectors.shape[0]
        if rows > have:
            grown = torch.zeros(min(self.max_tasks, max(rows, 2 * have)), self.stride, dtype=torch.float32,
                                device=self.flat.theta.device)
            if have:
                grown[:have].copy_(self.vectors)
            self.vectors = grown
            if self.importances is not None:
                self.importances = self._grown_like_vectors(self.importances)
        return self.vectors

    def _grown_like_vectors(self, old: Optional[torch.Tensor]) -> torch.Tensor:
        grown = torch.zeros_like(self.vectors)
        if old is not None:
            grown[:old.shape[0]].copy_(old)
        return grown

    def _checked_importance(self, importance) -> torch.Tensor:
        f = self.flat
        if not isinstance(importance, FlatDict) or list(importance.layout.entries) != list(f.entries):
            raise ValueError("TaskVectors: importance must be a FlatDict of this layout (fisher_finish's result, MAS's omega, "
                             "SI's importance)")
        if importance.flat.device != f.theta.device or importance.flat.dtype != torch.float32 or importance.flat.numel() != f.numel:
            raise ValueError(f"TaskVectors: importance must be {f.numel} float32 values on {f.theta.device}")
        return importance.flat

    def set_importance(self, language: str, importance: FlatDict):
        """Keep a per-parameter importance of a stored language (its own diagonal Fisher from `fisher_finish(None, fish, N, 1.0)`,
        not EWC's running sum over languages; MAS's omega; SI's importance) for merge("fisher"): copied into the language's row
        of `importances`, +0 in the alignment gaps."""
        if language not in self._rows:
            raise ValueError(f"TaskVectors: unknown language '{language}' (stored: {', '.join(self._rows) or 'none'})")
        values = self._checked_importance(importance)
        f = self.flat
        if self.importances is None or self.importances.shape != self.vectors.shape:
            self.importances = self._grown_like_vectors(self.importances)
        if self._inside is None:
            inside = torch.zeros(f.numel, dtype=torch.bool)
            for _, off, n, _ in f.entries:
                inside[off:off + n] = True
            self._inside = inside.to(f.theta.device)
        row = self.importances[self._rows[language], :f.numel]
        row.copy_(values)
        row.masked_fill_(~self._inside, 0.0)
        self._important.add(language)

    def importance(self, language: str) -> FlatDict:
        """name -> view into the language's row of `importances`."""
        if language not in self._important:
            raise ValueError(f"TaskVectors: no importance is stored for '{language}' "
                             f"(with one: {', '.join(l for l in self._rows if l in self._important) or 'none'})")
        return FlatDict(self.flat, self.importances[self._rows[language], :self.flat.numel])

    def set_base(self, optimizer: Optional["FusedAdamW"] = None):
        """theta (after any deferred update) and the module buffers, as they are now, become the common start.  Task vectors
        stored against an earlier base are dropped: they are differences from it."""
        self._attached(optimizer)
        flush_pending_updates()
        if self.base is None:
            self.base = FlatDict(self.flat, self.flat.theta.clone())
        else:
            self.base.flat.copy_(self.flat.theta)
        self.base_buffers = self._snapshot_buffers()
        self._rows, self.buffers = {}, {}
        self._forget_importances()

    def _forget_importances(self):
        self._important = set()
        if self.importances is not None:
            self.importances.zero_()

    def _need_base(self, what):
        if self.base is None:
            raise RuntimeError(f"TaskVectors.{what}: no base has been set; call set_base() before fine-tuning")

    def store(self, language: str, optimizer: Optional["FusedAdamW"] = None, importance: Optional[FlatDict] = None):
        """tau = theta - base (fp32, one rounding per element, +0 in the alignment gaps) becomes the language's row, the next free
        one on first use; the module buffers are kept with it.  Storing a language again overwrites its row.  `importance`: see
        set_importance (checked before anything is stored); without one, an importance stored earlier stays."""
        self._need_base("store")
        if importance is not None:
            self._checked_importance(importance)
        if language not in self._rows and len(self._rows) >= self.max_tasks:
            raise ValueError(f"TaskVectors: max_tasks = {self.max_tasks} languages are stored already; '{language}' would be one "
                             "more")
        self._attached(optimizer)
        flush_pending_updates()
        f = self.flat
        row = self._rows.get(language, len(self._rows))
        vectors = self._row_storage(row + 1)
        torch.sub(f.theta, self.base.flat, out=vectors[row, :f.numel])
        self._rows[language] = row
        self.buffers[language] = self._snapshot_buffers()
        if importance is not None:
            self.set_importance(language, importance)

    def drop(self, language: str):
        """Forget a language; the rows behind it move up, so the order of the others stays."""
        if language not in self._rows:
            raise ValueError(f"TaskVectors.drop: unknown language '{language}' (stored: {', '.join(self._rows) or 'none'})")
        row, last = self._rows.pop(language), len(self._rows)
        del self.buffers[language]
        self._important.discard(language)
        for buf in (self.vectors, self.importances):
            if buf is not None:
                for r in range(row, last):
                    buf[r].copy_(buf[r + 1])
                buf[last].zero_()
        self._rows = {lang: (r if r < row else r - 1) for lang, r in self._rows.items()}

    def task_vector(self, language: str) -> FlatDict:
        """name -> view into the language's row."""
        if language not in self._rows:
            raise ValueError(f"TaskVectors: unknown language '{language}' (stored: {', '.join(self._rows) or 'none'})")
        return FlatDict(self.flat, self.vectors[self._rows[language], :self.flat.numel])

    def restore_base(self, optimizer: Optional["FusedAdamW"] = None):
        """theta and the module buffers go back to the base, bit for bit, for fine-tuning the next language from the same
        start; the optimizer's bf16 shadow follows and its moments and step counters are zeroed."""
        self._need_base("restore_base")
        opt = self._attached(optimizer)
        flush_pending_updates()
        self.flat.theta.copy_(self.base.flat)
        if opt is not None and opt.shadow is not None:
            opt.shadow.copy_(self.flat.theta)
        self._load_buffers(self.base_buffers)
        self._weights_changed(opt)

    # -- the merge -------------------------------------------------------------------------------------------------
    def _checked_merge(self, method, languages, scale, weights, density, scope):
        """(names, coefficients, trim) of a merge, or ValueError; nothing is launched and nothing is changed here."""
        if method not in MERGE_METHODS:
            raise ValueError(f"TaskVectors.merge: unknown method '{method}' (one of {', '.join(MERGE_METHODS)})")
        if scope not in MERGE_SCOPES:
            raise ValueError(f"TaskVectors.merge: unknown scope '{scope}' (one of {', '.join(MERGE_SCOPES)})")
        names = self.languages() if languages is None else list(languages)
        if not names:
            raise ValueError("TaskVectors.merge: no language to merge")
        if len(set(names)) != len(names):
            raise ValueError("TaskVectors.merge: a language is listed twice")
        for n in names:
            if n not in self._rows:
                raise ValueError(f"TaskVectors.merge: unknown language '{n}' (stored: {', '.join(self._rows) or 'none'})")
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"TaskVectors.merge: scale must be finite (got {scale})")
        if method not in MERGE_WEIGHTED and weights is not None:
            raise ValueError(f"TaskVectors.merge: weights belong to 'task_arithmetic', 'fisher' and 'dare_linear', not to "
                             f"'{method}'")
        if method == "average" and scale != 1.0:
            raise ValueError("TaskVectors.merge: 'average' is the mean of the fine-tuned models, its scale is 1; use "
                             "'task_arithmetic' for a scaled sum")
        if weights is None:
            coef = [1.0 / len(names) if method == "average" else 1.0] * len(names)
        else:
            coef = [float(weights[n]) for n in names] if isinstance(weights, dict) else [float(w) for w in weights]
            if len(coef) != len(names):
                raise ValueError(f"TaskVectors.merge: {len(coef)} weights for {len(names)} languages")
            if not all(math.isfinite(c) for c in coef):
                raise ValueError("TaskVectors.merge: weights must be finite")
        trim = density_to_trim(density) if method == "ties" else None
        return names, coef, scale, trim

    def _checked_rule(self, method, names, coef, density, fisher_floor, seed, rescale) -> dict:
        """What "fisher", "dare_linear" and "dare_ties" need beyond _checked_merge, or ValueError; nothing is launched."""
        rule = {}
        if method == "fisher":
            if not all(c > 0.0 for c in coef):
                raise ValueError("TaskVectors.merge: the weights of 'fisher' must be > 0")
            floor = float(fisher_floor)
            if not (math.isfinite(floor) and floor >= 0.0):
                raise ValueError(f"TaskVectors.merge: fisher_floor must be finite and >= 0 (got {floor})")
            missing = [n for n in names if n not in self._important]
            if missing:
                raise ValueError(f"TaskVectors.merge: 'fisher' needs an importance for every language; none is stored for "
                                 f"{', '.join(repr(n) for n in missing)} (store(lang, opt, importance=...) or set_importance)")
            rule["fisher_floor"] = floor
        elif method in ("dare_linear", "dare_ties"):
            if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
                raise ValueError(f"TaskVectors.merge: seed must be an int in [0, 2^32) (got {seed!r})")
            rule["keep_threshold"], rule["keep_prob"] = density_to_keep(density, bool(rescale))
            rule.update(seed=seed, density=float(density), rescale=bool(rescale))
        return rule

    def _rows_of(self, names, buffer: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rows of `names`, in that order, as one [K, stride] tensor: a view when they are consecutive rows of `vectors`
        (every language in row order is), a gathered copy otherwise.  `buffer`: `importances` instead of `vectors`."""
        buffer = self.vectors if buffer is None else buffer
        idx = [self._rows[n] for n in names]
        if idx == list(range(idx[0], idx[0] + len(idx))):
            return buffer[idx[0]:idx[0] + len(idx)]
        return buffer.index_select(0, torch.tensor(idx, device=buffer.device))

    def merged_buffers(self, names) -> Dict[str, torch.Tensor]:
        """Floating-point buffers: the arithmetic mean over `names` (added in that order, then divided by their number, in the
        buffer's dtype); every other buffer: the last listed language's."""
        out = {}
        for key, last in self.buffers[names[-1]].items():
            if last.is_floating_point():
                acc = self.buffers[names[0]][key].clone()
                for n in names[1:]:
                    acc = acc + self.buffers[n][key]
                out[key] = acc / len(names)
            else:
                out[key] = last.clone()
        return out

    def _scope_map(self, scope) -> torch.Tensor:
        if scope not in self._scopes:
            nseg = len(self.flat.entries)
            self._scopes[scope] = (torch.arange(nseg, dtype=torch.int32) if scope == "tensor"
                                   else torch.zeros(nseg, dtype=torch.int32)).to(self.flat.theta.device)
        return self._scopes[scope]

    def merge(self, method: str, languages=None, *, scale=1.0, weights=None, density=0.2, scope="tensor",
              optimizer: Optional["FusedAdamW"] = None, fisher_floor=1e-6, seed=0, rescale=True) -> dict:
        """Merge `languages` (default: all, in row order) into theta; see the class docstring for the methods.  `weights`: one
        per listed language (a sequence, or a dict by language).  Returns {"method", "languages", "coefficients", "scale"} and,
        for "ties", "density", "trim", "scope" and per tensor and in total the number of weights with a surviving entry
        (`surviving`), with survivors of both signs (`conflicts`) and whose survivors cancelled to zero and so kept the base
        value (`cancelled`): one small device-to-host read.  "dare_ties" returns the same counts, and with "dare_linear" `seed`,
        `density` and `rescale`; "fisher" returns `fisher_floor` and, per tensor and in total, the weights where no language's
        importance exceeded the floor (`floored`: a plain weighted mean) and those whose denominator was zero and so kept the
        base value (`unweighted`)."""
        self._need_base("merge")
        names, coef, scale, trim = self._checked_merge(method, languages, scale, weights, density, scope)
        rule = self._checked_rule(method, names, coef, density, fisher_floor, seed, rescale)
        f = self.flat
        if not f.theta.is_cuda:
            raise RuntimeError("TaskVectors.merge runs on the HIP kernels: the parameters are not on the device")
        opt = self._attached(optimizer)
        flush_pending_updates()
        L, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream_ptr()
        rows, K = self._rows_of(names), len(names)
        nchunks, nseg = f.chunk_table.shape[0], len(f.entries)
        shadow = opt.shadow if opt is not None else None
        stats = {"method": method, "languages": names, "coefficients": coef, "scale": scale}
        if method == "ties":
            seg_of_scope = self._scope_map(scope)
            nscope = nseg if scope == "tensor" else 1
            need = L.ia_merge_trim_workspace_bytes(K, nscope)
            if self._trim_ws is None or self._trim_ws.numel() < need:
                self._trim_ws = torch.empty(need, dtype=torch.uint8, device=f.theta.device)
            if self._cutoffs is None:
                self._cutoffs = torch.zeros(self.max_tasks * nseg, dtype=torch.int32, device=f.theta.device)
            if self._seg_counts is None:
                self._seg_counts = torch.zeros(nseg, 3, dtype=torch.int32, device=f.theta.device)
            _lib.check(L.ia_merge_trim(ptr(rows), self.stride, K, ptr(f.chunk_table), nchunks, ptr(seg_of_scope), nscope, trim,
                                       ptr(self._cutoffs), ptr(self._trim_ws), self._trim_ws.numel(), stream), "ia_merge_trim")
            _lib.check(L.ia_merge_ties(ptr(f.theta), ptr(self.base.flat), ptr(rows), self.stride, K, ptr(self._cutoffs),
                                       ptr(seg_of_scope), nscope, scale, ptr(f.chunk_table), nchunks, nseg, ptr(shadow),
                                       ptr(self._seg_counts), stream), "ia_merge_ties")
        elif method == "fisher":
            if self._fisher_counts is None:
                self._fisher_counts = torch.zeros(nseg, 2, dtype=torch.int32, device=f.theta.device)
            _lib.check(L.ia_merge_fisher(ptr(f.theta), ptr(self.base.flat), ptr(rows), ptr(self._rows_of(names, self.importances)),
                                         self.stride, K, (ctypes.c_float * K)(*coef), rule["fisher_floor"], scale,
                                         ptr(f.chunk_table), nchunks, nseg, ptr(shadow), ptr(self._fisher_counts), stream),
                       "ia_merge_fisher")
        elif method == "dare_linear":
            _lib.check(L.ia_merge_linear_dare(ptr(f.theta), ptr(self.base.flat), ptr(rows), self.stride, K,
                                              (ctypes.c_float * K)(*coef), scale, ptr(f.chunk_table), nchunks, ptr(shadow),
                                              rule["seed"], rule["keep_threshold"], rule["keep_prob"], stream),
                       "ia_merge_linear_dare")
        elif method == "dare_ties":
            if self._seg_counts is None:
                self._seg_counts = torch.zeros(nseg, 3, dtype=torch.int32, device=f.theta.device)
            _lib.check(L.ia_merge_ties_dare(ptr(f.theta), ptr(self.base.flat), ptr(rows), self.stride, K, scale,
                                            ptr(f.chunk_table), nchunks, nseg, ptr(shadow), ptr(self._seg_counts),
                                            rule["seed"], rule["keep_threshold"], rule["keep_prob"], stream),
                       "ia_merge_ties_dare")
        else:
            _lib.check(L.ia_merge_linear(ptr(f.theta), ptr(self.base.flat), ptr(rows), self.stride, K,
                                         (ctypes.c_float * K)(*coef), scale, ptr(f.chunk_table), nchunks, ptr(shadow), stream),
                       "ia_merge_linear")
        self._load_buffers(self.merged_buffers(names))
        self._weights_changed(opt)
        if method == "fisher":
            per = {n: {"floored": c[0], "unweighted": c[1]} for (n, _, _, _), c in zip(f.entries, self._fisher_counts.tolist())}
            stats.update(fisher_floor=rule["fisher_floor"], tensors=per,
                         **{key: sum(t[key] for t in per.values()) for key in ("floored", "unweighted")})
        if method in ("dare_linear", "dare_ties"):
            stats.update(seed=rule["seed"], density=rule["density"], rescale=rule["rescale"])
        if method == "ties":
            stats.update(density=float(density), trim=trim, scope=scope)
        if method in ("ties", "dare_ties"):
            per = {n: {"surviving": c[0], "conflicts": c[1], "cancelled": c[2] - (k - c[0])}
                   for (n, _, k, _), c in zip(f.entries, self._seg_counts.tolist())}
            stats.update(tensors=per, **{key: sum(t[key] for t in per.values()) for key in ("surviving", "conflicts", "cancelled")})
        self.last_merge = stats
        return stats

    def cutoffs(self, ntasks: int, scope="tensor") -> torch.Tensor:
        """The magnitude cutoffs of the latest "ties" merge as int32 bit patterns [ntasks, scope segments] (a device view)."""
        nscope = len(self.flat.entries) if scope == "tensor" else 1
        return self._cutoffs[:ntasks * nscope].view(ntasks, nscope)

    # -- reports and resumable state -------------------------------------------------------------------------------
    def stats(self) -> dict:
        """Host-side bookkeeping only (no device read): the languages in row order, the rows allocated, the bytes held on the
        device and what the latest merge returned."""
        rows = 0 if self.vectors is None else self.vectors.shape[0]
        per_buffers = sum(b.numel() * b.element_size() for b in self.base_buffers.values())
        return {"languages": self.languages(), "rows_in_use": len(self._rows), "rows_allocated": rows,
                "max_tasks": self.max_tasks, "has_base": self.base is not None,
                "importance_languages": [lang for lang in self._rows if lang in self._important],
                "bytes_importances": 0 if self.importances is None else 4 * self.importances.shape[0] * self.stride,
                "bytes_vectors": 4 * rows * self.stride, "bytes_base": 4 * self.flat.numel if self.base is not None else 0,
                "bytes_buffers": per_buffers * (len(self.buffers) + (self.base is not None)), "last_merge": self.last_merge}

    def state_dict(self) -> dict:
        flush_pending_updates()
        cpu = lambda t: t.detach().to("cpu", copy=True)
        k, n = len(self._rows), self.flat.numel
        vectors = cpu(self.vectors[:k, :n]) if k else torch.zeros(0, n)
        sd = {"entries": list(self.flat.entries), "max_tasks": self.max_tasks,
              "base": cpu(self.base.flat) if self.base is not None else None,
              "base_buffers": {key: cpu(t) for key, t in self.base_buffers.items()},
              "task_languages": self.languages(), "vectors": vectors,
              "buffers": {lang: {key: cpu(t) for key, t in b.items()} for lang, b in self.buffers.items()}}
        important = [lang for lang in self._rows if lang in self._important]
        if important:                                            # only then: a state without importances keeps its key set
            sd["importance_languages"] = important
            sd["importances"] = cpu(self._rows_of(important, self.importances)[:, :n])
        return sd

    def load_state_dict(self, sd: dict, source="state dict"):
        """Inverse of state_dict(); refuses a state saved for another set of trainable tensors.  The weights are not part of
        this state: `restore_base()` or `merge()` puts them in step with it."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'masks' was saved for a different set of trainable tensors")
        if "vectors" not in sd or "task_languages" not in sd:
            raise ValueError(f"{source}: 'masks' does not hold task vectors")
        names = list(sd["task_languages"])
        if len(names) > self.max_tasks:
            raise ValueError(f"{source}: {len(names)} task vectors were saved, max_tasks here is {self.max_tasks}")
        if tuple(sd["vectors"].shape) != (len(names), self.flat.numel):
            raise ValueError(f"{source}: the saved task vectors are {tuple(sd['vectors'].shape)}, expected "
                             f"{(len(names), self.flat.numel)}")
        important = list(sd.get("importance_languages", []))
        if important and (not set(important) <= set(names) or "importances" not in sd or
                          tuple(sd["importances"].shape) != (len(important), self.flat.numel)):
            raise ValueError(f"{source}: the saved importances do not match the saved task vectors")
        flush_pending_updates()
        dev = self.flat.theta.device
        if sd["base"] is None:
            self.base = None
        elif self.base is None:
            self.base = FlatDict(self.flat, sd["base"].to(dev, copy=True))
        else:
            self.base.flat.copy_(sd["base"])
        self.base_buffers = {key: t.to(dev, copy=True) for key, t in sd["base_buffers"].items()}
        self._rows = {lang: r for r, lang in enumerate(names)}
        if names:
            vectors = self._row_storage(len(names))
            vectors.zero_()
            vectors[:len(names), :self.flat.numel].copy_(sd["vectors"])
        elif self.vectors is not None:
            self.vectors.zero_()
        self.buffers = {lang: {key: t.to(dev, copy=True) for key, t in b.items()} for lang, b in sd["buffers"].items()}
        self._forget_importances()
        if important:
            if self.importances is None or self.importances.shape != self.vectors.shape:
                self.importances = self._grown_like_vectors(None)
            for r, lang in enumerate(important):
                self.importances[self._rows[lang], :self.flat.numel].copy_(sd["importances"][r])
            self._important = set(important)


def lwf_kd_loss(loss, prob, prob_, pred_store_list, store_list, knowledge_distillation: float, kd_ctx: float):
    """R/cl_baseline_lwf.py:242-264.  Returns (total loss, rnnt_kd, ctc_kd) -- device tensors."""
    F = torch.nn.functional
    # fp32 arithmetic whatever the stash dtype (the bf16 path stashes bf16 lattices; kl_div evaluated in bf16 rounds
    # log(exp(i)) - j, a difference of nearly equal numbers, to 8 bits: observed 4.5 % off the fp32 value)
    ctc_kd_loss = F.kl_div(prob.float(), prob_.float().exp(), reduction='batchmean')
    from .ops.joint import LatticeStash, lattice_kd_term
    if isinstance(store_list, LatticeStash) and isinstance(pred_store_list, LatticeStash):
        rnnt_kd = lattice_kd_term(pred_store_list, store_list)   # fused joint: both lattices stay f16 in HBM, two streaming passes
    else:
        if isinstance(store_list, LatticeStash) or isinstance(pred_store_list, LatticeStash):
            raise ValueError("lwf_kd_loss: one of the two stashes is a fused-joint lattice and the other a list of tensors; "
                             "run the teacher and the student passes on the same joint path (joint.use_fused)")
        assert len(store_list) == len(pred_store_list)
        rnnt_kd = 0
        for i, j in zip(store_list, pred_store_list):
            rnnt_kd = rnnt_kd + F.kl_div(j.float(), i.float().exp(), reduction='batchmean')
        rnnt_kd = rnnt_kd / len(store_list)
    total = loss * (1 - knowledge_distillation) + knowledge_distillation * ((1 - kd_ctx) * rnnt_kd + kd_ctx * ctc_kd_loss)
    return total, rnnt_kd, ctc_kd_loss


def lwf_teacher_forward(model, flat: FlatParams, teacher: FlatDict, batch, lang_ids, host_lengths=None):
    """Teacher pass with the previous task's weights resident in HBM (R/cl_baseline_lwf.py:213-232 semantics:
    no_grad, store_sub_enc + detach)."""
    flush_pending_updates()
    m = getattr(model, "module", model)
    with torch.no_grad(), flat.weights(teacher):
        m.joint.store_sub_enc, m.joint.detach_sub_enc = True, True
        step = m._step
        _, _, prob_ = m.training_step(batch, lang_ids, return_probs=True, host_lengths=host_lengths, compute_wer=False)
        m._step = step  # same SpecAugment/dither draw for the student pass
        store_list = m.joint.store_list
    return prob_, store_list


# ----------------------------------------------------------------------------- optimizer + DP
MAX_PARAM_GROUPS = 64      # IA_MAX_PARAM_GROUPS of include/indicasr.h: the group table travels in the kernel arguments
_GROUP_KEYS = ("params", "match", "lr", "weight_decay", "name")


def _as_flat(model_or_flat) -> FlatParams:
    return model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)


def _default_no_decay(name: str, p: torch.Tensor) -> bool:
    return p.ndim <= 1 or name.endswith("pos_bias_u") or name.endswith("pos_bias_v")


def no_decay_groups(model_or_flat, no_decay=None) -> List[dict]:
    """`param_groups=` for FusedAdamW: ONE group with weight_decay=0.0 holding every trainable tensor for which
    `no_decay(name, parameter)` holds -- by default biases, norm scales and every other tensor with ndim <= 1, plus the
    relative-position biases `pos_bias_u` / `pos_bias_v` (Loshchilov & Hutter 2019 decay weights, not these).  Everything else
    stays in group 0 with the constructor's weight decay.  An empty list when nothing qualifies."""
    flat = _as_flat(model_or_flat)
    pred = no_decay or _default_no_decay
    names = [n for n, p in zip(flat.names, flat.params) if pred(n, p)]
    return [dict(params=names, weight_decay=0.0, name="no_decay")] if names else []


def layerwise_lr_groups(model_or_flat, lr, decay, no_decay_1d=True) -> List[dict]:
    """`param_groups=` for FusedAdamW: layer-wise learning-rate decay (Howard & Ruder 2018) over the hybrid model.  Depth 0 is
    `decoder.*`, `joint.*` and `ctc_decoder.*` at `lr`; `encoder.layers.i.*` sits at `lr * decay**(L - i)` with
    L = len(encoder.layers); `encoder.pre_encode.*` at `lr * decay**(L + 1)`.  With `no_decay_1d` every depth is split into
    its decayed tensors and a second group with weight_decay=0.0 (the predicate of `no_decay_groups`).  Depths without a
    trainable tensor are left out; a trainable tensor under none of these prefixes is not claimed and stays in group 0."""
    flat = _as_flat(model_or_flat)
    L = len(flat.model.encoder.layers)
    by_depth: Dict[int, List[str]] = {}
    for n in flat.names:
        if n.startswith(("decoder.", "joint.", "ctc_decoder.")):
            d = 0
        elif n.startswith("encoder.layers."):
            d = L - int(n.split(".")[2])
        elif n.startswith("encoder.pre_encode."):
            d = L + 1
        else:
            continue
        by_depth.setdefault(d, []).append(n)
    param = dict(zip(flat.names, flat.params))
    groups = []
    for d in sorted(by_depth):
        names, rate = by_depth[d], lr * decay ** d
        plain = [n for n in names if not (no_decay_1d and _default_no_decay(n, param[n]))]
        bare = [n for n in names if no_decay_1d and _default_no_decay(n, param[n])]
        if plain:
            groups.append(dict(params=plain, lr=rate, name=f"depth{d}"))
        if bare:
            groups.append(dict(params=bare, lr=rate, weight_decay=0.0, name=f"depth{d}.no_decay"))
    return groups


def _resolve_param_groups(flat: FlatParams, specs) -> List[List[str]]:
    """Names per group, group 0 first (every trainable tensor no spec claims); raises ValueError naming the offender."""
    specs = list(specs)
    if 1 + len(specs) > MAX_PARAM_GROUPS:
        raise ValueError(f"param_groups: {len(specs)} groups + group 0 exceed the limit of {MAX_PARAM_GROUPS} groups")
    by_id = {id(p): n for n, p in zip(flat.names, flat.params)}
    known, owner, out = set(flat.names), {}, []
    for k, spec in enumerate(specs, start=1):
        label = f"group {k}" + (f" ('{spec['name']}')" if isinstance(spec, dict) and "name" in spec else "")
        if not isinstance(spec, dict):
            raise ValueError(f"param_groups: {label} is not a dict")
        for key in spec:
            if key not in _GROUP_KEYS:
                raise ValueError(f"param_groups: {label} has the unknown key '{key}' (allowed: {', '.join(_GROUP_KEYS)}; betas, "
                                 "eps and the clip settings are per optimizer)")
        if ("params" in spec) == ("match" in spec):
            raise ValueError(f"param_groups: {label} needs either 'params' or 'match'")
        if "match" in spec:
            names = [n for n in flat.names if re.search(spec["match"], n)]
            if not names:
                raise ValueError(f"param_groups: {label}: match '{spec['match']}' matches no trainable tensor")
        else:
            given = spec["params"]
            given = [given] if isinstance(given, (str, torch.Tensor)) else list(given)
            names = []
            for item in given:
                if isinstance(item, str):
                    if item not in known:
                        raise ValueError(f"param_groups: {label}: '{item}' is not a trainable tensor of this FlatParams")
                    names.append(item)
                elif id(item) in by_id:
                    names.append(by_id[id(item)])
                else:
                    what = f"a tensor of shape {tuple(item.shape)}" if isinstance(item, torch.Tensor) else repr(item)
                    raise ValueError(f"param_groups: {label}: {what} is not a trainable tensor of this FlatParams")
        for n in names:
            if n in owner:
                raise ValueError(f"param_groups: '{n}' is claimed by {owner[n]} and by {label}")
            owner[n] = label
        out.append(names)
    return [[n for n in flat.names if n not in owner]] + out


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(model.parameters(), lr) of R/cl_baseline.py:137 as one launch over the flat buffers.
    step() first averages the flat gradient across ranks (RCCL all-reduce over xGMI) when a process group
    exists -- the reference wraps the model in DDP but never arms its reducer.

    A torch.optim.Optimizer, so torch.optim.lr_scheduler.* attach and write param_groups[k]["lr"]; zero_grad, step,
    state_dict and load_state_dict are this class's own, and the layout is fixed at construction (add_param_group raises).
    Per group: `lr` and `weight_decay`.  Per optimizer: `betas` and `eps` (a step that finds a group whose betas or eps differ
    from group 0's raises ValueError -- e.g. OneCycleLR needs cycle_momentum=False), and `max_grad_norm` / `skip_nonfinite`,
    which are read from group 0 only."""

    def __init__(self, model_or_flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, group=None,
                 bf16_shadow=None, defer_update=True, grad_exchange_dtype=None, max_grad_norm=None, skip_nonfinite=False,
                 track_grad_norm=False, path_integral=None, projection=None, param_groups=None, masks=None):
        """`max_grad_norm=c`: torch.nn.utils.clip_grad_norm_(parameters, c) applied inside the step, to the gradient the
        update consumes -- after the data-parallel all-reduce, so every rank clips the AVERAGED gradient by the same factor
        (the torch call between backward() and step() would clip each rank's local gradient: the exchange happens in here).
        `skip_nonfinite=True`: a step whose gradient norm is inf or NaN changes nothing (torch.amp.GradScaler.step's skip)
        and is counted.  `track_grad_norm=True`: measure the norms without clipping.  Norm, coefficient and counters stay
        on the device: `last_grad_norm`, `stats()`, `grad_norms()`.  With all three at their defaults the step is the plain
        ia_adamw_step_segmented.  `max_grad_norm` / `skip_nonfinite` live in param_groups[0] and are read per step, as lr is.
        The entry points named here and below are reached through ia_adamw_step_segmented_grouped (one group or many), whose
        operands select the same step; only masks (Piggyback, PackNet), GEM and RWalk have entry points of their own.

        `grad_exchange_dtype="bf16"` ("fp32 or bf16"): the data-parallel exchange all-reduces a bf16 image of the
        flat gradient (half the bytes over xGMI: 80 instead of 160 MB per step at 40 M trainable parameters); every rank
        then applies AdamW to the same bf16-rounded sum, so the weights stay identical across ranks.  None: fp32 exchange.

        `path_integral=si` (a `SynapticIntelligence` on the same FlatParams): the step runs ia_adamw_step_segmented_si, which
        also updates si.w from the averaged task gradient and the weights' movement and, once si.tasks_consolidated > 0, adds
        the surrogate's gradient 2 * si_c * omega * (theta - theta_star) -- AFTER the clip: norm and coefficient stay those of
        the task gradient (torch's clip_grad_norm_ on `loss + surrogate` would clip the total).  Every tensor is live then.
        The SI buffers are not optimizer state: they are saved through si.state_dict() / si.flat_dicts().
        `path_integral=rw` (an `RWalk`): the step runs ia_adamw_step_segmented_rwalk, which takes the group table itself.  It
        keeps rw.fisher as a moving average of the squared averaged task gradient, integrates rw.w as SI does and, on every
        rw.interval-th applied update, folds the path into rw.score; once rw.tasks_consolidated > 0 it adds
        2 * rw_lambda * importance * (theta - theta_star) after the clip.  Saved through rw.state_dict() / rw.flat_dicts().

        `projection=agem` (an `AveragedGEM` on the same FlatParams): once agem.has_reference, the step runs ia_agem_dots,
        ia_grad_norm_projected (if the norm is measured) and ia_adamw_step_segmented_projected: the averaged task gradient is
        projected off agem.ref when their dot is negative, then clipped.  Without a reference the step is the one described
        above.  Not combinable with `path_integral`; projection state is not optimizer state and is not in state_dict().
        `projection=gem` (a `GEM`): the same place in the step, with one constraint per stored task -- ia_gem_dots, ia_gem_solve,
        ia_grad_norm_gem (if the norm is measured) and ia_adamw_step_segmented_gem, which takes the group table itself.
        `projection=ogd` (an `OGD`): once a direction is stored, ia_ogd_dots and ia_ogd_project rewrite the averaged flat gradient
        in place, and the norm and step described above run on it unchanged: project, then clip.  The basis is saved through
        ogd.state_dict() / checkpoint.save_projection.

        `param_groups=[{...}, ...]`: dicts in torch's shape.  Each names its tensors with "params" (parameter names and / or
        the Parameter objects) or "match" (a regular expression, re.search on the parameter name), may override "lr" and / or
        "weight_decay", and may carry a "name".  Every trainable tensor nobody claims stays in group 0, which carries this
        constructor's values; `no_decay_groups` and `layerwise_lr_groups` build such lists.  All groups go through ONE launch
        (ia_adamw_step_segmented_grouped; clipping, the non-finite skip, path_integral and projection included).  A deferred
        update applies the lr / weight_decay its step() saw, whatever a scheduler has written since.

        `masks=pb` (a `Piggyback` on the same FlatParams): the step is ia_adamw_step_segmented_masked for one or many groups,
        after ia_grad_norm when the norm is measured (the norm is that of the task gradient, as without masks).  A masked tensor's
        scores are trained with its group's `lr`; its `weight_decay` is IGNORED (a score is not a weight, and decaying it towards
        zero would switch bits off by itself).  A free tensor takes the plain step, a frozen one is never written.  `exp_avg`,
        `exp_avg_sq` and the step counters of a masked tensor are those of its scores.  Not combinable with `path_integral` or
        `projection`.  The masks are not optimizer state: `pb.state_dict()` / `checkpoint.save_masks`.

        `masks=pn` (a `PackNet`): the step is ia_adamw_step_segmented_packed, after ia_grad_norm_packed when the norm is measured
        -- the norm of the gradient the step consumes: the trainable elements of packed tensors and the free tensors.  In a packed
        tensor the elements whose owner is `pn.train_owner` take the plain rule with the group's `lr` and `weight_decay`; every
        other element keeps its weight and moments.  The same refusals and the same place outside the optimizer state.

        `masks=lora` (a `LoRA`): after ia_grad_norm when the norm is measured (the norm and coefficient are the task gradient's over
        all tensors, as with Piggyback), the step is ia_lora_grad (the full dW of every adapted tensor becomes the gradients of
        its factors, from the pre-step factors), ia_adamw_step_segmented_kinds on the flat buffers (free tensors take the plain
        step bit for bit; frozen and adapted tensors' theta, full-size moments and step counters are not written),
        ia_adamw_step_segmented_kinds on the factor buffer (the same update rule; a factor takes the `lr` and `weight_decay` of
        its parent's group and is live when its parent received a gradient) and ia_lora_apply (theta = base + s * B @ A and the
        bf16 image of every tensor).  The factors, their moments and step counters belong to the LoRA object.  The same refusals
        and the same place outside the optimizer state."""
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else flat_of(model_or_flat)
        if masks is not None and (path_integral is not None or projection is not None):
            raise ValueError("masks cannot be combined with path_integral or projection: the masked weights do not move along "
                             "the gradient those methods constrain")
        if masks is not None and masks.flat is not self.flat:
            raise ValueError("masks belongs to another FlatParams")
        self.masks = masks
        if path_integral is not None and path_integral.flat is not self.flat:
            raise ValueError("path_integral belongs to another FlatParams")
        if projection is not None and path_integral is not None:
            raise ValueError("projection and path_integral cannot be combined: the path integral has no agreed meaning under a "
                             "projected gradient")
        if projection is not None and projection.flat is not self.flat:
            raise ValueError("projection belongs to another FlatParams")
        self.path_integral = path_integral
        self.projection = projection
        if grad_exchange_dtype not in (None, "fp32", "bf16"):
            raise ValueError("grad_exchange_dtype: None | 'fp32' | 'bf16'")
        self.grad_exchange_dtype = None if grad_exchange_dtype == "fp32" else grad_exchange_dtype
        self._g16 = None
        self.profile_exchange = False     # bench.py: HIP events around the wait for the exchange (exposed time per step)
        self.exchange_events = []
        self.exchange_bytes = 0           # bytes handed to the last all-reduce
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(self.flat.theta)
        self.exp_avg_sq = torch.zeros_like(self.flat.theta)
        self.step_count = 0
        # torch.optim.AdamW keeps one step counter per parameter and skips parameters whose .grad is None: per-tensor
        # counters + "received a gradient" flags live on the device (ia_adamw_step_segmented)
        nseg = len(self.flat.entries)
        self.seg_step = torch.zeros(nseg, dtype=torch.int32, device=self.flat.theta.device)
        self.seg_active = torch.zeros(nseg, dtype=torch.int32, device=self.flat.theta.device)
        self.group = group
        if (group is None and defer_update and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            # A communicator executes its collectives in issue order: on the default group the deferred 160 MB gradient
            # all-reduce (launched at step(), meant to run under the NEXT forward's frozen prefix) would sit in front of
            # that prefix's small SyncBatchNorm all-reduces and stall the first block until it has finished.  Its own
            # communicator (every rank constructs its optimizer at the same point of the program) lets both run side by side.
            self.group = dist.new_group()
        if bf16_shadow is None:  # the HIP GEMM paths consume bf16 weights: let the optimizer kernel emit them (one launch)
            bf16_shadow = self.flat.theta.is_cuda
        self.shadow = self.flat.theta.to(torch.bfloat16) if bf16_shadow else None
        group0 = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                      skip_nonfinite=skip_nonfinite, params=self.flat.params)
        if param_groups is None:
            self._group_names, groups = [list(self.flat.names)], [group0]
        else:
            self._group_names = _resolve_param_groups(self.flat, param_groups)
            param = dict(zip(self.flat.names, self.flat.params))
            groups = []
            for k, names in enumerate(self._group_names):
                spec = {} if k == 0 else param_groups[k - 1]
                g = dict(params=[param[n] for n in names], names=list(names), lr=spec.get("lr", lr),
                         weight_decay=spec.get("weight_decay", weight_decay), betas=betas, eps=eps)
                if k == 0:
                    g.update(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
                elif "name" in spec:
                    g["name"] = spec["name"]
                groups.append(g)
        self._layout_fixed = False
        torch.optim.Optimizer.__init__(self, groups, {})      # sets self.param_groups (through add_param_group) and self.state
        self._layout_fixed = True
        # tensor -> group, built once; the per-group lr / weight_decay go to the kernel by value at every step
        index = {n: k for k, names in enumerate(self._group_names) for n in names}
        self.seg_group = torch.tensor([index[n] for n in self.flat.names], dtype=torch.int32, device=self.flat.theta.device)
        self.track_grad_norm = track_grad_norm
        # {total_norm, coef, non-finite flag, max_norm} as fp32 + {clipped steps, skipped steps} as int32 in ONE device buffer
        # (stats() reads it in one copy); the per-tensor norms and the chunk sums are allocated by the first clipped step
        self._norm_buf = torch.zeros(6, dtype=torch.int32, device=self.flat.theta.device)
        self._norm_state = self._norm_buf[:4].view(torch.float32)
        self._norm_state.copy_(torch.tensor([float("nan"), 1.0, 0.0, 0.0]))
        self._counters = self._norm_buf[4:]
        self._seg_norm = self._norm_ws = None
        self.defer_update = defer_update   # data parallel only: overlap the gradient all-reduce with the next forward
        self._pending, self._zero_after_flush = None, False
        if masks is not None:
            masks._optimizer = weakref.ref(self)      # activate() / begin_language() rewrite this optimizer's bf16 shadow

    def add_param_group(self, param_group):
        if self._layout_fixed:
            raise NotImplementedError("FusedAdamW: the flat layout and its groups are fixed at construction; pass param_groups= "
                                      "to the constructor")
        super().add_param_group(param_group)

    def _group_hyper(self):
        """Every group's (lr, weight_decay) as floats; ValueError when a group's betas / eps left group 0's."""
        g0 = self.param_groups[0]
        for k, g in enumerate(self.param_groups[1:], start=1):
            for key in ("betas", "eps"):
                if key not in g:
                    continue
                same = tuple(g[key]) == tuple(g0[key]) if key == "betas" else g[key] == g0[key]
                if not same:
                    raise ValueError(f"FusedAdamW: param_groups[{k}]['{key}'] = {g[key]} differs from group 0's {g0[key]}: "
                                     f"{key} is one per optimizer (schedulers that cycle momentum need cycle_momentum=False)")
        return [float(g["lr"]) for g in self.param_groups], [float(g["weight_decay"]) for g in self.param_groups]

    def zero_grad(self, set_to_none: bool = False):
        if self._pending is not None:
            self._zero_after_flush = True   # the deferred update still has to consume these gradients
        else:
            self.flat.zero_grad()

    def _exchange_buffer(self):
        """The tensor the all-reduce runs on: the flat fp32 gradient itself, or its bf16 image (copied back by _exchange_done)."""
        if self.grad_exchange_dtype == "bf16":
            if self._g16 is None:
                self._g16 = torch.empty_like(self.flat.grad, dtype=torch.bfloat16)
            self._g16.copy_(self.flat.grad)
            buf = self._g16
        else:
            buf = self.flat.grad
        self.exchange_bytes = buf.numel() * buf.element_size()
        return buf

    def _exchange_done(self):
        if self.grad_exchange_dtype == "bf16":
            self.flat.grad.copy_(self._g16)

    def allreduce_grads(self):
        if dist.is_available() and dist.is_initialized():
            ws = dist.get_world_size(self.group)
            if ws > 1:
                dist.all_reduce(self._exchange_buffer(), group=self.group)
                self._exchange_done()
                return 1.0 / ws
        return 1.0

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def step(self, grad_scale: Optional[float] = None):
        """Single process: AdamW now.  Data parallel with `defer_update` (default): the all-reduce of the flat gradient is
        launched asynchronously and the AdamW kernel is deferred to flush(), which the model calls right before the first
        module that reads trainable weights in the NEXT forward -- the exchange over xGMI then runs under the front end,
        subsampling and the frozen encoder prefix, none of which read trainable weights, so the result is bit-identical to
        updating immediately.  Everything here that reads or swaps the flat weights flushes first."""
        self.flush()
        hyper = self._group_hyper()        # raises before anything is launched or exchanged
        ws = self._world()
        gs = 1.0 if grad_scale is None else grad_scale
        if ws > 1 and self.defer_update:
            work = dist.all_reduce(self._exchange_buffer(), group=self.group, async_op=True)
            # lr / weight_decay as they are NOW: a scheduler stepped before the next forward must not reach this update
            self._pending = (work, gs / ws, self.flat.all_grads_live, hyper)
            _PENDING_OPTIMIZERS.add(self)
            return
        self._apply(self.allreduce_grads() * gs, self.flat.all_grads_live, hyper)

    def flush(self):
        if self._pending is None:
            return
        work, scale, live, hyper = self._pending
        self._pending = None
        _PENDING_OPTIMIZERS.discard(self)
        if self.profile_exchange and self.flat.theta.is_cuda:   # how long the compute stream stalls for the exchange
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            work.wait()
            e1.record()
            self.exchange_events.append((e0, e1))
        else:
            work.wait()
        self._exchange_done()
        self._apply(scale, live, hyper)
        if self._zero_after_flush:
            self._zero_after_flush = False
            self.flat.zero_grad()

    # -- gradient norm / clip / skip ------------------------------------------------------------------------------
    @property
    def last_grad_norm(self) -> torch.Tensor:
        """0-dim device view of the latest step's gradient norm (NaN before the first measured step); no sync, valid until
        the next step."""
        return self._norm_state[0]

    def stats(self) -> dict:
        """One small device-to-host read: the latest norm and coefficient, and how many steps were clipped / skipped."""
        self.flush()
        host = self._norm_buf.cpu()
        norm, coef = host[:2].view(torch.float32).tolist()
        return {"grad_norm": norm, "clip_coef": coef, "clipped_steps": int(host[4]), "skipped_steps": int(host[5])}

    def grad_norms(self) -> Dict[str, float]:
        """name -> L2 norm of that tensor's gradient in the latest step (0 for a tensor that received none)."""
        self.flush()
        if self._seg_norm is None:
            raise RuntimeError("grad_norms(): no step has measured the gradient yet (max_grad_norm / skip_nonfinite / "
                               "track_grad_norm are all off, or step() has not run)")
        return dict(zip(self.flat.names, self._seg_norm.tolist()))

    def _apply(self, scale, all_live=False, hyper=None):
        """Dots (A-GEM / GEM / OGD: they also set the liveness flags; OGD projects here) -> norm of the gradient the step consumes
        (when measured) -> the step, all on the device.  One entry point per family of variants, for one or many parameter groups."""
        self.step_count += 1
        g = self.param_groups[0]
        lrs, wds = self._group_hyper() if hyper is None else hyper
        f, L, ptr, stream = self.flat, _lib.lib(), _lib.ptr, _lib.stream_ptr()
        max_norm, skip = g.get("max_grad_norm"), bool(g.get("skip_nonfinite", False))
        si, pb = self.path_integral, self.masks
        measured = max_norm is not None or skip or self.track_grad_norm
        penalised = si is not None and si.tasks_consolidated > 0
        all_live = bool(all_live) or penalised       # autograd on loss + surrogate gives every trainable tensor a gradient
        scale, nchunks, nseg, n = float(scale), f.chunk_table.shape[0], len(f.entries), len(lrs)
        proj = self.projection if self.projection is not None and self.projection.has_reference else None
        ogd, proj = (proj, None) if isinstance(proj, OGD) else (None, proj)
        gem, agem = (proj, None) if isinstance(proj, GEM) else (None, proj)
        if measured and self._seg_norm is None:
            self._seg_norm = torch.zeros(nseg, dtype=torch.float32, device=f.theta.device)
            self._norm_ws = torch.empty(L.ia_grad_norm_workspace_bytes(nchunks), dtype=torch.uint8, device=f.theta.device)
        live = None if all_live else ptr(self.seg_active)
        # what every step takes: head, betas, eps, scale, shadow, the group arrays, norm / skip / counters
        common = (ptr(f.theta), ptr(f.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(f.chunk_table), nchunks,
                  ptr(self.seg_active), ptr(self.seg_step), nseg, int(all_live), float(g["betas"][0]), float(g["betas"][1]),
                  float(g["eps"]), scale, ptr(self.shadow), ptr(self.seg_group), n, (ctypes.c_float * n)(*lrs),
                  (ctypes.c_float * n)(*wds), ptr(self._norm_state) if measured else None, int(skip),
                  ptr(self._counters) if measured else None)
        # ... and every norm: ia_grad_norm, or that of the projected gradient with the variant's rows behind it
        norm = (ptr(f.grad), ptr(f.chunk_table), nchunks, ptr(f.seg_chunk_begin), nseg, scale,
                0.0 if max_norm is None else float(max_norm), live, ptr(self._seg_norm), ptr(self._norm_state),
                ptr(self._norm_ws), self._norm_ws.numel()) if measured else None
        if ogd is not None:      # rewrites the flat gradient; the flags its dots set survive the liveness passes below
            ogd.project_step(live)
        if gem is not None:
            k, ws = len(gem.tasks()), gem.workspace(nchunks)
            rows = (ptr(gem.refs), gem.stride, k, ptr(gem.state))
            _lib.check(L.ia_gem_dots(ptr(f.grad), ptr(gem.refs), gem.stride, k, ptr(f.chunk_table), nchunks, nseg, scale, live, -1,
                                     ptr(gem.sums), ptr(ws), ws.numel(), stream), "ia_gem_dots")
            _lib.check(L.ia_gem_solve(ptr(gem.sums), ptr(gem.state), k, gem.memory_strength, gem.eps, stream), "ia_gem_solve")
            if measured:
                _lib.check(L.ia_grad_norm_gem(*norm, *rows, stream), "ia_grad_norm_gem")
            _lib.check(L.ia_adamw_step_segmented_gem(*common, *rows, ptr(gem.counters), stream), "ia_adamw_step_segmented_gem")
            return self._after_update()
        if agem is not None:
            ws = agem.workspace(nchunks)
            _lib.check(L.ia_agem_dots(ptr(f.grad), ptr(agem.ref.flat), ptr(f.chunk_table), nchunks, nseg, scale, live,
                                      ptr(agem.proj_state), ptr(ws), ws.numel(), stream), "ia_agem_dots")
            if measured:
                _lib.check(L.ia_grad_norm_projected(*norm, ptr(agem.ref.flat), ptr(agem.proj_state), stream),
                           "ia_grad_norm_projected")
        elif measured and isinstance(pb, PackNet):
            _lib.check(L.ia_grad_norm_packed(*norm, ptr(pb.owner), ptr(pb.seg_kind), int(pb.train_owner), stream),
                       "ia_grad_norm_packed")
        elif measured:
            _lib.check(L.ia_grad_norm(*norm, stream), "ia_grad_norm")
        if isinstance(pb, PackNet):
            _lib.check(L.ia_adamw_step_segmented_packed(*common, ptr(pb.owner), ptr(pb.seg_kind), int(pb.train_owner), stream),
                       "ia_adamw_step_segmented_packed")
            return self._after_update()
        if isinstance(pb, LoRA):
            pb._step(self, common, measured, skip, all_live, stream)
            return self._after_update()
        if pb is not None:
            _lib.check(L.ia_adamw_step_segmented_masked(*common, ptr(pb.base.flat), ptr(pb.scores.flat), ptr(pb.seg_kind),
                                                        pb.threshold, stream), "ia_adamw_step_segmented_masked")
            return self._after_update()
        if isinstance(si, RWalk):       # agem is None here: projection and path_integral are refused together
            rw, fp = si, lambda d: ptr(d.flat) if d is not None else None
            _lib.check(L.ia_adamw_step_segmented_rwalk(
                *common, ptr(rw.fisher.flat), fp(rw.w), fp(rw.anchor), fp(rw.score),
                ptr(rw.importance.flat) if penalised else None, ptr(rw.theta_star.flat) if penalised else None,
                rw.rw_lambda, rw.alpha, rw.eps, rw._next_fold(), stream), "ia_adamw_step_segmented_rwalk")
            return self._after_update()
        # plain, clipped, SI or projected: the operands that are present select the variant
        _lib.check(L.ia_adamw_step_segmented_grouped(
            *common, ptr(si.w.flat) if si is not None else None, ptr(si.omega.flat) if penalised else None,
            ptr(si.theta_star.flat) if penalised else None, float(si.si_c) if si is not None else 0.0,
            ptr(agem.ref.flat) if agem is not None else None, ptr(agem.proj_state) if agem is not None else None,
            ptr(agem.proj_counters) if agem is not None else None, stream), "ia_adamw_step_segmented_grouped")
        self._after_update()

    def _after_update(self):
        if self.flat.theta.is_cuda:
            global LAST_UPDATE_EVENT
            LAST_UPDATE_EVENT = torch.cuda.Event()
            LAST_UPDATE_EVENT.record()
        from .ops import fast
        fast.bump_weight_epoch()  # the kernel rewrote theta by raw pointer: bf16 weight shadows are stale now
        if self.shadow is not None:  # ... and were re-made by the same kernel: hand the views to the shadow cache
            for (n, o, k, shape), q in zip(self.flat.entries, self.flat.params):
                if q.dim() >= 2:
                    fast.register_flat_shadow(q, self.shadow[o:o + k].view(shape[0], -1))

    # -- resumable state --------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Moments, per-tensor step counters, hyper-parameters and the clip / skip counters as CPU tensors and plain values,
        with the flat layout they belong to (a pending deferred update is applied first)."""
        self.flush()
        counters = self._counters.cpu()
        sd = {"entries": list(self.flat.entries),
              "exp_avg": self.exp_avg.detach().to("cpu", copy=True), "exp_avg_sq": self.exp_avg_sq.detach().to("cpu", copy=True),
              "seg_step": self.seg_step.to("cpu", copy=True), "step_count": self.step_count,
              "param_group": {k: v for k, v in self.param_groups[0].items() if k not in ("params", "names")},
              "clipped_steps": int(counters[0]), "skipped_steps": int(counters[1])}
        if len(self.param_groups) > 1:      # the partition and every group's values (with whatever keys a scheduler added)
            sd["param_groups"] = [dict({k: v for k, v in g.items() if k != "params"}, names=list(names))
                                  for g, names in zip(self.param_groups, self._group_names)]
        return sd

    def load_state_dict(self, sd: dict, source="state dict"):
        """Inverse of state_dict(); refuses a state saved for another set of trainable tensors.  Weights and their bf16
        images are not part of the optimizer state and are left alone."""
        if [tuple(e[:3]) + (tuple(e[3]),) for e in sd["entries"]] != list(self.flat.entries):
            raise ValueError(f"{source}: 'optimizer' was saved for a different set of trainable tensors")
        saved_groups = sd.get("param_groups")
        partition = [list(g["names"]) for g in saved_groups] if saved_groups is not None else [list(self.flat.names)]
        if partition != self._group_names:
            raise ValueError(f"{source}: 'optimizer' was saved for a different partition into parameter groups "
                             f"({len(partition)} groups saved, {len(self._group_names)} here, compared by names and order)")
        self.flush()
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.seg_step.copy_(sd["seg_step"])
        self.step_count = int(sd["step_count"])
        hyper = dict(sd["param_group"])
        hyper["betas"] = tuple(hyper["betas"])
        self.param_groups[0].update(hyper)
        for g, saved in zip(self.param_groups, saved_groups or []):
            values = {k: v for k, v in saved.items() if k != "names"}
            if "betas" in values:
                values["betas"] = tuple(values["betas"])
            g.update(values)
        self._counters.copy_(torch.tensor([sd["clipped_steps"], sd["skipped_steps"]], dtype=torch.int32))


_PENDING_OPTIMIZERS = set()
LAST_UPDATE_EVENT = None   # recorded on the stream of the latest AdamW launch (side streams wait for it)


def flush_pending_updates():
    """Apply every deferred optimizer update (FusedAdamW.step under data parallelism).  Called by the model before the
    first module that reads trainable weights, and by every helper here that reads or swaps the flat weights."""
    for opt in list(_PENDING_OPTIMIZERS):
        opt.flush()
