"""torch.optim-compatible optimizers backed by the fused CDNA4 kernels.

Drop-in for the reference workloads' ``optim.SGD(momentum=0.9, wd=5e-4)``
and Adam optimizers: one multi-tensor kernel per
step instead of per-parameter elementwise ops.

The per-group tensor lists are assembled once and cached: gradients are
pre-created with the param's layout and never set to None (see
``_preinit_grads`` and workloads.common.zero_grads), so the param/grad/
state tensor identities are stable across steps — the cache removes
~100 us of per-step Python when the GPU step itself is ~2 ms.

Capturable mode (``capturable=True`` or ``max_grad_norm=...``): lr, the
step counter and the clip coefficient live in a device-resident scalar
block that the kernels read, so one captured hipGraph of ``step()`` stays
correct across steps, LR changes and session reuse.  With
``max_grad_norm`` the global L2 norm over ALL param groups is reduced on
device (deterministically, no atomics) and the clip is applied to the
gradient in registers inside the update kernel.  Unlike
``torch.nn.utils.clip_grad_norm_`` this does NOT modify ``.grad``: code
that reads gradients after ``step()`` (Accordion, GNS) keeps seeing the
raw values.  With both options at their defaults the by-value kernels run
exactly as before.
"""

from __future__ import annotations

import torch

from . import (
    SCALAR_GRAD_NORM,
    SCALAR_LR0,
    fused_adam,
    fused_adam_cap,
    fused_sgd,
    fused_sgd_cap,
    multi_tensor_sumsq_partials,
    new_scalar_block,
    num_chunks,
    optim_prologue,
    scalar_step_view,
)


def _load_state_inplace(opt, state_dict):
    """Copy a checkpoint's per-param state tensors INTO the optimizer's
    existing state tensors (same addresses) instead of replacing them —
    a session-cached hipGraph holds the old addresses.  Returns False on
    any structural mismatch (caller falls back to the replacing load)."""
    groups = opt.param_groups
    saved_groups = state_dict.get("param_groups")
    saved_state = state_dict.get("state", {})
    if saved_groups is None or len(saved_groups) != len(groups):
        return False
    # torch state_dict convention: params are indexed in group order
    own_params = [p for g in groups for p in g["params"]]
    saved_ids = [i for g in saved_groups for i in g["params"]]
    if len(own_params) != len(saved_ids):
        return False
    for p, sid in zip(own_params, saved_ids):
        saved = saved_state.get(sid, {})
        cur = opt.state.get(p, {})
        for key, val in saved.items():
            if torch.is_tensor(val) and val.dim() > 0:
                if key not in cur or cur[key].shape != val.shape:
                    return False
        for key, val in saved.items():
            if torch.is_tensor(val) and val.dim() > 0:
                cur[key].copy_(val.to(cur[key].device))
            else:
                cur[key] = val
    for g, sg in zip(groups, saved_groups):
        for k, v in sg.items():
            if k != "params":
                g[k] = v
    return True


def reset_optimizer_state_inplace(opt):
    """Zero all state tensors in place (fresh job reusing a cached
    session) without changing addresses."""
    for s in opt.state.values():
        for v in s.values():
            if torch.is_tensor(v) and v.dim() > 0:
                v.zero_()
    if isinstance(opt, FusedAdam):
        opt._step_count = 0
    if isinstance(opt, FusedSGD):
        opt._buffers_initialized = False
    if getattr(opt, "capturable", False) and opt._scalars is not None:
        # the device step is what a captured graph reads
        scalar_step_view(opt._scalars).zero_()


def _preinit_grads(param_groups):
    """Create zero gradients with each param's own memory layout before
    the first backward: autograd then accumulates into them, so grad
    layout always matches the param (a backward kernel is otherwise free
    to emit a different-layout grad, e.g. NCHW grads for channels_last
    1x1-conv weights) and grad addresses stay stable for the metadata
    cache and hipGraphs."""
    for group in param_groups:
        for p in group["params"]:
            if p.requires_grad and p.grad is None:
                p.grad = torch.zeros_like(p)


class _FusedOptimizer(torch.optim.Optimizer):
    """The step skeleton and the device-resident lr / step / clip state
    shared by the fused optimizers.  Subclasses provide

    * ``_build_lists()``: one ``(group, params, grads, ...)`` entry per
      param group, the tensor lists in the order their kernel takes them;
    * ``_advance()``: count one by-value step and return the keyword
      arguments it adds to every ``_launch``;
    * ``_launch(group, *lists, **step_kw)``: the by-value kernel;
    * ``_launch_cap(gi, group, *lists)``: the capturable kernel."""

    def __init__(self, params, defaults, max_grad_norm, capturable):
        super().__init__(params, defaults)
        _preinit_grads(self.param_groups)
        self._cached_lists = None
        self.max_grad_norm = max_grad_norm
        self.capturable = bool(capturable) or max_grad_norm is not None
        self._scalars = None    # scalar block, see ops/__init__.py
        self._partials = None   # per-chunk sum-of-squares workspace
        self._pushed_lr = None  # host mirror of the device lrs

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._ensure_lists()
        if self.capturable:
            self._begin_capturable_step()
        else:
            step_kw = self._advance()
        for gi, (group, *lists) in enumerate(self._cached_lists):
            if not lists[0]:
                continue
            if self.capturable:
                self._launch_cap(gi, group, *lists)
            else:
                self._launch(group, *lists, **step_kw)
        return loss

    def _ensure_lists(self):
        """Build (once) the tensor lists and, in capturable mode, the
        scalar block and partials workspace cached with them.  Both keep
        their addresses when the lists are rebuilt."""
        if self._cached_lists is None:
            self._cached_lists = self._build_lists()
        if not self.capturable:
            return
        if self._scalars is None:
            device = self.param_groups[0]["params"][0].device
            self._scalars = new_scalar_block(len(self.param_groups), device)
            self._pushed_lr = [None] * len(self.param_groups)
        chunks = sum(num_chunks(entry[2]) for entry in self._cached_lists)
        if self._partials is None or self._partials.numel() < max(1, chunks):
            self._partials = torch.zeros(
                max(1, chunks), dtype=torch.float32,
                device=self._scalars.device,
            )

    def _begin_capturable_step(self):
        """Norm partials (when clipping) + the one-block prologue."""
        if not _stream_is_capturing():
            self.sync_hyperparams()
        n = 0
        clip = self.max_grad_norm is not None
        if clip:
            for entry in self._cached_lists:
                if entry[1]:
                    n += multi_tensor_sumsq_partials(
                        entry[2], self._partials, n
                    )
        optim_prologue(
            self._partials, n, self._scalars,
            max_norm=float(self.max_grad_norm) if clip else 0.0, clip=clip,
        )

    def set_lr(self, value, group=None):
        """Set the learning rate of one param group (all when ``group`` is
        None).  In capturable mode the device scalar is written in place,
        so a captured graph picks the new value up on its next replay."""
        groups = range(len(self.param_groups)) if group is None else [group]
        for gi in groups:
            self.param_groups[gi]["lr"] = value
        self.sync_hyperparams()

    def sync_hyperparams(self):
        """Push any ``param_groups[i]['lr']`` that changed on the host
        (e.g. through a torch LR scheduler) to the device scalars.  No-op
        when nothing changed.  Call it outside a graph capture."""
        if not self.capturable:
            return
        self._ensure_lists()
        for gi, group in enumerate(self.param_groups):
            lr = float(group["lr"])
            if self._pushed_lr[gi] != lr:
                self._scalars[SCALAR_LR0 + gi].fill_(lr)
                self._pushed_lr[gi] = lr

    @property
    def grad_norm(self):
        """0-dim device tensor: global pre-clip gradient L2 norm of the
        last step (a view of the scalar block; no host sync).  Computed
        only when ``max_grad_norm`` is set, else 0."""
        if not self.capturable:
            raise RuntimeError("grad_norm requires a capturable optimizer")
        self._ensure_lists()
        return self._scalars[SCALAR_GRAD_NORM]

    def _device_step(self):
        return int(scalar_step_view(self._scalars).item())

    def _set_device_step(self, value):
        self._ensure_lists()
        scalar_step_view(self._scalars).fill_(int(value))
        # a checkpoint's param_groups may carry a different lr
        self.sync_hyperparams()


def _stream_is_capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class FusedSGD(_FusedOptimizer):
    def __init__(self, params, lr, momentum=0.0, dampening=0.0,
                 weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 capturable=False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening,
                        weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults, max_grad_norm, capturable)
        self._buffers_initialized = False

    def _build_lists(self):
        cached = []
        for group in self.param_groups:
            params, grads, bufs = [], [], []
            momentum = group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if momentum != 0 and "momentum_buffer" not in state:
                    state["momentum_buffer"] = torch.zeros_like(p)
                params.append(p)
                grads.append(p.grad)
                bufs.append(
                    state["momentum_buffer"] if momentum != 0 else p.grad
                )
            cached.append((group, params, grads, bufs))
        return cached

    def _advance(self):
        buf_initialized = self._buffers_initialized
        self._buffers_initialized = True
        return dict(buf_initialized=buf_initialized)

    @staticmethod
    def _hyper(group):
        return {k: group[k] for k in
                ("momentum", "dampening", "weight_decay", "nesterov")}

    def _launch(self, group, params, grads, bufs, buf_initialized):
        fused_sgd(params, grads, bufs, lr=group["lr"],
                  buf_initialized=buf_initialized, **self._hyper(group))

    def _launch_cap(self, gi, group, params, grads, bufs):
        fused_sgd_cap(params, grads, bufs, self._scalars, gi,
                      **self._hyper(group))

    def state_dict(self):
        d = super().state_dict()
        if self.capturable:
            self._ensure_lists()
            d["swq_step_count"] = self._device_step()
        return d

    def load_state_dict(self, state_dict):
        saved_step = state_dict.get("swq_step_count")
        state_dict = {k: v for k, v in state_dict.items()
                      if k != "swq_step_count"}
        if self.capturable:
            self._ensure_lists()  # state tensors exist: load in place
        # in place, addresses unchanged: cached lists (and any captured
        # graph) stay valid
        if not _load_state_inplace(self, state_dict):
            super().load_state_dict(state_dict)
            self._cached_lists = None  # state tensors were replaced
        # restored momentum buffers must accumulate, not be overwritten
        self._buffers_initialized = any(
            "momentum_buffer" in s for s in self.state.values()
        )
        if self.capturable:
            # into the existing device word; a checkpoint without a step
            # (stock SGD, non-capturable FusedSGD) resumes past the
            # first-step branch iff it carries momentum buffers
            if saved_step is None:
                saved_step = 1 if self._buffers_initialized else 0
            self._set_device_step(saved_step)


class FusedAdam(_FusedOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, adamw=False, amsgrad=False,
                 max_grad_norm=None, capturable=False):
        assert not amsgrad, "amsgrad not supported by the fused kernel"
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay, adamw=adamw)
        super().__init__(params, defaults, max_grad_norm, capturable)
        self._step_count = 0

    def _build_lists(self):
        cached = []
        for group in self.param_groups:
            params, grads, avgs, sqs = [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "exp_avg" not in state:
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                params.append(p)
                grads.append(p.grad)
                avgs.append(state["exp_avg"])
                sqs.append(state["exp_avg_sq"])
            cached.append((group, params, grads, avgs, sqs))
        return cached

    def _advance(self):
        self._step_count += 1
        return dict(step=self._step_count)

    @staticmethod
    def _hyper(group):
        beta1, beta2 = group["betas"]
        return dict(beta1=beta1, beta2=beta2, eps=group["eps"],
                    weight_decay=group["weight_decay"], adamw=group["adamw"])

    def _launch(self, group, params, grads, avgs, sqs, step):
        fused_adam(params, grads, avgs, sqs, lr=group["lr"], step=step,
                   **self._hyper(group))

    def _launch_cap(self, gi, group, params, grads, avgs, sqs):
        fused_adam_cap(params, grads, avgs, sqs, self._scalars, gi,
                       **self._hyper(group))

    def state_dict(self):
        d = super().state_dict()
        if self.capturable:
            self._ensure_lists()
            self._step_count = self._device_step()
        d["swq_step_count"] = self._step_count
        return d

    def load_state_dict(self, state_dict):
        # read without mutating the caller's dict; a checkpoint written by
        # stock torch.optim.Adam carries per-param 'step' entries instead —
        # derive the count from those so bias correction resumes correctly
        if "swq_step_count" in state_dict:
            self._step_count = state_dict["swq_step_count"]
            state_dict = {k: v for k, v in state_dict.items()
                          if k != "swq_step_count"}
        else:
            steps = [
                int(s["step"].item() if torch.is_tensor(s.get("step"))
                    else s.get("step", 0))
                for s in state_dict.get("state", {}).values()
            ]
            self._step_count = max(steps) if steps else 0
        if self.capturable:
            # into the existing device word: a captured graph keeps reading
            # the same address
            self._set_device_step(self._step_count)
        # drop a stock-Adam 'step' scalar so the in-place path does not
        # stash it; our step count is _step_count
        slim = {
            "param_groups": state_dict.get("param_groups"),
            "state": {
                k: {kk: vv for kk, vv in s.items() if kk != "step"}
                for k, s in state_dict.get("state", {}).items()
            },
        }
        if not _load_state_inplace(self, slim):
            super().load_state_dict(state_dict)
            self._cached_lists = None
        self.sync_hyperparams()


class FusedAdamW(FusedAdam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, max_grad_norm=None, capturable=False):
        super().__init__(params, lr, betas, eps, weight_decay, adamw=True,
                         max_grad_norm=max_grad_norm, capturable=capturable)
