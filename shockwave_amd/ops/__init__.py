"""Fused multi-tensor ops: CDNA4 HIP kernels with torch fp32 reference.

Dispatch rule:

* device (ROCm) tensors -> the compiled ``shockwave_amd.ops._C`` extension.
  If the extension is missing on a GPU machine the call raises — there is
  NO silent eager fallback on GPU (the HIP path must be the one that runs).
* CPU tensors -> pure-torch reference implementations of the same math,
  used by CPU tests and as the numerics baseline for the GPU kernels.
"""

from __future__ import annotations

import math
from typing import List, Tuple

import torch

try:
    from . import _C  # compiled by setup.py build_ext --inplace

    HAVE_EXT = True
except ImportError:  # pragma: no cover - exercised on CPU-only boxes
    _C = None
    HAVE_EXT = False


def _require_ext():
    if not HAVE_EXT:
        raise RuntimeError(
            "shockwave_amd.ops._C extension not built; run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace`. "
            "GPU tensors are never silently handled in eager mode."
        )


# ---------------------------------------------------------------------------
# fused SGD
# ---------------------------------------------------------------------------

def fused_sgd(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    momentum_bufs: List[torch.Tensor],
    lr: float,
    momentum: float = 0.0,
    dampening: float = 0.0,
    weight_decay: float = 0.0,
    nesterov: bool = False,
    buf_initialized: bool = True,
) -> None:
    if params[0].is_cuda:
        _require_ext()
        _C.fused_sgd(
            params, grads, momentum_bufs, lr, momentum, dampening,
            weight_decay, nesterov, buf_initialized,
        )
        return
    for p, g, b in zip(params, grads, momentum_bufs):
        d_p = g.clone()
        if weight_decay != 0:
            d_p.add_(p, alpha=weight_decay)
        if momentum != 0:
            if not buf_initialized:
                b.copy_(d_p)
            else:
                b.mul_(momentum).add_(d_p, alpha=1 - dampening)
            d_p = d_p.add(b, alpha=momentum) if nesterov else b.clone()
        p.add_(d_p, alpha=-lr)


# ---------------------------------------------------------------------------
# fused Adam
# ---------------------------------------------------------------------------

def fused_adam(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    exp_avgs: List[torch.Tensor],
    exp_avg_sqs: List[torch.Tensor],
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    step: int = 1,
    adamw: bool = False,
) -> None:
    if params[0].is_cuda:
        _require_ext()
        _C.fused_adam(
            params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps,
            weight_decay, step, adamw,
        )
        return
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        g = g.clone()
        if adamw:
            p.mul_(1 - lr * weight_decay)
        elif weight_decay != 0:
            g.add_(p, alpha=weight_decay)
        m.mul_(beta1).add_(g, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)


# ---------------------------------------------------------------------------
# Accordion helpers
# ---------------------------------------------------------------------------

def multi_tensor_accum(
    dsts: List[torch.Tensor], srcs: List[torch.Tensor], alpha: float = 1.0
) -> None:
    """dst += alpha * src elementwise for each tensor pair."""
    if dsts[0].is_cuda:
        _require_ext()
        _C.multi_tensor_accum(dsts, srcs, alpha)
        return
    for d, s in zip(dsts, srcs):
        d.add_(s, alpha=alpha)


def multi_tensor_l2norm(tensors: List[torch.Tensor]) -> torch.Tensor:
    """Per-tensor L2 norms, returned as a 1-D tensor of len(tensors)."""
    if tensors[0].is_cuda:
        _require_ext()
        out = torch.empty(
            len(tensors), dtype=torch.float32, device=tensors[0].device
        )
        _C.multi_tensor_l2norm_sq(tensors, out)
        return out.sqrt()
    return torch.stack([t.norm() for t in tensors])


# ---------------------------------------------------------------------------
# GNS estimator
# ---------------------------------------------------------------------------

def gns_window_stats(
    window_grads: List[torch.Tensor],
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(||mean of window||^2, ||last grad||^2) over flat fp32 grads."""
    if window_grads[0].is_cuda:
        _require_ext()
        out = torch.empty(
            2, dtype=torch.float32, device=window_grads[0].device
        )
        _C.gns_window_stats(window_grads, out)
        return out[0], out[1]
    mean = torch.stack(window_grads).mean(dim=0)
    return (mean * mean).sum(), (window_grads[-1] * window_grads[-1]).sum()


# ---------------------------------------------------------------------------
# capturable (graph-safe) optimizer steps: scalars in device memory
# ---------------------------------------------------------------------------
#
# Scalar block: one contiguous fp32 tensor per optimizer, 32-bit words
#   [0] grad_norm  [1] clip_coef  [2] step (int32 bits)  [3] reserved
#   [4+g] lr of param group g
# The kernels take the layout from csrc/swq_layout.h.  The CPU path must
# work without the extension, so the constants are repeated here and
# checked against the extension's when it is there.

CHUNK_ELEMS = 32768
SCALAR_GRAD_NORM = 0
SCALAR_CLIP_COEF = 1
SCALAR_STEP = 2
SCALAR_LR0 = 4


def _check_layout(ext) -> None:
    """Raise unless ``ext`` was compiled with this module's layout."""
    for name in ("CHUNK_ELEMS", "SCALAR_GRAD_NORM", "SCALAR_CLIP_COEF",
                 "SCALAR_STEP", "SCALAR_LR0"):
        if globals()[name] != getattr(ext, name):
            raise RuntimeError(
                f"shockwave_amd.ops.{name} = {globals()[name]} but the "
                f"extension was built with {getattr(ext, name)} "
                "(csrc/swq_layout.h)"
            )


if HAVE_EXT:
    _check_layout(_C)


def num_chunks(tensors: List[torch.Tensor]) -> int:
    """Blocks (= partial sums) the multi-tensor kernels use for a list."""
    return sum((t.numel() + CHUNK_ELEMS - 1) // CHUNK_ELEMS for t in tensors)


def new_scalar_block(num_groups: int, device) -> torch.Tensor:
    """Zeroed scalar block (step 0, clip_coef 1) for ``num_groups`` lrs."""
    block = torch.zeros(SCALAR_LR0 + num_groups, dtype=torch.float32,
                        device=device)
    block[SCALAR_CLIP_COEF] = 1.0
    return block


def scalar_step_view(scalars: torch.Tensor) -> torch.Tensor:
    """int32 view (shape [1]) of the step word of a scalar block."""
    return scalars.view(torch.int32)[SCALAR_STEP:SCALAR_STEP + 1]


def multi_tensor_sumsq_partials(
    tensors: List[torch.Tensor], partials: torch.Tensor, offset: int = 0
) -> int:
    """partials[offset + b] = sum of squares of chunk b of ``tensors``
    (32K-element chunks, tensor-major).  Returns the chunk count."""
    if tensors[0].is_cuda:
        _require_ext()
        return _C.multi_tensor_sumsq_partials(tensors, partials, offset)
    b = offset
    for t in tensors:
        flat = t.reshape(-1)
        for c in range(0, flat.numel(), CHUNK_ELEMS):
            chunk = flat[c:c + CHUNK_ELEMS]
            partials[b] = (chunk * chunk).sum()
            b += 1
    assert b <= partials.numel(), "partials workspace too small"
    return b - offset


def optim_prologue(
    partials: torch.Tensor,
    num_partials: int,
    scalars: torch.Tensor,
    max_norm: float = 0.0,
    clip: bool = False,
) -> None:
    """Start one optimizer step: grad_norm = sqrt(sum(partials[:n])),
    clip_coef = min(1, max_norm / (grad_norm + 1e-6)) (1 when ``clip`` is
    off), step += 1 — all written into ``scalars`` on its device."""
    if scalars.is_cuda:
        _require_ext()
        _C.optim_prologue(partials, num_partials, scalars, max_norm, clip)
        return
    norm = partials[:num_partials].sum().sqrt()
    scalars[SCALAR_GRAD_NORM] = norm
    if clip:
        scalars[SCALAR_CLIP_COEF] = torch.clamp(
            max_norm / (norm + 1e-6), max=1.0
        )
    else:
        scalars[SCALAR_CLIP_COEF] = 1.0
    scalar_step_view(scalars).add_(1)


def fused_sgd_cap(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    momentum_bufs: List[torch.Tensor],
    scalars: torch.Tensor,
    group: int = 0,
    momentum: float = 0.0,
    dampening: float = 0.0,
    weight_decay: float = 0.0,
    nesterov: bool = False,
) -> None:
    """``fused_sgd`` with lr, the first-step flag (step == 1 after the
    prologue's advance) and clip_coef read from ``scalars``.  The gradient
    is scaled by clip_coef on the fly; ``grads`` are not modified."""
    if params[0].is_cuda:
        _require_ext()
        _C.fused_sgd_cap(
            params, grads, momentum_bufs, scalars, group, momentum,
            dampening, weight_decay, nesterov,
        )
        return
    coef = scalars[SCALAR_CLIP_COEF]
    step = int(scalar_step_view(scalars).item())
    fused_sgd(
        params, [g * coef for g in grads], momentum_bufs,
        lr=float(scalars[SCALAR_LR0 + group]), momentum=momentum,
        dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
        buf_initialized=(step - 1) != 0,
    )


def fused_adam_cap(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    exp_avgs: List[torch.Tensor],
    exp_avg_sqs: List[torch.Tensor],
    scalars: torch.Tensor,
    group: int = 0,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    adamw: bool = False,
) -> None:
    """``fused_adam`` with lr, step and clip_coef read from ``scalars``.
    The gradient is scaled by clip_coef on the fly; ``grads`` are not
    modified."""
    if params[0].is_cuda:
        _require_ext()
        _C.fused_adam_cap(
            params, grads, exp_avgs, exp_avg_sqs, scalars, group, beta1,
            beta2, eps, weight_decay, adamw,
        )
        return
    coef = scalars[SCALAR_CLIP_COEF]
    fused_adam(
        params, [g * coef for g in grads], exp_avgs, exp_avg_sqs,
        lr=float(scalars[SCALAR_LR0 + group]), beta1=beta1, beta2=beta2,
        eps=eps, weight_decay=weight_decay,
        step=int(scalar_step_view(scalars).item()), adamw=adamw,
    )
