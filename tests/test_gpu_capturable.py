"""GPU tests of the capturable fused optimizers (capturable_ops.hip):
device-side lr / step, the fused global-norm clip, and hipGraph replay.

References are torch.optim (+ torch.nn.utils.clip_grad_norm_) run eagerly
on the same device, with the tolerances of tests/test_gpu_ops.py; the
clip-off and eager-vs-replay comparisons are bit-exact.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X", allow_module_level=True)

from shockwave_amd import ops
from shockwave_amd.ops.optim import (
    FusedAdam,
    FusedSGD,
    reset_optimizer_state_inplace,
)

assert ops.HAVE_EXT, "HIP extension must be built (fail loudly, no fallback)"

DEV = torch.device("cuda:0")
# tail only, vector + tail, exactly one chunk, one chunk + 1, several chunks
SIZES = [3, 1000, 32768, 32769, 3 * 32768 + 5]
PARAM_TOL = dict(rtol=1e-4, atol=1e-6)
NORM_TOL = dict(rtol=1e-4, atol=1e-5)


def make_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV))
            for s in SIZES]


def make_grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(s, generator=g).to(DEV) for s in SIZES]


def set_grads(params, grads):
    """Copy into the existing .grad (stable staging buffers)."""
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def true_norm(grads):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item()


def capture_step(opt):
    """Capture one opt.step() (nothing executes during capture)."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return graph


def eager_warmup(opt, params, first_step, n):
    """n eager steps on a side stream, as graph capture wants."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for step in range(first_step, first_step + n):
            set_grads(params, make_grads(step))
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def assert_params_close(mine, ref):
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a.data, b.data, **PARAM_TOL)


def assert_params_equal(mine, ref):
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a.data, b.data, rtol=0, atol=0)


# ---------------------------------------------------------------------------
# clip active
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_clip_active_matches_torch(kind):
    a, b = make_params(), make_params()
    grads = make_grads(0)
    norm = true_norm(grads)
    max_norm = 0.1 * norm
    if kind == "sgd":
        kw = dict(lr=0.1, momentum=0.9, weight_decay=5e-4)
        mine = FusedSGD(a, max_grad_norm=max_norm, **kw)
        ref = torch.optim.SGD(b, **kw)
    else:
        kw = dict(lr=1e-3, weight_decay=1e-2)
        mine = FusedAdam(a, max_grad_norm=max_norm, **kw)
        ref = torch.optim.Adam(b, **kw)
    for _ in range(3):
        set_grads(a, grads)
        set_grads(b, grads)  # clip_grad_norm_ rewrites the ref's .grad
        mine.step()
        ref_norm = torch.nn.utils.clip_grad_norm_(b, max_norm)
        ref.step()
        torch.testing.assert_close(mine.grad_norm, ref_norm, **NORM_TOL)
        torch.testing.assert_close(
            mine.grad_norm.item(), norm, **NORM_TOL
        )
        # the fused clip scales in registers: .grad stays raw
        for p, g in zip(a, grads):
            assert torch.equal(p.grad, g)
    assert_params_close(a, b)


# ---------------------------------------------------------------------------
# clip inactive: the _cap kernels are the by-value kernels, bit for bit
# ---------------------------------------------------------------------------

def _cap_workspace(grads, lr):
    scalars = ops.new_scalar_block(1, DEV)
    scalars[ops.SCALAR_LR0].fill_(lr)
    partials = torch.zeros(ops.num_chunks(grads), device=DEV)
    return scalars, partials


def _cap_prologue(grads, scalars, partials):
    n = ops.multi_tensor_sumsq_partials(grads, partials, 0)
    assert n == partials.numel()
    ops.optim_prologue(partials, n, scalars, max_norm=1e30, clip=True)


@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [
    (0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 5e-4, True),
    (0.9, 0.5, 0.0, False),
])
def test_sgd_cap_bit_identical_to_fused_sgd(momentum, dampening, wd, nesterov):
    p_cap = [p.data for p in make_params()]
    p_old = [p.clone() for p in p_cap]
    m_cap = [torch.zeros_like(p) for p in p_cap]
    m_old = [torch.zeros_like(p) for p in p_cap]
    grads = make_grads(0)
    scalars, partials = _cap_workspace(grads, 0.1)
    kw = dict(momentum=momentum, dampening=dampening, weight_decay=wd,
              nesterov=nesterov)
    for step in range(3):
        _cap_prologue(grads, scalars, partials)
        ops.fused_sgd_cap(p_cap, grads, m_cap, scalars, 0, **kw)
        ops.fused_sgd(p_old, grads, m_old, lr=0.1,
                      buf_initialized=(step > 0), **kw)
    torch.cuda.synchronize()
    assert scalars[ops.SCALAR_CLIP_COEF].item() == 1.0
    assert ops.scalar_step_view(scalars).item() == 3
    for a, b in zip(p_cap + m_cap, p_old + m_old):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


@pytest.mark.parametrize("adamw,wd", [(False, 0.0), (False, 1e-2), (True, 1e-2)])
def test_adam_cap_bit_identical_to_fused_adam(adamw, wd):
    p_cap = [p.data for p in make_params()]
    p_old = [p.clone() for p in p_cap]
    state_cap = [[torch.zeros_like(p) for p in p_cap] for _ in range(2)]
    state_old = [[torch.zeros_like(p) for p in p_cap] for _ in range(2)]
    grads = make_grads(0)
    scalars, partials = _cap_workspace(grads, 1e-3)
    for step in range(1, 4):
        _cap_prologue(grads, scalars, partials)
        ops.fused_adam_cap(p_cap, grads, *state_cap, scalars, 0,
                           weight_decay=wd, adamw=adamw)
        ops.fused_adam(p_old, grads, *state_old, lr=1e-3, weight_decay=wd,
                       step=step, adamw=adamw)
    torch.cuda.synchronize()
    assert scalars[ops.SCALAR_CLIP_COEF].item() == 1.0
    for a, b in zip(p_cap + state_cap[0] + state_cap[1],
                    p_old + state_old[0] + state_old[1]):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_l2norm_sq_bit_identical_to_sumsq_partials():
    """The two kernels share one sum-of-squares body.  Tail only, float4
    loop only (1000 = 250 x 4), float4 loop + tail, exactly one chunk:
    every tensor is a single chunk, so l2norm's one atomicAdd onto a
    zeroed word is exact and must equal the plain store of the partials
    kernel.  Against fp64: a thread adds at most 32 float4 terms, then 8
    shuffle/LDS levels, so well under 100 roundings of 6e-8 each."""
    g = torch.Generator().manual_seed(7)
    sizes = (3, 1000, 1003, 32768)
    tensors = [torch.randn(s, generator=g).to(DEV) for s in sizes]
    out = torch.empty(len(tensors), device=DEV)
    partials = torch.full((len(tensors),), -1.0, device=DEV)
    ops._C.multi_tensor_l2norm_sq(tensors, out)
    assert ops.multi_tensor_sumsq_partials(tensors, partials, 0) == len(sizes)
    torch.cuda.synchronize()
    assert torch.equal(out, partials)
    want = torch.stack([(t.double() ** 2).sum() for t in tensors])
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=0)


def test_partials_workspace_bounds_are_checked():
    grads = make_grads(0)
    partials = torch.zeros(ops.num_chunks(grads) - 1, device=DEV)
    with pytest.raises(RuntimeError):
        ops.multi_tensor_sumsq_partials(grads, partials, 0)
    partials = torch.zeros(ops.num_chunks(grads), device=DEV)
    with pytest.raises(RuntimeError):
        ops.multi_tensor_sumsq_partials(grads, partials, 1)
    with pytest.raises(RuntimeError):
        ops.optim_prologue(partials, partials.numel() + 1,
                           ops.new_scalar_block(1, DEV), 1.0, True)
    with pytest.raises(RuntimeError):
        ops.fused_sgd_cap(grads, grads, grads,
                          ops.new_scalar_block(1, DEV), 1)


# ---------------------------------------------------------------------------
# two param groups: different lr, one global norm
# ---------------------------------------------------------------------------

def test_two_param_groups_one_global_norm():
    a, b = make_params(), make_params()
    grads = make_grads(0)
    norm = true_norm(grads)
    max_norm = 0.1 * norm

    def groups(ps):
        return [{"params": ps[:2], "lr": 0.1}, {"params": ps[2:], "lr": 0.02}]

    mine = FusedSGD(groups(a), lr=0.1, momentum=0.9, max_grad_norm=max_norm)
    ref = torch.optim.SGD(groups(b), lr=0.1, momentum=0.9)
    for _ in range(3):
        set_grads(a, grads)
        set_grads(b, grads)
        mine.step()
        ref_norm = torch.nn.utils.clip_grad_norm_(b, max_norm)
        ref.step()
        torch.testing.assert_close(mine.grad_norm, ref_norm, **NORM_TOL)
    assert_params_close(a, b)


# ---------------------------------------------------------------------------
# hipGraph replay
# ---------------------------------------------------------------------------

def test_adam_under_replay_matches_eager_torch():
    """One captured step() replayed for steps 4..10: the bias corrections
    must follow the device step, not the step at capture."""
    a, b = make_params(), make_params()
    mine = FusedAdam(a, lr=1e-3, capturable=True)
    ref = torch.optim.Adam(b, lr=1e-3)
    eager_warmup(mine, a, first_step=1, n=3)
    graph = capture_step(mine)
    for step in range(4, 11):
        set_grads(a, make_grads(step))
        graph.replay()
    for step in range(1, 11):
        set_grads(b, make_grads(step))
        ref.step()
    assert mine.state_dict()["swq_step_count"] == 10
    assert_params_close(a, b)


def test_lr_change_under_replay():
    a, b, c = make_params(), make_params(), make_params()
    kw = dict(lr=0.1, momentum=0.9, max_grad_norm=50.0)
    graphed = FusedSGD(a, **kw)
    eager = FusedSGD(b, **kw)
    ref = torch.optim.SGD(c, lr=0.1, momentum=0.9)

    eager_warmup(graphed, a, first_step=1, n=3)
    graph = capture_step(graphed)
    for step in range(4, 8):
        if step == 6:
            graphed.set_lr(0.01)
        set_grads(a, make_grads(step))
        graph.replay()

    for step in range(1, 8):
        if step == 6:
            eager.set_lr(0.01)
            ref.param_groups[0]["lr"] = 0.01
        grads = make_grads(step)
        set_grads(b, grads)
        eager.step()
        set_grads(c, grads)
        torch.nn.utils.clip_grad_norm_(c, 50.0)
        ref.step()

    assert_params_close(a, c)
    # same kernels, fixed-order norm reduction: replay == eager, bit for bit
    assert_params_equal(a, b)
    torch.testing.assert_close(graphed.grad_norm, eager.grad_norm,
                               rtol=0, atol=0)


def test_session_reset_under_replay():
    a = make_params()
    kw = dict(lr=0.1, momentum=0.9, dampening=0.5)
    mine = FusedSGD(a, capturable=True, **kw)
    eager_warmup(mine, a, first_step=1, n=3)
    graph = capture_step(mine)
    for step in range(4, 6):
        set_grads(a, make_grads(step))
        graph.replay()

    reset_optimizer_state_inplace(mine)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    fresh = torch.optim.SGD(b, **kw)
    grads = make_grads(6)
    set_grads(a, grads)
    set_grads(b, grads)
    graph.replay()
    fresh.step()
    assert mine.state_dict()["swq_step_count"] == 1
    assert_params_close(a, b)
    torch.testing.assert_close(
        mine.state[a[-1]]["momentum_buffer"],
        fresh.state[b[-1]]["momentum_buffer"], **PARAM_TOL
    )
