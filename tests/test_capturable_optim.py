"""Capturable fused optimizers on the CPU path: device-side lr / step,
global-norm clipping folded into the step, and the loop wiring.

The CPU path of every op is the pure-torch statement of what the HIP
kernels compute, so these tests pin the semantics; tests/
test_gpu_capturable.py checks the kernels against the same references.
"""

import copy
import types

import pytest
import torch

from shockwave_amd import ops
from shockwave_amd.ops.optim import (
    FusedAdam,
    FusedAdamW,
    FusedSGD,
    reset_optimizer_state_inplace,
)

SIZES = [3, 1000, 32769]
PARAM_TOL = dict(rtol=1e-4, atol=1e-6)
NORM_TOL = dict(rtol=1e-4, atol=1e-5)


def make_params(seed=0, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in sizes]


def make_grads(step, sizes=SIZES, scale=1.0):
    g = torch.Generator().manual_seed(1000 + step)
    return [scale * torch.randn(s, generator=g) for s in sizes]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def run_pair(mine, mine_params, ref, ref_params, max_norm, steps=3):
    norms = []
    for step in range(steps):
        grads = make_grads(step)
        set_grads(mine_params, grads)
        set_grads(ref_params, grads)
        mine.step()
        norms.append((
            mine.grad_norm.clone(),
            torch.nn.utils.clip_grad_norm_(ref_params, max_norm),
        ))
        ref.step()
        # the fused clip leaves .grad alone
        for p, g in zip(mine_params, grads):
            assert torch.equal(p.grad, g)
    for a, b in zip(mine_params, ref_params):
        torch.testing.assert_close(a.data, b.data, **PARAM_TOL)
    return norms


@pytest.mark.parametrize("momentum,wd,nesterov,dampening", [
    (0.0, 0.0, False, 0.0), (0.9, 5e-4, False, 0.0), (0.9, 0.0, True, 0.0),
    (0.9, 0.0, False, 0.5),
])
def test_sgd_clip_matches_torch(momentum, wd, nesterov, dampening):
    a, b = make_params(), make_params()
    kw = dict(lr=0.1, momentum=momentum, weight_decay=wd, nesterov=nesterov,
              dampening=dampening)
    mine = FusedSGD(a, max_grad_norm=2.0, **kw)
    assert mine.capturable
    norms = run_pair(mine, a, torch.optim.SGD(b, **kw), b, 2.0)
    for got, want in norms:
        assert want > 2.0  # the clip is active
        torch.testing.assert_close(got, want, **NORM_TOL)


@pytest.mark.parametrize("cls,ref_cls,wd", [
    (FusedAdam, torch.optim.Adam, 0.0),
    (FusedAdam, torch.optim.Adam, 1e-2),
    (FusedAdamW, torch.optim.AdamW, 1e-2),
])
def test_adam_clip_matches_torch(cls, ref_cls, wd):
    a, b = make_params(), make_params()
    mine = cls(a, lr=1e-3, weight_decay=wd, max_grad_norm=2.0)
    norms = run_pair(mine, a, ref_cls(b, lr=1e-3, weight_decay=wd), b, 2.0)
    for got, want in norms:
        torch.testing.assert_close(got, want, **NORM_TOL)


def test_two_groups_share_one_global_norm():
    a, b = make_params(), make_params()

    def groups(ps):
        return [{"params": ps[:2], "lr": 0.1}, {"params": ps[2:], "lr": 0.01}]

    mine = FusedSGD(groups(a), lr=0.1, momentum=0.9, max_grad_norm=1.5)
    ref = torch.optim.SGD(groups(b), lr=0.1, momentum=0.9)
    norms = run_pair(mine, a, ref, b, 1.5)
    for got, want in norms:
        torch.testing.assert_close(got, want, **NORM_TOL)


def test_huge_max_norm_equals_unclipped():
    a, b = make_params(), make_params()
    mine = FusedSGD(a, lr=0.1, momentum=0.9, max_grad_norm=1e30)
    plain = FusedSGD(b, lr=0.1, momentum=0.9)
    assert not plain.capturable
    for step in range(3):
        grads = make_grads(step)
        set_grads(a, grads)
        set_grads(b, grads)
        mine.step()
        plain.step()
        assert float(mine._scalars[ops.SCALAR_CLIP_COEF]) == 1.0
    for x, y in zip(a, b):
        assert torch.equal(x.data, y.data)


def test_zero_grads_give_unit_coef_and_no_nan():
    a = make_params()
    before = [p.detach().clone() for p in a]
    mine = FusedAdam(a, lr=1e-3, max_grad_norm=0.25)
    set_grads(a, [torch.zeros(s) for s in SIZES])
    mine.step()
    assert float(mine._scalars[ops.SCALAR_CLIP_COEF]) == 1.0
    assert float(mine.grad_norm) == 0.0
    for p, p0 in zip(a, before):
        assert torch.isfinite(p).all()
        assert torch.equal(p.data, p0)


def test_defaults_keep_the_by_value_path():
    a = make_params()
    opt = FusedSGD(a, lr=0.1, momentum=0.9)
    set_grads(a, make_grads(0))
    opt.step()
    assert not opt.capturable and opt._scalars is None
    with pytest.raises(RuntimeError):
        opt.grad_norm


def test_set_lr_and_sync_hyperparams():
    a, b = make_params(), make_params()
    mine = FusedSGD(a, lr=0.1, momentum=0.9, capturable=True)
    ref = torch.optim.SGD(b, lr=0.1, momentum=0.9)
    for step in range(4):
        if step == 2:
            mine.set_lr(0.01)
            ref.param_groups[0]["lr"] = 0.01
            assert mine.param_groups[0]["lr"] == 0.01
            torch.testing.assert_close(
                mine._scalars[ops.SCALAR_LR0], torch.tensor(0.01)
            )
        grads = make_grads(step)
        set_grads(a, grads)
        set_grads(b, grads)
        mine.step()
        ref.step()
    for x, y in zip(a, b):
        torch.testing.assert_close(x.data, y.data, **PARAM_TOL)

    # per-group set_lr, and sync as a no-op when nothing changed
    two = FusedSGD([{"params": a[:1]}, {"params": a[1:]}], lr=0.5,
                   capturable=True)
    two.set_lr(0.25, group=1)
    assert [g["lr"] for g in two.param_groups] == [0.5, 0.25]
    block = two._scalars.clone()
    two.sync_hyperparams()
    assert torch.equal(two._scalars, block)
    assert two._scalars[ops.SCALAR_LR0 + 1].item() == 0.25


def test_torch_scheduler_drives_param_groups():
    a, b = make_params(), make_params()
    mine = FusedAdam(a, lr=1e-2, capturable=True)
    ref = torch.optim.Adam(b, lr=1e-2)
    sched_a = torch.optim.lr_scheduler.StepLR(mine, step_size=2, gamma=0.1)
    sched_b = torch.optim.lr_scheduler.StepLR(ref, step_size=2, gamma=0.1)
    for step in range(5):
        grads = make_grads(step)
        set_grads(a, grads)
        set_grads(b, grads)
        mine.sync_hyperparams()
        mine.step()
        ref.step()
        sched_a.step()
        sched_b.step()
    assert mine.param_groups[0]["lr"] == pytest.approx(1e-4)
    for x, y in zip(a, b):
        torch.testing.assert_close(x.data, y.data, **PARAM_TOL)


def test_state_dict_round_trips_the_step_in_place():
    a = make_params()
    mine = FusedAdam(a, lr=1e-3, capturable=True)
    for step in range(3):
        set_grads(a, make_grads(step))
        mine.step()
    sd = copy.deepcopy(mine.state_dict())
    assert sd["swq_step_count"] == 3

    b = make_params(seed=5)
    other = FusedAdam(b, lr=1e-3, capturable=True)
    set_grads(b, make_grads(0))
    other.step()
    block_ptr = other._scalars.data_ptr()
    avg_ptr = other.state[b[0]]["exp_avg"].data_ptr()
    other.load_state_dict(sd)
    assert other._scalars.data_ptr() == block_ptr
    assert other.state[b[0]]["exp_avg"].data_ptr() == avg_ptr
    assert other._device_step() == 3
    assert other.state_dict()["swq_step_count"] == 3

    # the resumed optimizer continues exactly like the original
    with torch.no_grad():
        for x, y in zip(b, a):
            x.copy_(y)
    grads = make_grads(7)
    set_grads(a, grads)
    set_grads(b, grads)
    mine.step()
    other.step()
    for x, y in zip(a, b):
        assert torch.equal(x.data, y.data)


def test_reset_zeroes_the_device_step():
    a = make_params()
    mine = FusedSGD(a, lr=0.1, momentum=0.9, dampening=0.5, capturable=True)
    for step in range(2):
        set_grads(a, make_grads(step))
        mine.step()
    assert mine._device_step() == 2
    reset_optimizer_state_inplace(mine)
    assert mine._device_step() == 0

    # next step is step 1 of a fresh optimizer (buf = d_p, no dampening)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    fresh = torch.optim.SGD(b, lr=0.1, momentum=0.9, dampening=0.5)
    grads = make_grads(9)
    set_grads(a, grads)
    set_grads(b, grads)
    mine.step()
    fresh.step()
    for x, y in zip(a, b):
        torch.testing.assert_close(x.data, y.data, **PARAM_TOL)


@pytest.mark.parametrize("source", ["torch", "fused_by_value"])
def test_foreign_adam_checkpoint_loads(source):
    b = make_params()
    if source == "torch":
        src = torch.optim.Adam(b, lr=1e-3)
    else:
        src = FusedAdam(b, lr=1e-3)
    for step in range(4):
        set_grads(b, make_grads(step))
        src.step()
    sd = copy.deepcopy(src.state_dict())

    a = [torch.nn.Parameter(p.detach().clone()) for p in b]
    mine = FusedAdam(a, lr=1e-3, capturable=True)
    mine.load_state_dict(sd)
    assert mine._device_step() == 4
    grads = make_grads(4)
    set_grads(a, grads)
    set_grads(b, grads)
    mine.step()
    src.step()
    for x, y in zip(a, b):
        torch.testing.assert_close(x.data, y.data, **PARAM_TOL)


def test_sgd_checkpoint_without_step_resumes_past_first_step():
    b = make_params()
    src = FusedSGD(b, lr=0.1, momentum=0.9, dampening=0.5)
    for step in range(2):
        set_grads(b, make_grads(step))
        src.step()
    sd = copy.deepcopy(src.state_dict())
    a = [torch.nn.Parameter(p.detach().clone()) for p in b]
    mine = FusedSGD(a, lr=0.1, momentum=0.9, dampening=0.5, capturable=True)
    mine.load_state_dict(sd)
    grads = make_grads(2)
    set_grads(a, grads)
    set_grads(b, grads)
    mine.step()
    src.step()
    for x, y in zip(a, b):
        torch.testing.assert_close(x.data, y.data, **PARAM_TOL)


def test_gpu_tensors_without_extension_raise(monkeypatch):
    monkeypatch.setattr(ops, "HAVE_EXT", False)

    class FakeCuda:
        is_cuda = True

    t = [FakeCuda()]
    with pytest.raises(RuntimeError):
        ops.multi_tensor_sumsq_partials(t, None)
    with pytest.raises(RuntimeError):
        ops.optim_prologue(None, 0, FakeCuda())
    with pytest.raises(RuntimeError):
        ops.fused_sgd_cap(t, t, t, None)
    with pytest.raises(RuntimeError):
        ops.fused_adam_cap(t, t, t, t, None)


# ---------------------------------------------------------------------------
# layout constants: the Python copy against csrc/swq_layout.h
# ---------------------------------------------------------------------------

LAYOUT_CONSTANTS = ["CHUNK_ELEMS", "SCALAR_GRAD_NORM", "SCALAR_CLIP_COEF",
                    "SCALAR_STEP", "SCALAR_LR0"]


def test_layout_constants_match_the_extension():
    if not ops.HAVE_EXT:
        pytest.skip("extension not built")
    for name in LAYOUT_CONSTANTS:
        assert getattr(ops._C, name) == getattr(ops, name), name


@pytest.mark.parametrize("name", LAYOUT_CONSTANTS)
def test_layout_check_raises_on_mismatch(monkeypatch, name):
    ext = types.SimpleNamespace(
        **{n: getattr(ops, n) for n in LAYOUT_CONSTANTS}
    )
    ops._check_layout(ext)  # agreement passes
    monkeypatch.setattr(ext, name, getattr(ops, name) + 1)
    with pytest.raises(RuntimeError, match=name):
        ops._check_layout(ext)
    # the Python side drifting is caught the same way
    monkeypatch.undo()
    monkeypatch.setattr(ops, name, getattr(ops, name) + 1)
    with pytest.raises(RuntimeError, match=name):
        ops._check_layout(ext)


# ---------------------------------------------------------------------------
# loop wiring
# ---------------------------------------------------------------------------

def _stub_opt(lr, capturable=None):
    opt = types.SimpleNamespace(param_groups=[{"lr": lr}])
    if capturable is not None:
        opt.capturable = capturable
    return opt


def test_graph_reuse_rule():
    from shockwave_amd.workloads.loop import can_reuse_graph

    sess = types.SimpleNamespace(graphed=object(), capture_lr=0.1)
    # today's rule for by-value optimizers
    assert can_reuse_graph(sess, _stub_opt(0.1))
    assert not can_reuse_graph(sess, _stub_opt(0.05))
    assert not can_reuse_graph(sess, _stub_opt(0.05, capturable=False))
    # device-side lr: reuse across LR changes
    assert can_reuse_graph(sess, _stub_opt(0.05, capturable=True))
    # nothing captured yet
    empty = types.SimpleNamespace(graphed=None, capture_lr=None)
    assert not can_reuse_graph(empty, _stub_opt(0.1, capturable=True))


def test_warmup_schedule_formula():
    from shockwave_amd.workloads.families import transformer_warmup_lr

    d_model, warm = 512, 8
    for n in [1, 2, 7, 8, 9, 100]:
        want = (1.0 / d_model ** 0.5) * min(1.0 / n ** 0.5, n / warm ** 1.5)
        assert transformer_warmup_lr(d_model, warm, n) == pytest.approx(
            want, rel=1e-12
        )
    # rises during warm-up, peaks at n == N, decays afterwards
    lrs = [transformer_warmup_lr(d_model, warm, n) for n in range(1, 20)]
    assert max(lrs) == lrs[warm - 1]
    assert lrs[0] < lrs[1] and lrs[-1] < lrs[warm - 1]


@pytest.fixture
def workload_env(monkeypatch):
    from shockwave_amd.workloads import session

    monkeypatch.setenv("SWQ_SESSION_CACHE", "0")
    session.clear()
    yield
    session.clear()


def test_lm_main_apply_clip(workload_env):
    from shockwave_amd.workloads.families import lm_main

    assert lm_main(["--batch_size", "4", "--apply_clip"],
                   max_steps_override=4) == 4


def test_translation_main_warmup(workload_env):
    from shockwave_amd.workloads.families import translation_main

    assert translation_main(
        ["-batch_size", "2", "-n_warmup_steps", "8"], max_steps_override=4
    ) == 4
