"""LeaseIterator: behaviour transcript against a recorded golden, plus the
state-machine tests that used to live in test_rpc_runtime.py.

The transcript runner drives the iterator only through its stable surface
(constructor, iter/next/len, the public properties and methods, an
injected scripted client, the round log file, the GAVEL_* variables) under
a scripted clock, so every scenario runs in milliseconds and its result is
exact.  ``python tests/test_lease_iterator.py --record`` rewrites the
golden; under pytest each scenario must equal it exactly.
"""

import contextlib
import gc
import json
import os
import sys
import tempfile
import weakref

import pytest
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from shockwave_amd.runtime import lease_iterator  # noqa: E402
from shockwave_amd.runtime.lease_iterator import (  # noqa: E402
    LeaseIterator,
    NullLeaseClient,
)

GOLDEN = os.path.join(
    os.path.dirname(os.path.abspath(__file__)),
    "golden", "lease_iterator", "transcripts.json",
)


class FakeLeaseClient:
    """Scripted lease behavior for iterator state-machine tests."""

    def __init__(self, leases):
        self.leases = list(leases)  # [(max_steps, max_duration)]
        self.init_calls = 0
        self.update_calls = 0
        self.rr_calls = []

    def init(self):
        self.init_calls += 1
        ms, md = self.leases.pop(0)
        return ms, md, 0

    def update_lease(self, steps, duration, max_steps, max_duration):
        self.update_calls += 1
        if self.leases:
            ms, md = self.leases.pop(0)
        else:
            ms, md = max_steps, max_duration
        return ms, md, 0, 1e9

    def update_resource_requirement(self, big, small):
        self.rr_calls.append((big, small))


# -- transcript runner --------------------------------------------------------


class ScriptedClock:
    """Stands in for the ``time`` module as the iterator module sees it."""

    def __init__(self):
        self.now = 0.0

    def time(self):
        return self.now

    def advance(self, seconds):
        self.now += seconds


class ScriptedClient:
    """Replays scripted grants and records every call with its arguments."""

    def __init__(self, init, updates=()):
        self.init_reply = init
        self.updates = list(updates)
        self.calls = []

    def init(self):
        self.calls.append(["init"])
        return self.init_reply

    def update_lease(self, steps, duration, max_steps, max_duration):
        self.calls.append(
            ["update_lease", steps, round(duration, 6), max_steps,
             round(max_duration, 6)]
        )
        if self.updates:
            return self.updates.pop(0)
        return max_steps, max_duration, 0, 1e9  # lease unchanged

    def update_resource_requirement(self, big_bs, small_bs):
        self.calls.append(["update_resource_requirement", big_bs, small_bs])


class Rig:
    """One scenario's world: scripted clock, counting barrier stubs, a clean
    GAVEL_* environment, a private checkpoint directory, and the transcript
    that the scenario fills in."""

    def __init__(self, root, env=None, distributed=False):
        self.root = root
        self.env = env or {}
        self.distributed = distributed
        self.clock = ScriptedClock()
        self.barriers = 0
        self.out = {"epochs": []}
        self._dirs = 0

    @contextlib.contextmanager
    def installed(self):
        dist = lease_iterator.torch.distributed
        saved_env = {k: v for k, v in os.environ.items()
                     if k.startswith("GAVEL_")}
        saved = (lease_iterator.time, dist.is_initialized, dist.barrier)

        def barrier(*args, **kwargs):
            self.barriers += 1

        for k in saved_env:
            del os.environ[k]
        os.environ.update(self.env)
        lease_iterator.time = self.clock
        dist.is_initialized = lambda: self.distributed
        dist.barrier = barrier
        try:
            yield self
        finally:
            lease_iterator.time, dist.is_initialized, dist.barrier = saved
            for k in self.env:
                os.environ.pop(k, None)
            os.environ.update(saved_env)

    def checkpoint_dir(self):
        self._dirs += 1
        return os.path.join(self.root, f"ckpt{self._dirs}")

    def make(self, loader, client, ckpt=None, **kwargs):
        return LeaseIterator(
            loader, ckpt or self.checkpoint_dir(),
            kwargs.pop("load", lambda: None), kwargs.pop("save", lambda: None),
            client=client, **kwargs,
        )

    def drive(self, it, dt, max_epochs=40, startup=0.0):
        """Consume epochs until ``done``; one simulated step takes ``dt``."""
        self.clock.advance(startup)
        seen = set()
        for _ in range(max_epochs):
            yielded = 0
            for batch in it:
                seen.add(id(batch))
                yielded += 1
                self.clock.advance(dt)
            self.out["epochs"].append({
                "yielded_before_stop": yielded,
                "steps": it.steps,
                "duration": round(it.duration, 6),
                "done": it.done,
                "barriers": self.barriers,
            })
            if it.done:
                break
        self.out["distinct_batches"] = len(seen)

    def log_lines(self, ckpt):
        """{relative log path: lines from ``[EVENT]`` on}."""
        logs = {}
        for base, _, files in sorted(os.walk(os.path.join(ckpt, ".gavel"))):
            for name in sorted(files):
                path = os.path.join(base, name)
                with open(path) as f:
                    logs[os.path.relpath(path, ckpt)] = [
                        line.rstrip("\n").split("] ", 1)[1] for line in f
                    ]
        return logs

    def finish(self, it, client, ckpt):
        if it is not None:
            it.close()
        self.out["client_calls"] = getattr(client, "calls", None)
        self.out["barriers"] = self.barriers
        self.out["log"] = self.log_lines(ckpt)
        return self.out


def items(n):
    return [(i,) for i in range(n)]


def _lease_run(rig, init, updates=(), n=100, dt=0.5, **kwargs):
    startup = kwargs.pop("startup", 0.0)
    client = ScriptedClient(init, updates)
    ckpt = rig.checkpoint_dir()
    it = rig.make(items(n), client, ckpt=ckpt, **kwargs)
    rig.out["len"] = len(it)
    rig.drive(it, dt, startup=startup)
    return rig.finish(it, client, ckpt)


def a_step_lease_one_renewal(rig):
    return _lease_run(rig, (8, 1e9, 0), [(16, 1e9, 0, 1e9)])


def b_time_lease_with_extra_time(rig):
    return _lease_run(rig, (1e9, 10.0, 2.0), n=5, dt=1.0)


def c_time_renewal_against_stored_sum(rig):
    return _lease_run(rig, (1e9, 10.0, 2.0), [(1e9, 20.0, 0, 1e9)],
                      n=200, dt=0.1)


def c3_time_renewal_over_short_epochs(rig):
    # as c, but epochs end before the renewal: their PROGRESS lines carry the
    # accumulated float duration, and each epoch-ending call is left uncharged
    return _lease_run(rig, (1e9, 10.0, 2.0), [(1e9, 20.0, 0, 1e9)],
                      n=60, dt=0.1)


def c2_time_grant_below_stored_sum(rig):
    # 11.0 s is more than the 10.0 s granted but less than the stored
    # 10.0 + 2.0, so it counts as "not extended" and then shortens the lease
    return _lease_run(rig, (1e9, 10.0, 2.0), [(1e9, 11.0, 0, 1e9)],
                      n=250, dt=0.1)


def d_synthetic(rig):
    return _lease_run(rig, (12, 1e9, 0), [(24, 1e9, 0, 1e9)], n=4,
                      synthetic_data=True)


def e_init_over_deadline(rig):
    return _lease_run(rig, (100, 50.0, 0, 500.0, 100.0),
                      write_on_close=False)


def f_deadline_at_renewal(rig):
    return _lease_run(rig, (4, 1e9, 0), [(1000, 1e9, 1e6, 100)],
                      write_on_close=False)


def g_legacy_init_then_unchanged_lease(rig):
    return _lease_run(rig, (6, 1e9, 0), startup=0.25)


def h_null_client_three_epochs(rig):
    ckpt = rig.checkpoint_dir()
    client = NullLeaseClient()
    it = rig.make(items(30), client, ckpt=ckpt, write_on_close=False)
    rig.drive(it, 0.5, max_epochs=3)
    return rig.finish(it, client, ckpt)


def h2_no_client_no_scheduler_env(rig):
    ckpt = rig.checkpoint_dir()
    it = rig.make(items(7), None, ckpt=ckpt)
    rig.drive(it, 0.5, max_epochs=2)
    return rig.finish(it, None, ckpt)


def i_distributed_expiry(rig):
    return _lease_run(rig, (5, 1e9, 0), n=3)


def i_distributed_deadline(rig):
    return f_deadline_at_renewal(rig)


def i_distributed_rescale(rig):
    client = ScriptedClient((100, 1e9, 0))
    ckpt = rig.checkpoint_dir()
    it = rig.make(items(10), client, ckpt=ckpt)
    it.update_resource_requirement(True, False)
    rig.out["done_after_rescale"] = it.done
    return rig.finish(it, client, ckpt)


def _close_run(rig, write_on_close):
    client = ScriptedClient((100, 1e9, 0))
    ckpt = rig.checkpoint_dir()
    it = rig.make(items(10), client, ckpt=ckpt, write_on_close=write_on_close)
    for _ in zip(range(3), it):
        rig.clock.advance(0.5)
    it.complete()
    rig.out["done_after_complete"] = it.done
    it.write_progress()
    # an atexit hook is a bound method, so it keeps its instance alive:
    # the instance can be collected exactly when no hook of it remains
    alive = weakref.ref(it)
    it.close()
    try:
        it.close()
        rig.out["second_close"] = "no-op"
    except Exception as e:  # recorded, whichever it is
        rig.out["second_close"] = type(e).__name__
    del it
    gc.collect()
    rig.out["instance_released_after_close"] = alive() is None

    # ... and an instance that was never closed is held until exit
    unclosed = rig.make(items(1), ScriptedClient((1, 1e9, 0)),
                        write_on_close=write_on_close)
    alive = weakref.ref(unclosed)
    del unclosed
    gc.collect()
    rig.out["unclosed_instance_held_for_exit"] = alive() is not None
    if alive() is not None:
        alive().close()
    return rig.finish(None, client, ckpt)


def j_write_on_close_true(rig):
    return _close_run(rig, True)


def j_write_on_close_false(rig):
    return _close_run(rig, False)


def k_checkpoint_hooks(rig):
    seen = []

    def load(*args, **kwargs):
        seen.append(["load", list(args), kwargs])
        return "loaded"

    def save(*args, **kwargs):
        seen.append(["save", list(args), kwargs])
        return "saved"

    client = ScriptedClient((100, 1e9, 0))
    ckpt = rig.checkpoint_dir()
    it = rig.make(items(10), client, ckpt=ckpt, load=load, save=save)
    rig.out["load_returned"] = it.load_checkpoint("model.chkpt", strict=True)
    rig.out["save_returned"] = it.save_checkpoint({"epoch": 1}, "model.chkpt")
    rig.out["hook_calls"] = seen
    return rig.finish(it, client, ckpt)


def l_stale_handler_of_same_job_round(rig):
    """A second lease of the same (job, worker, round) in one process must
    not write into the first one's file, closed or not."""
    first_dir, second_dir = rig.checkpoint_dir(), rig.checkpoint_dir()
    first = rig.make(items(3), ScriptedClient((100, 1e9, 0)), ckpt=first_dir)
    client = ScriptedClient((2, 1e9, 0))
    second = rig.make(items(3), client, ckpt=second_dir)
    rig.drive(second, 0.5)
    first.close()
    out = rig.finish(second, client, second_dir)
    out["first_log"] = rig.log_lines(first_dir)
    return out


def m_rejects_non_iterable(rig):
    try:
        rig.make(42, ScriptedClient((1, 1, 0)))
        rig.out["raised"] = None
    except Exception as e:
        rig.out["raised"] = type(e).__name__
    return rig.out


SCENARIOS = {
    f.__name__: (f, env, distributed)
    for f, env, distributed in [
        (a_step_lease_one_renewal,
         {"GAVEL_JOB_ID": "7", "GAVEL_WORKER_ID": "1", "GAVEL_ROUND_ID": "3"},
         False),
        (b_time_lease_with_extra_time, None, False),
        (c_time_renewal_against_stored_sum, None, False),
        (c2_time_grant_below_stored_sum, None, False),
        (c3_time_renewal_over_short_epochs, None, False),
        (d_synthetic, None, False),
        (e_init_over_deadline, None, False),
        (f_deadline_at_renewal, None, False),
        (g_legacy_init_then_unchanged_lease, None, False),
        (h_null_client_three_epochs, None, False),
        (h2_no_client_no_scheduler_env, None, False),
        (i_distributed_expiry, None, True),
        (i_distributed_deadline, None, True),
        (i_distributed_rescale, None, True),
        (j_write_on_close_true, None, False),
        (j_write_on_close_false, None, False),
        (k_checkpoint_hooks, None, False),
        (l_stale_handler_of_same_job_round, {"GAVEL_JOB_ID": "9"}, False),
        (m_rejects_non_iterable, None, False),
    ]
}


def run_scenario(name):
    scenario, env, distributed = SCENARIOS[name]
    with tempfile.TemporaryDirectory() as root:
        with Rig(root, env, distributed).installed() as rig:
            # through JSON, so that it compares like the recorded golden
            return json.loads(json.dumps(scenario(rig)))


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_scenario():
    assert sorted(load_golden()) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_transcript_matches_golden(name):
    assert run_scenario(name) == load_golden()[name]


# -- the lease meter on its own: no filesystem, no clock, no torch ------------


class TestLeaseMeter:
    def test_first_grant_budgets_75pct_of_it(self):
        m = lease_iterator.LeaseMeter()
        m.grant(8, 100.0)
        assert (m.max_steps, m.max_duration) == (8, 100.0)
        assert (m.step_budget, m.time_budget) == (6.0, 75.0)

    def test_extension_budgets_the_rest_plus_75pct_of_what_it_adds(self):
        m = lease_iterator.LeaseMeter()
        m.grant(8, 100.0)
        m.steps, m.duration = 6, 60.0
        m.grant(16, 200.0)
        assert (m.step_budget, m.time_budget) == (2 + 6.0, 40.0 + 75.0)

    def test_unchanged_grant_is_final(self):
        m = lease_iterator.LeaseMeter()
        m.grant(6, 50.0)
        m.grant(6, 50.0)
        assert m.step_budget == m.time_budget == lease_iterator.INFINITY

    def test_extra_time_is_folded_in_and_the_next_grant_compared_with_the_sum(self):
        m = lease_iterator.LeaseMeter()
        m.grant(1e9, 10.0, 2.0)
        assert m.max_duration == 12.0 and m.time_budget == 7.5 + 2.0
        m.grant(1e9, 11.0)  # below 10 + 2: not an extension, yet it is stored
        assert m.time_budget == lease_iterator.INFINITY
        assert m.max_duration == 11.0


# -- state-machine tests ------------------------------------------------------


class TestLeaseIterator:
    def _data(self, n=100):
        return [(torch.zeros(1), torch.zeros(1)) for _ in range(n)]

    def test_expires_at_max_steps(self, tmp_path):
        client = FakeLeaseClient([(5, 1e9)])
        it = LeaseIterator(
            self._data(), str(tmp_path), lambda: None, lambda s: None,
            client=client, write_on_close=False,
        )
        consumed = list(it)
        assert len(consumed) == 5
        assert it.done

    def test_renews_at_75pct(self, tmp_path):
        client = FakeLeaseClient([(8, 1e9), (16, 1e9)])
        it = LeaseIterator(
            self._data(), str(tmp_path), lambda: None, lambda s: None,
            client=client, write_on_close=False,
        )
        consumed = list(it)
        # renewal granted at 75% of 8 steps -> extended to 16 total
        assert client.update_calls >= 1
        assert len(consumed) == 16
        assert it.done

    def test_infinite_lease_runs_all_data(self, tmp_path):
        it = LeaseIterator(
            self._data(30), str(tmp_path), lambda: None, lambda s: None,
            client=NullLeaseClient(), write_on_close=False,
        )
        assert len(list(it)) == 30
        assert not it.done

    def test_update_resource_requirement_sets_done(self, tmp_path):
        client = FakeLeaseClient([(100, 1e9)])
        it = LeaseIterator(
            self._data(), str(tmp_path), lambda: None, lambda s: None,
            client=client, write_on_close=False,
        )
        it.update_resource_requirement(True, False)
        assert it.done
        assert client.rr_calls == [(True, False)]

    def test_deadline_abort(self, tmp_path):
        class DeadlineClient(FakeLeaseClient):
            def update_lease(self, steps, duration, max_steps, max_duration):
                self.update_calls += 1
                return 1000, 1e9, 1e6, 100  # run_time >> deadline

        client = DeadlineClient([(4, 1e9)])
        it = LeaseIterator(
            self._data(), str(tmp_path), lambda: None, lambda s: None,
            client=client, write_on_close=False,
        )
        consumed = list(it)
        assert it.done  # completed via deadline mechanism
        assert len(consumed) < 1000

    def test_log_format_scrapeable(self, tmp_path):
        os.environ["GAVEL_ROUND_ID"] = "3"
        os.environ["GAVEL_WORKER_ID"] = "1"
        try:
            client = FakeLeaseClient([(5, 1e9)])
            it = LeaseIterator(
                self._data(), str(tmp_path), lambda: None, lambda s: None,
                client=client, write_on_close=False,
            )
            list(it)
            it.write_progress()
            from shockwave_amd.runtime.dispatcher import LOG_LINE_RE

            log_file = tmp_path / ".gavel" / "round=3" / "worker=1.log"
            steps = None
            for line in open(log_file):
                m = LOG_LINE_RE.match(line)
                if m and m.group("event") == "PROGRESS" and m.group("status") == "STEPS":
                    steps = int(float(m.group("msg")))
            assert steps == 5
        finally:
            del os.environ["GAVEL_ROUND_ID"]
            del os.environ["GAVEL_WORKER_ID"]

    def test_max_steps_and_max_duration_are_public(self, tmp_path):
        it = LeaseIterator(
            self._data(), str(tmp_path), lambda: None, lambda s: None,
            client=FakeLeaseClient([(5, 123.0)]), write_on_close=False,
        )
        assert (it.max_steps, it.max_duration) == (5, 123.0)
        it.close()


def record():
    result = {name: run_scenario(name) for name in sorted(SCENARIOS)}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(result)} scenarios to {GOLDEN}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_lease_iterator.py --record")
    record()
