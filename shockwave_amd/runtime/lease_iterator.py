"""LeaseIterator — the lease-preemptible training iterator.

Wraps any iterable data loader so that the scheduler can preempt the loop.
Behaviour, protocol and log match the reference's GavelIterator
(scheduler/gavel_iterator.py:32-361).  Three parts:

* ``LeaseMeter`` — pure bookkeeping: progress, the granted lease, and when
  to ask for the next one (at 75% of each extension);
* ``RoundLog`` — the ``[time] [EVENT] [STATUS] msg`` file that the dispatcher
  scrapes for (steps, duration): ``checkpoint_dir/.gavel/round=R/worker=W.log``;
* ``LeaseIterator`` — the glue.  It takes a lease on construction and
  renews it when the meter says so.  On expiry it sets ``done``, barriers
  all ranks of a distributed job and raises StopIteration: the cooperative
  preemption point.  Once the projected run time exceeds the deadline it
  completes the job by itself.  ``update_resource_requirement`` reports an
  Accordion/GNS batch-size change and triggers checkpoint + restart.

Environment contract (the reference's names): GAVEL_JOB_ID, GAVEL_WORKER_ID,
GAVEL_ROUND_ID, GAVEL_SCHED_ADDR, GAVEL_SCHED_PORT.  The scheduler client is
injected (``client=``) or built from these; with neither, ``NullLeaseClient``
grants an infinite lease for standalone runs.
"""

import atexit
import collections.abc
import logging
import os
import time
import torch
from filelock import FileLock

INFINITY = 1e9
LEASE_UPDATE_FRACTION = 0.75
LOG_FORMAT = "[{asctime}] [{event}] [{status}] {message}"
DATE_FORMAT = "%Y-%m-%d %H:%M:%S"


class NullLeaseClient:
    """Infinite lease; used for standalone runs and unit tests."""

    def init(self):
        return INFINITY, INFINITY, 0, 0, INFINITY

    def update_lease(self, steps, duration, max_steps, max_duration):
        return INFINITY, INFINITY, 0, INFINITY

    def update_resource_requirement(self, big_bs, small_bs):
        pass


class LeaseMeter:
    """Progress against the current lease, and when to renew it: plain state
    and the grant arithmetic, no I/O.  ``LeaseIterator.__next__`` is its one
    writer, and does its per-step arithmetic in line to keep a step cheap.

    ``steps`` / ``duration`` count every step and all wall time; the lease is
    spent when either reaches the granted ``max_steps`` / ``max_duration``.
    Each grant also sets two renewal budgets, in steps and in seconds: what is
    left of the old lease plus 75% of what the grant adds.  A grant that adds
    nothing is final and disables that budget.  Every yielded batch is charged
    to both budgets, and renewal is due once either is used up.

    Two oddities are the reference's (gavel_iterator.py:112-171, :293-354)
    and are kept, since changing either changes when jobs renew and stop:

    * Only yielded batches are charged.  The call that ends an epoch adds
      its wall time to ``duration`` (and, with synthetic data, its step to
      ``steps``) but charges nothing, so renewal comes later than 75% by
      that much per epoch, and a lease that is short against the epoch
      length can expire without ever asking for renewal.
    * ``max_duration`` is stored with the grant's ``extra_time`` added, and
      the next grant is compared with that sum: a duration between the two
      counts as "adds nothing", yet still replaces the stored value.
    """

    __slots__ = ("steps", "duration", "max_steps", "max_duration",
                 "step_budget", "time_budget")

    def __init__(self):
        self.steps = 0
        self.duration = 0.0
        self.max_steps = self.max_duration = 0
        self.step_budget = self.time_budget = INFINITY

    def grant(self, max_steps, max_duration, extra_time=0):
        if max_steps == self.max_steps:
            self.step_budget = INFINITY
        else:
            unused = self.max_steps - self.steps
            added = max_steps - self.max_steps
            self.step_budget = unused + added * LEASE_UPDATE_FRACTION
        if max_duration <= self.max_duration:
            self.time_budget = INFINITY
        else:
            unused = self.max_duration - self.duration
            added = max_duration - self.max_duration
            self.time_budget = unused + added * LEASE_UPDATE_FRACTION + extra_time
        self.max_steps = max_steps
        self.max_duration = max_duration + extra_time


class RoundLog:
    """The per-(job, worker, round) event file that the dispatcher scrapes."""

    def __init__(self, checkpoint_dir, job_id, worker_id, round_id):
        round_dir = os.path.join(checkpoint_dir, ".gavel", f"round={round_id}")
        os.makedirs(checkpoint_dir, exist_ok=True)
        with FileLock(os.path.join(checkpoint_dir, ".gavel.lock")):
            os.makedirs(round_dir, exist_ok=True)
        filelock_chatter = logging.getLogger("filelock")
        filelock_chatter.setLevel(logging.CRITICAL)
        # a warm runner that takes this lease again must drop the stale handler
        name = f"lease_iterator.{job_id}.{worker_id}.{round_id}"
        self.logger = logging.getLogger(name)
        self.logger.propagate = False
        self.logger.setLevel(logging.DEBUG)
        for stale in list(self.logger.handlers):
            self.logger.removeHandler(stale)
        self.path = os.path.join(round_dir, f"worker={worker_id}.log")
        self._handler = logging.FileHandler(self.path)
        line = logging.Formatter(fmt=LOG_FORMAT, datefmt=DATE_FORMAT, style="{")
        self._handler.setFormatter(line)
        self.logger.addHandler(self._handler)

    def event(self, event, status, message=""):
        self.logger.info(message, extra={"event": event, "status": status})

    def flush(self):
        self._handler.flush()

    def close(self):
        self.logger.removeHandler(self._handler)
        self._handler.close()


def _grant_fields(reply, first):
    """(max_steps, max_duration, extra_time, run_time, deadline) from what
    ``init()`` (3 values, or all 5) or ``update_lease()`` (4 values) returned.
    Any other length fails to unpack, here or in the caller."""
    if first:
        return reply if len(reply) == 5 else (*reply, 0, 0)
    max_steps, max_duration, run_time, deadline = reply
    return max_steps, max_duration, 0, run_time, deadline


class LeaseIterator:
    def __init__(
        self,
        data_loader,
        checkpoint_dir,
        load_checkpoint_func,
        save_checkpoint_func,
        synthetic_data=False,
        write_on_close=True,
        verbose=True,
        client=None,
    ):
        if not isinstance(data_loader, collections.abc.Iterable):
            raise ValueError(f"data loader of uniterable type {type(data_loader)}")
        self._loader = data_loader
        self._synthetic = synthetic_data
        self._first_batch = None  # synthetic mode replays it for every step
        self._load_hook = load_checkpoint_func
        self._save_hook = save_checkpoint_func
        self._progress_on_close = write_on_close

        job_id = int(os.environ.get("GAVEL_JOB_ID", -1))
        worker_id = int(os.environ.get("GAVEL_WORKER_ID", 0))
        round_id = int(os.environ.get("GAVEL_ROUND_ID", 0))
        sched_addr = os.environ.get("GAVEL_SCHED_ADDR")
        self._log = RoundLog(checkpoint_dir, job_id, worker_id, round_id)
        if client is None and job_id >= 0 and sched_addr:
            from ..rpc.iterator_client import IteratorRpcClient
            client = IteratorRpcClient(
                job_id, worker_id, sched_addr,
                int(os.environ.get("GAVEL_SCHED_PORT", 0)), self._log.logger,
            )
        self._client = NullLeaseClient() if client is None else client
        # crash insurance; close() takes it back
        atexit.register(self._at_exit)

        self._done = False
        self._meter = LeaseMeter()
        self._renew(first=True)
        self._log_progress()
        # the clock runs from construction, so that slow storage reads before
        # the first step count against the lease (gavel_iterator.py:96-106)
        self._last_call = time.time()

    def __iter__(self):
        self._fetch = iter(self._loader).__next__
        return self

    def __len__(self):
        return len(self._loader)

    def __next__(self):
        now = time.time()
        elapsed = now - self._last_call
        self._last_call = now
        m = self._meter
        m.duration += elapsed
        if m.step_budget <= 0 or m.time_budget <= 0:
            self._renew()
        if m.duration >= m.max_duration or m.steps >= m.max_steps:
            self._expire()
        synthetic = self._synthetic
        batch = self._first_batch if synthetic else None
        if batch is None:
            try:
                batch = self._fetch()
            except StopIteration:
                self._log_progress()
                raise
        m.steps += 1
        if synthetic:
            self._first_batch = batch
            if m.steps % len(self._loader) == 0:
                raise StopIteration  # the step counts but is charged to no budget
        m.step_budget -= 1
        m.time_budget -= elapsed
        return batch

    done = property(lambda self: self._done)
    steps = property(lambda self: self._meter.steps)
    duration = property(lambda self: self._meter.duration)
    max_steps = property(lambda self: self._meter.max_steps)
    max_duration = property(lambda self: self._meter.max_duration)

    def write_progress(self):
        """Write a PROGRESS STEPS/DURATION pair, which the dispatcher scrapes."""
        self._log_progress()
        self._log.flush()

    def close(self):
        """Release the log handler and drop the atexit hook: a clean end must
        not leave one per lease piling up inside a long-lived warm runner."""
        atexit.unregister(self._at_exit)
        self._log.close()

    def complete(self, timeout=False):
        self._done = True
        if not self._progress_on_close:
            self._log_progress()
        self._log.event("LEASE", "COMPLETE")

    def update_resource_requirement(self, big_bs, small_bs):
        self._done = True  # checkpoint now; scheduler rescales + restarts
        self._client.update_resource_requirement(big_bs, small_bs)

    def load_checkpoint(self, *args, **kwargs):
        self._log.event("LOAD CHECKPOINT", "BEGIN")
        loaded = self._load_hook(*args, **kwargs)
        self._log.event("LOAD CHECKPOINT", "END")
        return loaded

    def save_checkpoint(self, *args, **kwargs):
        self._log.event("SAVE CHECKPOINT", "BEGIN")
        saved = self._save_hook(*args, **kwargs)
        self._log.event("SAVE CHECKPOINT", "END")
        return saved

    def _log_progress(self):
        self._log.event("PROGRESS", "STEPS", str(self._meter.steps))
        self._log.event("PROGRESS", "DURATION", str(self._meter.duration))

    # private names that code written against the previous version reaches for
    _write_info = _log_progress
    _file_handler = property(lambda self: self._log._handler)

    def _at_exit(self):
        if self._progress_on_close:
            self._log_progress()
        self._log.close()

    def _renew(self, first=False):
        """Take the first lease or ask for the next.  A job over its deadline
        completes itself: at init with an empty lease, later by stopping."""
        m = self._meter
        max_steps, max_duration, extra_time, run_time, deadline = _grant_fields(
            self._client.init() if first else self._client.update_lease(
                m.steps, m.duration, m.max_steps, m.max_duration), first
        )
        if first:
            if deadline and run_time > deadline:
                self._log.event("LEASE", "DEADLINE",
                                "run time already exceeds deadline at init")
                self.complete(True)
                max_steps = max_duration = 0
        elif m.duration + run_time > deadline:
            self._log.event("LEASE", "DEADLINE",
                            "projected run time exceeds deadline")
            self.complete(True)
            raise StopIteration
        m.grant(max_steps, max_duration, extra_time)

    def _expire(self):
        m = self._meter
        self._done = True
        self._log.event("LEASE", "EXPIRED", f"{m.steps} / {m.max_steps} steps, "
                        f"{m.duration:.4f} / {m.max_duration:.4f} seconds")
        dist = torch.distributed
        if dist.is_initialized():
            dist.barrier()
        raise StopIteration


# Alias for drop-in use by reference-style workloads.
GavelIterator = LeaseIterator
