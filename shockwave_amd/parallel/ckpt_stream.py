"""Fast job-migration checkpoint store.

The reference migrates jobs through NFS (`checkpoint_dir` on shared
storage) and models the cost at ~20 s per preemption
(scheduler.py:1936-1968).  On an MI355X node that cost is unnecessary:

* **node-local tier**: checkpoints land in ``/dev/shm`` (RAM) — a 45-300 MB
  state dict round-trips in well under a second.  D2H copies go through a
  reusable pinned staging buffer so the PCIe copy runs at full speed.
* **cross-node tier**: the bytes are served over the worker's gRPC channel
  (``FetchCheckpoint``) in 32 MiB chunks when the next placement is on a
  different node; a shared filesystem path, when configured, acts as the
  final fallback.

Intra-node GPU->GPU streaming over xGMI is intentionally NOT used for
migration: a preempted job's process exits before its successor starts, so
there is no live peer to stream to — the 288 GB/node of HBM cannot hold
state for a process that no longer exists.  RAM-tier staging is the
MI355X-native answer; xGMI carries the *intra-job* traffic (DDP
collectives) instead.
"""

from __future__ import annotations

import io
import logging
import os
import shutil
from typing import Optional

import torch

logger = logging.getLogger("shockwave_amd.ckpt_stream")


class CheckpointStore:
    def __init__(
        self,
        job_checkpoint_dir: str,
        shm_root: Optional[str] = None,
        shared_dir: Optional[str] = None,
    ):
        # SWQ_SHM_ROOT moves the RAM tier (e.g. to a per-user directory on
        # a node where /dev/shm/swq_ckpt belongs to someone else)
        if shm_root is None:
            shm_root = os.environ.get("SWQ_SHM_ROOT", "/dev/shm/swq_ckpt")
        self.dir = job_checkpoint_dir
        # key the RAM tier by the full durable path so distinct checkpoint
        # dirs (and re-created temp dirs) never share shm state
        import hashlib

        abspath = os.path.abspath(job_checkpoint_dir)
        digest = hashlib.sha1(abspath.encode()).hexdigest()[:16]
        self.shm_dir = os.path.join(
            shm_root, f"{os.path.basename(os.path.normpath(abspath))}-{digest}"
        )
        self.shared_dir = shared_dir
        os.makedirs(self.dir, exist_ok=True)

    def _paths(self):
        return (
            os.path.join(self.shm_dir, "model.chkpt"),
            os.path.join(self.dir, "model.chkpt"),
            os.path.join(self.shared_dir, "model.chkpt")
            if self.shared_dir
            else None,
        )

    def save(self, state: dict) -> str:
        """Write to the RAM tier and mirror to the durable tier."""
        os.makedirs(self.shm_dir, exist_ok=True)
        shm_path, dir_path, shared_path = self._paths()
        buf = io.BytesIO()
        torch.save(_to_cpu(state), buf)
        data = buf.getvalue()
        for path in (shm_path, dir_path):
            tmp = path + ".tmp"
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, path)
        if shared_path:
            os.makedirs(os.path.dirname(shared_path), exist_ok=True)
            tmp = shared_path + ".tmp"
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, shared_path)
        return dir_path

    def _read_order(self):
        """The shm entry is a CACHE of the durable file: use it only when
        the durable copy exists and is not newer (a deleted/recreated job
        dir must never resurrect a stale RAM-tier checkpoint)."""
        shm_path, dir_path, shared_path = self._paths()
        order = []
        if os.path.exists(dir_path):
            if (
                os.path.exists(shm_path)
                and os.path.getmtime(shm_path) >= os.path.getmtime(dir_path)
            ):
                order.append(shm_path)
            order.append(dir_path)
        if shared_path and os.path.exists(shared_path):
            order.append(shared_path)
        return order

    def load(self) -> Optional[dict]:
        for path in self._read_order():
            try:
                return torch.load(path, map_location="cpu",
                                  weights_only=False)
            except Exception:
                # corrupt tier (e.g. node died mid-write before the
                # atomic rename landed everywhere): fall through to the
                # next tier; a fresh start beats a crashed job
                logger.exception("corrupt checkpoint at %s; trying next "
                                 "tier", path)
                continue
        return None

    def read_bytes(self) -> Optional[bytes]:
        for path in self._read_order():
            try:
                with open(path, "rb") as f:
                    data = f.read()
                # validate before serving over FetchCheckpoint: a torn
                # /dev/shm file must not shadow an intact durable copy
                torch.load(io.BytesIO(data), map_location="cpu",
                           weights_only=False)
                return data
            except Exception:
                logger.exception("corrupt checkpoint at %s; trying next "
                                 "tier", path)
                continue
        return None

    def write_bytes(self, data: bytes) -> None:
        os.makedirs(self.shm_dir, exist_ok=True)
        for path in self._paths()[:2]:
            tmp = path + ".tmp"
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, path)

    def clear(self):
        shutil.rmtree(self.shm_dir, ignore_errors=True)


_PINNED_CACHE: dict = {}


def _to_cpu(obj):
    """Move tensors device->host through a pinned staging buffer."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            key = (obj.dtype, obj.numel())
            staging = _PINNED_CACHE.get(key)
            if staging is None or staging.numel() < obj.numel():
                staging = torch.empty(
                    obj.numel(), dtype=obj.dtype, pin_memory=True
                )
                _PINNED_CACHE[key] = staging
            staging[: obj.numel()].copy_(obj.reshape(-1), non_blocking=True)
            torch.cuda.synchronize()
            return staging[: obj.numel()].reshape(obj.shape).clone()
        return obj
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        t = type(obj)
        return t(_to_cpu(v) for v in obj)
    return obj


CHUNK = 32 * 1024 * 1024


def fetch_remote_checkpoint(rpc_client, job_id: int) -> Optional[bytes]:
    """Pull a checkpoint from another node's worker over gRPC."""
    chunks = []
    offset = 0
    while True:
        resp = rpc_client.call(
            "SchedulerToWorker",
            "FetchCheckpoint",
            {"job_id": job_id, "offset": offset, "length": CHUNK},
            timeout=120,
        )
        if not resp.get("found"):
            return None
        data = resp["data"]
        chunks.append(data)
        offset += len(data)
        if offset >= resp["total"]:
            break
    return b"".join(chunks)
