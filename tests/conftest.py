import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: tests that require an MI355X GPU (run via gpurun)"
    )
    config.addinivalue_line("markers", "slow: long-running tests")
    # the checkpoint RAM tier defaults to one fixed directory per node;
    # give the suite (and the workers it spawns) a private one so a run
    # never depends on who created that directory first
    if "SWQ_SHM_ROOT" not in os.environ:
        import tempfile

        base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
        config._swq_shm_root = tempfile.mkdtemp(prefix="swq_ckpt_", dir=base)
        os.environ["SWQ_SHM_ROOT"] = config._swq_shm_root


def pytest_unconfigure(config):
    root = getattr(config, "_swq_shm_root", None)
    if root:
        import shutil

        shutil.rmtree(root, ignore_errors=True)
        os.environ.pop("SWQ_SHM_ROOT", None)


@pytest.fixture(scope="session")
def oracle_path():
    path = os.path.join(os.path.dirname(__file__), "..", "traces", "mi355x_throughputs.json")
    assert os.path.exists(path)
    return path


@pytest.fixture(scope="session")
def throughputs(oracle_path):
    from shockwave_amd.core.throughputs import read_throughputs

    return read_throughputs(oracle_path)
