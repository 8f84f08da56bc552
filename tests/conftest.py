import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "perf: asserts on wall-clock time; collected LAST so that `pytest -x` reaches every parity "
                                       "test before a noisy box can stop the run")


def pytest_collection_modifyitems(session, config, items):
    """Every test that holds the clock to a bound (marker `perf`) runs after every test that holds the bits: a slow or shared
    box then costs the timing tests only, never the parity evidence behind them in file order (`pytest -x -m gpu`)."""
    items.sort(key=lambda item: 1 if item.get_closest_marker("perf") else 0)   # (stable: file order kept inside each class)


_two_rank = None


HYBRID_WAIT_S = 900   # the four hybrid ranks' whole run, waited for before any test starts


def _start_ranks(worker, world, prefix):
    """`world` processes of tests/<worker> (RANK WORLD PORT OUT), each logging to OUT/rank<r>.log."""
    import socket
    import subprocess
    import tempfile

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tempfile.mkdtemp(prefix=prefix)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    logs = [open(os.path.join(out, f"rank{r}.log"), "w") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", worker), str(r), str(world), str(port), out],
                              env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    return procs, out, logs


def pytest_collection_finish(session):
    """tests/test_gpu_two_rank.py: its worker processes must be started before THIS process initialises the GPU
    (collection imports the test modules but runs no kernel).  Only when that test is among the collected (not
    deselected) items and a device node exists -- /dev/kfd: probing through torch could initialise HIP in this
    process on builds without amdsmi.  The four ranks of the hybrid layout (2 query groups x 2 key shards:
    tests/hybrid_worker.py) run first and are waited for here; then the two ranks of tests/two_rank_worker.py start and
    run beside the other tests.  So at most four processes have the GPU open at once (the hybrid ranks; later this
    process, the two ranks and a child process a test starts), and the tests collect the reports."""
    global _two_rank
    if _two_rank is not None or os.environ.get("RAGRAPH_SKIP_TWO_RANK") == "1":
        return
    if not any("test_gpu_two_rank" in item.nodeid for item in session.items) or not os.path.exists("/dev/kfd"):
        return
    import subprocess
    import time

    procs4, out4, logs4 = _start_ranks("hybrid_worker.py", 4, "ragraph_hybrid_")
    deadline = time.monotonic() + HYBRID_WAIT_S
    for p in procs4:
        try:
            p.wait(timeout=max(deadline - time.monotonic(), 1))
        except subprocess.TimeoutExpired:   # (its missing report fails test_four_ranks_hybrid_layout)
            break
    for p in procs4:
        if p.poll() is None:
            p.kill()
            p.wait()
    procs, out, logs = _start_ranks("two_rank_worker.py", 2, "ragraph_two_rank_")
    _two_rank = (procs, out, logs, procs4, out4, logs4)


def pytest_sessionfinish(session, exitstatus):
    if _two_rank is not None:
        import shutil

        for p in list(_two_rank[0]) + list(_two_rank[3]):
            if p.poll() is None:
                p.kill()
            p.wait()
        for f in list(_two_rank[2]) + list(_two_rank[5]):
            f.close()
        if exitstatus == 0:   # (a failed session keeps the workers' logs and reports for the post-mortem)
            shutil.rmtree(_two_rank[1], ignore_errors=True)
            shutil.rmtree(_two_rank[4], ignore_errors=True)


@pytest.fixture(scope="session")
def two_rank_job():
    return _two_rank


@pytest.fixture(scope="session")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")
