import asyncio
import os
import sys

import pytest

# Make the repo root importable regardless of pytest invocation directory.
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: requires a real MI355X GPU (run on the GPU box)")


@pytest.fixture
def run():
    """Run a coroutine to completion (we avoid a pytest-asyncio dependency)."""

    def _run(coro):
        return asyncio.run(coro)

    return _run


@pytest.fixture
def sock_dir():
    """A short-lived directory for unix sockets. sockaddr_un.sun_path holds
    at most 107 bytes, and pytest's tmp_path (base temp + user + test name)
    can exceed that, so sockets get a directory with a short path instead."""
    import shutil
    import tempfile

    base = tempfile.gettempdir()
    if len(base) > 60:
        base = "/tmp"
    d = tempfile.mkdtemp(prefix="gda-", dir=base)
    try:
        yield d
    finally:
        shutil.rmtree(d, ignore_errors=True)


def require_gpu():
    try:
        import torch

        if not torch.cuda.is_available():
            pytest.skip("no GPU available")
    except Exception:
        pytest.skip("torch unavailable")
