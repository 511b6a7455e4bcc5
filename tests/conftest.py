import os
import pathlib
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# wass_stereo hands its frame to a per-GPU resident worker when it can (wass_amd/host/stereo_server.hpp).  The tests of the executable
# itself run it in-process; tests/test_server.py switches the server on, with a socket directory and an idle time-out of its own.
os.environ.setdefault("WASS_NO_SERVER", "1")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    """The CPU oracle (test infrastructure only)."""
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="session")
def gpu_ctx():
    """A libwassgpu context on device 0; fails loudly if the HIP library or the GPU is missing."""
    import wass_amd
    ctx = wass_amd.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def sockroot(tmp_path):
    """Where the tests make their socket directories.  A Unix socket's path holds at most 107 bytes (sun_path) and the server binds
    <dir>/wass_stereo_<uid>_gpu<g>.sock -- a longer one makes every caller compute in-process -- so where pytest's tmp_path is too
    deep for <tmp_path>/sockN/<name>, a short directory of the temporary area is used instead and removed afterwards."""
    budget = 107 - len("/sock99/wass_stereo_4294967295_gpu99.sock")
    if len(str(tmp_path)) <= budget:
        yield tmp_path
        return
    for base in (tempfile.gettempdir(), "/tmp"):
        if len(base) + len("/wss_XXXXXXXX") <= budget and os.access(base, os.W_OK):
            d = tempfile.mkdtemp(prefix="wss_", dir=base)
            break
    else:
        pytest.fail(f"no writable temporary directory short enough for a Unix socket path (tmp_path: {tmp_path})")
    yield pathlib.Path(d)
    shutil.rmtree(d, ignore_errors=True)
