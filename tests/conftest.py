import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP) device")
    config.addinivalue_line("markers", "slow: long-running CPU test")


def pytest_collection_modifyitems(config, items):
    have_gpu = torch.cuda.is_available()
    skip_gpu = pytest.mark.skip(reason="no HIP device")
    for it in items:
        if "gpu" in it.keywords and not have_gpu:
            it.add_marker(skip_gpu)


@pytest.fixture
def golden_dir():
    """Data files of the reference project (CSV, shipped checkpoints, result logs), stored with
    the tests; ``oracle/make_golden.py`` writes them."""
    return GOLDEN


@pytest.fixture(scope="session")
def ref_out():
    """What the reference's own functions return on the tests' seeded inputs
    (``oracle/make_golden.py``), read-only."""
    import numpy as np

    with np.load(GOLDEN / "reference_outputs.npz") as d:
        out = {k: d[k] for k in d.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from vi_normflows_amd.ops._ext import native

    native()  # fail loudly if the HIP library is missing
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def _gemm_backend_guard():
    """No test may leak a GEMM backend change into later tests (GPU tests must exercise the
    hand-written MFMA kernels unless they opt out explicitly)."""
    from vi_normflows_amd.ops import gemm

    prev = gemm.backend()
    yield
    assert gemm.backend() == prev, f"test changed the GEMM backend to {gemm.backend()}"


@pytest.fixture
def kpaths(monkeypatch):
    """kpaths(cpl_xbf16=0, ...): switch engine kernel paths (utils.config.KernelPaths) for the
    engines constructed afterwards in this test, through VINF_KERNEL_PATHS (merged with what
    earlier calls of the same test set)."""
    cur = {}

    def set_(**kw):
        cur.update({k: int(bool(v)) for k, v in kw.items()})
        monkeypatch.setenv("VINF_KERNEL_PATHS", ",".join(f"{k}={v}" for k, v in cur.items()))
    return set_
