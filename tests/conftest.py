import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU and the built kernels")
    config.addinivalue_line("markers", "slow: long-running CPU test")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


REF_DATA = os.path.join(ROOT, "tests", "golden", "test_fsl.tar.gz")


@pytest.fixture(scope="session")
def _fs_golden(tmp_path_factory):
    """``tests/golden/test_fsl.tar.gz`` (the reference's ``datasets/test_fsl``: inputspec.json and
    per site a covariate CSV plus one aseg-stats text file per subject) unpacked once per run."""
    import tarfile
    d = tmp_path_factory.mktemp("golden")
    with tarfile.open(REF_DATA) as t:
        t.extractall(d)
    return str(d / "test_fsl")


@pytest.fixture
def fs_data_root(_fs_golden):
    """The reference's shipped 5-site FreeSurfer simulator data (read-only)."""
    return _fs_golden
