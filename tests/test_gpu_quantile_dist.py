"""ht.percentile on split device arrays (tests/quantile_checks.py) at 2 and 3 ranks on the one card, in
the gloo host-staged world of test_gpu_dist.py."""
import pytest
import torch

from . import quantile_checks
from ._dist import run_distributed_batch

pytestmark = pytest.mark.gpu

NAMES = [n for n in dir(quantile_checks) if n.startswith("check_")]
ENV = {"HEAT_AMD_DEFAULT_DEVICE": "gpu", "HEAT_COMM_TIMEOUT": "60"}
_BATCH = {}


@pytest.mark.parametrize("nprocs", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_percentile_on_split_arrays(name, nprocs):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if nprocs not in _BATCH:
        _BATCH[nprocs] = run_distributed_batch("tests.quantile_checks", NAMES, nprocs, timeout=300, env_extra=ENV,
                                               keep_gpu=True)
    ok, err = _BATCH[nprocs][name]
    if not ok:
        pytest.fail("check {} failed at {} ranks:\n{}".format(name, nprocs, err))
