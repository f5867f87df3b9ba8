"""Split-array checks of ht.percentile on the radix-select kernels (run by test_gpu_quantile_dist.py
in 2 and 3 ranks): values against np.percentile of the global data within 4 eps * max(|lo|, |hi|),
through the kernels (PATH_COUNTS["percentile:native"]) and without any personalised exchange - the
distributed sort is gone."""
import numpy as np

import heat_amd as ht
from heat_amd.core.communication import PATH_COUNTS

Q = [0, 12.5, 50, 99.9, 100]


def _exchanges():
    return sum(v for k, v in PATH_COUNTS.items() if k.startswith("alltoallv"))


def _check(a, split, axis):
    x = ht.array(a, split=split)
    assert x.larray.is_cuda
    for method in ("linear", "lower", "nearest"):
        native, sent = PATH_COUNTS["percentile:native"], _exchanges()
        res = ht.percentile(x, Q, axis=axis, interpolation=method)
        assert PATH_COUNTS["percentile:native"] == native + 1 and _exchanges() == sent
        got = res.numpy()
        a64 = a.astype(np.float64)
        want = np.percentile(a64, Q, axis=axis, method=method)
        lo = np.abs(np.percentile(a64, Q, axis=axis, method="lower"))
        hi = np.abs(np.percentile(a64, Q, axis=axis, method="higher"))
        tol = 0 if method != "linear" else 4 * np.finfo(a.dtype).eps * np.maximum(lo, hi)
        assert got.shape == want.shape and got.dtype == a.dtype
        assert (np.abs(got.astype(np.float64) - want) <= tol).all(), (method, got, want)


def _values(shape, dtype):
    return (np.random.default_rng(sum(shape)).gamma(2.0, 1.5, shape) - 2.0).astype(dtype)


def check_along_split_flat():
    for dtype in (np.float32, np.float64):
        _check(_values((1001,), dtype), 0, 0)


def check_along_split_matrix():
    for dtype in (np.float32, np.float64):
        _check(_values((1001, 6), dtype), 0, 0)


def check_off_split():
    _check(_values((6, 1001), np.float32), 0, 1)


def check_rank_without_elements():
    _check(np.array([3.5, -1.25], dtype=np.float32), 0, 0)
