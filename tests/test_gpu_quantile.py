"""The radix-select kernels (csrc/quantile.hip) behind ops.order_statistics and ht.percentile / median,
against NumPy on the same values: order statistics must be equal (selection is exact), interpolated
percentiles within 4 eps(result dtype) * max(|lo|, |hi|) of np.percentile on the float64 cast - three
roundings of lo + (hi - lo) * frac plus the rounding of frac."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _data(shape, dtype):
    """Negatives, +-0, +-inf, subnormals, gamma values, ~30 % drawn from 3 repeated values."""
    rng = np.random.default_rng(sum(shape) + 11)
    a = (rng.gamma(2.0, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(dtype)
    tiny = np.finfo(dtype).tiny
    special = np.array([0.0, -0.0, np.inf, -np.inf, tiny / 4, -tiny / 8, 1.5, 1.5, 1.5, -2.25, -2.25, -2.25,
                        7.0, 7.0, 7.0], dtype=dtype)
    pick = rng.random(shape) < 0.35
    a[pick] = rng.choice(special, int(pick.sum()))
    return a


def _device_pair(shape, dtype, lead=0):
    """The test values on the host and on the device, `lead` elements past an aligned buffer."""
    a = _data((shape[0] + lead,) + tuple(shape[1:]), dtype)
    return a[lead:], torch.from_numpy(a).to(_dev())[lead:]


def _ranks(kind, n):
    r = {"first": [0], "last": [n - 1], "middle": [(n - 1) // 2, n // 2],
         "nine": [int(round(f * (n - 1))) for f in np.linspace(0.03, 0.97, 9)],
         "many": list(range(0, 40 * 7, 7))}[kind]
    return sorted(set(min(v, n - 1) for v in r))


# flat: one wave, one chunk against several, an unaligned start (lead 1); last axis: short rows, many
# rows, rows split over blocks; axis 0: one row, the scalar-column tail, more than one column tile,
# many chunks; a middle axis (one copy)
CASES = [((1,), None, 0), ((2,), None, 0), ((255,), None, 0), ((257,), None, 0), ((16389,), None, 0),
         ((100003,), None, 1), ((5, 1000), 1, 0), ((1000, 7), 1, 0), ((3, 70001), 1, 0), ((1, 5), 0, 0),
         ((4097, 3), 0, 0), ((64, 1025), 0, 0), ((70001, 130), 0, 0), ((4, 33, 5), 1, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["first", "last", "middle", "nine", "many"])
@pytest.mark.parametrize("shape,axis,lead", CASES)
def test_order_statistics(shape, axis, lead, kind, dtype):
    from heat_amd import ops

    a, x = _device_pair(shape, dtype, lead)
    ranks = _ranks(kind, a.size if axis is None else a.shape[axis])
    got = ops.order_statistics(x, ranks, axis).cpu().numpy()
    want = np.moveaxis(np.take(np.sort(a, axis=axis), ranks, axis=0 if axis is None else axis),
                       0 if axis is None else axis, 0)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert (got == want).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["equal", "nan"])
@pytest.mark.parametrize("shape,axis,lead", [((100003,), None, 1), ((4097, 3), 0, 0)])
def test_order_statistics_equal_and_nan(shape, axis, lead, variant, dtype):
    """All elements equal: every key is under the prefix, more than the compaction cap, so the digit
    passes read the input. One NaN: its slice yields NaN, the others stay exact."""
    from heat_amd import ops

    full = _data((shape[0] + lead,) + tuple(shape[1:]), dtype)
    full = np.full_like(full, -3.75) if variant == "equal" else full.copy()
    if variant == "nan":
        full[(4000,) + (1,) * (full.ndim - 1)] = np.nan
    a, x = full[lead:], torch.from_numpy(full).to(_dev())[lead:]   # `lead` elements past an aligned buffer
    n = a.shape[0]
    ranks = sorted({0, (n - 1) // 2, n // 2, n - 1})
    got = ops.order_statistics(x, ranks, axis).cpu().numpy().reshape(len(ranks), -1)
    want = np.sort(a, axis=0)[ranks].reshape(len(ranks), -1)
    bad = np.isnan(a).any(axis=0).reshape(-1)
    assert np.isnan(got[:, bad]).all() and (got[:, ~bad] == want[:, ~bad]).all()


def _close(got, a, q, axis, method):
    """got against np.percentile of the float64 cast: equal for the picking methods, else the bound."""
    want = np.percentile(a.astype(np.float64), q, axis=axis, method=method)
    assert got.shape == want.shape
    if method in ("lower", "higher", "nearest"):
        assert (got == want).all()
        return
    lo = np.abs(np.percentile(a.astype(np.float64), q, axis=axis, method="lower"))
    hi = np.abs(np.percentile(a.astype(np.float64), q, axis=axis, method="higher"))
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 4 * np.finfo(got.dtype).eps * np.maximum(lo, hi)).all()


def test_past_the_sort_limit():
    """2^24 + 5 elements: one more than torch.quantile takes."""
    import heat_amd as ht
    from heat_amd import ops

    n = 2 ** 24 + 5
    a = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    x = torch.from_numpy(a).to(_dev())
    ranks = [0, n // 2, n - 1]
    got = ops.order_statistics(x, ranks).cpu().numpy()
    assert (got == np.partition(a, ranks)[ranks]).all()
    med = ht.median(ht.array(x, device="gpu")).larray.cpu().numpy()
    _close(med, a, 50.0, None, "linear")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("axis", [None, 0, 1])
@pytest.mark.parametrize("method", ["linear", "lower", "higher", "midpoint", "nearest"])
@pytest.mark.parametrize("q", [50.0, [0, 12.5, 50, 99.9, 100]])
def test_percentile(q, method, axis, native, dtype, monkeypatch):
    """Both paths are held to the bound: the kernels, and torch.quantile with HEAT_QUANTILE_NATIVE=0
    (which interpolates device float32 data on a float64 copy, its float32 position being too coarse)."""
    import heat_amd as ht
    from heat_amd.core.communication import PATH_COUNTS

    _dev()
    if not native:
        monkeypatch.setenv("HEAT_QUANTILE_NATIVE", "0")
    a = np.random.default_rng(5).gamma(2.0, 1.5, (4097, 35)).astype(dtype) - 2.0
    x = ht.array(a, device="gpu")
    before = PATH_COUNTS["percentile:native"]
    got = ht.percentile(x, q, axis=axis, interpolation=method).larray.cpu().numpy()
    assert PATH_COUNTS["percentile:native"] - before == (1 if native else 0)
    assert got.dtype == dtype
    _close(got, a, q, axis, method)
