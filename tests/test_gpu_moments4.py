"""The fused (n, mean, M2, M3, M4) kernels (csrc/moments4.hip) and the skew / kurtosis path on them,
against a two-pass NumPy reference in extended precision on the same values.

Bounds: n * 2^-53 times a small conditioning constant, 1e-10 at these sizes (n <= 1e5):
|M_k - ref_k| <= 1e-10 n sigma^k, |mean - ref| <= 1e-12 (|mean| + sigma)."""
import functools

import numpy as np
import pytest
import torch

LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
DTYPES = [np.float32, np.float64]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _data(shape, dtype, offset=0.0):
    a = np.random.default_rng(sum(shape) + 7).gamma(2.0, 1.5, shape)   # skewed: M3 is not near zero
    return (a + offset).astype(dtype)


def _ref(a, axis):
    w = a.astype(LD)
    mu = w.mean(axis=axis, keepdims=True)
    d = w - mu
    n = w.size if axis is None else w.shape[axis]
    mu = mu.reshape(()) if axis is None else mu.squeeze(axis)
    return (n, mu) + tuple((d ** k).sum(axis=axis) for k in (2, 3, 4))


def _check(got, a, axis):
    got = [np.asarray(g.cpu().numpy(), dtype=LD) for g in got]
    n, mu, *m = _ref(a, axis)
    sigma = np.sqrt(m[0] / n)
    assert got[0].shape == mu.shape and (got[0] == n).all()
    err = np.abs(got[1] - mu) / (np.abs(mu) + sigma)
    print("mean", float(np.max(err)))
    assert (np.abs(got[1] - mu) <= 1e-12 * (np.abs(mu) + sigma)).all()
    for k, g, r in zip((2, 3, 4), got[2:], m):
        print("M%d" % k, float(np.max(np.abs(g - r) / np.maximum(n * sigma ** k, LD(1e-300)))))
        assert (np.abs(g - r) <= 1e-10 * n * sigma ** k).all(), k


# flat: head / body / tail edges, one chunk against several, an unaligned start (lead 1); last axis:
# the wave-per-row kernel and rows split over blocks; axis 0: one column, a scalar-column tail, more
# than one column block, the two-level merge; a middle axis (one copy)
CASES = [((1,), None, 0), ((3,), None, 0), ((255,), None, 0), ((257,), None, 0), ((16389,), None, 0),
         ((100003,), None, 1), ((5, 1000), 1, 0), ((1000, 7), 1, 0), ((3, 70001), 1, 0), ((1, 5), 0, 0),
         ((4097, 3), 0, 0), ((64, 1025), 0, 0), ((70001, 130), 0, 0), ((4, 33, 5), 1, 0)]


def _device_pair(shape, dtype, lead=0, offset=0.0):
    """The test values on the host and on the device, `lead` elements past an aligned buffer."""
    a = _data((shape[0] + lead,) + tuple(shape[1:]), dtype, offset)
    return a[lead:], torch.from_numpy(a).to(_dev())[lead:]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,axis,lead", CASES)
def test_moments4(shape, axis, lead, dtype):
    from heat_amd import ops

    a, x = _device_pair(shape, dtype, lead)
    _check(ops.moments4(x, axis), a, axis)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,offset", [(np.float32, 1e4), (np.float64, 1e6)])
@pytest.mark.parametrize("shape,axis", [((16389,), None), ((4097, 3), 0)])
def test_moments4_large_offset(shape, axis, dtype, offset):
    """Unshifted or badly shifted sums fail here by orders of magnitude. Measured: at most 4e-13 n
    sigma^4 for float32 + 1e4; for float64 + 1e6 over 9 merged column chunks 4.3e-11 n sigma^4 in M4
    (4.5e-12 in M3): the chunk means are doubles at 1e6, and ulp(1e6) / sigma = 5e-11 enters the
    merge's delta."""
    from heat_amd import ops

    a, x = _device_pair(shape, dtype, offset=offset)
    _check(ops.moments4(x, axis), a, axis)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape,axis", [((100003,), None), ((3, 70001), 1), ((5, 1000), 1), ((4097, 6), 0)])
def test_moments4_constant(shape, axis, dtype):
    from heat_amd import ops

    c = 1.0 / 3.0 if dtype == torch.float64 else 0.1   # full mantissas: sums of them round
    x = torch.full(shape, c, dtype=dtype, device=_dev())
    n, mu, m2, m3, m4 = ops.moments4(x, axis)
    assert torch.equal(mu, torch.full_like(mu, float(x.reshape(-1)[0])))
    for m in (m2, m3, m4):
        assert torch.equal(m, torch.zeros_like(m))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,axis,where", [((5, 1000), 1, (2, 17)), ((4097, 3), 0, (4000, 1)),
                                              ((3, 70001), 1, (1, 69999))])
def test_moments4_nan(shape, axis, where, dtype):
    from heat_amd import ops

    _, x = _device_pair(shape, dtype)
    x = x.clone()
    x[where] = float("nan")
    bad = torch.zeros(shape[1 - axis], dtype=torch.bool, device=x.device)
    bad[where[1 - axis]] = True
    for m in ops.moments4(x, axis)[1:]:
        assert torch.equal(torch.isnan(m), bad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,axis", [((100003,), None), ((3, 70001), 1), ((70001, 130), 0)])
def test_moments4_bit_reproducible(shape, axis, dtype):
    from heat_amd import ops

    _, x = _device_pair(shape, dtype)
    first, second = torch.stack(ops.moments4(x, axis)), torch.stack(ops.moments4(x, axis))
    assert torch.equal(first, second)


def test_merge_moments4():
    """Three uneven parts, one of them empty, merge to the whole array's quintuple (host tensors)."""
    from heat_amd import ops

    a = _data((1000, 3), np.float64)
    t = torch.from_numpy(a)
    parts = [ops.moments4(p, 0) for p in (t[:137], t[137:137], t[137:])]
    merged = ops.merge_moments4(*(torch.stack(f) for f in zip(*parts)), 0)
    _check(merged, a, 0)
    _check(ops.moments4(t, 0), a, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [None, 0, 1])
def test_skew_kurtosis_device(gpu, axis, dtype):
    import heat_amd as ht

    a = _data((3000, 17), dtype)
    x = ht.array(a)
    assert x.larray.is_cuda
    n, _, M2, M3, M4 = _ref(a, axis)
    rtol = 1e-8 if dtype == np.float64 else 1e-5
    for unbiased in (False, True):
        g1 = (M3 / n) / (M2 / n) ** LD(1.5)
        if unbiased:
            g1 = g1 * np.sqrt(LD(n * (n - 1))) / (n - 2)
        got = ht.skew(x, axis=axis, unbiased=unbiased)
        assert got.larray.dtype == x.larray.dtype
        np.testing.assert_allclose(got.larray.cpu().numpy(), g1.astype(np.float64), rtol=rtol)
        for fisher in (False, True):
            g2 = (M4 / n) / (M2 / n) ** 2
            if unbiased:
                g2 = ((n + 1) * (g2 - 3) + 6) * (n - 1) / LD((n - 2) * (n - 3)) + 3
            g2 = g2 - 3 if fisher else g2
            got = ht.kurtosis(x, axis=axis, unbiased=unbiased, Fischer=fisher)
            np.testing.assert_allclose(got.larray.cpu().numpy(), g2.astype(np.float64), rtol=rtol)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,axis", [((1 << 24,), None), ((1 << 14, 1 << 10), 0)])
def test_kurtosis_no_full_size_temporaries(gpu, shape, axis):
    """The fp64 copy of the two-pass path alone is twice the input; the fused pass allocates its
    outputs and chunk partials."""
    import heat_amd as ht

    x = ht.random.rand(*shape)
    assert x.larray.is_cuda and x.larray.dtype == torch.float32
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ht.kurtosis(x, axis=axis)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert extra < x.larray.numel() * x.larray.element_size() // 4, extra
