"""Native float64 distance kernels (``ops/csrc/cdist_f64.hip`` behind ``ops.cdist_f64``) against plain
broadcast fp64 expressions on the CPU: fragment map / stage / ring / tail edges on exact integers,
error bounds on random data, near-identical rows, strided views and ``out=``, the symmetric mode and
the public float64 routes."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
# (metric, exact): the three expansion modes, the three exact ones and manhattan
_ALL = [("sqeuclidean", False), ("euclidean", False), ("gaussian", False), ("sqeuclidean", True),
        ("euclidean", True), ("gaussian", True), ("manhattan", False)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _ref(x, y):
    d = x[:, None, :] - y[None, :, :]
    return (d * d).sum(-1), d.abs().sum(-1)


@functools.lru_cache(maxsize=None)
def _random(m, n, f, scale):
    g = torch.Generator().manual_seed(m + 3 * n + 7 * f)
    x = scale * torch.randn(m, f, generator=g, dtype=torch.float64)
    y = scale * torch.randn(n, f, generator=g, dtype=torch.float64)
    return (x, y) + _ref(x, y)


def _sigma(d2):
    return float(d2.max() / 16) ** 0.5    # d2 / (2 sigma^2) <= 8


def _assert_close(res, x, y, d2, d1, metric, exact, sigma):
    """Squared error <= 4 (f + 2) u (|x|^2 + |y|^2) for the expansion, <= 4 (f + 2) u d2 for the
    difference form (manhattan: on d1); euclidean through its square; gaussian: rtol 2^-48 on top
    of the propagated d2 bound."""
    c = 4 * (x.shape[1] + 2) * U
    if metric == "manhattan":
        err, bound = (res - d1).abs(), c * d1
    else:
        b2 = c * (d2 if exact else (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :])
        if metric == "gaussian":
            s = 1.0 / (2.0 * sigma * sigma)
            ref = torch.exp(-s * d2)
            err, bound = (res - ref).abs(), ref * (2.0 ** -48 + torch.expm1(s * b2))
        else:
            err, bound = ((res * res if metric == "euclidean" else res) - d2).abs(), b2
    assert torch.all(err <= bound), (metric, exact, float((err - bound).max()))


@pytest.mark.parametrize("m,n,f", [(1, 1, 1), (129, 131, 1), (130, 260, 7), (257, 191, 8), (258, 192, 9),
                                   (256, 256, 32), (256, 128, 40), (300, 129, 37), (64, 2000, 200)])
def test_cdist_f64_exact_integers(m, n, f):
    """Entries from {-8..8}: every product and partial sum is exact in fp64, so a wrong fragment
    map, k-slot mismatch, tail handling or store map changes the result outright."""
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(m + n + f)
    x = torch.randint(-8, 9, (m, f), generator=g).double()
    y = torch.randint(-8, 9, (n, f), generator=g).double()
    d2, d1 = _ref(x, y)
    X, Y = x.to(dev), y.to(dev)
    assert torch.equal(ops.cdist_f64(X, Y, "sqeuclidean").cpu(), d2)
    assert torch.equal(ops.cdist_f64(X, Y, "sqeuclidean", exact=True).cpu(), d2)
    assert torch.equal(ops.cdist_f64(X, Y, "manhattan").cpu(), d1)


@pytest.mark.parametrize("metric,exact", _ALL)
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("m,n,f", [(513, 257, 64), (300, 129, 200)])
def test_cdist_f64_random(m, n, f, scale, metric, exact):
    from heat_amd import ops

    dev = _dev()
    x, y, d2, d1 = _random(m, n, f, scale)
    sigma = _sigma(d2)
    res = ops.cdist_f64(x.to(dev), y.to(dev), metric, sigma=sigma, exact=exact).cpu()
    assert res.dtype == torch.float64 and res.shape == (m, n)
    _assert_close(res, x, y, d2, d1, metric, exact, sigma)


def test_cdist_f64_near_identical_rows():
    """d2(i, i) ~ 6e-17 with |x|^2 ~ 6e7: only the difference kernel can meet the relative bound,
    so ``exact=True`` must reach it (the expansion's rounding of |x|^2 alone is ~1e-8). The fp64
    broadcast reference itself stays within 2 (f + 2) u d2 of an 80-bit evaluation for this seed."""
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(3)
    x = 1e3 * torch.randn(200, 64, generator=g, dtype=torch.float64)
    y = x + 1e-9 * torch.randn(200, 64, generator=g, dtype=torch.float64)
    d2, d1 = _ref(x, y)
    X, Y = x.to(dev), y.to(dev)
    _assert_close(ops.cdist_f64(X, Y, "sqeuclidean", exact=True).cpu(), x, y, d2, d1, "sqeuclidean", True, 1.0)
    _assert_close(ops.cdist_f64(X, Y, "euclidean", exact=True).cpu(), x, y, d2, d1, "euclidean", True, 1.0)
    err = (ops.cdist_f64(X, Y, "sqeuclidean").cpu() - d2).abs().diagonal()
    assert torch.all(err > 4 * 66 * U * d2.diagonal())


@pytest.mark.parametrize("metric,exact", _ALL)
def test_cdist_f64_views_and_out(metric, exact):
    """Row-strided operand views whose last row ends where the storage ends, X's base only 8-byte
    aligned; the result goes into the first n columns of a wider matrix with an odd row stride."""
    from heat_amd import ops

    dev = _dev()
    m, n, f, ld = 150, 131, 38, 40
    x, y, d2, d1 = _random(m, n, f, 1.0)
    bx = torch.zeros(1 + (m - 1) * ld + f, dtype=torch.float64, device=dev)
    by = torch.zeros((n - 1) * ld + f, dtype=torch.float64, device=dev)
    X, Y = bx[1:].as_strided((m, f), (ld, 1)), by.as_strided((n, f), (ld, 1))
    X.copy_(x)
    Y.copy_(y)
    assert X.data_ptr() % 16 == 8 and Y.data_ptr() % 16 == 0
    wide = torch.full((m, n + 4), -1.0, dtype=torch.float64, device=dev)
    sigma = _sigma(d2)
    ops.cdist_f64(X, Y, metric, sigma=sigma, out=wide[:, :n], exact=exact)
    _assert_close(wide[:, :n].cpu(), x, y, d2, d1, metric, exact, sigma)
    assert torch.all(wide[:, n:] == -1.0)


@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
def test_cdist_f64_symmetric(metric):
    from heat_amd import ops

    dev = _dev()
    X = torch.randn(300, 70, generator=torch.Generator().manual_seed(70), dtype=torch.float64).to(dev)
    s = ops.cdist_f64(X, X, metric, exact=True, symmetric=True)
    assert torch.equal(s, ops.cdist_f64(X, X.clone(), metric, exact=True))
    assert torch.equal(s, s.t()) and torch.all(s.diagonal() == 0)


def test_float64_distances_route_to_cdist_f64(gpu, monkeypatch):
    import heat_amd as ht
    from heat_amd.ops import kernels

    rng = np.random.default_rng(4)
    x, y = rng.normal(size=(300, 37)), rng.normal(size=(200, 37))
    dxy = np.sqrt(((x[:, None] - y[None]) ** 2).sum(-1))
    dxx = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    calls, real = [], kernels.cdist_f64
    monkeypatch.setattr(kernels, "cdist_f64", lambda *a, **k: calls.append(a[0].dtype) or real(*a, **k))
    cases = [(lambda X, Y: ht.spatial.cdist(X, Y), dxy, 1e-12),
             (lambda X, Y: ht.spatial.cdist(X), dxx, 1e-12),
             (lambda X, Y: ht.spatial.cdist(X, Y, quadratic_expansion=True), dxy, 1e-9),
             (lambda X, Y: ht.spatial.rbf(X, Y, sigma=2.0), np.exp(-dxy ** 2 / 8.0), 1e-12),
             (lambda X, Y: ht.spatial.manhattan(X, Y), np.abs(x[:, None] - y[None]).sum(-1), 1e-12),
             (lambda X, Y: ht.spatial.cdist_topk(X, Y, k=3)[0], np.sort(dxy, axis=1)[:, :3], 1e-12)]
    X, Y = ht.array(x, device="gpu"), ht.array(y, device="gpu")
    X32, Y32 = ht.array(x.astype(np.float32), device="gpu"), ht.array(y.astype(np.float32), device="gpu")
    assert X.dtype == ht.float64
    for call, ref, rtol in cases:
        n = len(calls)
        res = call(X, Y)
        assert len(calls) > n and res.dtype == ht.float64
        assert np.allclose(res.numpy(), ref, rtol=rtol, atol=0)
        n = len(calls)
        assert call(X32, Y32).dtype == ht.float32 and len(calls) == n
    assert all(d == torch.float64 for d in calls)
