"""Native float64 k-means (``ops/csrc/kmeans_f64.hip`` behind ``ops.kmeans_assign_f64``, the fp64 update
of ``kmeans.hip`` and the fp64 ``kmeans_finalize``) against plain broadcast fp64 expressions on the CPU:
fragment map / centroid tiles / stage / ring / tail edges and the tie rule on exact integers, error
bounds on random and on far-shifted data, strided views, the deterministic update and the public
``ht.cluster.KMeans`` route."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
_SHAPES = [(1, 1, 1), (129, 1, 3), (130, 17, 7), (257, 129, 8), (300, 130, 9), (128, 256, 32), (200, 260, 37),
           (64, 300, 200)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _d2(x, c):
    return ((x[:, None] - c[None]) ** 2).sum(-1)


def _shifted(n, k, f):
    """k unit-spaced grid centres shifted by 1e4 per coordinate, n points 0.05 around them."""
    g = torch.Generator().manual_seed(n + k + f)
    j = torch.arange(k)
    c = torch.zeros(k, f, dtype=torch.float64)
    for a in range(min(f, 4)):
        c[:, a] = (j // 6 ** a) % 6
    c += 1e4
    x = c[torch.arange(n) % k] + 0.05 * torch.randn(n, f, generator=g, dtype=torch.float64)
    return x, c


@functools.lru_cache(maxsize=None)
def _random(n, k, f):
    if (n, k, f) == (400, 130, 5):
        x, c = _shifted(n, k, f)
    else:
        g = torch.Generator().manual_seed(n + 3 * k + 7 * f)
        x = torch.randn(n, f, generator=g, dtype=torch.float64)
        c = torch.randn(k, f, generator=g, dtype=torch.float64)
    return x, c, _d2(x, c)


def _check_assign(labels, mind, x, c, d2):
    """d2(i, label_i) - min_j d2(i, j) <= 2 b_i and |mind_i - min_j d2(i, j)| <= b_i with
    b_i = 4 (f + 2) u (|x_i|^2 + max_j |c_j|^2), the expansion bound of test_gpu_cdist_f64.py."""
    b = 4 * (x.shape[1] + 2) * U * ((x * x).sum(1) + (c * c).sum(1).max())
    best = d2.min(1).values
    assert labels.dtype == torch.int32 and mind.dtype == torch.float64
    lab = labels.cpu().long()
    assert torch.all((lab >= 0) & (lab < c.shape[0]))
    assert torch.all(d2.gather(1, lab[:, None])[:, 0] - best <= 2 * b)
    assert torch.all((mind.cpu() - best).abs() <= b)
    return b


@pytest.mark.parametrize("n,k,f", _SHAPES)
def test_assign_f64_exact_integers(n, k, f):
    """Entries from {-8..8} and every third centroid a copy of an earlier one: every score is exact,
    so labels are NumPy's first-index argmin and mind is the reference, bit for bit."""
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(n + k + f)
    x = torch.randint(-8, 9, (n, f), generator=g).double()
    c = torch.randint(-8, 9, (k, f), generator=g).double()
    for j in range(2, k, 3):
        c[j] = c[j // 2]
    d2 = _d2(x, c)
    labels, mind = ops.kmeans_assign_f64(x.to(dev), c.to(dev))
    assert np.array_equal(labels.cpu().numpy(), np.argmin(d2.numpy(), axis=1))
    assert torch.equal(mind.cpu(), d2.min(1).values)
    assert ops.kmeans_assign_f64(x.to(dev), c.to(dev), want_mind=False)[1] is None


@pytest.mark.parametrize("n,k,f", _SHAPES + [(400, 130, 5)])
def test_assign_f64_random(n, k, f):
    from heat_amd import ops

    dev = _dev()
    x, c, d2 = _random(n, k, f)
    labels, mind = ops.kmeans_assign_f64(x.to(dev), c.to(dev))
    b = _check_assign(labels, mind, x, c, d2)
    if (n, k, f) == (400, 130, 5):   # shifted: the reference's own margin excludes a flip
        two = torch.topk(d2, 2, dim=1, largest=False).values
        assert torch.all(two[:, 1] - two[:, 0] > 2 * b)
        assert torch.equal(labels.cpu().long(), d2.argmin(1))
        lab32, mind32 = ops.kmeans_assign(x.to(dev), c.to(dev))   # the public op: fp64 kernel, fp32 mind
        assert torch.equal(lab32, labels) and mind32.dtype == torch.float32


@pytest.mark.parametrize("n,k,f", [(200, 260, 37), (400, 130, 5)])
def test_assign_f64_strided_views(n, k, f):
    """X a column slice of a wider tensor with an odd leading dimension, C every other row."""
    from heat_amd import ops

    dev = _dev()
    x, c, d2 = _random(n, k, f)
    wide = torch.zeros((n, f + 4), dtype=torch.float64, device=dev)
    X = wide[:, 1:f + 1]
    X.copy_(x)
    C = torch.zeros((2 * k, f), dtype=torch.float64, device=dev)[::2]
    C.copy_(c)
    assert X.stride(0) % 2 == 1 and not C.is_contiguous()
    _check_assign(*ops.kmeans_assign_f64(X, C), x, c, d2)


@pytest.mark.parametrize("n,k,f", [(1, 1, 1), (255, 3, 5), (257, 130, 8), (5000, 17, 37)])
def test_update_f64(n, k, f):
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(n + k + f)
    lab = torch.randint(0, k, (n,), generator=g)
    if k > 2:
        lab[lab == 1] = 0          # an empty cluster
        lab[n // 2] = k            # labels outside [0, k) are ignored
        lab[n // 3] = -1
    ok = (lab >= 0) & (lab < k)
    for x in (torch.randint(-8, 9, (n, f), generator=g).double(), torch.randn(n, f, generator=g, dtype=torch.float64)):
        ref = torch.zeros(k, f, dtype=torch.float64).index_add_(0, lab[ok], x[ok])
        cnt = torch.bincount(lab[ok], minlength=k).double()
        sums, counts = ops.kmeans_update_f64(x.to(dev), lab.to(dev).int(), k)
        assert sums.dtype == counts.dtype == torch.float64
        assert torch.equal(counts.cpu(), cnt)
        absum = torch.zeros(k, f, dtype=torch.float64).index_add_(0, lab[ok], x[ok].abs())
        assert torch.all((sums.cpu() - ref).abs() <= cnt[:, None] * U * absum)   # integers: the bound is 0
        again = ops.kmeans_update(x.to(dev), lab.to(dev).int(), k)                # the public op, second call
        assert torch.equal(again[0], sums) and torch.equal(again[1], counts)


def test_finalize_f64():
    from heat_amd import ops

    dev = _dev()
    k, f = 130, 37
    g = torch.Generator().manual_seed(5)
    C = torch.randn(k, f, generator=g, dtype=torch.float64)
    sums = torch.randn(k, f, generator=g, dtype=torch.float64) * 50
    counts = torch.randint(1, 90, (k,), generator=g).double()
    counts[7] = 0
    packed = torch.cat([sums.reshape(-1), counts])
    ref = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], C)
    for args in ((packed.to(dev), C.to(dev)), (None, C.to(dev), sums.to(dev), counts.to(dev))):
        newC, shift = ops.kmeans_finalize(*args)
        assert newC.dtype == torch.float64 and shift.dtype == torch.float64
        assert torch.allclose(newC.cpu(), ref, rtol=1e-14, atol=0) and torch.equal(newC[7].cpu(), C[7])
        assert torch.allclose(shift.cpu(), ((C - ref) ** 2).sum(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("k", [3, 130])
def test_kmeans_float64_public_route(gpu, monkeypatch, k):
    import heat_amd as ht
    from heat_amd.ops import kernels

    n, f = 5 * k + 20, 5
    x, c = _shifted(n, k, f)
    c0 = c + 0.1 * torch.randn(k, f, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
    C = c0.clone()
    for _ in range(5):           # CPU fp64 Lloyd from the same start
        lab = _d2(x, C).argmin(1)
        cnt = torch.bincount(lab, minlength=k).double()
        s = torch.zeros(k, f, dtype=torch.float64).index_add_(0, lab, x)
        C = torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1)[:, None], C)
    calls = []
    for name in ("kmeans_assign_f64", "kmeans_update_f64"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _n=name, _r=real, **kw: calls.append(_n) or _r(*a, **kw))
    X = ht.array(x.numpy(), device="gpu")
    assert X.dtype == ht.float64
    km = ht.cluster.KMeans(n_clusters=k, init=ht.array(c0.numpy(), device="gpu"), max_iter=5, tol=None).fit(X)
    assert km.cluster_centers_.dtype == ht.float64
    assert np.array_equal(km.labels_.numpy().ravel(), lab.numpy())
    assert np.allclose(km.cluster_centers_.numpy(), C.numpy(), rtol=1e-12, atol=0)
    assert np.array_equal(km.predict(X).numpy().ravel(), _d2(x, C).argmin(1).numpy())
    assert calls.count("kmeans_assign_f64") == 6 and calls.count("kmeans_update_f64") == 5
