"""Fused float64 k-nearest-neighbour kernels (``ops/csrc/knn_f64.hip`` behind ``ops.cdist_f64(..., topk=k)``,
``ops.knn_topk``, ``ht.spatial.cdist_topk`` and ``ht.classification.KNeighborsClassifier``) against plain
broadcast fp64 on the CPU with a stable argsort: fragment map, list insertion across lane groups and
tiles, ring / tail / odd-f edges, nt < 128, the split merge and the tie rule on exact integers; random
and far-shifted data whose own margins exclude a changed neighbour; strided views."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _ref(q, t, k):
    d2 = ((q[:, None] - t[None]) ** 2).sum(-1)
    order = torch.from_numpy(np.argsort(d2.numpy(), axis=1, kind="stable"))
    return d2, order[:, :k], torch.gather(d2, 1, order[:, :k + 1])


def _shifted(n, seed):
    """130 unit-spaced grid centres (5 features) shifted by 1e3 per coordinate, n rows 0.05 around them."""
    j = torch.arange(130)
    c = torch.zeros(130, 5, dtype=torch.float64)
    for a in range(4):
        c[:, a] = (j // 6 ** a) % 6
    c += 1e3
    return c[torch.arange(n) % 130] + 0.05 * torch.randn(n, 5, generator=torch.Generator().manual_seed(seed),
                                                         dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _data(kind, nq, nt, f, k):
    if kind == "shifted":
        q, t = _shifted(nq, 1), _shifted(nt, 2)
    elif kind == "int":   # every third row of T a copy of an earlier one: exact scores, massive ties
        g = torch.Generator().manual_seed(nq + nt + f)
        q = torch.randint(-8, 9, (nq, f), generator=g).double()
        t = torch.randint(-8, 9, (nt, f), generator=g).double()
        for j in range(2, nt, 3):
            t[j] = t[j // 2]
    else:
        g = torch.Generator().manual_seed(nq + 3 * nt + 7 * f)
        q = torch.randn(nq, f, generator=g, dtype=torch.float64)
        t = torch.randn(nt, f, generator=g, dtype=torch.float64)
    return (q, t) + _ref(q, t, k)


def _margin_ok(q, t, dk):
    """The reference's gaps among each query's first k + 1 distances exceed twice the expansion bound
    b_i = 4 (f + 2) u (|q_i|^2 + max |t_j|^2) of test_gpu_kmeans_f64.py: no neighbour can change."""
    b = 4 * (q.shape[1] + 2) * U * ((q * q).sum(1) + (t * t).sum(1).max())
    return bool(torch.all((dk[:, 1:] - dk[:, :-1]).min(1).values > 2 * b))


@pytest.mark.parametrize("nq,nt,f,k,splits", [
    (1, 1, 1, 1, None), (129, 1, 3, 1, None), (130, 17, 7, 8, None), (257, 129, 8, 16, None), (300, 130, 9, 5, None),
    (128, 256, 32, 16, None), (200, 260, 37, 3, None), (64, 300, 200, 16, None), (5, 3000, 12, 8, None),
    (5, 3000, 12, 8, 4)])
def test_knn_f64_exact_integers(nq, nt, f, k, splits):
    from heat_amd import ops

    dev = _dev()
    q, t, d2, idx, dk = _data("int", nq, nt, f, min(k, nt))
    dist, ind = ops.cdist_f64(q.to(dev), t.to(dev), "sqeuclidean", topk=k, _splits=splits)
    assert dist.dtype == torch.float64 and ind.dtype == torch.int64 and dist.shape == ind.shape == (nq, k)
    assert torch.equal(ind.cpu(), idx) and torch.equal(dist.cpu(), dk[:, :k])
    root = ops.cdist_f64(q.to(dev), t.to(dev), "euclidean", topk=k)
    assert torch.equal(root[1].cpu(), idx) and torch.allclose(root[0].cpu(), dk[:, :k].sqrt(), rtol=2 * U, atol=0)


def test_knn_f64_padding_and_arguments():
    from heat_amd import ops

    dev = _dev()
    q, t, d2, idx, dk = _data("int", 10, 3, 4, 3)
    dist, ind = ops.knn_topk(q.to(dev), t.to(dev), 5)
    assert torch.equal(ind[:, :3].cpu(), idx) and torch.equal(dist[:, :3].cpu(), dk)
    assert torch.all(ind[:, 3:] == -1) and torch.all(torch.isinf(dist[:, 3:])) and dist.dtype == torch.float64
    for bad in (dict(metric="manhattan"), dict(out=torch.empty(10, 3, dtype=torch.float64, device=dev)),
                dict(symmetric=True), dict(topk=17)):
        with pytest.raises(ValueError):
            ops.cdist_f64(q.to(dev), t.to(dev), **{"metric": "sqeuclidean", "topk": 2, **bad})


@pytest.mark.parametrize("nq,nt,f,k", [(300, 260, 37, 16), (257, 129, 8, 16), (64, 300, 200, 16)])
def test_knn_f64_random(nq, nt, f, k):
    from heat_amd import ops

    dev = _dev()
    q, t, d2, idx, dk = _data("random", nq, nt, f, k)
    assert _margin_ok(q, t, dk)
    dist, ind = ops.cdist_f64(q.to(dev), t.to(dev), "sqeuclidean", topk=k)
    assert torch.equal(ind.cpu(), idx)
    assert torch.all((dist.cpu() - dk[:, :k]).abs() <= 4 * (f + 2) * U * dk[:, :k])


def test_knn_f64_shifted_public_routes(gpu):
    """Offset 1e3 against unit spacing: a float32 copy of the operands changes neighbours, float64 may not."""
    import heat_amd as ht
    from heat_amd import ops

    dev = _dev()
    q, t, d2, idx, dk = _data("shifted", 400, 390, 5, 8)
    assert _margin_ok(q, t, dk)
    dist, ind = ops.knn_topk(q.to(dev), t.to(dev), 8)
    assert dist.dtype == torch.float64 and torch.equal(ind.cpu(), idx)
    votes = torch.nn.functional.one_hot(idx % 7, 7).sum(1)
    knn = ht.classification.KNeighborsClassifier(n_neighbors=8)
    knn.fit(ht.array(t.numpy(), device="gpu"), ht.array((np.arange(390) % 7), device="gpu"))
    pred = torch.from_numpy(knn.predict(ht.array(q.numpy(), device="gpu")).numpy()).reshape(-1, 1)
    assert torch.equal(votes.gather(1, pred)[:, 0], votes.max(1).values)
    d, i = ht.spatial.cdist_topk(ht.array(q.numpy(), device="gpu"), ht.array(t.numpy(), device="gpu"), k=8)
    assert d.dtype == ht.float64 and np.array_equal(i.numpy(), idx.numpy())


def test_knn_f64_strided_views():
    """Q a column slice of a wider tensor with an odd leading dimension, T every other row."""
    from heat_amd import ops

    dev = _dev()
    nq, nt, f, k = 200, 260, 37, 3
    q, t, d2, idx, dk = _data("random", nq, nt, f, k)
    Q = torch.zeros((nq, f + 4), dtype=torch.float64, device=dev)[:, 1:f + 1]
    Q.copy_(q)
    T = torch.zeros((2 * nt, f), dtype=torch.float64, device=dev)[::2]
    T.copy_(t)
    assert Q.stride(0) % 2 == 1 and not T.is_contiguous() and _margin_ok(q, t, dk)
    dist, ind = ops.cdist_f64(Q, T, "sqeuclidean", topk=k)
    assert torch.equal(ind.cpu(), idx)
    assert torch.all((dist.cpu() - dk[:, :k]).abs() <= 4 * (f + 2) * U * dk[:, :k])
