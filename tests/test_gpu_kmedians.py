"""Native k-medians / k-medoids kernels (csrc/kmedians.hip) against plain float64 CPU references:
ops.l1_assign, ops.l1_to_label, ops.cluster_medians and the two estimators on device data."""
import numpy as np
import pytest
import torch

import heat_amd as ht
from heat_amd import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]


def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _int_case(n, f, k, dtype, seed=0):
    """Integer-valued points and centroids in [-8, 8] (every sum exact in both precisions), centroid
    row 0 repeated at the end and every 7th point equal to a centroid; float64 L1 matrix on the CPU."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-8, 9, (n, f), generator=g).to(dtype)
    C = torch.randint(-8, 9, (k, f), generator=g).to(dtype)
    if k > 1:
        C[k - 1] = C[0]
    X[::7] = C[torch.arange(0, n, 7) % k]
    d = torch.stack([(X.double() - c.double()).abs().sum(1) for c in C], 1)
    return X, C, d


def _shapes():
    L = ops.lib()
    return [(1, 1, 1), (129, 3, 2), (257, 18, 17), (1000, 65, 130), (200, 5, L.ha_l1_centroid_tile(64) + 1),
            (L.ha_l1_point_block() + 1, 7, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_assign_exact(dtype):
    dev = _native()
    for n, f, k in _shapes():
        X, C, d = _int_case(n, f, k, dtype)
        lab, mind = ops.l1_assign(X.to(dev), C.to(dev))
        assert lab.dtype == torch.int32 and torch.equal(lab.cpu().long(), torch.argmin(d, 1)), (n, f, k)
        assert torch.equal(mind.cpu().double(), d.min(1).values), (n, f, k)
    # row-strided view whose last row ends at the end of its allocation
    X, C, d = _int_case(300, 128, 8, dtype)
    flat = torch.zeros(299 * 131 + 128, dtype=dtype, device=dev)
    view = flat.as_strided((300, 128), (131, 1))
    view.copy_(X)
    lab, mind = ops.l1_assign(view, C.to(dev))
    assert torch.equal(lab.cpu().long(), torch.argmin(d, 1)) and torch.equal(mind.cpu().double(), d.min(1).values)
    assert ops.l1_assign(view, C.to(dev), want_mind=False)[1] is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_assign_rounded(dtype):
    dev = _native()
    n, f, k = 1000, 65, 130
    g = torch.Generator().manual_seed(1)
    X, C = torch.randn(n, f, generator=g).to(dtype), torch.randn(k, f, generator=g).to(dtype)
    d1 = torch.stack([(X.double() - c.double()).abs().sum(1) for c in C], 1)
    lab, mind = ops.l1_assign(X.to(dev), C.to(dev))
    u = torch.finfo(dtype).eps / 2
    chosen = d1.gather(1, lab.cpu().long().unsqueeze(1)).squeeze(1)
    assert bool((chosen <= d1.min(1).values * (1 + 8 * (f + 2) * u)).all())
    assert bool(((mind.cpu().double() - chosen).abs() <= 4 * (f + 2) * u * chosen).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_to_label(dtype):
    dev = _native()
    for n, f, k in _shapes():
        X, M, d = _int_case(n, f, k, dtype)
        lab = torch.randint(0, k, (n,), generator=torch.Generator().manual_seed(2))
        got = ops.l1_to_label(X.to(dev), M.to(dev), lab.to(dev))
        assert got.dtype == dtype and torch.equal(got.cpu().double(), d.gather(1, lab.unsqueeze(1)).squeeze(1)), (n, f, k)


def _median_ref(X, lab, k):
    Xd, lab = X.double().numpy(), lab.numpy()
    med = np.zeros((k, X.shape[1]))
    for c in range(k):
        if (lab == c).any():
            med[c] = np.median(Xd[lab == c], axis=0)
    return torch.from_numpy(med).to(X.dtype), np.bincount(lab, minlength=k)


def _median_cases(dtype):
    g = torch.Generator().manual_seed(3)
    seg = ops.lib().ha_med_segment()
    for f in (1, 3, 64, 65):
        # odd and even sizes, an empty cluster (2), a one-member cluster (3)
        lab = torch.cat([torch.zeros(101), torch.ones(100), torch.full((1,), 3), torch.randint(4, 6, (300,), generator=g)])
        yield "sizes f={}".format(f), torch.randn(len(lab), f, generator=g).to(dtype), lab.long(), 6
    yield "one cluster", torch.randn(500, 5, generator=g).to(dtype), torch.zeros(500).long(), 3
    five = torch.tensor([-2.5, -0.0, 0.0, 1.0, 3.0])
    yield "five values", five[torch.randint(0, 5, (1000, 6), generator=g)].to(dtype), torch.randint(0, 4, (1000,), generator=g), 4
    yield "shared entry", torch.randn(2 * seg + 101, 3, generator=g).to(dtype), \
        torch.cat([torch.zeros(2 * seg + 1), torch.ones(100)]).long(), 2
    if dtype == torch.float64:
        fine = 1 + torch.randperm(600, generator=g).double().reshape(200, 3) * 2.0 ** -52
        yield "all digits", fine, torch.randint(0, 2, (200,), generator=g), 2
    else:
        wide = torch.randn(400, 4, generator=g) * 10.0 ** (torch.rand(400, 4, generator=g) * 60 - 30)
        yield "full range", wide.float(), torch.randint(0, 3, (400,), generator=g), 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_medians_exact(dtype):
    dev = _native()
    for name, X, lab, k in _median_cases(dtype):
        want, cnt = _median_ref(X, lab, k)
        med, counts = ops.cluster_medians(X.to(dev), lab.to(dev), k)
        assert med.dtype == dtype and counts.dtype == torch.float64
        assert np.array_equal(counts.cpu().numpy(), cnt), name
        live = torch.from_numpy(cnt > 0)
        assert torch.equal(med.cpu()[live], want[live]), name

        # two identical ranks: sums double, maxima stay
        def twice(t, op):
            if op == "sum":
                t.mul_(2)

        want2, cnt2 = _median_ref(torch.cat([X, X]), torch.cat([lab, lab]), k)
        med2, counts2 = ops.cluster_medians(X.to(dev), lab.to(dev), k, allreduce=twice)
        assert np.array_equal(counts2.cpu().numpy(), cnt2), name
        assert torch.equal(med2.cpu()[live], want2[live]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("est", ["KMedians", "KMedoids"])
def test_estimators_match_host_path(dtype, est):
    _native()
    g = torch.Generator().manual_seed(4)
    blobs = torch.cat([torch.randint(-3, 4, (150, 5), generator=g) + 40 * b for b in range(3)]).to(dtype)
    blobs = blobs[torch.randperm(len(blobs), generator=g)]
    init = torch.stack([torch.full((5,), 40.0 * b + 1) for b in range(3)]).to(dtype)
    fits = []
    for device in ("cpu", "gpu"):
        x = ht.array(blobs, device=device)
        assert x.larray.is_cuda == (device == "gpu")
        kw = dict(n_clusters=3, init=ht.array(init, device=device), max_iter=3)
        model = ht.cluster.KMedians(tol=None, **kw) if est == "KMedians" else ht.cluster.KMedoids(**kw)
        model.fit(x)
        fits.append((model.cluster_centers_.larray.cpu(), model.labels_.larray.cpu(), model.predict(x).larray.cpu()))
    for host, dev in zip(*fits):
        assert torch.equal(host, dev)
