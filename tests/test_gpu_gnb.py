"""The fused Gaussian naive Bayes kernels (csrc/gnb.hip) and the estimator on them, against NumPy
references in extended precision on the same values.

Moment bounds (summation error of n_c float64 terms, R = max |x - column mean|): counts exact for unit
weights, |mean - ref| <= n_c 2^-50 R, |M2 - ref| <= n_c^2 2^-50 R^2. Likelihood bound, elementwise:
|jll - ref| <= 2 (f + 4) u (0.5 quad + |sum log term| + |log prior|), u = 2^-24 / 2^-53; log_proba the same
plus k u; argmax equal to the reference wherever its top-two gap exceeds twice the bound."""
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


def _blobs(m, f, k, dtype, offset=0.0, empty=None):
    """m rows around k centres 8 sigma apart (unit spread), their classes (none in `empty`)."""
    rng = np.random.default_rng(1000 * m + 10 * f + k)
    y = rng.integers(0, k, m)
    if empty is not None:
        y[y == empty] = (empty + 1) % k
    x = rng.standard_normal((m, f)) + 8.0 * ((y[:, None] + np.arange(f)[None, :]) % k) + offset
    return x.astype(dtype), y


def _check_moments(got, a, y, k, w=None):
    cnt, mean, m2 = (np.asarray(g.cpu().numpy(), dtype=LD) for g in got)
    x = a.astype(LD)
    w = np.ones(len(y), dtype=LD) if w is None else w.astype(LD)
    R = np.abs(x - x.mean(axis=0)).max()
    for c in range(k):
        sel = y == c
        n_c, W = int(sel.sum()), w[sel].sum()
        mu = (x[sel] * w[sel, None]).sum(axis=0) / W if W > 0 else np.zeros(a.shape[1], dtype=LD)
        ref2 = ((x[sel] - mu) ** 2 * w[sel, None]).sum(axis=0)
        print(c, n_c, float(np.abs(mean[c] - mu).max()), float(np.abs(m2[c] - ref2).max()))
        assert cnt[c] == W   # unit weights and the test's halves sum exactly
        assert (np.abs(mean[c] - mu) <= n_c * LD(2) ** -50 * R).all(), c
        assert (np.abs(m2[c] - ref2) <= n_c ** 2 * LD(2) ** -50 * R ** 2).all(), c


# (m, f, k): row-group and batch tails, 16-feature block tails, class-tile edges; the last four run several
# chunks through both merge levels
MOMENT_CASES = [(1, 1, 1), (3, 7, 2), (67, 17, 16), (67, 64, 17), (4099, 130, 2), (4099, 64, 64), (4099, 7, 16),
                (40000, 17, 2), (40000, 64, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,f,k", MOMENT_CASES)
def test_class_moments(m, f, k, dtype):
    from heat_amd import ops

    a, y = _blobs(m, f, k, dtype)
    x, idx = torch.from_numpy(a).to(_dev()), torch.from_numpy(y).to(_dev())
    first, second = ops.class_moments(x, idx, k), ops.class_moments(x, idx, k)
    assert all(torch.equal(p, q) for p, q in zip(first, second))   # bit-identical run to run
    _check_moments(first, a, y, k)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["strided", "empty_class", "weights", "offset"])
def test_class_moments_variants(variant, dtype):
    """A strided row view, a class without rows, weights with zeros, and a common offset of 1e4 at unit
    spread (k = 1: unshifted sums miss the M2 bound by about five orders of magnitude)."""
    from heat_amd import ops

    m, f, k = 4099, 17, 3
    if variant == "offset":
        a = (np.random.default_rng(5).standard_normal((m, f)) + 1e4).astype(dtype)
        y = np.zeros(m, dtype=np.int64)
        k = 1
    else:
        a, y = _blobs(m, f, k, dtype, empty=1 if variant == "empty_class" else None)
    x = torch.from_numpy(a).to(_dev())
    w = None
    if variant == "strided":
        big = torch.zeros((m, f + 5), dtype=x.dtype, device=x.device)
        big[:, 3:3 + f] = x
        x = big[:, 3:3 + f]
        assert not x.is_contiguous()
    if variant == "weights":
        w = np.random.default_rng(6).integers(0, 3, m).astype(np.float64) / 2   # 0, 0.5, 1
        assert (w == 0).any()
    got = ops.class_moments(x, torch.from_numpy(y).to(x.device), k, None if w is None else torch.from_numpy(w).to(x.device))
    if variant == "empty_class":
        assert all(float(g[1].abs().max()) == 0.0 for g in got)
    _check_moments(got, a, y, k, w)


def _jll_ref(a, theta, sigma, log_prior):
    """(jll, elementwise bound without u) in extended precision from the rounded parameters."""
    x, th, sg, lp = (np.asarray(v).astype(LD) for v in (a, theta, sigma, log_prior))
    quad = ((x[:, None, :] - th[None]) ** 2 / sg[None]).sum(axis=2)
    logs = np.log(2 * LD(np.pi) * sg).sum(axis=1)
    jll = lp[None] - LD(0.5) * logs[None] - LD(0.5) * quad
    return jll, 2 * (a.shape[1] + 4) * (LD(0.5) * quad + np.abs(LD(0.5) * logs)[None] + np.abs(lp)[None])


def _lse(v):
    mx = v.max(axis=1, keepdims=True)
    return mx + np.log(np.exp(v - mx).sum(axis=1, keepdims=True))


# (m, f, k, variant)
JLL_CASES = [(1, 1, 1, None), (3, 7, 2, None), (67, 17, 16, None), (67, 130, 17, None), (4099, 64, 64, None),
             (4099, 33, 3, "tiny_sigma"), (4099, 9, 4, "tie"), (4099, 17, 3, "strided")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,f,k,variant", JLL_CASES)
def test_gnb_jll(m, f, k, variant, dtype):
    from heat_amd import ops

    u = LD(2) ** (-24 if dtype == np.float32 else -53)
    a, y = _blobs(m, f, k, dtype)
    rng = np.random.default_rng(f + k)
    theta = (8.0 * ((np.arange(k)[:, None] + np.arange(f)[None, :]) % k)).astype(dtype)
    sigma = rng.uniform(0.8, 1.25, (k, f)).astype(dtype)
    prior = rng.uniform(0.5, 1.0, k)
    log_prior = np.log(prior / prior.sum()).astype(dtype)
    if variant == "tiny_sigma":   # var_smoothing's floor: the expanded form cancels here
        sigma[:, 0] = 1e6
        sigma[1, 5] = 1e-3
    if variant == "tie":          # classes 1 and 3 identical: 1 must win over 3
        theta[3], sigma[3], log_prior[3] = theta[1], sigma[1], log_prior[1]
    x = torch.from_numpy(a).to(_dev())
    if variant == "strided":
        big = torch.zeros((m, f + 5), dtype=x.dtype, device=x.device)
        big[:, 3:3 + f] = x
        x = big[:, 3:3 + f]
    th, sg, lp = (torch.from_numpy(v).to(x.device) for v in (theta, sigma, log_prior))
    ref, bound = _jll_ref(a, theta, sigma, log_prior)

    jll = np.asarray(ops.gnb_jll(x, th, sg, lp, out="jll").cpu().numpy(), dtype=LD)
    print("jll", float((np.abs(jll - ref) / (bound * u)).max()))
    assert jll.shape == (m, k) and (np.abs(jll - ref) <= bound * u).all()

    logp = np.asarray(ops.gnb_jll(x, th, sg, lp, out="log_proba").cpu().numpy(), dtype=LD)
    lbound = bound * u + k * u
    print("log_proba", float((np.abs(logp - (ref - _lse(ref))) / lbound).max()))
    assert (np.abs(logp - (ref - _lse(ref))) <= lbound).all()
    assert (np.abs(_lse(logp)) <= lbound.min(axis=1, keepdims=True)).all()

    lab = ops.gnb_jll(x, th, sg, lp, out="argmax")
    assert lab.dtype == torch.int64 and lab.shape == (m,)
    lab = lab.cpu().numpy()
    if variant == "tie":
        assert not (lab == 3).any() and (lab == 1).any()
        ref[:, 3] = -np.inf
        bound[:, 3] = 0
    top2 = np.sort(ref, axis=1)[:, -2:] if k > 1 else np.stack([np.full(m, -np.inf, dtype=LD), ref[:, 0]], axis=1)
    sure = top2[:, 1] - top2[:, 0] > 2 * bound.max(axis=1) * u
    assert sure.mean() >= 0.99
    assert (lab[sure] == ref.argmax(axis=1)[sure]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussiannb_device_end_to_end(gpu, dtype):
    """fit / predict / predict_log_proba on device data against the same estimator on the host copy; the
    fused kernels must have run (this fails before csrc/gnb.hip)."""
    import heat_amd as ht
    from heat_amd.core.communication import PATH_COUNTS

    a, y = _blobs(2000, 9, 3, dtype)
    xd, yd = ht.array(a), ht.array(y)
    assert xd.larray.is_cuda
    before = dict(PATH_COUNTS)
    dev = ht.naive_bayes.GaussianNB().fit(xd, yd)
    lab, logp = dev.predict(xd), dev.predict_log_proba(xd)
    assert PATH_COUNTS["gnb_fit:native"] == before.get("gnb_fit:native", 0) + 1
    assert PATH_COUNTS["gnb_predict:native"] == before.get("gnb_predict:native", 0) + 2
    host = ht.naive_bayes.GaussianNB().fit(ht.array(a, device="cpu"), ht.array(y, device="cpu"))
    n_c, R = np.bincount(y).max(), np.abs(a.astype(LD) - a.astype(LD).mean(axis=0)).max()
    ulp = float(np.finfo(dtype).eps)   # theta_ and sigma_ are kept in the data's type
    for name, tol in (("theta_", n_c * 2.0 ** -50 * R), ("sigma_", n_c * 2.0 ** -50 * R ** 2), ("class_prior_", 0.0)):
        d, h = (getattr(e, name).larray.cpu().numpy().astype(LD) for e in (dev, host))
        assert (np.abs(d - h) <= 2 * float(tol) + ulp * np.abs(h)).all(), name
    ref, bound = _jll_ref(a, host.theta_.larray.numpy(), host.sigma_.larray.numpy(),
                          np.log(host.class_prior_.larray.numpy()))
    u = LD(2) ** (-24 if dtype == np.float32 else -53)
    top2 = np.sort(ref, axis=1)[:, -2:]
    sure = top2[:, 1] - top2[:, 0] > 2 * bound.max(axis=1) * u
    assert sure.mean() >= 0.99
    assert (lab.larray.cpu().numpy()[sure] == host.predict(ht.array(a, device="cpu")).larray.numpy()[sure]).all()
    assert logp.larray.dtype == xd.larray.dtype and logp.shape == (2000, 3)
    assert (np.abs(_lse(logp.larray.cpu().numpy().astype(LD))) <= (bound.min(axis=1, keepdims=True) + 3) * u).all()
