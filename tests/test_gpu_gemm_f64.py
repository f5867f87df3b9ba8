"""Native fp64 MFMA GEMM (``ops/csrc/gemm_f64.hip``) against the fp64 torch product on the CPU: every
operand layout, tile / stage / ring edges, epilogue modes, upper tiles, split-K and the public route."""
import pytest
import torch

pytestmark = pytest.mark.gpu
_LAYOUTS = ["nn", "tn", "nt", "tt"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _bound(a, b):
    # both sides carry at most K u |a||b| of rounding (u = 2^-53); doubled like test_gpu_gemm._bound
    return 4 * a.shape[1] * 2.0 ** -53 * (a.abs() @ b.abs()) + 1e-300


@pytest.mark.parametrize("m,k,n", [(1, 7, 1), (129, 1, 131), (256, 16, 256), (130, 32, 260), (130, 40, 260),
                                   (300, 257, 129), (2000, 34, 6), (64, 4096, 64), (513, 1024, 257)])
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_gemm_f64_layouts(m, k, n, layout):
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(m * 7 + k * 3 + n)
    a = torch.randn(m, k, generator=g, dtype=torch.float64)
    b = torch.randn(k, n, generator=g, dtype=torch.float64)
    A = a.to(dev) if layout[0] == "n" else a.t().contiguous().to(dev).t()
    B = b.to(dev) if layout[1] == "n" else b.t().contiguous().to(dev).t()
    err = (ops.gemm_f64(A, B).cpu() - a @ b).abs()
    assert torch.all(err <= _bound(a, b)), err.max()


@pytest.mark.parametrize("m,k,n", [(257, 300, 191), (258, 300, 192)])
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_gemm_f64_exact_integers(m, k, n, layout):
    """Integer operands: every product and partial sum is exact, so a transposed or permuted
    fragment map or an A/B k-slot disagreement changes the result outright. The odd shape runs the
    pipelined kernel for ``nt`` only (odd leading dimensions take the gemm64 fallback), the even
    one for all four layouts."""
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-8, 9, (m, k), generator=g).double()
    b = torch.randint(-8, 9, (k, n), generator=g).double()
    A = a.to(dev) if layout[0] == "n" else a.t().contiguous().to(dev).t()
    B = b.to(dev) if layout[1] == "n" else b.t().contiguous().to(dev).t()
    assert torch.equal(ops.gemm_f64(A, B).cpu(), a @ b)


@pytest.mark.parametrize("mode", ["accumulate", "rowblock", "alpha"])
def test_gemm_f64_epilogue(mode):
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(5)
    a = torch.randn(300, 200, generator=g, dtype=torch.float64)
    b = torch.randn(200, 140, generator=g, dtype=torch.float64)
    A, B = a.to(dev), b.to(dev)
    ref, bound = a @ b, _bound(a, b)
    if mode == "accumulate":
        c = ops.gemm_f64(A, B, out=torch.ones(300, 140, dtype=torch.float64, device=dev), accumulate=True).cpu()
        ref = 1 + ref
    elif mode == "rowblock":
        big = torch.zeros(700, 140, dtype=torch.float64, device=dev)
        ops.gemm_f64(A, B, out=big[200:500])
        assert torch.all(big[:200] == 0) and torch.all(big[500:] == 0)
        c = big[200:500].cpu()
    else:
        # slice views, both operands k-contiguous with an even leading dimension and an odd K
        a, b = a[:, :199], b[:199]
        c = ops.gemm_f64(A[:, :199], B.t().contiguous().t()[:199], alpha=-0.5).cpu()
        ref, bound = -0.5 * (a @ b), 0.5 * _bound(a, b)
    assert torch.all((c - ref).abs() <= bound), (c - ref).abs().max()


@pytest.mark.parametrize("n", [300, 130])
def test_gemm_f64_upper(n):
    from heat_amd import ops

    dev = _dev()
    x = torch.randn(1500, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    X = x.to(dev)
    out = torch.full((n, n), -7.25, dtype=torch.float64, device=dev)
    c = ops.gemm_f64(X.t(), X, out=out, upper=True).cpu()
    up = torch.ones(n, n, dtype=torch.bool).triu()
    assert torch.all(((c - x.t() @ x).abs() <= _bound(x.t(), x))[up])
    assert torch.all(c[~up] == -7.25)


@pytest.mark.parametrize("k", [20003, 20004])
@pytest.mark.parametrize("layout", ["nn", "tn"])
def test_gemm_f64_splitk(layout, k):
    """(20003, nn) has an odd lda and runs the gemm64 fallback, which ignores ``slices``; the other
    three cases run the split-K kernel."""
    from heat_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(11)
    a = torch.randn(256, k, generator=g, dtype=torch.float64)
    b = torch.randn(k, 128, generator=g, dtype=torch.float64)
    A = a.to(dev) if layout[0] == "n" else a.t().contiguous().to(dev).t()
    B = b.to(dev)
    c = ops.gemm_f64(A, B, slices=5)
    assert torch.all((c.cpu() - a @ b).abs() <= _bound(a, b))
    assert torch.equal(ops.gemm_f64(A, B, slices=5), c)


def test_gemm_f64_splitk_default():
    from heat_amd import ops

    dev = _dev()
    assert ops.lib().ha_gemm_f64_slices(512, 512, 200000, ops.num_cus(dev)) > 1
    g = torch.Generator().manual_seed(13)
    a = torch.randn(512, 200000, generator=g, dtype=torch.float64)
    b = torch.randn(200000, 512, generator=g, dtype=torch.float64)
    assert torch.all((ops.gemm_f64(a.to(dev), b.to(dev)).cpu() - a @ b).abs() <= _bound(a, b))


def test_float64_matmul_and_cov_route_to_gemm_f64(gpu):
    import numpy as np
    import heat_amd as ht
    import heat_amd.ops as _ops

    rng = np.random.default_rng(2)
    a, b, x = rng.normal(size=(700, 300)), rng.normal(size=(300, 520)), rng.normal(size=(600, 3000))
    p, q = rng.normal(size=(512, 8192)), rng.normal(size=(8192, 512))
    calls = []
    real = _ops.gemm_f64

    def spy(*args, **kw):
        calls.append(args[0].dtype)
        return real(*args, **kw)

    _ops.gemm_f64 = spy
    try:
        for sa, sb in ((None, None), (0, None), (None, 1)):
            A, B = ht.array(a, split=sa, device="gpu"), ht.array(b, split=sb, device="gpu")
            assert A.dtype == ht.float64
            # 30 output tiles and K = 300: the measured library rule (basics._library_better_f64)
            assert np.allclose(ht.matmul(A, B).numpy(), a @ b, rtol=1e-12)
            # 16 output tiles and a deep K: the kernel's split-K class, every split case
            n = len(calls)
            P, Q = ht.array(p, split=sa, device="gpu"), ht.array(q, split=sb, device="gpu")
            assert np.allclose(ht.matmul(P, Q).numpy(), p @ q, rtol=1e-12)
            assert len(calls) > n
        n = len(calls)
        assert np.allclose(ht.cov(ht.array(x, device="gpu")).numpy(), np.cov(x), rtol=1e-12)
        assert len(calls) > n and all(d == torch.float64 for d in calls)
        n = len(calls)
        ht.matmul(ht.array(a.astype(np.float32), device="gpu"), ht.array(b.astype(np.float32), device="gpu"))
        assert len(calls) == n
    finally:
        _ops.gemm_f64 = real
