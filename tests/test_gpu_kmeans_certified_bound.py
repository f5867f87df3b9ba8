"""Per-centroid certificate of the one-term k-means filter (``ops.kmeans_assign(certified=True)``):
rigour where centroid norms differ by orders of magnitude, exact ties, and the fraction of points
it leaves to the 3-term re-check at a benchmark-like shape. Every reference is fp64 torch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from heat_amd import ops

    assert ops.available(), "native library must load on a GPU box"
    return torch.device("cuda", 0)


def _certified(X, C):
    """(certified labels, re-checked count, full-kernel labels) of the device tensors X, C."""
    from heat_amd import ops

    packed = ops.kmeans_pack_points(X)
    lab, mind = ops.kmeans_assign(X, C, want_mind=False, packed=packed, certified=True)
    assert mind is None
    nre = int(ops.kmeans_assign.last_rechecked.item())
    full, _ = ops.kmeans_assign(X, C, want_mind=True, packed=packed)
    return lab, nre, full


def _assert_minimal(X, C, lab):
    """d(x, c_label) - d_min <= 2e-6 (|x|^2 + max |c|^2) in fp64, for every point."""
    Xd, Cd = X.double(), C.double()
    d = torch.cdist(Xd, Cd) ** 2
    ref_min, _ = d.min(1)
    chosen = d.gather(1, lab.long().unsqueeze(1)).squeeze(1)
    tol = 2e-6 * ((Xd * Xd).sum(1) + (Cd * Cd).sum(1).max())
    assert torch.all(chosen - ref_min <= tol), (chosen - ref_min - tol).max()


def _pow2_scale(mx):
    """2^-e with mx 2^-e in [0.5, 1) (1 where mx == 0): the kernels' row scale."""
    _, e = torch.frexp(mx)
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), -e), torch.ones_like(mx))


def _one_term_scores(X, C):
    """s_x (x.c - |c|^2 / 2) from the fp16 hi planes of the power-of-two scaled rows only, summed in
    fp64: what the filter's single MFMA term sees."""
    sx = _pow2_scale(X.abs().amax(1))
    sc = _pow2_scale(C.abs().amax(1))
    hx = (X * sx.unsqueeze(1)).half().double()
    hc = (C * sc.unsqueeze(1)).half().double() / sc.double().unsqueeze(1)
    return hx @ hc.T - sx.double().unsqueeze(1) * (0.5 * (C.double() ** 2).sum(1))


@pytest.mark.parametrize("f", [64, 100])
def test_rigour_heterogeneous_norms(f):
    """n = 300 (one full and one partial workgroup), k = 129 (two centroid chunks, the second
    nearly all padding), centroid norms over 1e-3 .. 1e3. Half the points sit next to the bisector
    of a large-norm centroid b and its nearest competitor a there (a smaller-norm one), on either
    side at a relative distance eps, 2e-5 <= |eps| <= 1e-4: the two scores differ by eps |b - a|^2,
    a fraction of the one-term error bound (2^-10) and of the same size as the one-term error
    itself, so the hi-only scores mis-order some pairs - a filter that certified them would label
    them wrongly. The gap is still above the 3-term kernel's worst case ((f + 5) 2^-24 + 3 2^-22 of
    |x||c| + u for both centroids, about 1.1e-5 |b|^2 at f = 100 against >= 1.6e-5 |b|^2), so the
    labels of these points must be EXACTLY the fp64 argmin. The other half are normal points at
    random scales."""
    dev = _dev()
    n, k = 300, 129
    g = torch.Generator(device="cpu").manual_seed(1000 + f)
    scales = torch.logspace(-3, 3, k, dtype=torch.float64)[torch.randperm(k, generator=g)]
    C = (torch.randn(k, f, generator=g, dtype=torch.float64) * scales.unsqueeze(1)).float().double()
    large = scales.argsort()[k - k // 2:]
    half = n // 2
    b = large[torch.randint(0, large.numel(), (half,), generator=g)]
    x0 = 0.5 * C[b] + torch.randn(half, f, generator=g, dtype=torch.float64) * scales[b].unsqueeze(1) * 0.1
    d0 = torch.cdist(x0, C) ** 2
    d0[torch.arange(half), b] = float("inf")
    a = d0.argmin(1)                                   # b's nearest competitor at x0
    dirv = C[b] - C[a]
    w = x0 - 0.5 * (C[a] + C[b])
    w -= (w * dirv).sum(1, keepdim=True) / (dirv * dirv).sum(1, keepdim=True) * dirv   # onto the bisector
    eps = (2e-5 + 8e-5 * torch.rand(half, 1, generator=g, dtype=torch.float64)) * \
        (torch.randint(0, 2, (half, 1), generator=g) * 2 - 1)
    near = 0.5 * (C[a] + C[b]) + w + eps * dirv
    rest = torch.randn(n - half, f, generator=g, dtype=torch.float64) * \
        scales[torch.randint(0, k, (n - half,), generator=g)].unsqueeze(1)
    perm = torch.randperm(n, generator=g)
    X = torch.cat([near, rest])[perm].float()
    pos = torch.empty(n, dtype=torch.long)
    pos[perm] = torch.arange(n)
    pos = pos[:half]                                   # rows of the near points in X
    # preconditions, in fp64 on the float32 inputs: the pair really is the top two, with the
    # intended gap, and the one-term scores get some of these points wrong
    d = torch.cdist(X.double(), C) ** 2
    top = d[pos].topk(3, dim=1, largest=False)
    pair = ((top.indices[:, :2] == a.unsqueeze(1)) | (top.indices[:, :2] == b.unsqueeze(1))).all(1)
    rel_gap = (top.values[:, 1] - top.values[:, 0]) / (2 * (dirv * dirv).sum(1))
    pair &= (rel_gap >= 1.9e-5) & (rel_gap <= 1.01e-4)
    pair &= (C[a].norm(dim=1) <= 0.5 * C[b].norm(dim=1))
    hard = pos[pair]
    ref = d.argmin(1)
    one_term = _one_term_scores(X, C.float()).argmax(1)
    misordered = int((one_term[hard] != ref[hard]).sum())
    print("pairs that are the fp64 top two: {} of {}, mis-ordered by one term: {}".format(hard.numel(), half, misordered))
    assert hard.numel() >= 100, hard.numel()
    assert misordered >= 5, misordered
    X, Cf = X.to(dev), C.float().to(dev)
    lab, nre, full = _certified(X, Cf)
    assert 0 <= nre <= n
    _assert_minimal(X, Cf, lab)
    assert torch.equal(lab[hard.to(dev)].long().cpu(), ref[hard]), "a near-bisector point is mislabelled"
    assert (lab == full).float().mean() >= 0.999


def test_exact_ties():
    """Every centroid has an exact duplicate: no point can be certified, and the re-checked labels
    are minimal."""
    dev = _dev()
    n, k, f = 1000, 64, 64
    g = torch.Generator(device="cpu").manual_seed(77)
    C = torch.randn(k, f, generator=g)
    C[1::2] = C[0::2]
    X = torch.cat([torch.randn(n // 2, f, generator=g), C[torch.randint(0, k, (n - n // 2,), generator=g)]])
    X, C = X.to(dev), C.to(dev)
    lab, nre, full = _certified(X, C)
    assert nre == n, nre
    _assert_minimal(X, C, lab)
    assert (lab == full).float().mean() >= 0.999


def _bf16_up(x):
    """Non-negative fp32 rounded up to bf16 (kept as fp32)."""
    bits = x.float().contiguous().view(torch.int32)
    return (((bits + 0xFFFF) >> 16) << 16).view(torch.float32)


def _model_uncertain(X, C):
    """Fraction of points the documented per-centroid bound leaves uncertain: scores from the fp16
    hi planes of the power-of-two scaled rows (fp64 sums),
    E_c(x) = xn g_c + s_x 2^-14 u_c with g_c = 1.08 2^-10 |c|, every factor rounded up to bf16 as in
    the kernel, certified iff U_b - 2 E_b > max_{c != b} U_c for b = argmax U, U = score + E."""
    sx = _pow2_scale(X.abs().amax(1))
    sc = _pow2_scale(C.abs().amax(1))
    hx = (X * sx.unsqueeze(1)).half().double()
    hc = (C * sc.unsqueeze(1)).half().double()
    sq = (C.double() ** 2).sum(1)
    xn = _bf16_up((hx.norm(dim=1) * (1 + 2.0 ** -10 + 2.0 ** -9)).float()).double()
    gc = _bf16_up((1.08 * 2.0 ** -10 * sq.sqrt() * sc.double()).float()).double() / sc.double()
    uc = _bf16_up((2.0 ** -15 * sq * sc.double()).float()).double() / sc.double()
    unc = 0
    for i in range(0, X.shape[0], 8192):
        s = slice(i, i + 8192)
        score = hx[s] @ (hc / sc.double().unsqueeze(1)).T - sx[s].double().unsqueeze(1) * (0.5 * sq)
        E = xn[s].unsqueeze(1) * gc + sx[s].double().unsqueeze(1) * uc
        top, idx = (score + E).topk(2, dim=1)
        unc += int((~(top[:, 0] - 2 * E.gather(1, idx[:, :1]).squeeze(1) > top[:, 1])).sum())
    return unc / X.shape[0]


@pytest.fixture(scope="module")
def bench_like():
    """65536 x 64 standard normal points; 1024 of them as centroids, and the centroids after one
    fp64 Lloyd update (empty clusters keep theirs)."""
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(4242)
    X = torch.randn(65536, 64, generator=g).to(dev)
    C0 = X[torch.randperm(X.shape[0], generator=g)[:1024].to(dev)].clone()
    Xd = X.double()
    lab = torch.cdist(Xd, C0.double()).argmin(1)
    sums = torch.zeros(1024, 64, dtype=torch.float64, device=dev).index_add_(0, lab, Xd)
    cnt = torch.zeros(1024, dtype=torch.float64, device=dev).index_add_(0, lab, torch.ones_like(lab, dtype=torch.float64))
    C1 = torch.where(cnt.unsqueeze(1) > 0, sums / cnt.clamp(min=1).unsqueeze(1), C0.double()).float()
    return X, C0, C1


@pytest.mark.parametrize("which", ["init", "updated"])
def test_effectiveness_benchmark_shape(bench_like, which):
    """The filter leaves no more points to the re-check than its documented bound (plus 2 % for
    points the fp32 accumulation order moves across the threshold), and that bound leaves at most
    10 % - a bound built on the largest centroid norm leaves 12.9 % after the update."""
    X, C0, C1 = bench_like
    C = C0 if which == "init" else C1
    n = X.shape[0]
    q_model = _model_uncertain(X, C)
    lab, nre, full = _certified(X, C)
    print("q_model {:.4f} rechecked {:.4f}".format(q_model, nre / n))
    assert q_model <= 0.10, q_model
    assert nre / n <= q_model + 0.02, (nre / n, q_model)
    # and no fewer (same slack): a kernel that charges less than the documented bound is not rigorous
    assert nre / n >= q_model - 0.02, (nre / n, q_model)
    _assert_minimal(X, C, lab)
    assert (lab == full).float().mean() >= 0.999
