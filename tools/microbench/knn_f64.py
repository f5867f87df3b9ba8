"""Device float64 nearest neighbours on the fused kernels (csrc/knn_f64.hip) against what the same public
call ran before them, one process, alternating the two per round: ops.knn_topk + sqrt (what
ht.spatial.cdist_topk runs per block) at nq = nt in
{4e4, 2.5e5, 1e6}, f in {18, 64, 128}, k in {1, 8, 16}, and a few-queries case (nq = 256, nt = 1e6) that
runs the split columns. "Before" is cdist_topk's tile path: exact cdist_f64 tiles of 2^24 entries in HBM,
topk, a threshold, two where passes, a second topk and a gather per tile, then the square root. Its
query blocks are independent, so it is timed on the first --parent-rows queries and scaled to nq (the
row says so: parent_rows); indices are compared on those rows. For k = 1 the row also holds
ops.kmeans_assign_f64 on the same shape: the same matrix loop without lists. Every case is warmed up
and timed with device events. One JSON line per case and round to --out (default
profiles/knn_f64_r10.jsonl); --cases keeps the cases whose "n<nq>x<nt>f<f>k<k>" name contains the
given text. Fails without a GPU."""
import argparse
import json

import torch

import heat_amd as ht
from heat_amd import ops

CASES = [(n, n, f, k) for n in (40000, 250000, 1000000) for f in (18, 64, 128) for k in (1, 8, 16)]
CASES += [(256, 1000000, f, k) for f in (18, 128) for k in (1, 16)]


def parent_topk(x, y, k):
    nq = x.shape[0]
    step = max(1, (1 << 24) // max(y.shape[0], 1))
    ds, ids = [], []
    for q0 in range(0, nq, step):
        d = ops.cdist(x[q0: q0 + step], y, "sqeuclidean", exact=True)
        thr = torch.topk(d, k, dim=1, largest=False).values[:, -1:]
        col = torch.arange(d.shape[1], device=d.device).expand_as(d)
        key = torch.where(d < thr, torch.full_like(col, -1),
                          torch.where(d == thr, col, torch.full_like(col, d.shape[1])))
        di = torch.topk(key, k, dim=1, largest=False).indices
        ds.append(torch.gather(d, 1, di))
        ids.append(di)
    return torch.sqrt(torch.clamp(torch.cat(ds), min=0)), torch.cat(ids)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/knn_f64_r10.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-rows", type=int, default=4096)
    ap.add_argument("--cases", default="")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("knn_f64 microbench: needs a GPU and the native library")
    ht.use_device("gpu")
    ht.random.seed(0)
    with open(args.out, "a") as fo:
        for nq, nt, f, k in CASES:
            name = "n{}x{}f{}k{}".format(nq, nt, f, k)
            if args.cases not in name:
                continue
            X, Y = ht.random.randn(nq, f, dtype=ht.float64), ht.random.randn(nt, f, dtype=ht.float64)
            x, y = X.larray, Y.larray
            pr = min(nq, args.parent_rows)
            # the fused kernels through the op (cdist_topk itself sends few queries with k > 8 to the tiles)
            native = lambda: ops.knn_topk(x, y, k)[0].sqrt_()   # noqa: E731
            before = lambda: parent_topk(x[:pr], y, k)        # noqa: E731
            # the tile path returns a block's neighbours unordered (cdist_topk's merge orders them): sets
            got, want = ops.knn_topk(x, y, k)[1][:pr].sort(1).values, before()[1].sort(1).values
            agree = float((got == want).all(1).double().mean())
            timed(native, 1)
            for rnd in range(args.rounds):
                t_n, t_p = timed(native, args.reps), timed(before, args.reps) * nq / pr
                row = {"case": name, "nq": nq, "nt": nt, "f": f, "k": k, "round": rnd, "reps": args.reps,
                       "native_ms": round(t_n, 3), "parent_ms": round(t_p, 3), "parent_rows": pr,
                       "native_vs_parent": round(t_n / t_p, 5), "tflops": round(2e-9 * nq * nt * f / t_n, 2),
                       "rows_agree_with_parent": agree}
                if k == 1:
                    row["kmeans_assign_f64_ms"] = round(timed(lambda: ops.kmeans_assign_f64(x, y, want_mind=True),
                                                              args.reps), 3)
                fo.write(json.dumps(row) + "\n")
                fo.flush()
                print(json.dumps(row), flush=True)
            del X, Y, x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
