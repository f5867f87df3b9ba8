"""One Lloyd iteration (assign + update) of KMedians and of KMedoids on device data: n = 4e6, f = 64,
k in {8, 128}, float32 and float64. --modes picks the legs: "native" (csrc/kmedians.hip), "native_fixed"
(the radix select with the worst-case pass count instead of the host read of the pass count) and
"torch" (HEAT_KMEDIANS_NATIVE=0, read per call: the torch path of the same commit - the cdist matrix
+ argmin, the key bisection with its 2 x 32 / 2 x 64 contended float64 index_add_ passes, the n x f
difference tensor). Whole-call times (host clock around a fit with max_iter=1 that ends in a device
synchronise) and the peak device memory the call allocates on top of the data. One JSON line per
case, leg and round (round -1 is the warm-up) is printed and appended to --out (default
profiles/kmedians.jsonl) as soon as the leg ends. Fails without a GPU."""
import argparse
import json
import os
import time

import torch

import heat_amd as ht
from heat_amd import ops

LEGS = {"native": ("1", False), "native_fixed": ("1", True), "torch": ("0", False)}


def one_iteration(est, x, init, k):
    """(seconds, peak extra bytes) of one fit with max_iter=1."""
    kw = dict(n_clusters=k, init=init, max_iter=1)
    model = ht.cluster.KMedians(tol=None, **kw) if est == "KMedians" else ht.cluster.KMedoids(**kw)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    model.fit(x)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/kmedians.jsonl")
    ap.add_argument("--n", type=int, default=4000000)
    ap.add_argument("--f", type=int, default=64)
    ap.add_argument("--ks", default="8,128")
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="native,torch")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("kmedians microbench: needs a GPU and the native library")
    with open(args.out, "a") as out:
        for dtype in (getattr(torch, d) for d in args.dtypes.split(",")):
            g = torch.Generator(device="cuda").manual_seed(0)
            for k in (int(v) for v in args.ks.split(",")):
                # k blobs, so that clusters are tight the way converging fits see them
                X = torch.randn(args.n, args.f, generator=g, device="cuda", dtype=dtype)
                X += 8 * torch.randint(0, k, (args.n, 1), generator=g, device="cuda").to(dtype)
                x = ht.array(X)
                init = ht.array(X[:: args.n // k][:k].clone())
                for est in ("KMedians", "KMedoids"):
                    for rnd in range(-1, args.rounds):
                        for leg in args.modes.split(","):
                            os.environ["HEAT_KMEDIANS_NATIVE"], ops.kernels._MED_FIXED_PASSES = LEGS[leg]
                            t, peak = one_iteration(est, x, init, k)
                            row = {"est": est, "dtype": str(dtype).split(".")[1], "n": args.n, "f": args.f, "k": k,
                                   "leg": leg, "round": rnd, "ms": round(t * 1e3, 2),
                                   "peak_extra_mb": round(peak / 2 ** 20, 1)}
                            out.write(json.dumps(row) + "\n")
                            out.flush()
                            print(json.dumps(row), flush=True)
                os.environ["HEAT_KMEDIANS_NATIVE"], ops.kernels._MED_FIXED_PASSES = "1", False
                del X, x, init
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
