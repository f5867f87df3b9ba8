"""Device float64 k-means on the native kernels (csrc/kmeans_f64.hip, the fp64 update of kmeans.hip, the
fp64 kmeans_finalize) against what the same public calls ran before them, one process, alternating the
two per round: one Lloyd step (KMeans.step, tol=None), ops.kmeans_assign and ops.kmeans_update, at
n = 4e6, f in {18, 64, 128, 200}, k in {8, 128, 1024}. "Before" is, for the assignment, a float32 copy
of the points + the fp32 kernel (f <= 128) or addmm + min over an n x k float64 matrix (f > 128; there
n is 1e6 at k = 1024 so that the matrix stays at 8 GB); for the update index_add_ + bincount; for the
step those two + the torch epilogue. The old assignment at f <= 128 is not float64-accurate, so its
time is not a time of the same result. Every case is warmed up and timed with device events (a
"before" that takes more than 0.5 s per call is timed by its single warm-up call). One JSON
line per case, kind and round to --out (default profiles/kmeans_f64_r09.jsonl); --cases keeps the
cases whose "f<f>k<k>" name contains the given text. Fails without a GPU."""
import argparse
import ctypes
import json

import torch

import heat_amd as ht
from heat_amd import ops
from heat_amd.ops import kernels

CASES = [(1000000 if f > 128 and k == 1024 else 4000000, f, k) for f in (18, 64, 128, 200) for k in (8, 128, 1024)]


def parent_assign(X, C):
    n, f = X.shape
    k = C.shape[0]
    if f <= 128:
        Xa, Ca = kernels._rows_f32_aligned(X), kernels._rows_f32_aligned(C)
        L, fa = ops.lib(), Xa.shape[1]
        fpad, kpad = ctypes.c_int(), ctypes.c_int()
        ws = torch.empty(L.ha_km_workspace_floats(k, fa, ctypes.byref(fpad), ctypes.byref(kpad)), dtype=torch.float32,
                         device=X.device)
        labels = torch.empty(n, dtype=torch.int32, device=X.device)
        ops.check(L.ha_km_assign(kernels._ptr(Xa), n, fa, Xa.stride(0), kernels._ptr(Ca), k, Ca.stride(0),
                                 kernels._ptr(ws), kernels._ptr(labels), kernels._ptr(None),
                                 ctypes.c_void_p(ops.stream_ptr(X.device))), "ha_km_assign")
        return labels
    d = torch.addmm((C * C).sum(1).unsqueeze(0), X, C.t(), beta=1.0, alpha=-2.0)
    return torch.min(d, dim=1)[1].to(torch.int32)


def parent_update(X, labels, k):
    lab = labels.to(torch.int64)
    sums = torch.zeros((k, X.shape[1]), dtype=X.dtype, device=X.device)
    sums.index_add_(0, lab, X)
    return sums, torch.bincount(lab, minlength=k).to(sums.dtype)


def parent_step(X, C):
    sums, counts = parent_update(X, parent_assign(X, C), C.shape[0])
    newC = torch.where(counts.unsqueeze(1) > 0, sums / counts.clamp(min=1).unsqueeze(1), C)
    return newC, ((C - newC) ** 2).sum()


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
    ap.add_argument("--out", default="profiles/kmeans_f64_r09.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("kmeans_f64 microbench: needs a GPU and the native library")
    ht.use_device("gpu")
    ht.random.seed(0)
    with open(args.out, "w") as fo:
        for n, f, k in CASES:
            name = "f{}k{}".format(f, k)
            if args.cases not in name:
                continue
            x = ht.random.randn(n, f, dtype=ht.float64)
            X = x.larray
            C = X[torch.randperm(n, device=X.device)[:k]].clone()
            km = ht.cluster.KMeans(n_clusters=k, init=ht.array(C.cpu().numpy(), device="gpu"), tol=None)
            labels = ops.kmeans_assign(X, C, want_mind=False)[0]
            agree = float((labels == parent_assign(X, C)).double().mean())
            kinds = [("step", lambda: km.step(x), lambda: parent_step(X, C)),
                     ("assign", lambda: ops.kmeans_assign(X, C, want_mind=False), lambda: parent_assign(X, C)),
                     ("update", lambda: ops.kmeans_update(X, labels, k), lambda: parent_update(X, labels, k))]
            for kind, native, before in kinds:
                timed(native, 2)
                warm = timed(before, 1)
                # float64 index_add_ with few clusters takes seconds per call (atomics on k x f
                # addresses): such a "before" is timed by that one call and not run again
                slow = warm > 500.0
                for rnd in range(args.rounds):
                    t_n, t_p = timed(native, args.reps), (warm if slow else timed(before, args.reps))
                    row = {"case": name, "kind": kind, "n": n, "f": f, "k": k, "round": rnd, "reps": args.reps,
                           "parent_reps": 1 if slow else args.reps,
                           "native_ms": round(t_n, 4), "parent_ms": round(t_p, 4),
                           "native_vs_parent": round(t_n / t_p, 4), "x_gbs": round(8.0 * n * f / t_n / 1e6, 1),
                           "labels_agree_with_parent": agree}
                    fo.write(json.dumps(row) + "\n")
                    fo.flush()
                    print(json.dumps(row), flush=True)
            del x, X, C, km, labels, kinds
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
