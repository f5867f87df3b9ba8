"""The fp64 MFMA GEMM (csrc/gemm_f64.hip behind ops.gemm_f64) against the library DGEMM, one process,
alternating the two per round: 1024^3 .. 8192^3, the tall 1.25e5 x 4096 x 4096 product and the
split-K shape 512^2 x 1e6. The library side is what float64 products ran on before - torch.matmul
through basics._mm_blocked, which keeps every library operand below HEAT_BLAS_MAX_BYTES (one plain
torch.matmul for all but the two 4 GB shapes). Every shape is warmed up, timed with device events,
and the two results are compared. One JSON line per shape and round (time, TF from 2 M N K, ratio)
to --out (default profiles/gemm_f64_r07.jsonl). --shapes / --gram time other products (the rows
behind basics._library_better_f64). Fails without a GPU."""
import argparse
import json

import torch

from heat_amd import ops
from heat_amd.core.linalg import basics

SHAPES = [(1024, 1024, 1024), (2048, 2048, 2048), (4096, 4096, 4096), (8192, 8192, 8192),
          (125000, 4096, 4096), (512, 512, 1000000)]


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
    ap.add_argument("--out", default="profiles/gemm_f64_r07.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="M,N,K;M,N,K;... instead of the standard list")
    ap.add_argument("--gram", default=None, help="K,n;K,n;... : x^T x of a [K, n] matrix the way fgemm runs Gram "
                    "products (upper tiles + mirror) against the library on the transposed view")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    if args.gram:
        shapes = [(int(n), int(n), int(k)) for k, n in (s.split(",") for s in args.gram.split(";"))]
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("gemm_f64 microbench: needs a GPU and the native library")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with open(args.out, "w") as f:
        for M, N, K in shapes:
            if args.gram:
                b = torch.randn(K, N, dtype=torch.float64, device=dev)
                a = b.t()
            else:
                a = torch.randn(M, K, dtype=torch.float64, device=dev)
                b = torch.randn(K, N, dtype=torch.float64, device=dev)
            flop = 2.0 * M * N * K

            def native():
                if not args.gram:
                    return ops.gemm_f64(a, b)
                u = ops.gemm_f64(a, b, upper=True)
                return u + torch.triu(u, 1).t()

            def library():
                return basics._mm_blocked(a, b)

            reps = max(2, min(50, int(2e12 / flop)))
            diff = float((native() - library()).abs().max())   # also the warm-up of both
            timed(native, 2), timed(library, 2)
            slices = int(ops.lib().ha_gemm_f64_slices(M, N, K, ops.num_cus(dev)))
            for rnd in range(args.rounds):
                t_n, t_l = timed(native, reps), timed(library, reps)
                row = {"M": M, "N": N, "K": K, "gram": bool(args.gram), "round": rnd, "reps": reps, "slices": slices,
                       "gemm_f64_ms": round(t_n, 4), "library_ms": round(t_l, 4),
                       "gemm_f64_tf": round(flop / t_n / 1e9, 2), "library_tf": round(flop / t_l / 1e9, 2),
                       "native_vs_library": round(t_n / t_l, 3), "max_abs_diff": diff}
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(json.dumps(row), flush=True)
            del a, b
            torch.cuda.empty_cache()

if __name__ == "__main__":
    main()
