"""ht.kurtosis and ht.skew on device tensors next to ht.mean of the same tensor and axis (the one-pass
HBM floor): axis None, 0 and 1 on 1e6 x 1000 float32 and 5e5 x 1000 float64 (exponential data, so the
third moment is not near zero). One process; every call is warmed up, then timed with device events over
--reps calls, --rounds times. It only uses the public interface, so the same script measures the code
before and after csrc/moments4.hip: --label names the code it ran on. One JSON line per case and round is
appended to --out (default profiles/moments4.jsonl), with the ratio to the mean pass and the bytes of the
input over the time. Run it under a time limit (timeout 600 python tools/microbench/moments4.py).
Fails without a GPU."""
import argparse
import json

import torch

import heat_amd as ht
from heat_amd import ops

CASES = [("f32", ht.float32, 1000000, 1000), ("f64", ht.float64, 500000, 1000)]


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
    ap.add_argument("--out", default="profiles/moments4.jsonl")
    ap.add_argument("--label", default="new")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scale the row counts (rehearsals)")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("moments4 microbench: needs a GPU and the native library")
    ht.use_device("gpu")
    ht.random.seed(0)
    with open(args.out, "a") as fo:
        for name, dtype, rows, cols in CASES:
            rows = max(1, int(rows * args.rows_scale))
            X = ht.random.rand(rows, cols, dtype=dtype)
            X.larray.clamp_(min=1e-7).log_().neg_()
            nbytes = X.larray.numel() * X.larray.element_size()
            for axis in (None, 0, 1):
                fns = {"kurtosis": lambda: ht.kurtosis(X, axis=axis), "skew": lambda: ht.skew(X, axis=axis),
                       "mean": lambda: ht.mean(X, axis=axis)}
                for fn in fns.values():
                    timed(fn, 2)
                for rnd in range(args.rounds):
                    t = {k: timed(fn, args.reps) for k, fn in fns.items()}
                    row = {"label": args.label, "case": name, "shape": [rows, cols], "axis": axis, "round": rnd,
                           "reps": args.reps, "mean_ms": round(t["mean"], 4)}
                    for k in ("kurtosis", "skew"):
                        row[k + "_ms"] = round(t[k], 4)
                        row[k + "_vs_mean"] = round(t[k] / t["mean"], 3)
                        row[k + "_input_tb_s"] = round(nbytes / t[k] * 1e-9, 3)
                    fo.write(json.dumps(row) + "\n")
                    fo.flush()
                    print(json.dumps(row), flush=True)
            del X
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
