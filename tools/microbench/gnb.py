"""GaussianNB fit / predict / predict_log_proba on one GPU: the fused kernels (csrc/gnb.hip) next to the
torch path of the same commit (HEAT_GNB_NATIVE=0, read per call) and to ht.mean(x, axis=0) of the same
array, the one-pass HBM floor. 1e7 x 64 with 10 classes, float32 and float64. One process; every call is
warmed up, then timed with device events over --reps calls, --rounds times; the peak of the extra device
memory of one call is recorded beside the time. The torch predict path builds an m x k x f temporary, so
it is measured on --old-rows rows (default 1e6) and reported per row as well; the torch fit takes seconds
per call at this size, so the torch path is timed over --old-reps calls (default 1) per round, and
--skip-old leaves it out (kernel traces). One JSON line per case and round is appended to --out (default
profiles/gnb.jsonl). Run it from the repository root under a time limit
(PYTHONPATH=. timeout 900 python tools/microbench/gnb.py). Fails without a GPU."""
import argparse
import json
import os

import torch

import heat_amd as ht
from heat_amd import ops

CASES = [("f32", ht.float32, 10000000, 64), ("f64", ht.float64, 10000000, 64)]
K = 10


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gnb.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scale the row counts (rehearsals)")
    ap.add_argument("--old-rows", type=int, default=1000000, help="rows of the torch-path predict")
    ap.add_argument("--old-reps", type=int, default=1, help="timed calls of the torch path per round")
    ap.add_argument("--skip-old", action="store_true", help="fused path only (kernel traces)")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("gnb microbench: needs a GPU and the native library")
    ht.use_device("gpu")
    ht.random.seed(0)
    with open(args.out, "a") as fo:
        for name, dtype, rows, cols in CASES:
            rows = max(K, int(rows * args.rows_scale))
            old_rows = min(rows, args.old_rows)
            X = ht.random.randn(rows, cols, dtype=dtype)
            y = ht.array(torch.arange(rows, device=X.larray.device) % K)
            X.larray.add_((y.larray % K).to(X.larray.dtype).unsqueeze(1), alpha=4.0)
            Xs, ys = X[:old_rows], y[:old_rows]
            est = ht.naive_bayes.GaussianNB().fit(X, y)
            nbytes = X.larray.numel() * X.larray.element_size()
            fns = {"fit": lambda a, b: ht.naive_bayes.GaussianNB().fit(a, b),
                   "predict": lambda a, b: est.predict(a),
                   "predict_log_proba": lambda a, b: est.predict_log_proba(a)}
            timed(lambda: ht.mean(X, axis=0), 2)
            old_peak = {}
            for rnd in range(args.rounds):
                row = {"case": name, "shape": [rows, cols], "k": K, "round": rnd, "reps": args.reps,
                       "old_rows": old_rows, "mean_ms": round(timed(lambda: ht.mean(X, axis=0), args.reps), 4)}
                for key, fn in fns.items():
                    os.environ["HEAT_GNB_NATIVE"] = "1"
                    timed(lambda: fn(X, y), 1)
                    t = timed(lambda: fn(X, y), args.reps)
                    row[key + "_ms"] = round(t, 4)
                    row[key + "_vs_mean"] = round(t / row["mean_ms"], 3)
                    row[key + "_input_tb_s"] = round(nbytes / t * 1e-9, 3)
                    row[key + "_peak_mb"] = round(peak_extra(lambda: fn(X, y)) / 2 ** 20, 1)
                    if args.skip_old:
                        continue
                    # the torch fit takes seconds at this size (index_add_ atomics): one warm call in
                    # round 0 (it also gives the peak), then --old-reps calls per round
                    os.environ["HEAT_GNB_NATIVE"] = "0"
                    a, b = (X, y) if key == "fit" else (Xs, ys)
                    if rnd == 0:
                        old_peak[key] = round(peak_extra(lambda: fn(a, b)) / 2 ** 20, 1)
                    t_old = timed(lambda: fn(a, b), args.old_reps)
                    row[key + "_old_ms"] = round(t_old, 4)
                    row[key + "_old_rows"] = a.shape[0]
                    row[key + "_old_peak_mb"] = old_peak[key]
                    row[key + "_speedup_per_row"] = round((t_old / a.shape[0]) / (t / rows), 2)
                    os.environ["HEAT_GNB_NATIVE"] = "1"
                fo.write(json.dumps(row) + "\n")
                fo.flush()
                print(json.dumps(row), flush=True)
            del X, y, Xs, ys, est
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
