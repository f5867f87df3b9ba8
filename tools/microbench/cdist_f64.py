"""The float64 distance kernels (csrc/cdist_f64.hip behind ops.cdist_f64) against the torch expressions
that device float64 distances ran on before, one process, alternating the two per round: 40000 x 40000
at f = 18 and 128 for expansion-euclidean, exact-euclidean and manhattan, the symmetric exact call at
f = 128 and one small case (2000 x 2000 x 18). Every case is warmed up, timed with device events, and
both results are compared with the plain broadcast fp64 expression on 192 sampled rows
(native_max_abs_err, parent_max_abs_err: a parent time beside an error that is not rounding is the
time of an incomplete result). One JSON line per case and round (native ms, parent ms, GB/s of output
written by the native call) to --out (default profiles/cdist_f64_r08.jsonl). --cases keeps the cases
whose name contains the given text. Fails without a GPU."""
import argparse
import json

import torch

from heat_amd import ops

# (name, metric, exact, symmetric)
KINDS = [("expansion-euclidean", "euclidean", False, False), ("exact-euclidean", "euclidean", True, False),
         ("manhattan", "manhattan", False, False)]
CASES = [(40000, 40000, f) + k for f in (18, 128) for k in KINDS] + \
        [(40000, 40000, 128, "symmetric-exact-euclidean", "euclidean", True, True)] + \
        [(2000, 2000, 18) + k for k in KINDS]


def parent(x, y, metric, exact):
    """What ops.cdist computed for device float64 operands before the native kernels."""
    if metric == "manhattan":
        return torch.cdist(x, y, p=1)
    if exact:
        return (torch.cdist(x, y, p=2, compute_mode="donot_use_mm_for_euclid_dist") ** 2).sqrt()
    xn = (x * x).sum(1, keepdim=True)
    yn = (y * y).sum(1).unsqueeze(0)
    return torch.sqrt(torch.clamp(torch.addmm(xn + yn, x, y.t(), beta=1.0, alpha=-2.0), min=0))


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
    ap.add_argument("--out", default="profiles/cdist_f64_r08.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("cdist_f64 microbench: needs a GPU and the native library")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with open(args.out, "w") as fo:
        for m, n, f, name, metric, exact, sym in CASES:
            if args.cases not in name:
                continue
            x = torch.randn(m, f, dtype=torch.float64, device=dev)
            y = x if sym else torch.randn(n, f, dtype=torch.float64, device=dev)
            out = torch.empty(m, n, dtype=torch.float64, device=dev)

            def native():
                return ops.cdist_f64(x, y, metric, out=out, exact=exact, symmetric=sym)

            def before():
                return parent(x, y, metric, exact)

            # both results against the plain broadcast expression on the first, the last and 64
            # random rows (also the warm-up of both). torch.cdist's difference kernels leave most of
            # a 40000 x 40000 float64 result unwritten, so the two are not compared with each other.
            rows = torch.cat([torch.arange(0, 64), torch.randint(0, m, (64,)), torch.arange(m - 64, m)]).to(dev)
            d = x[rows][:, None, :] - y[None, :, :]
            ref = d.abs().sum(-1) if metric == "manhattan" else (d * d).sum(-1).sqrt()
            del d
            err_n = float((native()[rows] - ref).abs().max())
            err_p = float((before()[rows] - ref).abs().max())
            del ref
            big = m * n > 1 << 28
            reps = 3 if big else 50
            timed(native, 2), timed(before, 1 if big else 2)
            for rnd in range(args.rounds):
                t_n, t_p = timed(native, reps), timed(before, reps)
                row = {"case": name, "m": m, "n": n, "f": f, "round": rnd, "reps": reps, "native_ms": round(t_n, 4),
                       "parent_ms": round(t_p, 4), "native_out_gbs": round(8.0 * m * n / t_n / 1e6, 1),
                       "native_vs_parent": round(t_n / t_p, 4), "native_max_abs_err": err_n,
                       "parent_max_abs_err": err_p}
                fo.write(json.dumps(row) + "\n")
                fo.flush()
                print(json.dumps(row), flush=True)
            del x, y, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
