"""ht.median / ht.percentile on device data through the radix-select kernels (csrc/quantile.hip): 1e9
float32 flat, 1e6 x 1000 float32 along axis None / 0 / 1, 5e5 x 1000 float64, a 9-quantile call and an
all-equal array (nothing to compact). Legs per case:
  native       ht.percentile on the kernels;
  mean         the ht.mean call on the same array - the one-pass yardstick;
  fallback     ht.percentile with HEAT_QUANTILE_NATIVE=0 (read per call) on THIS commit: torch.quantile,
               for float32 data on a float64 copy of the array;
  parent_expr  the expression the parent commit ran for these calls, written out here:
               torch.quantile(t, q / 100, dim, interpolation="linear") on the tensor in its own type,
               no copy - not a run of the parent commit itself.
fallback and parent_expr run only where a slice has at most 2^24 elements - elsewhere the row says
"unsupported". Whole-call times (host clock around a call that ends in a device synchronise). One JSON
line per case, leg and round (round -1 is the warm-up) is printed and appended to --out (default
profiles/quantile.jsonl) as soon as the leg ends. --scale divides the leading dimension. Fails without
a GPU."""
import argparse
import json
import os
import time

import torch

import heat_amd as ht
from heat_amd import ops

NINE = [10, 20, 30, 40, 50, 60, 70, 80, 90]
# (name, shape, dtype, axis, q, all equal)
CASES = [("flat_1e9", (1000000000,), "float32", None, 50.0, False),
         ("1e6x1000_none", (1000000, 1000), "float32", None, 50.0, False),
         ("1e6x1000_axis0", (1000000, 1000), "float32", 0, 50.0, False),
         ("1e6x1000_axis1", (1000000, 1000), "float32", 1, 50.0, False),
         ("5e5x1000_f64_axis0", (500000, 1000), "float64", 0, 50.0, False),
         ("5e5x1000_f64_none", (500000, 1000), "float64", None, 50.0, False),
         ("1e6x1000_axis0_nine", (1000000, 1000), "float32", 0, NINE, False),
         ("flat_1e9_nine", (1000000000,), "float32", None, NINE, False),
         ("flat_1e9_equal", (1000000000,), "float32", None, 50.0, True)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/quantile.jsonl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--modes", default="native,mean,fallback,parent_expr")
    args = ap.parse_args()
    if not (torch.cuda.is_available() and ops.available()):
        raise SystemExit("quantile microbench: needs a GPU and the native library")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as out:
        for name, shape, dtype, axis, q, equal in CASES:
            if name not in args.cases.split(","):
                continue
            shape = (shape[0] // args.scale,) + shape[1:]
            g = torch.Generator(device="cuda").manual_seed(0)
            X = torch.empty(shape, device="cuda", dtype=getattr(torch, dtype))
            X.fill_(1.25) if equal else X.normal_(generator=g)
            x = ht.array(X, copy=False)
            slice_len = X.numel() if axis is None else shape[axis]
            for leg in args.modes.split(","):
                for rnd in range(-1, args.rounds):
                    row = {"case": name, "shape": list(shape), "dtype": dtype, "axis": axis,
                           "q": q if isinstance(q, list) else [q], "leg": leg, "round": rnd}
                    if leg in ("fallback", "parent_expr") and slice_len > 2 ** 24:
                        row.update(round=0, ms=None, note="unsupported: torch.quantile takes at most 2^24 per slice")
                    else:
                        os.environ["HEAT_QUANTILE_NATIVE"] = "0" if leg == "fallback" else "1"
                        if leg == "mean":
                            call = lambda: ht.mean(x, axis=axis)
                        elif leg == "parent_expr":
                            qt = torch.tensor([v / 100.0 for v in row["q"]], dtype=X.dtype, device=X.device)
                            t, dim = (X.reshape(-1), 0) if axis is None else (X, axis)
                            call = lambda: torch.quantile(t, qt, dim=dim, interpolation="linear")
                        else:
                            call = lambda: ht.percentile(x, q, axis=axis)
                        row["ms"] = round(timed(call) * 1e3, 3)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
                    print(json.dumps(row), flush=True)
                    if row["ms"] is None:
                        break
            os.environ["HEAT_QUANTILE_NATIVE"] = "1"
            del X, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
