#!/usr/bin/env python
"""Reduce a `rocprofv3 --kernel-trace` CSV of a plain `bench.py` run to the layer chain's boundary table (profiles/store_policy.txt).

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python bench.py --gpus 1 --steps 20 --warmup 3
    python scripts/layer_boundary_trace.py OUT/**/*_kernel_trace.csv [--label parent]

A layer is five consecutive dispatches, in this order: QKV+attention, c_proj (+residual +ln_2), expert up-projection (+SwiGLU), expert
down-projection (K-slice slabs), combine (+ln_1).  For each kernel: mean and median duration, mean and median gap from its end to its successor's start (the
successor of `combine` is the next layer's QKV+attention, or the head kernel behind the last layer: only in-chain successors are counted),
and the layer period = start of one QKV+attention to the start of the next.  Tracing adds a little to every gap, equally to both arms of an
A/B; the end-to-end figure is bench.py's, taken with the profiler off.
"""
import argparse
import csv
import glob
import re
import statistics as st
import sys

CHAIN = [("qkv+attention", r"qkv_attn_kernel"),
         ("c_proj+resid+ln2", r"gemm_bf16_kernel<"),
         ("up+swiglu", r"gemm_pp_kernel<4,"),
         ("down_4slabs", r"gemm_pp_kernel<0,"),
         ("combine+ln1", r"combine_norm_row_kernel")]


def classify(name):
    for i, (_, pat) in enumerate(CHAIN):
        if re.search(pat, name):
            return i
    return -1


def reduce_trace(rows):
    """rows: [(kernel name, start ns, end ns)] -> ([(name, n, mean dur, mean gap, median dur, median gap)] in us, layers, mean period, median period)."""
    rows = sorted(rows, key=lambda r: r[1])
    kinds = [classify(r[0]) for r in rows]
    dur = [[] for _ in CHAIN]
    gap = [[] for _ in CHAIN]
    period = []
    n_layers = 0
    i, prev_layer_at = 0, None
    while i + len(CHAIN) <= len(rows):
        if kinds[i:i + len(CHAIN)] != list(range(len(CHAIN))):
            i += 1
            continue
        n_layers += 1
        for j in range(len(CHAIN)):
            dur[j].append((rows[i + j][2] - rows[i + j][1]) / 1e3)
            if j + 1 < len(CHAIN):
                gap[j].append((rows[i + j + 1][1] - rows[i + j][2]) / 1e3)
        if prev_layer_at == i - len(CHAIN):                          # back-to-back layers of one forward
            gap[-1].append((rows[i][1] - rows[i - 1][2]) / 1e3)
            period.append((rows[i][1] - rows[i - len(CHAIN)][1]) / 1e3)
        prev_layer_at = i
        i += len(CHAIN)
    nan = float("nan")
    table = [(CHAIN[j][0], len(dur[j]), st.mean(dur[j]) if dur[j] else nan, st.mean(gap[j]) if gap[j] else nan,
              st.median(dur[j]) if dur[j] else nan, st.median(gap[j]) if gap[j] else nan) for j in range(len(CHAIN))]
    return table, n_layers, (st.mean(period) if period else float("nan")), (st.median(period) if period else float("nan"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv", nargs="+", help="kernel-trace CSV file(s) or glob(s)")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    files = [f for pat in a.csv for f in (glob.glob(pat, recursive=True) or [pat])]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    if not rows:
        sys.exit("no kernel dispatches in " + ", ".join(files))
    table, n_layers, period, period_med = reduce_trace(rows)
    if not n_layers:
        sys.exit("the five-kernel layer chain does not occur in this trace")
    print(f"# {a.label or files[0]}: {n_layers} layers")
    print(f"{'kernel':<20}{'n':>7}{'dur us':>10}{'gap us':>10}{'dur+gap':>10}{'med dur':>10}{'med gap':>10}{'med d+g':>10}")
    sd = sg = md = mg = 0.0
    for name, n, d, g, dm, gm in table:
        print(f"{name:<20}{n:>7}{d:>10.2f}{g:>10.2f}{d + g:>10.2f}{dm:>10.2f}{gm:>10.2f}{dm + gm:>10.2f}")
        sd += d; sg += g; md += dm; mg += gm
    print(f"{'sum':<20}{'':>7}{sd:>10.2f}{sg:>10.2f}{sd + sg:>10.2f}{md:>10.2f}{mg:>10.2f}{md + mg:>10.2f}")
    print(f"layer period (QKV+attention start to the next): mean {period:.2f} us, median {period_med:.2f} us")


if __name__ == "__main__":
    main()
