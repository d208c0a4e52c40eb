#!/usr/bin/env python3
"""Microbenchmark the CDNA4 fused kernels: achieved HBM bandwidth.

Each kernel is HBM-bound; the table reports moved bytes / time against the
~6.3 TB/s achievable ceiling (MI355X_MICROARCH.md).  Run under rocprofv3
for per-kernel confirmation; results land in profiles/kernel_bandwidth.md
when --out is given.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from shockwave_amd import ops


def time_kernel(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e-3  # seconds


def split_sizes(total, pieces=60, seed=0):
    """Realistic multi-tensor shape mix (ResNet-like layer sizes)."""
    import random

    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, total), pieces - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def run(total_params, label, out_lines):
    dev = "cuda:0"
    sizes = split_sizes(total_params)
    p = [torch.randn(s, device=dev) for s in sizes]
    g = [torch.randn(s, device=dev) for s in sizes]
    m = [torch.zeros(s, device=dev) for s in sizes]
    v = [torch.zeros(s, device=dev) for s in sizes]
    B = 4 * total_params  # bytes per tensor list

    rows = []

    t = time_kernel(lambda: ops.fused_sgd(p, g, m, lr=0.1, momentum=0.9,
                                          weight_decay=5e-4))
    rows.append(("swq_fused_sgd", (3 + 2) * B, t))  # r:p,g,m w:p,m

    t = time_kernel(lambda: ops.fused_adam(p, g, m, v, lr=1e-3, step=10))
    rows.append(("swq_fused_adam", (4 + 3) * B, t))  # r:p,g,m,v w:p,m,v

    t = time_kernel(lambda: ops.multi_tensor_accum(m, g, 1.0))
    rows.append(("swq_multi_tensor_accum", 3 * B, t))  # r:m,g w:m

    t = time_kernel(lambda: ops.multi_tensor_l2norm(g))
    rows.append(("swq_multi_tensor_l2norm_sq", 1 * B, t))

    flat = [torch.randn(total_params, device=dev) for _ in range(4)]
    t = time_kernel(lambda: ops.gns_window_stats(flat))
    rows.append(("swq_gns_window_stats (W=4)", 4 * B, t))

    out_lines.append(f"\n### {label} ({total_params/1e6:.1f} M params)\n")
    out_lines.append("| kernel | bytes moved | time (us) | GB/s |")
    out_lines.append("|---|---|---|---|")
    for name, bytes_, secs in rows:
        gbs = bytes_ / secs / 1e9
        line = f"| {name} | {bytes_/1e6:.0f} MB | {secs*1e6:.1f} | {gbs:.0f} |"
        out_lines.append(line)
        print(f"{label:10s} {name:30s} {secs*1e6:8.1f} us  {gbs:7.0f} GB/s")


def run_capturable(total_params, label, out_lines, rounds=9):
    """Capturable (_cap) kernels and the fused clipped step against the
    by-value kernels and the torch clip route: same tensor lists, same
    run, variants interleaved in a new order every round.  Reports the
    median and the min..max spread over the rounds."""
    import statistics

    dev = "cuda:0"
    sizes = split_sizes(total_params)
    p = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in sizes]
    pd = [x.data for x in p]
    g = [torch.randn(s, device=dev) for s in sizes]
    for x, gx in zip(p, g):
        x.grad = gx
    m = [torch.zeros(s, device=dev) for s in sizes]
    v = [torch.zeros(s, device=dev) for s in sizes]
    B = 4 * total_params  # bytes per tensor list

    scalars = ops.new_scalar_block(1, dev)
    scalars[ops.SCALAR_LR0].fill_(1e-3)
    partials = torch.zeros(ops.num_chunks(g), device=dev)
    n_part = partials.numel()
    sgd_kw = dict(momentum=0.9, weight_decay=5e-4)

    def sgd():
        ops.fused_sgd(pd, g, m, lr=1e-3, **sgd_kw)

    def sgd_cap():
        ops.fused_sgd_cap(pd, g, m, scalars, 0, **sgd_kw)

    def adam():
        ops.fused_adam(pd, g, m, v, lr=1e-3, step=10)

    def adam_cap():
        ops.fused_adam_cap(pd, g, m, v, scalars, 0)

    def clipped_step():
        ops.multi_tensor_sumsq_partials(g, partials, 0)
        ops.optim_prologue(partials, n_part, scalars, 1e30, True)
        ops.fused_sgd_cap(pd, g, m, scalars, 0, **sgd_kw)

    def torch_clip_route():
        torch.nn.utils.clip_grad_norm_(p, 1e30)
        ops.fused_sgd(pd, g, m, lr=1e-3, **sgd_kw)

    # the by-value kernels appear twice: the gap between the two runs of
    # the SAME kernel is the spread any difference has to exceed
    variants = [
        ("swq_fused_sgd", sgd, 5 * B),
        ("swq_fused_sgd (repeat)", sgd, 5 * B),
        ("swq_fused_sgd_cap", sgd_cap, 5 * B),
        ("swq_fused_adam", adam, 7 * B),
        ("swq_fused_adam (repeat)", adam, 7 * B),
        ("swq_fused_adam_cap", adam_cap, 7 * B),
        # r:g | r:p,g,m w:p,m
        ("clipped step (partials+prologue+sgd_cap)", clipped_step, 6 * B),
        # at least r:g (norm) + r:g w:g (scale) + r:p,g,m w:p,m
        ("clip_grad_norm_ + swq_fused_sgd", torch_clip_route, 8 * B),
    ]
    # a fresh seeded order every round, so no variant always runs behind
    # the same neighbour (clock and cache state carry over between them)
    import random

    rng = random.Random(0)
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, _ in rng.sample(variants, len(variants)):
            times[name].append(time_kernel(fn, iters=30, warmup=5))

    med = {k: statistics.median(t) for k, t in times.items()}
    base = {
        "swq_fused_sgd (repeat)": "swq_fused_sgd",
        "swq_fused_sgd_cap": "swq_fused_sgd",
        "swq_fused_adam (repeat)": "swq_fused_adam",
        "swq_fused_adam_cap": "swq_fused_adam",
        "clipped step (partials+prologue+sgd_cap)":
            "clip_grad_norm_ + swq_fused_sgd",
    }
    out_lines.append(f"\n### {label} ({total_params/1e6:.1f} M params)\n")
    out_lines.append("| variant | min bytes | median (us) | min..max (us) "
                     "| GB/s | ratio |")
    out_lines.append("|---|---|---|---|---|---|")
    for name, _, bytes_ in variants:
        t = med[name]
        ratio = (f"{t / med[base[name]]:.3f} x {base[name]}"
                 if name in base else "")
        line = (f"| {name} | {bytes_/1e6:.0f} MB | {t*1e6:.1f} | "
                f"{min(times[name])*1e6:.1f}..{max(times[name])*1e6:.1f} | "
                f"{bytes_/t/1e9:.0f} | {ratio} |")
        out_lines.append(line)
        print(f"{label:10s} {line}")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=None)
    ap.add_argument("--capturable-out", default=None,
                    help="run the capturable-optimizer comparison instead "
                         "and write its table here")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    if args.capturable_out:
        lines = ["# Capturable fused optimizers vs by-value kernels "
                 "(MI355X, fp32)", "",
                 "Produced by `scripts/bench_kernels.py --capturable-out`.",
                 "Variants are interleaved, in a new seeded order every round,",
                 "in one process on the same tensor lists; 9 rounds x 30 timed",
                 "calls each.",
                 "`ratio` divides a variant's median by its baseline's.",
                 "The `(repeat)` rows time the same by-value kernel a second",
                 "time: their ratio is the run-to-run spread."]
        run_capturable(11_200_000, "ResNet-18", lines)
        run_capturable(25_600_000, "ResNet-50", lines)
        run_capturable(100_000_000, "100M", lines)
        with open(args.capturable_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"wrote {args.capturable_out}")
        return
    lines = ["# Fused-kernel achieved bandwidth (MI355X, fp32)",
             "", "Ceiling: ~6300 GB/s (measured float4 copy,",
             "MI355X_MICROARCH.md).  Bytes counted as reads+writes of each",
             "tensor list touched."]
    run(11_200_000, "ResNet-18", lines)   # ~ResNet-18 param count
    run(25_600_000, "ResNet-50", lines)
    run(100_000_000, "100M", lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
