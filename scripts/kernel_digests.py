#!/usr/bin/env python3
"""Digest every fused-kernel entry point on fixed inputs, to show that a
kernel refactor left the results bit-identical.

A test in the tree cannot see the commit before it, so: run this on the old
commit and on the new one (one MI355X, same software), then

    python scripts/kernel_digests.py --compare old.txt new.txt

Inputs come from seeded CPU generators.  Each case prints one SHA-256 over
the raw bytes of all its outputs copied to the host.  The atomics-based
results (l2norm over a multi-chunk tensor, gns over several blocks) depend
on the order the blocks arrive in; those print the values instead and are
compared with rtol=1e-5, as in tests/test_gpu_ops.py.
"""

import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

# tail only, vector only, exactly one chunk, one chunk + 1, several chunks
SIZES = [3, 1000, 32768, 32769, 3 * 32768 + 5]
CHUNK = 32768
# momentum, dampening, weight_decay, nesterov: the sets of
# tests/test_gpu_ops.py::TestFusedSGD and of the _cap bit-identity test
SGD_SETS = [
    (0.0, 0.0, 0.0, False), (0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True),
    (0.9, 0.0, 5e-4, True), (0.9, 0.5, 0.0, False),
]
ADAM_SETS = [(False, 0.0), (False, 1e-2), (True, 1e-2)]  # adamw, wd
RTOL = 1e-5


def run_cases(emit):
    import torch

    from shockwave_amd import ops

    assert torch.cuda.is_available() and ops.HAVE_EXT
    dev = torch.device("cuda:0")

    def rand(seed, sizes=SIZES):
        g = torch.Generator().manual_seed(seed)
        return [torch.randn(s, generator=g).to(dev) for s in sizes]

    def zeros():
        return [torch.zeros(s, device=dev) for s in SIZES]

    def digest(name, *lists):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for ts in lists:
            for t in ts:
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
        emit(f"{name} sha256 {h.hexdigest()}")

    def values(name, ts):
        torch.cuda.synchronize()
        vals = " ".join(repr(float(v)) for t in ts for v in t.reshape(-1))
        emit(f"{name} values {vals}")

    for mom, damp, wd, nest in SGD_SETS:
        p, m = rand(0), zeros()
        for step in range(3):
            ops.fused_sgd(p, rand(100 + step), m, lr=0.1, momentum=mom,
                          dampening=damp, weight_decay=wd, nesterov=nest,
                          buf_initialized=step > 0)
        digest(f"fused_sgd mom={mom} damp={damp} wd={wd} nest={nest}", p, m)

    for adamw, wd in ADAM_SETS:
        p, m, v = rand(1), zeros(), zeros()
        for step in range(1, 4):
            ops.fused_adam(p, rand(200 + step), m, v, lr=1e-3,
                           weight_decay=wd, step=step, adamw=adamw)
        digest(f"fused_adam adamw={adamw} wd={wd}", p, m, v)

    # capturable kernels: clip inactive, and active at half the true norm
    grads = rand(300)
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item()
    for clip, max_norm in [("off", 1e30), ("on", 0.5 * norm)]:
        partials = torch.zeros(ops.num_chunks(grads), device=dev)

        def prologue(scalars):
            n = ops.multi_tensor_sumsq_partials(grads, partials, 0)
            ops.optim_prologue(partials, n, scalars, max_norm, True)

        for mom, damp, wd, nest in SGD_SETS:
            scalars = ops.new_scalar_block(1, dev)
            scalars[ops.SCALAR_LR0].fill_(0.1)
            p, m = rand(0), zeros()
            for _ in range(3):
                prologue(scalars)
                ops.fused_sgd_cap(p, grads, m, scalars, 0, momentum=mom,
                                  dampening=damp, weight_decay=wd,
                                  nesterov=nest)
            digest(f"fused_sgd_cap clip={clip} mom={mom} damp={damp} "
                   f"wd={wd} nest={nest}", p, m, [scalars])
        for adamw, wd in ADAM_SETS:
            scalars = ops.new_scalar_block(1, dev)
            scalars[ops.SCALAR_LR0].fill_(1e-3)
            p, m, v = rand(1), zeros(), zeros()
            for _ in range(3):
                prologue(scalars)
                ops.fused_adam_cap(p, grads, m, v, scalars, 0,
                                   weight_decay=wd, adamw=adamw)
            digest(f"fused_adam_cap clip={clip} adamw={adamw} wd={wd}",
                   p, m, v, [scalars])

    dst = rand(2)
    ops.multi_tensor_accum(dst, rand(3), 2.5)
    digest("multi_tensor_accum alpha=2.5", dst)

    ts = rand(4)
    norms = ops.multi_tensor_l2norm(ts)
    one = [i for i, s in enumerate(SIZES) if s <= CHUNK]
    many = [i for i, s in enumerate(SIZES) if s > CHUNK]
    digest("multi_tensor_l2norm single-chunk tensors", [norms[one]])
    values("multi_tensor_l2norm multi-chunk tensors", [norms[many]])

    partials = torch.zeros(ops.num_chunks(ts), device=dev)
    scalars = ops.new_scalar_block(1, dev)
    n = ops.multi_tensor_sumsq_partials(ts, partials, 0)
    ops.optim_prologue(partials, n, scalars, 1.0, True)
    digest("multi_tensor_sumsq_partials + optim_prologue",
           [partials, scalars])

    for window in (2, 8):
        for n in (1000, (1 << 20) + 7):
            gs = rand(500 + window, sizes=[n] * window)
            values(f"gns_window_stats window={window} n={n}",
                   ops.gns_window_stats(gs))


def parse(path):
    cases = {}
    with open(path) as f:
        for line in f:
            for kind in (" sha256 ", " values "):
                if kind in line:
                    name, rest = line.rstrip("\n").split(kind)
                    cases[name] = (kind.strip(), rest)
    return cases


def compare(old_path, new_path):
    """Markdown table of both runs; exit status 1 unless every case agrees."""
    old, new = parse(old_path), parse(new_path)
    assert old and old.keys() == new.keys(), "the runs list different cases"
    bad = 0
    print("| case | old | new | |")
    print("|---|---|---|---|")
    for name, (kind, a) in old.items():
        b = new[name][1]
        if kind == "sha256":
            ok = a == b
            a, b = a[:16], b[:16]
        else:
            xs = [float(x) for x in a.split()]
            ys = [float(y) for y in b.split()]
            ok = len(xs) == len(ys) and all(
                abs(x - y) <= RTOL * abs(x) for x, y in zip(xs, ys))
        bad += not ok
        verdict = (("equal" if kind == "sha256" else f"rtol {RTOL:g}")
                   if ok else "DIFFERS")
        print(f"| {name} | {a} | {b} | {verdict} |")
    print(f"\n{len(old) - bad} of {len(old)} cases agree.")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=None, help="also write the lines here")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    run_cases(emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
