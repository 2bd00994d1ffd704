"""Time of the backward of the generator's grey heads on the device (bsr_heads_grad, csrc/heads_grad_kernels.h), one JSON line, also
written to --out (profiles/heads_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies y and mask22, d_gs comes from
generator_grad.heads_example_inputs(seed 0), and HeadsGrad.backward reads y in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  kernel_ms              the mean device time of each of the chain's launches, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/heads_grad_bench.py --calls-only
                             python tools/heads_grad_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.
  rates                  with --stats: per launch the bytes it moves and its GB/s; per matrix launch also its executed GFLOP with the pads
                         counted (98 -> 100 rows of the data gradient, 98 -> 112 of the kernel gradient), TFLOP/s and share of the
                         157.3 TFLOP/s fp32 matrix bound.
  parity                 with --parity, per (H, W, B) of the device tests' sizes the worst scaled error of the five outputs against
                         generator_grad.heads_grad on the device's own mask; e2e_measured is the largest, the figure the device test's
                         bound is 4 x of.

    python tools/heads_grad_bench.py [--batch 32] [--size 256] [--iters 200] [--parity] [--stats CSV] [--out FILE] [--calls-only]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_FLOPS = 157.3e12
KERNELS = ("hg_entry_kernel", "hg_dgrad_kernel", "hg_wgrad_kernel", "hg_fold_kernel", "hg_finish_kernel")


def flops(N):
    """kernel -> the FLOP its launch executes on N pixels, the pads counted."""
    return {"hg_dgrad_kernel": 2.0 * N * 100 * 64, "hg_wgrad_kernel": 2.0 * N * 112 * 64}


def bytes_moved(N, slices):
    """kernel -> the bytes its launch reads and writes once each (the halo's re-reads of g2 and the per-workgroup reads of the 25.6 KB
    image, which the caches serve, are not counted)."""
    part = 4 * slices * 112 * 64 * 4
    return {"hg_entry_kernel": N * (12 + 12 + 4 + 8 + 4) + N / 256 * 16, "hg_dgrad_kernel": N * (8 + 256), "hg_wgrad_kernel": N * (8 + 256) + part,
            "hg_fold_kernel": part * 98 / 112 + 98 * 64 * 12, "hg_finish_kernel": N / 256 * 16}


def kernel_stats(path):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in KERNELS if k in found}


def parity():
    """The device tests' cases: heads_grad_cases.case(H, W, B, 1) over GPU_SIZES."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads_grad_cases as cases
    from blindshadowremoval_amd import HeadsGrad, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = HeadsGrad(0)
    for H, W, B in cases.GPU_SIZES:
        wt, inputs, y, d_gs = cases.case(H, W, B, 1)
        runner.load_weights(wt)
        res = runner.heads_grad(*[torch.from_numpy(a).to(dev) for a in (inputs, cases.mask22_of(wt, inputs, y), y, d_gs)], keep=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        st = host.heads_grad(wt, inputs, y, d_gs, acts={"mask": got["mask"]})
        each = {name: float("%.3g" % cases.worst_scaled_diff(got, st, (name,))[0]) for name in cases.OUTPUTS}
        worst = cases.worst_scaled_diff(got, st)
        out.append({"H": H, "W": W, "batch": B, "scaled_error_device_mask": float("%.3g" % worst[0]), "at": worst[1], "each": each})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="the kernel statistics CSV of a profiled --calls-only run")
    ap.add_argument("--calls-only", action="store_true", help="the warm-up and the calls, nothing else: the program to profile")
    ap.add_argument("--parity", action="store_true", help="the end-to-end scaled errors over the device tests' sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import Generator, HeadsGrad, _lib, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("heads_grad_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    N = B * S * S
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = HeadsGrad(0)
    runner.load_weights(weights)
    d_gs = torch.from_numpy(host.heads_example_inputs(S, S, B, seed=0)[2]).to(dev)

    def timed(fn, iters):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            res = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, res

    im, uv = torch.rand((B, S, S, 3), device=dev), torch.rand((B, S, S, 3), device=dev)
    gen = Generator(device=0)
    gen.load_weights(weights)
    outs = gen(im, uv, None, chuck=2, training=False)
    mask22 = outs[2]
    call = lambda: runner.backward(gen, im, mask22, d_gs)                              # noqa: E731
    if args.calls_only:
        timed(call, min(args.iters, 20))
        return
    ms, res = timed(call, args.iters)
    spread = [timed(call, args.iters)[0] for _ in range(2)]
    gen.close()
    slices = int(_lib.load().bsr_heads_grad_partials(B, S, S))
    kernel_ms = kernel_stats(args.stats) if args.stats else None
    rates = None
    if kernel_ms and all(k in kernel_ms for k in KERNELS):
        rates = []
        fl = flops(N)
        for kernel, nbytes in bytes_moved(N, slices).items():
            row = {"launch": kernel, "ms": kernel_ms[kernel], "mbytes_moved": round(nbytes / 1e6, 2), "gbytes_per_s": round(nbytes / kernel_ms[kernel] / 1e6, 1)}
            if kernel in fl:
                t = fl[kernel] / kernel_ms[kernel] / 1e9
                row.update(gflop_executed=round(fl[kernel] / 1e9, 2), tflops=round(t, 1), share_of_matrix_bound=round(t * 1e12 / MATRIX_FLOPS, 3))
            rates.append(row)
    flat = res[""]
    line = {"batch": B, "size": S, "pixels": N, "slices": slices, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_y_l1": float(res["d_y"].abs().sum().cpu()), "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread],
            "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None, "rates": rates,
            "chain_kernel_ms": round(sum(kernel_ms[k] for k in KERNELS), 5) if rates else None, "stage_budget": 1e-5}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_mask"] for p in line["parity"])
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
