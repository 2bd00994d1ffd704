"""Time of the generator's colour tail backward on the device (bsr_clr_tail_grad, csrc/clr_tail_grad_kernels.h), one JSON line, also
written to --out (profiles/clr_tail_grad_bench.json).

B items of S x S from generator_grad.example_inputs(seed 0), weights from init_weights(1), through ColourTail.tail_grad.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  kernel_ms              the mean device time of each of the chain's six launches, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/clr_tail_bench.py --calls-only
                             python tools/clr_tail_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.  The --calls-only program also runs the generator's
                         forward, so the same trace holds the fused forward clr_conv1 launch (conv_n16_kernel<3,3,GS,TAIL>).
  rates                  with --stats: the kernel-gradient launch's TFLOP/s (2 x 9 x 65 x 16 a pixel) beside the a1 launch of the same
                         FLOP, and its share of the 157.3 TFLOP/s fp32 matrix bound; the data-gradient launch's TFLOP/s (2 x 9 x 16 x 65
                         a pixel); the bytes per second of launches 2 (a1 and g_con read, gz1 written: 140 bytes a pixel) and 4 (gz1
                         read, d_f and d_gs written, 324 bytes a pixel) against 8 TB/s.
  parity                 with --parity, per (H, W, B) of the device tests' sizes the worst scaled error of the twelve outputs against
                         generator_grad.tail_grad on the device's own activations, and against the statement's own float64 forward;
                         e2e_measured is the largest of the former, the figure the device test's bound is 4 x of.
  build                  with --build FILE, the compiler's register and LDS figures of the new kernels (a JSON object, merged in as is).

    python tools/clr_tail_bench.py [--batch 32] [--size 256] [--iters 1000] [--parity] [--stats CSV] [--build FILE] [--out FILE] [--calls-only]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_FLOPS = 157.3e12
HBM_BYTES_PER_S = 8.0e12
# the launches in order; the a1 launch is the one conv_n16_kernel instantiation without the fused tail that has the gs group
KERNELS = ("conv_n16_kernel<3, 3, true, false", "clr_tail_pixel_kernel", "clr_wgrad_kernel", "clr_dgrad_kernel", "clr_fold_kernel", "clr_finish_kernel")
FORWARD_KERNEL = "conv_n16_kernel<3, 3, true, true"
PARITY_SIZES = ((8, 32, 1), (16, 64, 2), (24, 96, 3), (32, 256, 1))


def kernel_stats(path, kernels):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in kernels:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in kernels if k in found}


def parity():
    """The device tests' cases: clr_tail_grad_cases.case(H, W, B, 1)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import clr_tail_grad_cases as cases
    from blindshadowremoval_amd import ColourTail, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = ColourTail(0)
    for H, W, B in PARITY_SIZES:
        w, *arrays = cases.case(H, W, B, 1)
        runner.load_weights(w)
        res = runner.tail_grad(*[torch.from_numpy(a).to(dev) for a in arrays], keep=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        on_dev = cases.worst_scaled_diff(got, host.tail_grad(w, *arrays, acts={"a1": got["a1"], "a2": got["a2"]}))
        own = cases.worst_scaled_diff(got, host.tail_grad(w, *arrays))
        out.append({"H": H, "W": W, "batch": B, "scaled_error_device_acts": float("%.3g" % on_dev[0]), "at": on_dev[1],
                    "scaled_error_own_forward": float("%.3g" % own[0]), "own_at": own[1]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="the kernel statistics CSV of a profiled --calls-only run")
    ap.add_argument("--calls-only", action="store_true", help="the warm-up and the calls, nothing else: the program to profile")
    ap.add_argument("--parity", action="store_true", help="the end-to-end scaled errors over the device tests' sizes")
    ap.add_argument("--build", default=None, help="a JSON file of the compiler's register and LDS figures, merged in under `build`")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clr_tail_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import ColourTail, Generator, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("clr_tail_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in host.example_inputs(S, S, B, seed=0)]
    weights = init_weights(1)
    runner = ColourTail(0)
    runner.load_weights(weights)

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

    gen = Generator(device=0)
    gen.load_weights(weights)
    im, uv = torch.rand((B, S, S, 3), device=dev), torch.rand((B, S, S, 3), device=dev)
    if args.calls_only:
        timed(lambda: runner.tail_grad(*t), min(args.iters, 20))
        timed(lambda: gen(im, uv, None, chuck=2, training=False), 10)
        return
    ms, res = timed(lambda: runner.tail_grad(*t), args.iters)
    spread = [timed(lambda: runner.tail_grad(*t), args.iters)[0] for _ in range(2)]
    gen_ms = [timed(lambda: gen(im, uv, None, chuck=2, training=False), 20)[0] for _ in range(3)]
    outs = gen(im, uv, None, chuck=2, training=False)
    in_place = [timed(lambda: runner.backward(gen, outs[0], t[2], t[3]), args.iters)[0]]
    gen.close()
    npix = B * S * S
    kernel_ms = kernel_stats(args.stats, KERNELS + (FORWARD_KERNEL,)) if args.stats else None
    rates = None
    if kernel_ms and all(k in kernel_ms for k in KERNELS):
        wflop, dflop = 2 * 9 * 65 * 16 * npix, 2 * 9 * 16 * 65 * npix
        wt = wflop / kernel_ms[KERNELS[2]] / 1e9
        rates = {"wgrad_gflop": round(wflop / 1e9, 3), "wgrad_tflops": round(wt, 1), "wgrad_share_of_matrix_bound": round(wt * 1e12 / MATRIX_FLOPS, 3),
                 "a1_tflops": round(wflop / kernel_ms[KERNELS[0]] / 1e9, 1),
                 "forward_fused_tflops": round(wflop / kernel_ms[FORWARD_KERNEL] / 1e9, 1) if FORWARD_KERNEL in kernel_ms else None,
                 "dgrad_tflops": round(dflop / kernel_ms[KERNELS[3]] / 1e9, 1),
                 "pixel_tb_per_s": round(140 * npix / kernel_ms[KERNELS[1]] / 1e9, 3), "dgrad_tb_per_s": round(324 * npix / kernel_ms[KERNELS[3]] / 1e9, 3),
                 "hbm_tb_per_s": HBM_BYTES_PER_S / 1e12}
    flat = res[""]
    line = {"batch": B, "size": S, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_f_l1": float(res["d_f"].abs().sum().cpu()), "d_gs_l1": float(res["d_gs"].abs().sum().cpu()),
            "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread], "backward_in_place_ms_per_call": round(in_place[0], 4),
            "generator_ms_per_call": [round(v, 3) for v in gen_ms], "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None, "rates": rates,
            "chain_kernel_ms": round(sum(kernel_ms[k] for k in KERNELS), 5) if rates else None, "stage_budget": 1e-5}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_acts"] for p in line["parity"])
    if args.build:
        with open(args.build) as f:
            line["build"] = json.load(f)
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
