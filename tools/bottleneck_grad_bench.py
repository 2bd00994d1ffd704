"""Time of the backward of res_stack/5's lower half on the device (bsr_bottleneck_grad, csrc/bottleneck_grad_kernels.h), one JSON line,
also written to --out (profiles/bottleneck_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies res4, d_y3 and d_skip come from
generator_grad.bottleneck_example_inputs(seed 0), and BottleneckGrad.backward reads xin in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  kernel_ms              the mean device time of each of the chain's launches, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bottleneck_grad_bench.py --calls-only
                             python tools/bottleneck_grad_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.  nl_tn_kernel runs twice in the chain (launches 7 and
                         8): its row is the mean of both.
  rates                  with --stats: per matrix launch its executed GFLOP, TFLOP/s and share of the 157.3 TFLOP/s fp32 matrix bound.
  forward_conv2_ms       the forward's own per-launch device events (Generator.get_launch_timing) of res5.conv2 on the same shape, as the
                         generator runs it (Winograd) and with BSR_WINO_CONV2=0 (the direct kernel): the row beside the two 3x3 launches.
  parity                 with --parity, per (h, w, B) of the device tests' sizes the worst scaled error of the thirteen outputs against
                         generator_grad.bottleneck_grad on the device's own a1, a2; e2e_measured is the largest, the figure the device
                         test's bound is 4 x of.

    python tools/bottleneck_grad_bench.py [--batch 32] [--size 256] [--iters 200] [--parity] [--stats CSV] [--out FILE] [--calls-only]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_FLOPS = 157.3e12
KERNELS = ("bn_entry_kernel", "bn_gemm_kernel<0>", "bn_conv3_kernel<0>", "bn_gemm_kernel<1>", "bn_conv3_kernel<1>", "bn_wgrad3_kernel", "nl_tn_kernel",
           "bn_gemm_kernel<2>", "bn_colsum_kernel", "bn_fold_kernel", "bn_finish_kernel")


def flops(N):
    """kernel -> the FLOP its launches execute on N pixels (nl_tn_kernel: both launches' mean, as its statistics row is)."""
    k3 = 2.0 * N * 9 * 128 * 128
    return {"bn_gemm_kernel<0>": 2.0 * N * 272 * 128, "bn_conv3_kernel<0>": k3, "bn_gemm_kernel<1>": 2.0 * N * 272 * 128, "bn_conv3_kernel<1>": k3,
            "bn_wgrad3_kernel": k3, "nl_tn_kernel": (2.0 * N * 128 * 384 + 2.0 * N * 320 * 128) / 2, "bn_gemm_kernel<2>": 2.0 * N * 128 * 384}


def kernel_stats(path):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in KERNELS if k in found}


def parity():
    """The device tests' cases: bottleneck_grad_cases.case(h, w, B, 1) over GPU_SIZES."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bottleneck_grad_cases as cases
    from blindshadowremoval_amd import BottleneckGrad, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = BottleneckGrad(0)
    for h, w, B in cases.GPU_SIZES:
        wt, xin, d_y3, d_skip = cases.case(h, w, B, 1)
        runner.load_weights(wt)
        res = runner.bottleneck_grad(*[torch.from_numpy(a).to(dev) for a in (xin, d_y3, d_skip)], keep=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        worst = cases.worst_scaled_diff(got, host.bottleneck_grad(wt, xin, d_y3, d_skip, acts={"a1": got["a1"], "a2": got["a2"]}))
        out.append({"h": h, "w": w, "batch": B, "scaled_error_device_acts": float("%.3g" % worst[0]), "at": worst[1]})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bottleneck_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import BottleneckGrad, Generator, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("bottleneck_grad_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    N = B * (S // 8) * (S // 8)
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = BottleneckGrad(0)
    runner.load_weights(weights)
    _, d_y3, d_skip = (torch.from_numpy(a).to(dev) for a in host.bottleneck_example_inputs(S // 8, S // 8, B, seed=0))

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

    def conv2_ms(direct):
        """res5.conv2's device time in a forward of a generator created with or without the Winograd form."""
        if direct:
            os.environ["BSR_WINO_CONV2"] = "0"
        try:
            g = Generator(device=0)
            g.load_weights(weights)
        finally:
            os.environ.pop("BSR_WINO_CONV2", None)
        for _ in range(3):
            g(im, uv, None, chuck=2, training=False)
        g.set_timing(True)
        g(im, uv, None, chuck=2, training=False)
        torch.cuda.synchronize()
        out = {name: round(ms, 5) for name, ms, _ in g.get_launch_timing() if name.startswith("res5.conv2")}
        g.close()
        return out

    gen = Generator(device=0)
    gen.load_weights(weights)
    forward = lambda: gen(im, uv, None, chuck=2, training=False)                      # noqa: E731
    call = lambda: runner.backward(gen, d_y3, d_skip)                                 # noqa: E731
    if args.calls_only:
        timed(forward, 10)
        timed(call, min(args.iters, 20))
        return
    forward()
    ms, res = timed(call, args.iters)
    spread = [timed(call, args.iters)[0] for _ in range(2)]
    gen.close()
    kernel_ms = kernel_stats(args.stats) if args.stats else None
    rates = None
    if kernel_ms and all(k in kernel_ms for k in KERNELS):
        rates = []
        for kernel, flop in flops(N).items():
            t = flop / kernel_ms[kernel] / 1e9
            rates.append({"launch": kernel, "gflop_executed": round(flop / 1e9, 2), "tflops": round(t, 1),
                          "share_of_matrix_bound": round(t * 1e12 / MATRIX_FLOPS, 3)})
    flat = res[""]
    line = {"batch": B, "size": S, "pixels": N, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_xin_l1": float(res["d_xin"].abs().sum().cpu()), "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread],
            "forward_conv2_ms": {"winograd": conv2_ms(False), "direct": conv2_ms(True)}, "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None,
            "rates": rates, "conv3x3_gflop": round(2.0 * N * 9 * 128 * 128 / 1e9, 2),
            "chain_kernel_ms": round(sum(kernel_ms[k] for k in KERNELS) + kernel_ms["nl_tn_kernel"], 5) if rates else None, "stage_budget": 1e-5}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_acts"] for p in line["parity"])
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
