"""Time of the generator's grey decoder backward on the device (bsr_grey_decoder_grad, csrc/grey_up_grad_kernels.h), one JSON line, also
written to --out (profiles/grey_decoder_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies res2, c2, c3, y, d_y comes from
generator_grad.grey_decoder_example_inputs(seed 0), and GreyDecoder.backward reads the four tensors in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  kernel_ms              the mean device time of each of the chain's launches, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/grey_decoder_bench.py --calls-only
                             python tools/grey_decoder_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.
  rates                  with --stats: per matrix launch its executed GFLOP (2 x 9 x C_in padded x C_out per coarse pixel: up1's 257
                         columns run as 288), TFLOP/s and share of the 157.3 TFLOP/s fp32 matrix bound, beside the colour decoder's launch
                         of the same kernel from profiles/clr_decoder_grad_bench.json.
  parity                 with --parity, per (H, W, B) of the device tests' sizes the worst scaled error of the fifteen outputs against
                         generator_grad.grey_decoder_grad on the device's own activations; e2e_measured is the largest, the figure the
                         device test's bound is 4 x of.
  build                  with --build FILE, the compiler's register and LDS figures of the kernels (a JSON object, merged in as is).

    python tools/grey_decoder_bench.py [--batch 32] [--size 256] [--iters 200] [--parity] [--stats CSV] [--build FILE] [--out FILE] [--calls-only]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_FLOPS = 157.3e12
# the launches in order (the mask launch runs only when maps are kept: not in a plain call)
KERNELS = ("up_wgrad_kernel<2, true>", "up_dgrad_kernel<8, true, 8, 4>", "up_wgrad_kernel<1, true>", "up_dgrad_kernel<5, true, 8, 6>",
           "up_wgrad_kernel<3, false>", "up_dgrad_kernel<6, false, 8, 0>", "up_fold_kernel", "up_finish_kernel")
LAYER_OF = ("up3", "up3", "up2", "up2", "up1", "up1")
CHANNELS = {"up1": (288, 96, 8), "up2": (160, 64, 4), "up3": (128, 64, 2)}       # C_in as executed, C_out, the image's size over the coarse grid's
# the colour decoder's launch of the same kernel (its rates' `launch`), where it has one
COLOUR_LAUNCH = {"up_wgrad_kernel<2, true>": "up_wgrad_kernel<2, true>", "up_dgrad_kernel<8, true, 8, 4>": "up_dgrad_kernel<8, true, 8>",
                 "up_wgrad_kernel<3, false>": "up_wgrad_kernel<3, false>", "up_dgrad_kernel<6, false, 8, 0>": "up_dgrad_kernel<6, false, 8>"}
PARITY_SIZES = ((32, 256, 1), (64, 256, 2), (96, 256, 3), (32, 512, 1))


def kernel_stats(path, kernels):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in kernels:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in kernels if k in found}


def colour_shares():
    path = os.path.join(ROOT, "profiles", "clr_decoder_grad_bench.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        rates = json.loads(f.readline()).get("rates") or []
    return {r["launch"]: r["share_of_matrix_bound"] for r in rates}


def parity():
    """The device tests' cases: grey_decoder_grad_cases.case(H / 8, W / 8, B, 1), up1, up2, y from grey_decoder_forward in float32."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import grey_decoder_grad_cases as cases
    from blindshadowremoval_amd import GreyDecoder, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = GreyDecoder(0)
    for H, W, B in PARITY_SIZES:
        w, x, x3, x2, d_y = cases.case(H // 8, W // 8, B, 1)
        up1, up2, y = cases.forward32(w, x, x3, x2)
        runner.load_weights(w)
        arrays = (x, np.concatenate([up1, x3], axis=3), np.concatenate([up2, x2], axis=3), y, d_y)
        res = runner.grey_decoder_grad(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays])
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        st = host.grey_decoder_grad(w, x, x3, x2, d_y, acts={"up1": up1, "up2": up2, "y": y})
        worst = cases.worst_scaled_diff(got, st)
        out.append({"H": H, "W": W, "batch": B, "scaled_error_device_acts": float("%.3g" % worst[0]), "at": worst[1],
                    "per_output": {n: float("%.3g" % cases.worst_scaled_diff(got, st, (n,))[0]) for n in cases.OUTPUTS}})
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
    ap.add_argument("--build", default=None, help="a JSON file of the compiler's register and LDS figures, merged in under `build`")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grey_decoder_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import Generator, GreyDecoder, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("grey_decoder_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = GreyDecoder(0)
    runner.load_weights(weights)
    d_y = torch.from_numpy(host.grey_decoder_example_inputs(S // 8, S // 8, B, seed=0)[3]).to(dev)

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
    forward = lambda: gen(im, uv, None, chuck=2, training=False)                      # noqa: E731
    timed(forward, 3)
    if args.calls_only:
        timed(lambda: runner.backward(gen, d_y), min(args.iters, 20))
        return
    ms, res = timed(lambda: runner.backward(gen, d_y), args.iters)
    spread = [timed(lambda: runner.backward(gen, d_y), args.iters)[0] for _ in range(2)]
    gen.close()
    kernel_ms = kernel_stats(args.stats, KERNELS) if args.stats else None
    rates = None
    if kernel_ms and all(k in kernel_ms for k in KERNELS):
        colour = colour_shares()
        rates = []
        for kernel, layer in zip(KERNELS[:6], LAYER_OF):
            cin, cout, div = CHANNELS[layer]
            flop = 2 * 9 * cin * cout * B * (S // div) * (S // div)
            t = flop / kernel_ms[kernel] / 1e9
            rates.append({"launch": kernel, "layer": layer, "ms": kernel_ms[kernel], "executed_gflop": round(flop / 1e9, 2), "tflops": round(t, 1),
                          "share_of_matrix_bound": round(t * 1e12 / MATRIX_FLOPS, 3),
                          "colour_decoder_share_same_kernel": colour.get(COLOUR_LAUNCH.get(kernel))})
    flat = res[""]
    line = {"batch": B, "size": S, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_x_l1": float(res["d_x"].abs().sum().cpu()), "d_x3_l1": float(res["d_x3"].abs().sum().cpu()), "d_x2_l1": float(res["d_x2"].abs().sum().cpu()),
            "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread], "kernel_ms": kernel_ms,
            "kernel_ms_unmeasured": kernel_ms is None, "rates": rates,
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
