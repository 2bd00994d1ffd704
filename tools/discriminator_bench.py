"""Time of train_step's three discriminators and GAN losses on the device (bsr_disc_losses, csrc/disc_kernels.h), one JSON line; the
record kept in profiles/discriminator_bench.json.

B items of S x S (2B discriminator rows) from discriminator.example_inputs(seed 0), weights from init_discriminator_weights(1),
through Discriminators.gan_losses.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it.
  kernel_ms              the mean device time of each kernel of the chain, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/discriminator_bench.py --calls-only
                             python tools/discriminator_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.
  matrix_bound_ms        the algorithmic work over the fp32 matrix peak, 157.3 TFLOP/s: per row the four stride-2 layers (2 x 16 C_in
                         C_out Ho^2, the 6 real input channels of the first) and the head (2 x 1024 h^2) of the three scales, from the
                         shapes; times_matrix_bound is the chain's kernel time (the call time without --stats) over it.
  hbm_bound_ms           the compulsory traffic at 8 TB/s: the three sources read once, every activation written and read once (the
                         materialised 8-channel inputs included).
  generator_ms_per_call  the fp32 generator forward at the same batch, by the same events; ratio_to_generator = device_ms_per_call / it.

    python tools/discriminator_bench.py [--batch 32] [--size 256] [--iters 3000] [--stats CSV] [--calls-only]

With --grad the call is Discriminators.gen_grad (bsr_disc_gen_grad, csrc/disc_grad_kernels.h: the forward's seven launches and the six of
d gen / d con_rgb) and the line, also written to --out (profiles/discriminator_grad_bench.json), holds
  device_ms_per_call       forward plus backward by device events, and forward_ms_per_call, the forward alone (gan_losses) in the same run,
                           beside forward_ms_parent, the figure of profiles/discriminator_bench.json, and its run-to-run spread there.
  kernel_ms                with --stats, all thirteen launches; conv_rate holds, per stride-2 layer, the forward launch's and the gradient
                           launch's TFLOP/s from the shapes (the gradient works on the B fake rows: half the forward's work; conv0's
                           gradient is wanted on 3 of its input channels only and is counted so).
  parity                   with --parity, per (S, B) of the device tests' sizes the scaled error max |grad - ref| / max |ref| against
                           discriminator.gen_grad on the device's own masks, and against the statement's own float64 forward; e2e_measured
                           is the largest of the former, the figure the device test's bound is 4 x of.
  build                    with --build FILE, the compiler's register and LDS figures of the new kernels (a JSON object, merged in as is).

    python tools/discriminator_bench.py --grad [--parity] [--stats CSV] [--build FILE] [--out FILE] [--calls-only]

With --wgrad the call is Discriminators.disc_grad (bsr_disc_wgrad, csrc/disc_wgrad_kernels.h: the forward's seven launches and the eleven of
d d_total_loss / d the discriminators' variables) and the line, written to --out (profiles/discriminator_wgrad_bench.json), holds
  device_ms_per_call       disc_grad by device events, beside gan_losses_ms_per_call and gen_grad_ms_per_call in the same run.
  kernel_ms                with --stats, all eighteen launches; wgrad_rate holds, per stride-2 layer, the forward launch's and the
                           kernel-gradient launch's TFLOP/s from the shapes (both work on all 2B rows and the 6 real input channels of
                           conv0: the same FLOP) and the latter's share of the 157.3 TFLOP/s fp32 matrix bound.
  parity                   with --parity, per (S, B) of the device tests' sizes and the hinge case the worst scaled error of a variable's
                           gradient against discriminator.disc_grad on the device's own masks and logits, and against the statement's
                           own float64 forward; e2e_measured is the largest of the former, the figure the device test's bound is 4 x of.
  build                    with --build FILE, the compiler's register and LDS figures of the new kernels.

    python tools/discriminator_bench.py --wgrad [--parity] [--stats CSV] [--build FILE] [--out FILE] [--calls-only]
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
KERNELS = ("disc_input_kernel", "disc_conv_kernel<8, 32>", "disc_conv_kernel<32, 32>", "disc_conv_kernel<32, 64>", "disc_conv_kernel<64, 64>",
           "disc_head_kernel", "disc_finish_kernel")
GRAD_KERNELS = ("disc_head_grad_kernel", "disc_dgrad_kernel<64, 64>", "disc_dgrad_kernel<64, 32>", "disc_dgrad_kernel<32, 32>", "disc_dgrad_in_kernel",
                "disc_gather_kernel")
PARITY_SIZES = ((32, 1), (32, 3), (64, 2), (128, 1))
WGRAD_KERNELS = ("disc_wgrad_seed_kernel", "disc_head_wgrad_kernel", "disc_wgrad_kernel<64, 64>", "disc_dgrad_kernel<64, 64>", "disc_wgrad_kernel<32, 64>",
                 "disc_dgrad_kernel<64, 32>", "disc_wgrad_kernel<32, 32>", "disc_dgrad_kernel<32, 32>", "disc_wgrad_kernel<8, 32>", "disc_wgrad_fold_kernel",
                 "disc_wgrad_finish_kernel")


def work(S):
    """(FLOP, bytes of compulsory traffic) per discriminator row, from the shapes."""
    from blindshadowremoval_amd import discriminator as host
    from blindshadowremoval_amd.weights import DISC_CH
    flop, floats = 0, 6 * S * S                                  # the sources: image 3 + mask 3 per pixel
    for k in (1, 2, 3):
        sides = host.map_sides(S, k)
        floats += 2 * 8 * sides[0] ** 2                          # the 8-channel input, written and read
        cin = 6
        for i, n in enumerate(DISC_CH):
            flop += 2 * 16 * cin * n * sides[i + 1] ** 2
            floats += 2 * n * sides[i + 1] ** 2
            cin = n
        flop += 2 * 16 * cin * sides[-1] ** 2
    return flop, 4 * floats


def kernel_stats(path, kernels=KERNELS):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in kernels:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in kernels} if len(found) == len(kernels) else None


def conv_flop(S, i, cin=None):
    """FLOP of stride-2 layer i per discriminator row over the three scales, from the shapes."""
    from blindshadowremoval_amd import discriminator as host
    from blindshadowremoval_amd.weights import DISC_CH
    cin = cin if cin is not None else (6 if i == 0 else DISC_CH[i - 1])
    return sum(2 * 16 * cin * DISC_CH[i] * host.map_sides(S, k)[i + 1] ** 2 for k in (1, 2, 3))


def parity():
    """The device tests' cases: init_discriminator_weights(3), discriminator.example_inputs(S, B, 1)."""
    import numpy as np
    import torch
    from blindshadowremoval_amd import Discriminators, discriminator as host
    from blindshadowremoval_amd.weights import init_discriminator_weights
    out, dev, weights = [], torch.device("cuda", 0), init_discriminator_weights(3)
    runner = Discriminators(0)
    runner.load_weights(weights)
    for S, B in PARITY_SIZES:
        arrays = host.example_inputs(S, B, 1)
        res = runner.gen_grad(*[torch.from_numpy(a).to(dev) for a in arrays], keep=True)
        torch.cuda.synchronize()
        grad, acts = res[2].cpu().numpy().astype(np.float64), {k: v.cpu().numpy() for k, v in res[3].items()}
        err = []
        for ref in (host.gen_grad(weights, *arrays, acts=acts)["grad"], host.gen_grad(weights, *arrays)["grad"]):
            err.append(float(np.abs(grad - ref).max() / np.abs(ref).max()))
        out.append({"size": S, "batch": B, "scaled_error_device_masks": float("%.3g" % err[0]), "scaled_error_own_forward": float("%.3g" % err[1])})
    return out


def main_grad(args, runner, weights, t, timed):
    import torch
    B, S = args.batch, args.size
    if args.calls_only:
        timed(lambda: runner.gen_grad(*t), min(args.iters, 20))
        return
    ms, res = timed(lambda: runner.gen_grad(*t), args.iters)
    fwd = [timed(lambda: runner.gan_losses(*t), args.iters)[0] for _ in range(2)]
    spread = [timed(lambda: runner.gen_grad(*t), args.iters)[0] for _ in range(2)]
    g = res[2]
    with open(os.path.join(ROOT, "profiles", "discriminator_bench.json")) as f:
        parent = json.loads(f.readline())
    kernel_ms = kernel_stats(args.stats, KERNELS + GRAD_KERNELS) if args.stats else None
    rate = None
    if kernel_ms:
        rate = {}
        fwd_names, grad_names = KERNELS[1:5], (GRAD_KERNELS[4], GRAD_KERNELS[3], GRAD_KERNELS[2], GRAD_KERNELS[1])
        for i in range(4):
            f_flop, g_flop = 2 * B * conv_flop(S, i), B * conv_flop(S, i, 3 if i == 0 else None)
            rate["conv%d" % i] = {"forward_kernel": fwd_names[i], "forward_gflop": round(f_flop / 1e9, 3),
                                  "forward_tflops": round(f_flop / kernel_ms[fwd_names[i]] / 1e9, 1), "grad_kernel": grad_names[i],
                                  "grad_gflop": round(g_flop / 1e9, 3), "grad_tflops": round(g_flop / kernel_ms[grad_names[i]] / 1e9, 1),
                                  "grad_ms_over_half_forward_ms": round(kernel_ms[grad_names[i]] / (0.5 * kernel_ms[fwd_names[i]]), 2)}
    line = {"batch": B, "size": S, "losses": [float(v) for v in res[0].cpu()], "grad_l1": float(g.abs().sum().cpu()), "grad_linf": float(g.abs().max().cpu()),
            "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread],
            "forward_ms_per_call": round(min(fwd), 4), "forward_ms_per_call_repeats": [round(v, 4) for v in fwd],
            "forward_ms_parent": parent["device_ms_per_call"], "forward_ms_parent_repeats": parent["device_ms_per_call_repeats"],
            "backward_ms_per_call": round(ms - min(fwd), 4), "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None, "conv_rate": rate,
            "backward_kernel_ms": round(sum(kernel_ms[k] for k in GRAD_KERNELS), 5) if kernel_ms else None}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_masks"] for p in line["parity"])
    if args.build:
        with open(args.build) as f:
            line["build"] = json.load(f)
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def wgrad_parity():
    """The device tests' cases: init_discriminator_weights(3), discriminator.example_inputs(S, B, 1), and the hinge case."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import discriminator_cases as dcases
    from blindshadowremoval_amd import Discriminators, discriminator as host
    from blindshadowremoval_amd.weights import discriminator_trainable_names, init_discriminator_weights
    out, dev, names = [], torch.device("cuda", 0), discriminator_trainable_names()
    runner = Discriminators(0)

    def worst(got, ref):
        return max(float(np.abs(got[n].astype(np.float64) - ref[n]).max() / np.abs(ref[n]).max()) for n in names if np.abs(ref[n]).max() > 0)
    for S, B in PARITY_SIZES + ((128, 2),):
        weights, arrays = (init_discriminator_weights(3), host.example_inputs(S, B, 1)) if (S, B) != (128, 2) else (lambda c: (c[0], c[1:]))(dcases.hinge_case())
        runner.load_weights(weights)
        res = runner.disc_grad(*[torch.from_numpy(a).to(dev) for a in arrays], keep=True, logits=True)
        torch.cuda.synchronize()
        grads = {k: v.cpu().numpy() for k, v in res[2].items()}
        logits, acts = [y.cpu().numpy() for y in res[3]], {k: v.cpu().numpy() for k, v in res[4].items()}
        err = [worst(grads, host.disc_grad(weights, *arrays, acts=acts, logits=logits)), worst(grads, host.disc_grad(weights, *arrays))]
        out.append({"size": S, "batch": B, "scaled_error_device_masks": float("%.3g" % err[0]), "scaled_error_own_forward": float("%.3g" % err[1])})
    return out


def main_wgrad(args, runner, t, timed):
    B, S = args.batch, args.size
    if args.calls_only:
        timed(lambda: runner.disc_grad(*t), min(args.iters, 20))
        return
    ms, res = timed(lambda: runner.disc_grad(*t), args.iters)
    fwd = [timed(lambda: runner.gan_losses(*t), args.iters)[0] for _ in range(2)]
    gen = [timed(lambda: runner.gen_grad(*t), args.iters)[0] for _ in range(2)]
    spread = [timed(lambda: runner.disc_grad(*t), args.iters)[0] for _ in range(2)]
    flat = res[2][""]
    kernel_ms = kernel_stats(args.stats, KERNELS + WGRAD_KERNELS) if args.stats else None
    rate = None
    if kernel_ms:
        rate = {}
        fwd_names, grad_names = KERNELS[1:5], (WGRAD_KERNELS[8], WGRAD_KERNELS[6], WGRAD_KERNELS[4], WGRAD_KERNELS[2])
        for i in range(4):
            flop = 2 * B * conv_flop(S, i)
            tflops = flop / kernel_ms[grad_names[i]] / 1e9
            rate["conv%d" % i] = {"forward_kernel": fwd_names[i], "gflop": round(flop / 1e9, 3), "forward_tflops": round(flop / kernel_ms[fwd_names[i]] / 1e9, 1),
                                  "wgrad_kernel": grad_names[i], "wgrad_tflops": round(tflops, 1), "wgrad_share_of_matrix_bound": round(tflops * 1e12 / MATRIX_FLOPS, 3),
                                  "wgrad_ms_over_forward_ms": round(kernel_ms[grad_names[i]] / kernel_ms[fwd_names[i]], 2)}
    line = {"batch": B, "size": S, "losses": [float(v) for v in res[0].cpu()], "d_grad_l1": float(flat.abs().sum().cpu()), "d_grad_linf": float(flat.abs().max().cpu()),
            "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread],
            "gan_losses_ms_per_call": round(min(fwd), 4), "gan_losses_ms_per_call_repeats": [round(v, 4) for v in fwd],
            "gen_grad_ms_per_call": round(min(gen), 4), "gen_grad_ms_per_call_repeats": [round(v, 4) for v in gen],
            "backward_ms_per_call": round(ms - min(fwd), 4), "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None, "wgrad_rate": rate,
            "backward_kernel_ms": round(sum(kernel_ms[k] for k in WGRAD_KERNELS), 5) if kernel_ms else None, "stage_budget": 1e-5,
            "stage_budget_note": "every stage figure measured on the device tests' sizes is below the fp32-class budget 1e-5; no stage budget is widened"}
    if args.parity:
        line["parity"] = wgrad_parity()
        line["e2e_measured"] = max(p["scaled_error_device_masks"] for p in line["parity"])
    if args.build:
        with open(args.build) as f:
            line["build"] = json.load(f)
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3000, help="calls per timed window: seconds of work, not a fraction of one")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="the kernel statistics CSV of a profiled --calls-only run")
    ap.add_argument("--calls-only", action="store_true", help="the warm-up and the calls, nothing else: the program to profile")
    ap.add_argument("--grad", action="store_true", help="time gen_grad (forward + d gen / d con_rgb) and the forward alone in the same run")
    ap.add_argument("--wgrad", action="store_true", help="time disc_grad (forward + d d_total_loss / d the variables) beside gan_losses and gen_grad")
    ap.add_argument("--parity", action="store_true", help="with --grad or --wgrad: the end-to-end scaled errors over the device tests' sizes")
    ap.add_argument("--build", default=None, help="with --grad: a JSON file of the compiler's register and LDS figures, merged in under `build`")
    ap.add_argument("--out", default=None, help="with --grad or --wgrad: where the line is written (profiles/discriminator_[w]grad_bench.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "discriminator_%s_bench.json" % ("wgrad" if args.wgrad else "grad"))
    import torch
    from blindshadowremoval_amd import Discriminators, discriminator as host
    from blindshadowremoval_amd.weights import init_discriminator_weights
    if not torch.cuda.is_available():
        raise SystemExit("discriminator_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in host.example_inputs(S, B, seed=0)]
    runner = Discriminators(0)
    weights = init_discriminator_weights(1)
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
    if args.wgrad:
        return main_wgrad(args, runner, t, timed)
    if args.grad:
        return main_grad(args, runner, weights, t, timed)
    if args.calls_only:
        timed(lambda: runner.gan_losses(*t), min(args.iters, 20))
        return
    ms, res = timed(lambda: runner.gan_losses(*t), args.iters)
    spread = [timed(lambda: runner.gan_losses(*t), args.iters)[0] for _ in range(2)]
    losses = [float(v) for v in res[0].cpu()]

    from blindshadowremoval_amd import Generator, init_weights
    gen = Generator(device=0)
    gen.load_weights(init_weights(1))
    im, uv = torch.rand((B, S, S, 3), device=dev), torch.rand((B, S, S, 3), device=dev)
    gen_ms, _ = timed(lambda: gen(im, uv, None, chuck=2, training=False), 20)
    gen.close()

    kernel_ms = kernel_stats(args.stats) if args.stats else None
    flop, nbytes = work(S)
    rows = 2 * B
    m_bound, h_bound = rows * flop / MATRIX_FLOPS * 1e3, rows * nbytes / HBM_BYTES_PER_S * 1e3
    chain = sum(kernel_ms.values()) if kernel_ms else ms
    print(json.dumps({"batch": B, "size": S, "rows": rows, "losses": losses, "device_ms_per_call": round(ms, 4),
                      "device_ms_per_call_repeats": [round(v, 4) for v in spread], "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None,
                      "gflop_per_row": round(flop / 1e9, 4), "gflop_per_call": round(rows * flop / 1e9, 2), "matrix_bound_ms": round(m_bound, 4),
                      "times_matrix_bound": round(chain / m_bound, 1), "hbm_bound_ms": round(h_bound, 4), "times_hbm_bound": round(chain / h_bound, 1),
                      "generator_ms_per_call": round(gen_ms, 3), "ratio_to_generator": round(ms / gen_ms, 4)}))


if __name__ == "__main__":
    main()
