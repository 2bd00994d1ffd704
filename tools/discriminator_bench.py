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


def kernel_stats(path):
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
    return {k: round(found[k], 5) for k in KERNELS} if len(found) == len(KERNELS) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3000, help="calls per timed window: seconds of work, not a fraction of one")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="the kernel statistics CSV of a profiled --calls-only run")
    ap.add_argument("--calls-only", action="store_true", help="the warm-up and the calls, nothing else: the program to profile")
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import Discriminators, discriminator as host
    from blindshadowremoval_amd.weights import init_discriminator_weights
    if not torch.cuda.is_available():
        raise SystemExit("discriminator_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in host.example_inputs(S, B, seed=0)]
    runner = Discriminators(0)
    runner.load_weights(init_discriminator_weights(1))

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
