"""Time of the device losses of train_step (bsr_train_losses, csrc/train_losses_kernels.h) beside the host statement, one JSON line.

B items of S x S from train_losses.example_inputs(seed 0) through TrainLosses.step_losses, with and without the three figures.
`device_ms_per_batch` / `device_ms_per_batch_figs`: device events around --iters calls after a warm-up, divided by --iters; the window
holds the allocation of the outputs, as a caller pays it.  `kernel_ms`: the device time of each of the chain's three kernels per batch,
from the profiler's kernel records of a separate run of --iters calls without figures; null, with `kernel_ms_unmeasured` true, where
the profiler returns no kernel record.  `host_ms_per_item`: train_losses.item_terms on one core, median of --host-items.
`hbm_bound_ms`: what the compulsory traffic allows at 8 TB/s — the five inputs read once (13 floats per pixel), the coarse planes
written and read once (6 x 1.33 floats per pixel each way) — and the chain's time as a multiple of it (`times_hbm_bound`).

    python tools/train_losses_bench.py [--batch 32] [--size 256] [--iters 20] [--host-items 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
KERNELS = ("losses_coarse_kernel", "losses_pixel_kernel", "losses_finish_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-items", type=int, default=3)
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import TrainLosses, train_losses as host
    B, S = args.batch, args.size
    arrays = host.example_inputs(S, B, seed=0)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in arrays]
    runner = TrainLosses(0)

    def timed(figs):
        for _ in range(args.warmup):
            runner.step_losses(*t, figs=figs)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            res = runner.step_losses(*t, figs=figs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters, res
    ms, res = timed(False)
    ms_figs, _ = timed(True)
    losses = [float(v) for v in res[0].cpu()]

    kernel_ms = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.iters):
                runner.step_losses(*t)
            torch.cuda.synchronize()
        found = {}
        for ev in prof.key_averages():
            for name in KERNELS:
                if name in ev.key:
                    total_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    found[name] = found.get(name, 0.0) + total_us / 1e3 / args.iters
        kernel_ms = {k: round(v, 4) for k, v in found.items()} if len(found) == len(KERNELS) else None
    except Exception as e:          # the profiler is optional: the figure is then reported as unmeasured
        sys.stderr.write("train_losses_bench: no per-kernel times (%s)\n" % e)

    host_ms = []
    for i in range(args.host_items):
        t0 = time.perf_counter()
        host.item_terms(*(a[i % B] for a in arrays))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    coarse = 6 * sum((S >> l) ** 2 for l in range(5))
    bound = (13 * S * S + 2 * coarse) * 4.0 * B / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"batch": B, "size": S, "losses": losses, "device_ms_per_batch": round(ms, 4), "device_ms_per_batch_figs": round(ms_figs, 4),
                      "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None, "host_ms_per_item": round(statistics.median(host_ms), 2),
                      "hbm_bound_ms": round(bound, 5),
                      "times_hbm_bound": round(sum(kernel_ms.values()) / bound, 1) if kernel_ms else None}))


if __name__ == "__main__":
    main()
