"""Time of the device losses of train_step (bsr_train_losses, csrc/train_losses_kernels.h) beside the host statement, one JSON line.

B items of S x S from train_losses.example_inputs(seed 0) through TrainLosses.step_losses, with and without the three figures.
`device_ms_per_batch` / `device_ms_per_batch_figs`: device events around --iters calls after a warm-up, divided by --iters; the window
holds the allocation of the outputs, as a caller pays it.  `kernel_ms`: the device time of each of the chain's three kernels per batch,
from the profiler's kernel records of a separate run of --iters calls without figures; null, with `kernel_ms_unmeasured` true, where
the profiler returns no kernel record.  `host_ms_per_item`: train_losses.item_terms on one core, median of --host-items.
`hbm_bound_ms`: what the compulsory traffic allows at 8 TB/s — the five inputs read once (13 floats per pixel), the coarse planes
written and read once (6 x 1.33 floats per pixel each way) — and the chain's time as a multiple of it (`times_hbm_bound`).

    python tools/train_losses_bench.py [--batch 32] [--size 256] [--iters 20] [--host-items 3]

With --grad the subject is the gradient call (bsr_train_losses_grad through TrainLosses.step_losses_grad under G_TOTAL_WEIGHTS) and the
line, also written to --out (profiles/train_losses_grad_bench.json), holds
  forward_ms_per_batch     step_losses in the same process, beside forward_ms_parent = 0.43, the parent's figure.
  grad_ms_per_batch        step_losses_grad (forward and backward, six launches), device events as above.
  kernel_ms                the six kernels' device times per batch from the profiler's records, as above.
  floor_ms                 five inputs read and four gradient floats written once, 17 floats per pixel, at 8 TB/s; design_extra_bytes:
                           what the chosen design moves on top per batch (the coarse planes written and read twice, mask_edge written
                           and read twice, the sign words written and read, the maps g_l written and read), each counted once per use.
  parity                   with --parity, per (S, B) of the device tests' sizes (inputs of seed 1, as the tests use) the scaled error
                           max |grad_con - ref| / max |ref| against the host statement; e2e_measured is the largest.

    python tools/train_losses_bench.py --grad [--parity] [--out FILE]
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
GRAD_KERNELS = KERNELS + ("losses_sign_kernel", "losses_upT_kernel", "losses_grad_kernel")
PARITY_SIZES = ((32, 1), (32, 3), (64, 2), (256, 1))          # tests/train_losses_grad_cases.GPU_SIZES
FORWARD_MS_PARENT = 0.43


def kernel_times(call, names, iters):
    """The device time per call of each kernel in `names` from the profiler's records; None where it returns no record of one."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
        found = {}
        for ev in prof.key_averages():
            for name in names:
                if name in ev.key:
                    total_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    found[name] = found.get(name, 0.0) + total_us / 1e3 / iters
        return {k: round(found[k], 4) for k in names} if len(found) == len(names) else None
    except Exception as e:          # the profiler is optional: the figure is then reported as unmeasured
        sys.stderr.write("train_losses_bench: no per-kernel times (%s)\n" % e)
        return None


def grad_main(args):
    import numpy as np
    import torch
    from blindshadowremoval_amd import TrainLosses, train_losses as host
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in host.example_inputs(S, B, seed=0)]
    up = torch.tensor(host.G_TOTAL_WEIGHTS, dtype=torch.float32).to(dev)
    runner = TrainLosses(0)

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            res = call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters, res
    grad_call = lambda: runner.step_losses_grad(*t, upstream=up)
    fwd_ms, _ = timed(lambda: runner.step_losses(*t))
    grad_ms, res = timed(grad_call)
    fwd_ms2, _ = timed(lambda: runner.step_losses(*t))
    kernel_ms = kernel_times(grad_call, GRAD_KERNELS, args.iters)
    px, coarse = B * S * S, B * 6 * sum((S >> l) ** 2 for l in range(5))
    maps = B * 3 * sum((S >> l) ** 2 for l in range(5))
    floor = 17 * px * 4.0 / HBM_BYTES_PER_S * 1e3
    extra = 4 * (3 * coarse + 3 * px + 2 * px + 2 * maps)
    line = {"batch": B, "size": S, "losses": [float(v) for v in res[0].cpu()], "forward_ms_per_batch": [round(fwd_ms, 4), round(fwd_ms2, 4)],
            "forward_ms_parent": FORWARD_MS_PARENT, "grad_ms_per_batch": round(grad_ms, 4), "kernel_ms": kernel_ms, "kernel_ms_unmeasured": kernel_ms is None,
            "floor_ms": round(floor, 5), "floor_bytes": 17 * px * 4, "design_extra_bytes": extra,
            "times_floor": round(sum(kernel_ms.values()) / floor, 1) if kernel_ms else None,
            "grad_l1_linf": {k: round(v, 9) for k, v in host.grad_norms(res[2].cpu().numpy(), res[3].cpu().numpy()).items()}}
    if args.parity:
        line["parity"] = []
        for s_, b_ in PARITY_SIZES:
            arrays = host.example_inputs(s_, b_, 1)
            got = runner.step_losses_grad(*[torch.from_numpy(a).to(dev) for a in arrays], upstream=up)
            ref = host.step_losses_grad(*arrays, upstream=np.array(host.G_TOTAL_WEIGHTS, np.float32))
            err = lambda g, r: float(np.abs(g.cpu().numpy().astype(np.float64) - r).max() / np.abs(r).max())
            line["parity"].append({"S": s_, "B": b_, "grad_con_scaled_error": err(got[3], ref["grad_con"].astype(np.float64)),
                                   "grad_gs_bit_identical": got[2].cpu().numpy().tobytes() == ref["grad_gs"].tobytes()})
        line["e2e_measured"] = max(p["grad_con_scaled_error"] for p in line["parity"])
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-items", type=int, default=3)
    ap.add_argument("--grad", action="store_true", help="time the gradient call instead and write the line to --out")
    ap.add_argument("--parity", action="store_true", help="with --grad: the end-to-end scaled errors over the device tests' sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_losses_grad_bench.json"), help="with --grad: where the line is written")
    args = ap.parse_args()
    if args.grad:
        return grad_main(args)
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
