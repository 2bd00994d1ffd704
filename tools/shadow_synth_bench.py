"""Time of the device shadow synthesis (bsr_shadow_synth, csrc/shadow_synth_kernels.h) beside the host statement, one JSON line.

B items of S x S, every item on the longest route (Perlin mask, spatially varying blur of base 2, subsurface scattering with r -> 15),
drawn from a fixed seed, through ShadowSynth.process_mask with `out=` reused.  `device_ms_per_batch`: device events around --iters
calls after a warm-up, divided by --iters; this window holds the packing and upload of the draws records, as a caller pays them.
`kernel_ms`: the device time of each of the chain's four kernels per batch, from the profiler's kernel records of a separate run of
--iters calls (the forward handle's timing hooks belong to a bsr_handle, which this entry does not take); null, with
`kernel_ms_unmeasured` true, where the profiler returns no kernel record.  `host_ms_per_item`: shadow_synth.process_item on one core,
median of --host-items.  `lds_bound_ms`: what the LDS traffic of the two blur kernels allows at 128 B / clk / CU, 256 CUs, 2.4 GHz —
the Gaussians read one float per tap per pass per pixel, the discs two prefix words per disc row per pixel — and each kernel's own
time as a multiple of its bound (`times_lds_bound`).

    python tools/shadow_synth_bench.py [--batch 32] [--size 256] [--iters 20] [--host-items 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LDS_BYTES_PER_S = 128 * 256 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-items", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from blindshadowremoval_amd import ShadowSynth, shadow_synth as host
    B, S = args.batch, args.size
    rng = np.random.default_rng(0)
    r = np.nextafter(np.float32(min(15.0, host.max_scale(S))), np.float32(0))
    while True:
        try:
            host.check_scale(r, S)
            break
        except ValueError:
            r = np.nextafter(r, np.float32(0))
    full = []
    for _ in range(B):
        d = host.draw(rng, S)
        d.u_mask, d.u_ss, d.u_bright, d.u_sv, d.r, d.blur_size = np.float32(0.2), np.float32(0.6), np.float32(0.8), np.float32(0.9), r, np.int32(2)
        full.append(d)
    arrays = host.example_inputs(S, B, seed=0)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in arrays]
    synth = ShadowSynth(0)
    out = synth.process_mask(*t, full)
    for _ in range(args.warmup):
        synth.process_mask(*t, full, out=out)
    torch.cuda.synchronize()
    assert int(out[3].abs().sum()) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        synth.process_mask(*t, full, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms_full = e0.elapsed_time(e1) / args.iters

    kernel_ms = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.iters):
                synth.process_mask(*t, full, out=out)
            torch.cuda.synchronize()
        found = {}
        for ev in prof.key_averages():
            for name in ("shadow_init_kernel", "shadow_perlin_kernel", "shadow_disc_kernel", "shadow_ss_kernel"):
                if name in ev.key:
                    total_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    found[name] = found.get(name, 0.0) + total_us / 1e3 / args.iters
        kernel_ms = {k: round(v, 4) for k, v in found.items()} if len(found) == 4 else None
    except Exception as e:          # the profiler is optional: the figure is then reported as unmeasured
        sys.stderr.write("shadow_synth_bench: no per-kernel times (%s)\n" % e)

    host_ms = []
    for i in range(args.host_items):
        t0 = time.perf_counter()
        host.process_item(*(a[i % B] for a in arrays), full[i % B])
        host_ms.append((time.perf_counter() - t0) * 1e3)
    taps = sum(len(host.gaussian_taps(host.level_sigma(lv, r))) for lv in range(6))
    gauss_bytes = 2.0 * taps * 4 * S * S * B
    disc_bytes = sum(2 * (2 * rr + 1) for rr in (2, 4, 8)) * 4.0 * S * S * B
    bound = {"shadow_ss_kernel": gauss_bytes / LDS_BYTES_PER_S * 1e3, "shadow_disc_kernel": disc_bytes / LDS_BYTES_PER_S * 1e3}
    print(json.dumps({"batch": B, "size": S, "r": float(r), "device_ms_per_batch": round(ms_full, 4), "kernel_ms": kernel_ms,
                      "kernel_ms_unmeasured": kernel_ms is None, "host_ms_per_item": round(statistics.median(host_ms), 2),
                      "lds_bound_ms": {k: round(v, 4) for k, v in bound.items()},
                      "times_lds_bound": {k: round(kernel_ms[k] / v, 2) for k, v in bound.items()} if kernel_ms else None}))


if __name__ == "__main__":
    main()
