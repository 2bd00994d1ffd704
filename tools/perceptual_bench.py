"""Time of train_step's VGG19 perceptual term on the device (bsr_vgg_per_loss, csrc/vgg_kernels.h), one JSON line; the record kept in
profiles/perceptual_bench.json.

B items of S x S (2B network rows) from perceptual.example_inputs(seed 0), weights from init_vgg_weights(1), through
Perceptual.per_loss.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it.
  launch_ms              the mean device time of each of the chain's 20 launches, in launch order, from the profiler's kernel trace of a
                         SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perceptual_bench.py --calls-only
                             python tools/perceptual_bench.py --trace DIR/<host>/<pid>_kernel_trace.csv
                         with the conv launches' achieved TFLOP/s beside them (conv_tflops); null, with launch_ms_unmeasured true,
                         without --trace.
  matrix_bound_ms        the algorithmic work over the fp32 matrix peak, 157.3 TFLOP/s: per row the thirteen layers (2 x 9 C_in C_out h^2,
                         the 3 real input channels of the first), from the shapes; achieved_tflops is that work over the call time,
                         conv_tflops_cin64 the same over the trace's conv launches with C_in >= 64.
  hbm_bound_ms           the compulsory traffic at 8 TB/s: the two sources read once, every activation written and read once (the
                         materialised 8-channel input and the pooled maps included), the weights once.
  host_check             item 0's sums row of the timed call against the host statement run on item 0 alone: the largest relative
                         difference of the five sums (the float64 statement against thirteen fp32 stages).
  e2e_scaled_error       (with --parity) the largest scaled error of a tapped feature against the float64 statement over the GPU
                         suite's sizes, tests/test_perceptual_gpu.py's E2E_MEASURED.
  generator_ms_per_call  the fp32 generator forward at the same batch, by the same events; ratio_to_generator = device_ms_per_call / it.

With --grad the timed call is Perceptual.per_loss_grad (bsr_vgg_per_loss_grad, csrc/vgg_grad_kernels.h): the forward's 20 launches and
the backward's 18, and the record is profiles/perceptual_grad_bench.json (--out).  Then also:
  forward_ms_per_call    Perceptual.per_loss by the same events in the same run; backward_ms_per_call = device_ms_per_call - it, and
                         backward_over_forward their ratio (the gradient layers do the forward layers' work on half the rows: 0.5 is the
                         expectation).
  launch_ms              all 38 launches; dgrad_tflops the gradient layers' achieved TFLOP/s (B rows, 2 x 9 C_in C_out h^2, the 3 real
                         input channels of block1_conv1) beside conv_tflops, the forward launches of the same shapes in the same trace.
  scratch_bytes          bsr_vgg_grad_scratch_bytes(B, S).
  e2e_scaled_error       (with --parity) the largest scaled error of grad against perceptual.per_loss_grad(acts = the device's
                         activations) over the GPU suite's sizes, tests/test_perceptual_grad_gpu.py's E2E_MEASURED; own_forward_error the
                         same against the statement on its own float64 forward (masks can flip there: reported, not held).

    python tools/perceptual_bench.py [--batch 32] [--size 256] [--iters 40] [--trace CSV] [--calls-only] [--parity] [--grad] [--out FILE]
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
LAUNCHES = 20


def launch_names():
    from blindshadowremoval_amd.weights import VGG_LAYERS
    names = ["vgg_input_kernel"]
    for n in VGG_LAYERS:
        if n.endswith("conv1") and n != "block1_conv1":
            names.append("vgg_pool_kernel block%d_pool" % (int(n[5]) - 1))
        names.append("vgg_conv_kernel " + n)
    return names + ["vgg_l1_kernel", "vgg_finish_kernel"]


def grad_launch_names():
    """The backward chain's 18 launches in order (perceptual_gpu.grad_stages)."""
    from blindshadowremoval_amd.weights import VGG_LAYERS
    names = ["vgg_seed_kernel"]
    for i in range(len(VGG_LAYERS) - 1, -1, -1):
        names.append("vgg_conv_kernel dgrad " + VGG_LAYERS[i])
        if i and VGG_LAYERS[i].endswith("conv1"):
            names.append("vgg_unpool_kernel block%d_pool" % (int(VGG_LAYERS[i][5]) - 1))
    return names


def layer_flops(S):
    """{layer: FLOP per network row}, from the shapes."""
    from blindshadowremoval_amd.weights import VGG_LAYERS, vgg_variable_shapes
    shapes = vgg_variable_shapes()
    return {n: 2 * 9 * shapes[n + "/kernel"][2] * shapes[n + "/kernel"][3] * (S >> (int(n[5]) - 1)) ** 2 for n in VGG_LAYERS}


def traffic_bytes(S):
    """Compulsory bytes per network row (the weights not included)."""
    from blindshadowremoval_amd.weights import VGG_BLOCKS
    floats = 3 * S * S + 2 * 8 * S * S
    for b, (ch, n) in enumerate(VGG_BLOCKS):
        h = S >> b
        floats += 2 * n * ch * h * h
        if b < 4:
            floats += 2 * ch * (h // 2) ** 2
    return 4 * floats


def trace_launches(path, names=None):
    """The kernel trace's vgg_* dispatches in start order, folded onto the chain's launches (`names`; the forward's 20 without):
    mean milliseconds per launch."""
    names = names or launch_names()
    LAUNCHES = len(names)
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            if "vgg_" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    if not rows or len(rows) % LAUNCHES:
        return None
    calls = len(rows) // LAUNCHES
    skip = min(5, calls - 1)                                   # the warm-up calls
    out = [0.0] * LAUNCHES
    for c in range(skip, calls):
        for j in range(LAUNCHES):
            s, e, name = rows[c * LAUNCHES + j]
            assert names[j].split(" ")[0] in name, (j, name)
            out[j] += (e - s) / 1e6
    return [v / (calls - skip) for v in out]


def parity():
    """The largest scaled error of a tapped feature against the float64 statement over the GPU suite's sizes."""
    import numpy as np
    import torch
    from blindshadowremoval_amd import Perceptual, perceptual as host
    from blindshadowremoval_amd.weights import VGG_TAPS, init_vgg_weights
    dev = torch.device("cuda", 0)
    w = init_vgg_weights(21)
    runner = Perceptual(0)
    runner.load_weights(w)
    worst = {}
    for S, B in ((32, 1), (32, 3), (64, 2), (128, 1)):
        gt, con = host.example_inputs(S, B, seed=300 + S + B)
        ref = host.per_loss(w, gt, con)["acts"]
        acts = runner.per_loss(torch.from_numpy(gt).to(dev), torch.from_numpy(con).to(dev), keep=True)[2]
        for n in VGG_TAPS:
            e = float(np.abs(acts[n].cpu().numpy().astype(np.float64) - ref[n]).max() / np.abs(ref[n]).max())
            worst["S=%d B=%d %s" % (S, B, n)] = e
    return worst


def grad_parity():
    """The largest scaled error of grad over the GPU suite's sizes and inputs: against the statement on the device's own activations,
    and against the statement on its own float64 forward."""
    import numpy as np
    import torch
    from blindshadowremoval_amd import Perceptual, perceptual as host
    from blindshadowremoval_amd.weights import init_vgg_weights
    dev = torch.device("cuda", 0)
    w = init_vgg_weights(21)
    runner = Perceptual(0)
    runner.load_weights(w)
    held, own = {}, {}
    for S, B in ((32, 1), (32, 3), (64, 2)):
        gt, con = host.example_inputs(S, B, seed=500 + S + B)
        res = runner.per_loss_grad(torch.from_numpy(gt).to(dev), torch.from_numpy(con).to(dev), keep=True)
        got = res[2].cpu().numpy().astype(np.float64)
        acts = {k: v.cpu().numpy() for k, v in res[3].items()}
        for out, ref in ((held, host.per_loss_grad(w, gt, con, acts=acts)["grad"]), (own, host.per_loss_grad(w, gt, con)["grad"])):
            out["S=%d B=%d" % (S, B)] = float(np.abs(got - ref).max() / np.abs(ref).max())
    return held, own


def grad_main(args):
    import numpy as np
    import torch
    from blindshadowremoval_amd import Perceptual, _lib, perceptual as host
    from blindshadowremoval_amd.weights import init_vgg_weights
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    arrays = host.example_inputs(S, B, seed=0)
    t = [torch.from_numpy(a).to(dev) for a in arrays]
    weights = init_vgg_weights(1)
    runner = Perceptual(0)
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
    if args.calls_only:
        timed(lambda: runner.per_loss_grad(*t), min(args.iters, 10))
        return
    ms, res = timed(lambda: runner.per_loss_grad(*t), args.iters)
    fwd_ms, fwd = timed(lambda: runner.per_loss(*t), args.iters)
    spread = [timed(lambda: runner.per_loss_grad(*t), args.iters)[0] for _ in range(2)]
    fwd_spread = [timed(lambda: runner.per_loss(*t), args.iters)[0] for _ in range(2)]
    loss, grad = float(res[0].cpu()[0]), res[2].cpu().numpy()
    assert res[0].cpu().numpy().tobytes() == fwd[0].cpu().numpy().tobytes()
    want0 = host.per_loss_grad(weights, arrays[0][:1], arrays[1][:1])["grad"] if B == 1 else None
    held, own = grad_parity() if args.parity else (None, None)
    runner = None
    torch.cuda.empty_cache()

    from blindshadowremoval_amd import Generator, init_weights
    gen = Generator(device=0)
    gen.load_weights(init_weights(1))
    im, uv = torch.rand((B, S, S, 3), device=dev), torch.rand((B, S, S, 3), device=dev)
    gen_ms, _ = timed(lambda: gen(im, uv, None, chuck=2, training=False), 20)
    gen.close()

    flops = layer_flops(S)
    names = launch_names() + grad_launch_names()
    launch_ms = trace_launches(args.trace, names) if args.trace else None
    conv_tflops = dgrad_tflops = None
    if launch_ms:
        by_name = dict(zip(names, launch_ms))
        conv_tflops = {n: round(2 * B * f / (by_name["vgg_conv_kernel " + n] * 1e-3) / 1e12, 1) for n, f in flops.items()}
        dgrad_tflops = {n: round(B * f / (by_name["vgg_conv_kernel dgrad " + n] * 1e-3) / 1e12, 1) for n, f in flops.items()}
    bwd_flop = B * sum(flops.values())
    out = {"batch": B, "size": S, "rows_forward": 2 * B, "rows_backward": B, "loss": loss, "grad_l1": float(np.abs(grad.astype(np.float64)).sum()),
           "grad_linf": float(np.abs(grad).max()), "device_ms_per_call": round(ms, 3), "device_ms_per_call_repeats": [round(v, 3) for v in spread],
           "forward_ms_per_call": round(fwd_ms, 3), "forward_ms_per_call_repeats": [round(v, 3) for v in fwd_spread],
           "backward_ms_per_call": round(ms - fwd_ms, 3), "backward_over_forward": round((ms - fwd_ms) / fwd_ms, 3),
           "launch_ms": dict(zip(names, [round(v, 4) for v in launch_ms])) if launch_ms else None, "launch_ms_unmeasured": launch_ms is None,
           "conv_tflops": conv_tflops, "dgrad_tflops": dgrad_tflops, "backward_gflop_per_call": round(bwd_flop / 1e9, 1),
           "backward_matrix_bound_ms": round(bwd_flop / MATRIX_FLOPS * 1e3, 3),
           "backward_fraction_of_matrix_peak": round(bwd_flop / MATRIX_FLOPS * 1e3 / (ms - fwd_ms), 3),
           "scratch_bytes": int(_lib.load().bsr_vgg_grad_scratch_bytes(B, S)), "forward_scratch_bytes": int(_lib.load().bsr_vgg_scratch_bytes(B, S)),
           "host_check": None if want0 is None else float(np.abs(grad - want0).max() / np.abs(want0).max()),
           "e2e_scaled_error": held, "e2e_scaled_error_max": max(held.values()) if held else None, "own_forward_error": own,
           "generator_ms_per_call": round(gen_ms, 3), "ratio_to_generator": round(ms / gen_ms, 3)}
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "perceptual_grad_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40, help="calls per timed window: seconds of work, not a fraction of one")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", default=None, help="the kernel trace CSV of a profiled --calls-only run")
    ap.add_argument("--calls-only", action="store_true", help="the warm-up and the calls, nothing else: the program to profile")
    ap.add_argument("--parity", action="store_true", help="also measure the tapped features against the float64 statement on the GPU suite's sizes")
    ap.add_argument("--grad", action="store_true", help="time per_loss_grad, forward + backward; the record is profiles/perceptual_grad_bench.json")
    ap.add_argument("--out", default=None, help="with --grad: where the JSON line is also written (default profiles/perceptual_grad_bench.json)")
    args = ap.parse_args()
    if args.grad:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("perceptual_bench: no GPU; nothing is measured without one")
        return grad_main(args)
    import numpy as np
    import torch
    from blindshadowremoval_amd import Perceptual, _lib, perceptual as host
    from blindshadowremoval_amd.weights import init_vgg_weights
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    dev = torch.device("cuda", 0)
    arrays = host.example_inputs(S, B, seed=0)
    t = [torch.from_numpy(a).to(dev) for a in arrays]
    weights = init_vgg_weights(1)
    runner = Perceptual(0)
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
    if args.calls_only:
        timed(lambda: runner.per_loss(*t), min(args.iters, 10))
        return
    ms, res = timed(lambda: runner.per_loss(*t), args.iters)
    spread = [timed(lambda: runner.per_loss(*t), args.iters)[0] for _ in range(2)]
    loss, sums0 = float(res[0].cpu()[0]), res[1][0].cpu().numpy()
    want0 = host.per_loss(weights, arrays[0][:1], arrays[1][:1])["sums"][0]
    host_check = float((np.abs(sums0 - want0) / want0).max())
    e2e = parity() if args.parity else None
    runner = None
    torch.cuda.empty_cache()

    from blindshadowremoval_amd import Generator, init_weights
    gen = Generator(device=0)
    gen.load_weights(init_weights(1))
    im, uv = torch.rand((B, S, S, 3), device=dev), torch.rand((B, S, S, 3), device=dev)
    gen_ms, _ = timed(lambda: gen(im, uv, None, chuck=2, training=False), 20)
    gen.close()

    rows = 2 * B
    flops = layer_flops(S)
    flop = sum(flops.values())
    launch_ms = trace_launches(args.trace) if args.trace else None
    conv_tflops = cin64 = None
    if launch_ms:
        by_name = dict(zip(launch_names(), launch_ms))
        conv_tflops = {n: round(rows * f / (by_name["vgg_conv_kernel " + n] * 1e-3) / 1e12, 1) for n, f in flops.items()}
        deep = [n for n in flops if n != "block1_conv1"]
        cin64 = round(rows * sum(flops[n] for n in deep) / (sum(by_name["vgg_conv_kernel " + n] for n in deep) * 1e-3) / 1e12, 1)
    nbytes = rows * traffic_bytes(S) + 4 * sum(int(np.prod(v.shape)) for v in weights.values())
    m_bound, h_bound = rows * flop / MATRIX_FLOPS * 1e3, nbytes / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"batch": B, "size": S, "rows": rows, "loss": loss, "device_ms_per_call": round(ms, 3),
                      "device_ms_per_call_repeats": [round(v, 3) for v in spread],
                      "launch_ms": dict(zip(launch_names(), [round(v, 4) for v in launch_ms])) if launch_ms else None, "launch_ms_unmeasured": launch_ms is None,
                      "conv_tflops": conv_tflops, "conv_tflops_cin64": cin64, "gflop_per_row": round(flop / 1e9, 3), "gflop_per_call": round(rows * flop / 1e9, 1),
                      "matrix_bound_ms": round(m_bound, 3), "achieved_tflops": round(rows * flop / (ms * 1e-3) / 1e12, 1),
                      "fraction_of_matrix_peak": round(m_bound / ms, 3), "hbm_bound_ms": round(h_bound, 3), "times_hbm_bound": round(ms / h_bound, 1),
                      "scratch_gb": round(int(_lib.load().bsr_vgg_scratch_bytes(B, S)) / 1e9, 2),
                      "host_check": host_check, "e2e_scaled_error": e2e, "e2e_scaled_error_max": max(e2e.values()) if e2e else None,
                      "generator_ms_per_call": round(gen_ms, 3), "ratio_to_generator": round(ms / gen_ms, 3)}))


if __name__ == "__main__":
    main()
