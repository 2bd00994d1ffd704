"""Time of the backward of res_stack/5's upper half on the device (bsr_nonlocal_grad, csrc/nonlocal_grad_kernels.h), one JSON line, also
written to --out (profiles/nonlocal_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies y3x5, res4, res5, d_x comes from
generator_grad.nonlocal_example_inputs(seed 0), and NonLocalGrad.backward reads the three tensors in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  kernel_ms              the mean device time of each of the chain's launches, from the profiler's kernel statistics of a SEPARATE run:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/nonlocal_grad_bench.py --calls-only
                             python tools/nonlocal_grad_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv
                         null, with kernel_ms_unmeasured true, without --stats.  The --calls-only program also runs the generator's
                         forward, so the same trace holds the forward's attention launches (forward_attention_rows: every row of the
                         statistics whose name holds "attention" and is not one of this chain's).
  forward_attw_ms        the forward's own per-launch device events (Generator.get_launch_timing) of res5.attw, the fused attention + w
                         launch of block 5.
  rates                  with --stats: per matrix launch its GFLOP, TFLOP/s and share of the 157.3 TFLOP/s fp32 matrix bound.  The FLOP
                         counted are the ones a launch EXECUTES, 2 T T 128 per image and product: the statistics launch forms S twice
                         and P g (3 products), the key-stationary kernel S, dP, d_g, d_phi (4), the query-stationary kernel S, dP,
                         d_theta (3).  attention_grad_algorithmic_gflop_per_image counts S, dP, d_g, d_phi, d_theta once each (5
                         products: 1.34 at T = 1024).
  parity                 with --parity, per (H, W, B) of the device tests' sizes the worst scaled error of the twelve outputs against
                         generator_grad.nonlocal_grad on the device's own out; e2e_measured is the largest, the figure the device test's
                         bound is 4 x of.
  build                  with --build FILE, the compiler's register and LDS figures of the new kernels (a JSON object, merged in as is).

    python tools/nonlocal_grad_bench.py [--batch 32] [--size 256] [--iters 200] [--parity] [--stats CSV] [--build FILE] [--out FILE] [--calls-only]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_FLOPS = 157.3e12
# the launches in order; nl_tn_kernel runs twice (launches 7 and 8), its row of the statistics is the mean of both
KERNELS = ("nl_entry_kernel", "nl_gemm_kernel<0>", "nl_att_stats_kernel", "nl_gemm_kernel<1>", "nl_att_bwd_key_kernel", "nl_att_bwd_query_kernel",
           "nl_tn_kernel", "nl_colsum_kernel", "nl_gemm_kernel<2>", "nl_fold_kernel", "nl_finish_kernel")
PARITY_SIZES = ((32, 256, 1), (64, 256, 2), (96, 256, 3), (32, 512, 1), (256, 256, 1))


def flops(B, T):
    """kernel -> the FLOP its launches execute on B images of T tokens (nl_tn_kernel: both launches' mean, as its statistics row is)."""
    N, prod = B * T, 2.0 * B * T * T * 128
    return {"nl_gemm_kernel<0>": 2.0 * N * 257 * 384, "nl_att_stats_kernel": 3 * prod, "nl_gemm_kernel<1>": 2.0 * N * 257 * 128,
            "nl_att_bwd_key_kernel": 4 * prod, "nl_att_bwd_query_kernel": 3 * prod, "nl_tn_kernel": (2.0 * N * 257 * 384 + 2.0 * N * 128 * 257) / 2,
            "nl_gemm_kernel<2>": 2.0 * N * 384 * 257}


def kernel_stats(path, kernels):
    found, rows = {}, []
    with open(path) as f:
        for row in csv.DictReader(f):
            mine = False
            for name in kernels:
                if name in row["Name"]:
                    found[name] = found.get(name, 0.0) + float(row["AverageNs"]) / 1e6
                    mine = True
            if "attention" in row["Name"] and not mine:
                rows.append({"name": row["Name"][:120], "calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 5)})
    return {k: round(found[k], 5) for k in kernels if k in found}, rows


def parity():
    """The device tests' cases: nonlocal_grad_cases.case(H / 8, W / 8, B, 1) through nonlocal_grad_cases.device_inputs."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nonlocal_grad_cases as cases
    from blindshadowremoval_amd import NonLocalGrad, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = NonLocalGrad(0)
    for H, W, B in PARITY_SIZES:
        w, y3, xin, d_out = cases.case(H // 8, W // 8, B, 1)
        arrays, y3_used = cases.device_inputs(w, y3, xin, d_out)
        runner.load_weights(w)
        res = runner.nonlocal_grad(*[torch.from_numpy(a).to(dev) for a in arrays])
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        worst = cases.worst_scaled_diff(got, host.nonlocal_grad(w, y3_used, xin, d_out, acts={"out": arrays[2]}))
        out.append({"H": H, "W": W, "batch": B, "scaled_error_device_out": float("%.3g" % worst[0]), "at": worst[1]})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlocal_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import Generator, NonLocalGrad, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("nonlocal_grad_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    T = (S // 8) * (S // 8)
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = NonLocalGrad(0)
    runner.load_weights(weights)
    d_x = torch.from_numpy(host.nonlocal_example_inputs(S // 8, S // 8, B, seed=0)[2]).to(dev)

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
    if args.calls_only:
        timed(forward, 10)
        timed(lambda: runner.backward(gen, d_x), min(args.iters, 20))
        return
    gen_ms = [timed(forward, 20)[0] for _ in range(3)]
    gen.set_timing(True)
    forward()
    torch.cuda.synchronize()
    attw_ms = {name: round(ms, 5) for name, ms, _ in gen.get_launch_timing() if name.startswith("res5.att")}
    gen.set_timing(False)
    forward()
    ms, res = timed(lambda: runner.backward(gen, d_x), args.iters)
    spread = [timed(lambda: runner.backward(gen, d_x), args.iters)[0] for _ in range(2)]
    gen.close()
    kernel_ms, forward_rows = kernel_stats(args.stats, KERNELS) if args.stats else (None, None)
    rates = None
    if kernel_ms and all(k in kernel_ms for k in KERNELS):
        rates = []
        for kernel, flop in flops(B, T).items():
            t = flop / kernel_ms[kernel] / 1e9
            rates.append({"launch": kernel, "gflop_executed": round(flop / 1e9, 2), "tflops": round(t, 1),
                          "share_of_matrix_bound": round(t * 1e12 / MATRIX_FLOPS, 3)})
    flat = res[""]
    line = {"batch": B, "size": S, "tokens": T, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_y3_l1": float(res["d_y3"].abs().sum().cpu()), "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread],
            "generator_ms_per_call": [round(v, 3) for v in gen_ms], "forward_attw_ms": attw_ms, "kernel_ms": kernel_ms,
            "kernel_ms_unmeasured": kernel_ms is None, "forward_attention_rows": forward_rows, "rates": rates,
            "attention_grad_algorithmic_gflop_per_image": round(5 * 2.0 * T * T * 128 / 1e9, 3),
            "projection_gflop_per_image": round(2.0 * T * 257 * 384 / 1e9, 3),
            "chain_kernel_ms": round(sum(kernel_ms[k] for k in KERNELS) + kernel_ms["nl_tn_kernel"], 5) if rates else None, "stage_budget": 1e-5}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_out"] for p in line["parity"])
    if args.build:
        with open(args.build) as f:
            line["build"] = json.load(f)
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
