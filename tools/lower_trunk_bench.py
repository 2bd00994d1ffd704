"""Time of the backward of res_stack/2, res_stack/1 and res_stack/0 on the device (bsr_lower_trunk_grad, csrc/block_chain_grad.h),
one JSON line, also written to --out (profiles/lower_trunk_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies the seven tensors, d_res2 comes from
generator_grad.lower_trunk_example_inputs(seed 0), and LowerTrunk.backward reads the seven tensors in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  narrow_launches        block 0's launches 2 (a1: K = 112), 8 (conv1's kernel gradient: two row tiles) and 9 (the data gradient: one
                         column tile) against block 1's (K = 272, five row tiles, three column tiles) from the same run: the chain
                         stopped after the launch and after the one before it (bsr_debug_lower_trunk_grad), device events around
                         --iters calls of each into outputs allocated beforehand, the difference of the two.
  parity                 with --parity, per (h, w, B) of the device tests' grids the worst scaled error of the 67 outputs against
                         generator_grad.lower_trunk_grad on the device's own activations; e2e_measured is the largest, the figure the
                         device test's bound is 4 x of.  Also `chained`: on a forward at (32, 256), B = 2 with init_weights(1) and
                         inputs from default_rng(21), the device walk over objective.BACKWARD's five stages, GreyDecoder.backward,
                         ColourTrunk.backward and LowerTrunk.backward against the eight host statements chained on the device's own
                         activations; chained_measured is its worst scaled error, the figure the device test's chained bound is 4 x of.
  scratch_bytes          bsr_lower_trunk_grad_scratch_bytes at these sizes.

    python tools/lower_trunk_bench.py [--batch 32] [--size 256] [--iters 100] [--parity] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parity():
    """The device tests' cases: lower_trunk_grad_cases.device_parity over GPU_SIZES."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lower_trunk_grad_cases as cases
    from blindshadowremoval_amd import LowerTrunk
    out = []
    runner = LowerTrunk(0)
    for h, w, B in cases.GPU_SIZES:
        _, _, _, got, worst, at, st = cases.device_parity(runner, h, w, B)
        out.append({"h": h, "w": w, "batch": B, "scaled_error_device_acts": float("%.3g" % worst), "at": at,
                    "per_output": {n: float("%.3g" % cases.worst_scaled_diff(got, st, (n,))[0]) for n in cases.OUTPUTS}})
    return out


def chained():
    """tests/test_lower_trunk_grad_gpu.py's test_the_whole_backward_chained as a measurement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lower_trunk_grad_cases as cases
    gen, w, inputs, outs, probes = cases.generated_forward()
    res, st, share = cases.whole_backward_chained(gen, w, inputs, outs, probes)
    worst, at = cases.worst_scaled_diff(res, st)
    gen.close()
    return {"H": 32, "W": 256, "batch": 2, "bmask_share": round(share, 4), "scaled_error_device_acts": float("%.3g" % worst), "at": at,
            "d_x0": float("%.3g" % cases.worst_scaled_diff(res, st, ("d_x0",))[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parity", action="store_true", help="the end-to-end scaled errors over the device tests' grids")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lower_trunk_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import Generator, LowerTrunk, _lib, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("lower_trunk_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    g = S // 8
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = LowerTrunk(0)
    runner.load_weights(weights)
    d_res2 = torch.from_numpy(host.lower_trunk_example_inputs(g, g, B, seed=0)[1]).to(dev)

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
    timed(lambda: gen(im, uv, None, chuck=2, training=False), 3)
    ms, res = timed(lambda: runner.backward(gen, d_res2), args.iters)
    spread = [timed(lambda: runner.backward(gen, d_res2), args.iters)[0] for _ in range(2)]
    # the chain stopped after launch n, into outputs allocated once: the prefix's time
    lib = _lib.load()
    ptrs, strides, _ = gen.last_lower_trunk()
    d_x0, flat = torch.empty((B, g, g, 99), device=dev), torch.empty((int(lib.bsr_lower_trunk_grad_floats()),), device=dev)
    scratch = ctypes.c_void_p(runner.stage_scratch(B, g, g))
    strided = [a for p, cs in zip(ptrs, strides) for a in (ctypes.c_void_p(p), int(cs))]

    def prefix(n):
        return timed(lambda: runner.call(runner._blob, ctypes.c_size_t(runner._blob.numel()), *strided, d_res2, B, g, g, d_x0, flat, scratch, n,
                                         symbol="bsr_debug_lower_trunk_grad"), args.iters)[0]

    narrow = {}
    for launch, what in ((2, "a1 = lrelu(xp w1f + b1f)"), (8, "xp^T gz1 partials"), (9, "d_xin = d_skip + gz1 w1t")):
        row = {"what": what}
        for block, first in ((1, 36), (0, 60)):                  # the bottleneck chain's launches of block 1 are 37..48, of block 0 61..72
            before, after = prefix(first + launch - 1), prefix(first + launch)
            row["block%d_ms" % block] = round(after - before, 4)
        row["block0_of_block1"] = round(row["block0_ms"] / row["block1_ms"], 3) if row["block1_ms"] > 0 else None
        narrow["launch_%d" % launch] = row
    assert torch.equal(runner.backward(gen, d_res2)[""], res[""])
    gen.close()
    flat = res[""]
    line = {"batch": B, "size": S, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_x0_l1": float(res["d_x0"].abs().sum().cpu()), "device_ms_per_call": round(ms, 4),
            "device_ms_per_call_repeats": [round(v, 4) for v in spread], "launches": len(runner.LAUNCHES), "narrow_launches": narrow,
            "colour_trunk_ms_per_call": 4.05, "scratch_bytes": int(lib.bsr_lower_trunk_grad_scratch_bytes(B, g, g)), "stage_budget": 1e-5}
    if args.parity:
        line["parity"] = parity()
        line["e2e_measured"] = max(p["scaled_error_device_acts"] for p in line["parity"])
        line["chained"] = chained()
        line["chained_measured"] = line["chained"]["scaled_error_device_acts"]
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
