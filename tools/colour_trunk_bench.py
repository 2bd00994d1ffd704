"""Time of the backward of res_stack/4, res_stack/3 and the hole on the device (bsr_colour_trunk_grad, csrc/colour_trunk_grad_kernels.h),
one JSON line, also written to --out (profiles/colour_trunk_grad_bench.json).

B items of S x S: the generator's forward on random images (weights from init_weights(1)) supplies y3x4, out4, y3x3, out3 and xh, d_xin
and d_x come from generator_grad.colour_trunk_example_inputs(seed 0), and ColourTrunk.backward reads the five tensors in place.
  device_ms_per_call     device events around --iters calls after a warm-up, divided by --iters; the window holds the allocation of
                         the outputs, as a caller pays it; device_ms_per_call_repeats two more windows.
  hole                   the chain's one new kernel alone (bsr_debug_hole_grad on the generator's own xh, the chain's d_xin3 and d_x)
                         against a plain device copy (Tensor.copy_) of half as many bytes, which reads and writes as many in all, in the
                         same run.  Both are timed as replays of a captured graph of 20 launches into outputs allocated beforehand, so
                         the host issues one replay per 20 launches and no window is bound by the host's launch rate.  `rotating`: the
                         20 launches walk four sets of buffers (four times the bytes, beyond the 256 MB last-level cache: the figure
                         HBM gives); `resident`: one set, which stays in that cache, as d_xin3 does in the chain.  Per form the ms per
                         launch, the bytes a launch moves (d_xin3's 261 and d_x's 257 floats a pixel read, 257 written, and bmask),
                         GB/s, the copy's, and the kernel's share of the copy's rate.
  parity                 with --parity, per (h, w, B) of the device tests' grids the worst scaled error of the 45 outputs against
                         generator_grad.colour_trunk_grad on the device's own activations; e2e_measured is the largest, the figure the
                         device test's bound is 4 x of.  Also `chained`: on a forward at (32, 256), B = 2 with init_weights(1) and
                         inputs from default_rng(21), the device walk over objective.BACKWARD's five stages, GreyDecoder.backward and
                         ColourTrunk.backward against the seven host statements chained on the device's own activations;
                         chained_measured is its worst scaled error, the figure the device test's chained bound is 4 x of.
  bmask_share            the share of pixels in the hole in the timed forward.
  scratch_bytes          bsr_colour_trunk_grad_scratch_bytes at these sizes.

    python tools/colour_trunk_bench.py [--batch 32] [--size 256] [--iters 200] [--parity] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parity():
    """The device tests' cases: colour_trunk_grad_cases.case(h, w, B, 1) through device_inputs."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import colour_trunk_grad_cases as cases
    from blindshadowremoval_amd import ColourTrunk, generator_grad as host
    out, dev = [], torch.device("cuda", 0)
    runner = ColourTrunk(0)
    for h, w, B in cases.GPU_SIZES:
        wt, x, bmask, uv, d_xin, d_x = cases.case(h, w, B, 1)
        arrays, (y3_4, y3_3) = cases.device_inputs(wt, x, bmask, uv)
        runner.load_weights(wt)
        res = runner.colour_trunk_grad(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays + (d_xin, d_x)], keep=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        st = host.colour_trunk_grad(wt, arrays[4], y3_3, arrays[3], y3_4, arrays[1], d_xin, d_x, acts=got)
        worst = cases.worst_scaled_diff(got, st)
        out.append({"h": h, "w": w, "batch": B, "scaled_error_device_acts": float("%.3g" % worst[0]), "at": worst[1],
                    "per_output": {n: float("%.3g" % cases.worst_scaled_diff(got, st, (n,))[0]) for n in cases.OUTPUTS}})
    return out


def chained():
    """tests/test_colour_trunk_grad_gpu.py's test_both_branches_chained as a measurement."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import colour_trunk_grad_cases as cases
    from blindshadowremoval_amd import ColourTrunk, Generator, GreyDecoder, generator_grad as host, init_weights, objective
    f32, dev = np.float32, torch.device("cuda", 0)
    w = init_weights(1)
    gen = Generator(device=0)
    gen.load_weights(w)
    rng = np.random.default_rng(21)
    inputs, uv = (torch.from_numpy(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32)).to(dev) for _ in range(2))
    gs, _, mask22, _ = gen(inputs, uv)
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = torch.from_numpy(g_con_a).to(dev), torch.from_numpy(g_gs_a).to(dev)
    table = tuple(s.name for s in objective.BACKWARD)
    walked = objective.device_walk(objective.device_runners(table, w), gen, dict(img=inputs, gs=gs, mask22=mask22, grad_con=g_con, grad_gs=g_gs),
                                   keep=("tail", "bottleneck", "heads"))
    grey, trunk = GreyDecoder(0), ColourTrunk(0)
    grey.load_weights(w)
    trunk.load_weights(w)
    g = grey.backward(gen, walked["heads"]["d_y"])
    res = {k: v.cpu().numpy() for k, v in trunk.backward(gen, walked["bottleneck"]["d_xin"], g["d_x"], keep=True).items()}
    torch.cuda.synchronize()
    names = ("xh", "y3x3", "res3", "y3x4", "res4", "y3x5", "res5", "res2", "up1", "x3", "up2", "x2", "y", "f1", "f2", "f")
    p = {k: gen.probe(k).cpu().numpy() for k in names}
    acts = lambda stage, keys: {k: walked[stage][k].cpu().numpy() for k in keys}            # noqa: E731
    st_t = host.tail_grad(w, gs.cpu().numpy(), p["f"], g_con_a, g_gs_a, acts=acts("tail", ("a1", "a2")))
    st_d = host.decoder_grad(w, p["res5"], st_t["d_f"], acts={"f1": p["f1"], "f2": p["f2"], "f": p["f"]})
    st_n = host.nonlocal_grad(w, (p["y3x5"][..., :257] - p["res4"][..., :257]).astype(f32), p["res4"], st_d["d_x"], acts={"out": p["res5"]})
    st_b = host.bottleneck_grad(w, p["res4"], st_n["d_y3"], st_n["d_skip"], acts=acts("bottleneck", ("a1", "a2")))
    st_h = host.heads_grad(w, inputs.cpu().numpy(), p["y"], st_t["d_gs"], acts=acts("heads", ("mask",)))
    st_g = host.grey_decoder_grad(w, p["res2"], p["x3"], p["x2"], st_h["d_y"], acts={"up1": p["up1"], "up2": p["up2"], "y": p["y"]})
    y3_4 = (p["y3x4"][..., :257] - p["res3"][..., :257]).astype(f32)
    y3_3 = (p["y3x3"][..., :257] - p["xh"][..., :257]).astype(f32)
    st_c = host.colour_trunk_grad(w, p["xh"], y3_3, p["res3"], y3_4, p["res4"], st_b["d_xin"], st_g["d_x"], acts=res)
    worst, at = cases.worst_scaled_diff(res, st_c)
    gen.close()
    return {"H": 32, "W": 256, "batch": 2, "bmask_share": round(float(p["xh"][..., 257].mean()), 4), "scaled_error_device_acts": float("%.3g" % worst),
            "at": at, "d_res2": float("%.3g" % cases.worst_scaled_diff(res, st_c, ("d_res2",))[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parity", action="store_true", help="the end-to-end scaled errors over the device tests' grids")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_trunk_grad_bench.json"))
    args = ap.parse_args()
    import torch
    from blindshadowremoval_amd import ColourTrunk, Generator, _lib, generator_grad as host, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("colour_trunk_bench: no GPU; nothing is measured without one")
    B, S = args.batch, args.size
    g = S // 8
    dev = torch.device("cuda", 0)
    weights = init_weights(1)
    runner = ColourTrunk(0)
    runner.load_weights(weights)
    _, _, _, d_xin, d_x = (torch.from_numpy(a).to(dev) for a in host.colour_trunk_example_inputs(g, g, B, seed=0))

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
    ms, res = timed(lambda: runner.backward(gen, d_xin, d_x), args.iters)
    spread = [timed(lambda: runner.backward(gen, d_xin, d_x), args.iters)[0] for _ in range(2)]
    kept = runner.backward(gen, d_xin, d_x, keep=True)
    xh = gen.probe("xh").clone()
    gen.close()
    # the hole kernel alone against a plain copy that moves as many bytes, both as replays of a captured graph of 20 launches
    N = B * g * g
    moved = 4 * N * (261 + 257 + 257 + 1)
    d_xin3 = kept["d_xin3"]
    assert torch.equal(runner.hole_grad(xh, d_xin3, d_x), kept["d_res2"])
    per_graph = 20

    def graphed(launch, sets):
        """ms per launch of `launch(r)` over buffer set r = 0..sets - 1 in rotation: `per_graph` launches captured once, replayed."""
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for r in range(sets):
                launch(r)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                for i in range(per_graph):
                    launch(i % sets)
        torch.cuda.current_stream().wait_stream(side)
        return timed(graph.replay, max(1, args.iters // per_graph))[0] / per_graph

    hole = {"bytes": moved, "launches_per_replay": per_graph}
    for form, sets in (("rotating", 4), ("resident", 1)):
        ins = [(xh.clone(), d_xin3.clone(), d_x.clone(), torch.empty_like(kept["d_res2"])) for _ in range(sets)]
        pairs = [(torch.rand((moved // 8,), device=dev), torch.empty((moved // 8,), device=dev)) for _ in range(sets)]
        hole_ms = graphed(lambda r: runner.call(ins[r][0], 261, ins[r][1], ins[r][2], B, g, g, ins[r][3], symbol="bsr_debug_hole_grad"), sets)
        copy_ms = graphed(lambda r: pairs[r][1].copy_(pairs[r][0]), sets)
        assert all(torch.equal(t[3], kept["d_res2"]) for t in ins)
        hole[form] = {"buffer_sets": sets, "ms": round(hole_ms, 5), "gb_per_s": round(moved / hole_ms / 1e6, 1), "copy_ms": round(copy_ms, 5),
                      "copy_gb_per_s": round(8 * (moved // 8) / copy_ms / 1e6, 1), "share_of_copy": round(copy_ms / hole_ms, 3)}
        del ins, pairs
    flat = res[""]
    line = {"batch": B, "size": S, "grad_l1": float(flat.abs().sum().cpu()), "grad_linf": float(flat.abs().max().cpu()),
            "d_res2_l1": float(res["d_res2"].abs().sum().cpu()), "bmask_share": round(float(xh[..., 257].mean().cpu()), 4),
            "device_ms_per_call": round(ms, 4), "device_ms_per_call_repeats": [round(v, 4) for v in spread], "launches": len(runner.LAUNCHES),
            "hole": hole, "scratch_bytes": int(_lib.load().bsr_colour_trunk_grad_scratch_bytes(B, g, g)), "stage_budget": 1e-5}
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
