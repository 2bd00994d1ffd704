"""Throughput of the RGB baseline forward (GeneratorRGB, /root/reference/model_RGB.py) beside the GSC forward, one JSON line.

B images of HxW, seeded synthetic weights and inputs, one forward at a time on the current stream, each shape warmed up; each figure is
(forwards in the window) x B / (wall time of the window, closed by a device synchronise), over a window of --seconds.  The two generators
alternate in --rounds windows each (RGB, GSC, RGB, GSC, ...) so both see the same host and clock; the JSON line gives the median window.
FLOPs per image are counted from the layer shapes (2 x MACs, `rgb_flops_per_image`); the share of the fp32 matrix-core peak is the
whole-forward rate over 157.3 TFLOP/s (MI355X fp32 MFMA, dense).

    python tools/rgb_bench.py [--batch 32] [--size 256] [--seconds 4] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
GSC_FLOPS_PER_IMAGE = 18.104e9     # the GSC forward at 256x256 (9 052 MMAC)


def rgb_flops_per_image(H=256, W=256):
    """2 x MACs of model_RGB.py's forward at HxW (pads, BN folding and the composed conv3|theta|phi|g GEMM not counted: the network's own
    arithmetic, as the reference states it)."""
    px, p2, p4, p8 = H * W, H * W // 4, H * W // 16, H * W // 64
    mac = px * 49 * 3 * 32                                          # conv1 7x7 3 -> 32
    mac += p2 * 9 * 32 * 64 + p4 * 9 * 64 * 64 + p8 * 9 * 64 * 96  # down1-3
    for cin in (99, 513, 513):                                      # res0-2
        mac += p8 * (cin * 256 + 9 * 256 * 256 + 256 * 513)         # conv1, conv2, conv3
        mac += p8 * 513 * 768 + 2 * p8 * p8 * 256 + p8 * 256 * 513  # theta|phi|g, S and P.V, w
    mac += p8 * 9 * 513 * 192 + p4 * 9 * 256 * 128 + p2 * 9 * 192 * 128     # up1-3 (ConvT: 9 taps per input pixel)
    mac += px * 49 * 128 * 3 + px * 49 * 3 * 3                      # conv2, conv3
    return 2.0 * mac


def window(fn, seconds):
    import torch
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rgb_bench.py measures the MI355X: no GPU here")
    from blindshadowremoval_amd import Generator, GeneratorRGB, init_weights
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    inp = torch.rand(B, S, S, 3, generator=g).cuda()
    uv = torch.rand(B, S, S, 3, generator=g).cuda()
    rgb = GeneratorRGB().load_weights(init_weights(1, variant="rgb"))
    gsc = Generator().load_weights(init_weights(1))
    rgb.reserve(B, S, S)
    con = torch.empty(B, S, S, 3, device="cuda")
    outs = tuple(torch.empty(B, S, S, c, device="cuda") for c in (1, 3, 3, 1))
    run_rgb = lambda: rgb(inp, uv, out=con)                        # noqa: E731
    run_gsc = lambda: gsc(inp, uv, out=outs)                       # noqa: E731
    for _ in range(args.warmup):
        run_rgb()
        run_gsc()
    torch.cuda.synchronize()
    rates = {"rgb": [], "gsc": []}
    for _ in range(args.rounds):
        for name, fn in (("rgb", run_rgb), ("gsc", run_gsc)):
            n, dt = window(fn, args.seconds)
            rates[name].append(n * B / dt)
    r, gs = statistics.median(rates["rgb"]), statistics.median(rates["gsc"])
    flops = rgb_flops_per_image(S, S)
    scale = (S * S) / (256.0 * 256.0)
    print(json.dumps({
        "metric": "rgb_forward_images_per_s", "value": round(r, 1), "unit": "images/s", "batch": B, "size": [S, S],
        "ms_per_forward": round(1e3 * B / r, 3), "gflop_per_image": round(flops / 1e9, 2),
        "frac_fp32_mfma_peak": round(r * flops / PEAK_F32_MFMA, 3),
        "gsc_images_per_s": round(gs, 1), "gsc_frac_fp32_mfma_peak": round(gs * GSC_FLOPS_PER_IMAGE * scale / PEAK_F32_MFMA, 3),
        "windows_s": args.seconds, "rounds": args.rounds,
        "rgb_windows": [round(x, 1) for x in rates["rgb"]], "gsc_windows": [round(x, 1) for x in rates["gsc"]],
        "device": torch.cuda.get_device_name(0),
    }))
    rgb.close()
    gsc.close()


if __name__ == "__main__":
    main()
