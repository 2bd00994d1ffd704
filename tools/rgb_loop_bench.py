"""Rate of the RGB baseline's UCB test loop (`FSRNetRGB.test`, train_RGB_test.py:357-505) against the GSC loop (`FSRNet.test`) in the
same process: the 100 golden UCB items (tests/golden/UCB, masks tests/golden/UCB_masks), rows prepared on the device, batch 16,
post-processing and PNG encoding on the device, `init_weights(1)` weights.  Each loop runs once untimed (code objects, workspaces,
pools) and then `--reps` times; the median rate and the wall-clock split of `FSRNet.timings` are printed as one JSON line.

    python tools/rgb_loop_bench.py [--reps 3] [--batch 16] [--out profiles/rgb_loop_ucb.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(model: str, batch: int, reps: int, out_dir: str):
    import torch
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config, FSRNet, FSRNetRGB
    from blindshadowremoval_amd.weights import init_weights
    golden = os.path.join(ROOT, "tests", "golden")
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(golden, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(golden, "UCB_masks")
    cfg.CHECKPOINT_DIR = os.path.join(out_dir, model)
    fsr = FSRNetRGB(cfg, weights=init_weights(1, variant="rgb")) if model == "rgb" else FSRNet(cfg, weights=init_weights(1))
    fsr.return_figs = False
    fsr.warm_pools(batch=batch)
    rates, splits = [], []
    try:
        for rep in range(reps + 1):
            ds = D.Dataset(cfg, "test", ucb=True, workers=max(1, D.cpu_share() * 3 // 4), device_prep=0, device_batch=batch)
            ds.warm()
            try:
                t0 = time.perf_counter()
                res = fsr.test(ds, batch=batch)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                ds.close()
            if rep == 0:                        # warm-up pass
                continue
            rates.append(len(res) / dt)
            splits.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in fsr.timings.items()})
        means = {k: s / max(c, 1) for k, (s, c) in fsr.log.losses.items()}
    finally:
        fsr.close()
    i = rates.index(statistics.median(rates))
    return {"images_per_sec": round(rates[i], 1), "all_rates": [round(r, 1) for r in rates], "timings": splits[i], "items": 100,
            "means": means}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rgb_loop_bench: needs a ROCm GPU")
    with tempfile.TemporaryDirectory(prefix="bsr_rgb_loop_") as tmp:
        line = {"loop": "FSRNetRGB.test vs FSRNet.test", "batch": args.batch, "post_and_png": "device", "prep": "device",
                "rgb": run("rgb", args.batch, args.reps, tmp), "gsc": run("gsc", args.batch, args.reps, tmp)}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
