"""Rate of the TSM model's UCB test loop (`FSRNetTSM.test`, train_with_TSM.py:369-618): the 100 golden UCB items (tests/golden/UCB,
masks tests/golden/UCB_masks), each as its image + mirror group (frame = 2), `batch` items per forward, post-processing and PNG encoding
on the device, `init_weights(1, variant="tsm")` weights, rows prepared on the host by `workers` loader processes, or with
`--device-groups` on the device (Dataset(device_groups=0): the workers inflate and triangulate only).  `--alternate` runs both forms in
turn, pass by pass, in one process — the comparison the two figures of profiles/tsm_loop_ucb_device.json come from.  The loop runs once
untimed and then `--reps` times; the median rate is printed as one JSON line.  `--post-only` instead runs the device post chain alone
(bsr_ucb_post_tsm) `--reps` times on one batch of `batch` items — the form to put under `rocprofv3 --kernel-trace --stats`.

    python tools/tsm_loop_bench.py [--reps 3] [--batch 16] [--workers N] [--device-groups | --alternate] [--post-only] [--out profiles/tsm_loop_ucb.json]
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
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cfg(out_dir):
    from blindshadowremoval_amd.fsrnet import Config
    cfg = Config(0)
    cfg.DATA_DIR_TEST = [os.path.join(GOLDEN, "UCB", "train", "input", "*")]
    cfg.UCB_MASK_ROOT = os.path.join(GOLDEN, "UCB_masks")
    cfg.CHECKPOINT_DIR = out_dir
    return cfg


def run_loop(batch: int, reps: int, out_dir: str, modes=("host",), workers=None):
    """`modes`: "host" / "device" — with both, every pass runs one after the other (alternately)."""
    import torch
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import FSRNetTSM
    from blindshadowremoval_amd.weights import init_weights
    cfg = _cfg(out_dir)
    fsr = FSRNetTSM(cfg, weights=init_weights(1, variant="tsm"))
    fsr.return_figs = False
    rates = {m: [] for m in modes}
    waits = {m: [] for m in modes}
    workers = workers or max(1, D.cpu_share() * 7 // 8)
    try:
        for rep in range(reps + 1):
            for mode in modes:
                kw = dict(device_groups=0, device_batch=batch) if mode == "device" else {}
                ds = D.Dataset(cfg, "test", dset="ucb_tsm", ucb=True, workers=workers, **kw)
                ds.warm()
                wait = [0.0]

                def timed(feed):                  # the loop's stage split: seconds this thread waits for its next element
                    while True:
                        t = time.perf_counter()
                        try:
                            el = next(feed)
                        except StopIteration:
                            return
                        wait[0] += time.perf_counter() - t
                        yield el
                ds.feed = timed(ds.feed)
                try:
                    t0 = time.perf_counter()
                    res = fsr.test(ds, batch=batch, mat_path=os.path.join(out_dir, "frac_in_nose.mat"))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    ds.close()
                if rep:
                    rates[mode].append(len(res) / dt)
                    waits[mode].append(wait[0] / dt)
        means = {k: s / max(c, 1) for k, (s, c) in fsr.log.losses.items()}
    finally:
        fsr.log.close()
    out = {m: {"images_per_sec": round(statistics.median(rates[m]), 1), "all_rates": [round(r, 1) for r in rates[m]],
               "prep_wait_share_of_pass": [round(x, 3) for x in waits[m]]} for m in modes}
    if len(modes) == 1:
        out = out[modes[0]]
    return {**out, "items": 100, "loader_workers": workers, "means": means}


def run_post(batch: int, reps: int):
    """The device post chain alone on `batch` items of tests/ucb_tsm_cases.py: mean wall time per call (synchronised)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from blindshadowremoval_amd.ucb_post_tsm_gpu import UcbPostTsmDevice
    from ucb_tsm_cases import cases
    cs = list(cases())
    cs = [cs[i % len(cs)] for i in range(batch)]
    rows = torch.from_numpy(np.stack([np.concatenate([r[..., 0:3], r[..., 3:6], c0, c1, d0], axis=2) for _, r, _, _, c0, c1, d0 in cs])).cuda()
    masks = torch.from_numpy(np.stack([np.stack([np.rint(m[k][:, :, 0] * 255).astype(np.uint8) for k in ("face_hair", "face", "nose")])
                                       for _, _, _, m, _, _, _ in cs])).cuda()
    boxes = torch.from_numpy(np.stack([np.asarray(b, np.float32).reshape(4) for _, _, b, _, _, _, _ in cs])).cuda()
    post = UcbPostTsmDevice(0)
    post.run(rows, masks, boxes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        post.run(rows, masks, boxes)
    torch.cuda.synchronize()
    return {"post_ms_per_call_wall": round((time.perf_counter() - t0) * 1e3 / reps, 3), "items_per_call": batch, "calls": reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--post-only", action="store_true")
    ap.add_argument("--workers", type=int, default=None, help="loader processes (default: 7/8 of the usable CPUs)")
    ap.add_argument("--device-groups", action="store_true", help="prepare the groups on the device (Dataset(device_groups=0))")
    ap.add_argument("--alternate", action="store_true", help="host loader and device groups alternately, pass by pass")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsm_loop_bench: needs a ROCm GPU")
    if args.post_only:
        line = {"stage": "bsr_ucb_post_tsm", **run_post(args.batch, args.reps)}
    else:
        with tempfile.TemporaryDirectory(prefix="bsr_tsm_loop_") as tmp:
            modes = ("host", "device") if args.alternate else (("device",) if args.device_groups else ("host",))
            line = {"loop": "FSRNetTSM.test", "batch": args.batch, "post_and_png": "device", "prep": "+".join(modes),
                    **run_loop(args.batch, args.reps, tmp, modes, args.workers)}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
