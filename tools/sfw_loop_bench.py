"""Rate of the GSC model's SFW evaluation loop (`FSRNet.testsfw`, train_test_GSC.py:750-838) and the cost of its scoring.

    python tools/sfw_loop_bench.py loop [--videos 150] [--reps 3] [--batch 16] [--out profiles/sfw_loop.json]
    python tools/sfw_loop_bench.py tsm-loop [--videos 150] [--reps 3] [--batch 16] [--workers N] [--out profiles/sfw_loop_device.json]
    python tools/sfw_loop_bench.py score [--iters 50]          # the scoring kernels alone, 16 items per call (run under rocprofv3)
    python tools/sfw_loop_bench.py host-auc [--items 20]       # the host AUC per item (fsrnet.roc_auc_score, and sklearn when present)

`loop`: a synthetic SFW tree of `--videos` folders, each a copy of tests/golden/sfw_synth/vid0 (two labelled frames per folder), is made
in a temporary directory at run time; `FSRNet.testsfw` runs over Dataset(dset='sfw_gsc') with `init_weights(1)`, once untimed and then
`--reps` times; the median rate is printed as one JSON line.  `score`: bsr_sfw_score on 16 items of the shape of an SFW item (scores with
heavy ties at 0 outside a face region, labels 0 / 1 / 2).  `tsm-loop`: the TSM model's SFW loop (`FSRNetTSM.testsfw` over
Dataset(dset='sfw'), `init_weights(1, variant="tsm")`) on the same tree, with the host loader and with device-prepared groups
(Dataset(device_groups=0)) ALTERNATELY, pass by pass, in one process: per form the median rate, every pass's rate and the share of each
pass the loop's thread spent waiting for its next element.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SYNTH = os.path.join(ROOT, "tests", "golden", "sfw_synth", "vid0")


def _items(b: int, s: int = 256, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:s, 0:s]
    face = np.clip(1.3 - ((yy - s / 2) ** 2 + (xx - s / 2) ** 2) / (0.35 * s) ** 2, 0, 1).astype(np.float32)
    out = np.empty((b, s, s, 3), np.float32)
    for j in range(b):
        out[j, ..., 0] = rng.integers(0, 3, (s, s))
        out[j, ..., 1] = rng.random((s, s), dtype=np.float32)
        out[j, ..., 2] = face
    return out


def loop(args):
    import torch
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config, FSRNet
    from blindshadowremoval_amd.weights import init_weights
    with tempfile.TemporaryDirectory(prefix="bsr_sfw_loop_") as tmp:
        for v in range(args.videos):
            shutil.copytree(SYNTH, os.path.join(tmp, "data", "vid%d" % v))
        cfg = Config(0)
        cfg.DATA_DIR_TEST = [os.path.join(tmp, "data", "*")]
        cfg.CHECKPOINT_DIR = os.path.join(tmp, "out")
        fsr = FSRNet(cfg, weights=init_weights(1))
        fsr.return_figs = False
        fsr.warm_pools(batch=args.batch)
        rates = []
        try:
            for rep in range(args.reps + 1):
                ds = D.Dataset(cfg, "test", dset="sfw_gsc", workers=max(1, D.cpu_share() * 7 // 8))
                ds.warm()
                try:
                    t0 = time.perf_counter()
                    res = fsr.testsfw(ds, batch=args.batch)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    ds.close()
                if rep:
                    rates.append(len(res) / dt)
            means = {k: s / max(c, 1) for k, (s, c) in fsr.log.losses.items()}
        finally:
            fsr.close()
    return {"loop": "FSRNet.testsfw", "items": len(res), "batch": args.batch, "images_per_sec": round(statistics.median(rates), 1),
            "all_rates": [round(r, 1) for r in rates], "loader_workers": max(1, D.cpu_share() * 7 // 8), "means": means}


def tsm_loop(args):
    import torch
    from blindshadowremoval_amd import dataset as D
    from blindshadowremoval_amd.fsrnet import Config, FSRNetTSM
    from blindshadowremoval_amd.weights import init_weights
    workers = args.workers or max(1, D.cpu_share() * 7 // 8)
    modes = ("host", "device")
    rates, waits = {m: [] for m in modes}, {m: [] for m in modes}
    with tempfile.TemporaryDirectory(prefix="bsr_sfw_tsm_loop_") as tmp:
        for v in range(args.videos):
            shutil.copytree(SYNTH, os.path.join(tmp, "data", "vid%d" % v))
        cfg = Config(0)
        cfg.DATA_DIR_TEST = [os.path.join(tmp, "data", "*")]
        cfg.CHECKPOINT_DIR = os.path.join(tmp, "out")
        fsr = FSRNetTSM(cfg, weights=init_weights(1, variant="tsm"))
        try:
            for rep in range(args.reps + 1):
                for mode in modes:
                    kw = dict(device_groups=0, device_batch=args.batch) if mode == "device" else {}
                    ds = D.Dataset(cfg, "test", dset="sfw", workers=workers, **kw)
                    ds.warm()
                    wait = [0.0]

                    def timed(feed):
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
                        res = fsr.testsfw(ds, batch=args.batch)
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
    return {"loop": "FSRNetTSM.testsfw", "prep": "host+device", "items": len(res), "batch": args.batch, **out, "loader_workers": workers, "means": means}


def score(args):
    import torch
    from blindshadowremoval_amd.sfw_post_gpu import SfwScoreDevice
    rows = torch.from_numpy(_items(16)).cuda()
    dev = SfwScoreDevice(0)
    dev.run(rows)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        dev.run(rows)
    torch.cuda.synchronize()
    return {"scoring": "bsr_sfw_score", "items_per_call": 16, "calls": args.iters, "wall_us_per_call": round((time.perf_counter() - t0) / args.iters * 1e6, 1)}


def host_auc(args):
    from blindshadowremoval_amd.fsrnet import roc_auc_score
    a = _items(args.items)
    out = {"host_auc": "per item of 65 538 scores", "items": args.items}
    extr = np.array([1, 0])
    fns = {"fsrnet.roc_auc_score": roc_auc_score}
    try:
        import sklearn.metrics
        fns["sklearn.metrics.roc_auc_score"] = sklearn.metrics.roc_auc_score
    except ImportError:
        pass
    for name, fn in fns.items():
        t0 = time.perf_counter()
        for j in range(args.items):
            fn(np.concatenate([extr, (a[j, ..., 0] == 2).reshape(-1)]), np.concatenate([extr, (a[j, ..., 1] * a[j, ..., 2]).reshape(-1)]))
        out[name + "_ms"] = round((time.perf_counter() - t0) / args.items * 1e3, 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=("loop", "tsm-loop", "score", "host-auc"))
    ap.add_argument("--videos", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--workers", type=int, default=None, help="tsm-loop: loader processes (default: 7/8 of the usable CPUs)")
    ap.add_argument("--items", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    line = {"loop": loop, "tsm-loop": tsm_loop, "score": score, "host-auc": host_auc}[args.mode](args)
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
