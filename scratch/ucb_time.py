"""Dev: event-timed device post-processing of one chain on 16 items of the UCB fixtures.

    python scratch/ucb_time.py [gsc|tsm|rgb] [--json FILE] [--tree DIR]

gsc: bsr_ucb_post, tsm: bsr_ucb_post_tsm, rgb: bsr_ucb_post_rgb; B = 16, S = 256, want_figs off and on, 30 timed calls each.  --tree names
another checkout whose built package is timed instead of this one's (an A/B against a parent commit; the batches are always this
tree's tests/*_cases.py).  --json appends one line per configuration to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch_of(chain, n=16):
    """-> (runner, rows, masks, boxes) of `chain`, n items, on the device"""
    import numpy as np
    import torch
    box = lambda b: np.asarray(b, np.float32).reshape(4)
    u8 = lambda m: np.rint(m[:, :, 0] * 255.0).astype(np.uint8)
    if chain == "gsc":
        from ucb_cases import cases
        from blindshadowremoval_amd.ucb_post_gpu import UcbPostDevice as Dev, MASK_ORDER
        base = list(cases())
        items = [base[i % len(base)] for i in range(n)]
        rows = [np.concatenate([row[..., 0:3], row[..., 3:6], con, dif], axis=2) for _, row, _, _, con, dif in items]
        masks = [np.stack([u8(m[k]) for k in MASK_ORDER]) for _, _, _, m, _, _ in items]
    elif chain == "tsm":
        from ucb_tsm_cases import cases
        from blindshadowremoval_amd.ucb_post_tsm_gpu import UcbPostTsmDevice as Dev
        base = list(cases())
        items = [base[i % len(base)] for i in range(n)]
        rows = [np.concatenate([row[..., 0:3], row[..., 3:6], c0, c1, d0], axis=2) for _, row, _, _, c0, c1, d0 in items]
        masks = [np.stack([u8(m[k]) for k in ("face_hair", "face", "nose")]) for _, _, _, m, _, _, _ in items]
    else:
        from ucb_cases import cases
        from blindshadowremoval_amd.ucb_post_rgb_gpu import UcbPostRgbDevice as Dev
        base = list(cases())
        items = [base[i % len(base)] for i in range(n)]
        rows = [np.concatenate([row[..., 0:3], row[..., 3:6], con], axis=2) for _, row, _, _, con, _ in items]
        masks = [u8(m["face_hair"]) for _, _, _, m, _, _ in items]
    boxes = [box(it[2]) for it in items]
    dev = lambda a: torch.from_numpy(np.stack(a)).cuda()
    return Dev(0), dev(rows), dev(masks), dev(boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("chain", nargs="?", default="gsc", choices=("gsc", "tsm", "rgb"))
    ap.add_argument("--json")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    post, rows, masks, boxes = batch_of(args.chain)
    for figs in (False, True):
        fn = lambda: post.run(rows, masks, boxes, want_figs=figs)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
        ts.sort()
        print("%s, 16 items, want_figs=%s: median %.3f ms (min %.3f)" % (post.SYMBOL, figs, ts[len(ts) // 2], ts[0]))
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps({"tree": args.tree, "chain": args.chain, "want_figs": figs, "median_ms": round(ts[len(ts) // 2], 4),
                                    "min_ms": round(ts[0], 4)}) + "\n")


if __name__ == "__main__":
    main()
