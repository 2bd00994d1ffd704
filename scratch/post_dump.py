"""Dev: every output of the four device post-processing calls on fixed batches, as one .npz (to compare two builds byte for byte).

    python scratch/post_dump.py OUT.npz [--tree DIR]          # dump (DIR: the checkout whose built package runs; default this one)
    python scratch/post_dump.py --compare A.npz B.npz         # exit status 1 unless every array is byte-for-byte equal

bsr_ucb_post, bsr_ucb_post_tsm, bsr_ucb_post_rgb on the 16-item batches of scratch/ucb_time.py, want_figs off and on, and bsr_sfw_score
on the 16 items of tests/test_sfw_score_gpu.py: losses, nose_stats, strips, figs, status (SFW: losses, auc, pred, label, status)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(out, tree):
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scratch"))
    import torch
    from ucb_time import batch_of
    arrays = {}
    names = {"gsc": ("losses", "strips", "figs", "status"), "tsm": ("losses", "nose_stats", "strips", "figs", "status"),
             "rgb": ("losses", "strips", "figs", "status")}
    for chain in ("gsc", "tsm", "rgb"):
        post, rows, masks, boxes = batch_of(chain)
        for figs in (False, True):
            res = post.run(rows, masks, boxes, want_figs=figs)
            torch.cuda.synchronize()
            for name, t in zip(names[chain], res):
                if t is not None:
                    arrays["%s/figs%d/%s" % (chain, figs, name)] = t.cpu().numpy()
    import test_sfw_score_gpu as sfw
    for name, a in zip(("losses", "auc", "pred", "label", "status"), sfw._run(sfw._items(), times=1)[0]):
        arrays["sfw/%s" % name] = a
    np.savez(out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arrays), sum(a.nbytes for a in arrays.values())))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        print("%-22s %-8s %-22s %s" % (k, a[k].dtype, a[k].shape, "equal" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
    print("%d arrays, %d differ or are missing: %s" % (len(a.files), len(bad), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1], sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--tree" else ROOT)
