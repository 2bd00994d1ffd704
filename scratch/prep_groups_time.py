"""Dev: event-timed bsr_prep_groups on 16 UCB groups (copy + both kernels), python scratch/prep_groups_time.py — the form to put under
`rocprofv3 --kernel-trace --stats`."""
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blindshadowremoval_amd import dataset as D, prep  # noqa: E402

if __name__ == "__main__":
    items = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "UCB", "train", "input", "*", "*.npy")), key=D.natural_key)[:16]

    def gt(p):
        parts = p.split("/")
        return os.path.splitext("/".join(parts[:-3] + ["gt"] + parts[-2:]))[0] + ".png"
    parts = [prep.host_part_group((p, gt(p), 256)) for p in items]
    dp = prep.DevicePrep(0, 256, planes=6)
    dp.rows(parts)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dp.rows(parts)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    print("bsr_prep_groups, 16 groups of 2 x 256x256x16: median %.3f ms (copy + kernels)" % ts[len(ts) // 2])
