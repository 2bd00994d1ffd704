"""Generate tests/golden/disc_ckpt_inventory.json from the reference's own checkpoint index files: the names and shapes of the
``discriminator_{1,2,3}/*`` variables of the three runs (GSC, TSM, RGB), beside tools/make_inventory_fixture.py's table of the
generators.  The fixture is DATA (names and shapes only); it pins weights.discriminator_variable_shapes().

Run on the machine that holds the reference:  python tools/make_disc_inventory_fixture.py
"""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blindshadowremoval_amd.tf_bundle import discriminator_inventory  # noqa: E402

REF = "/root/reference/log"
out = {}
for idx in sorted(glob.glob(os.path.join(REF, "*", "ckpt-*.index"))):
    run = os.path.basename(os.path.dirname(idx))
    tag = "tsm" if run.endswith("with-TSM") else ("rgb" if run.endswith("RGB-model") else "gsc")
    inv = discriminator_inventory(idx)
    out[tag] = {"index": os.path.basename(idx), "run": run, "n_variables": len(inv),
                "n_params": int(sum(int(np.prod(s)) for s in inv.values())),
                "variables": {k: list(v) for k, v in sorted(inv.items())}}
dst = os.path.join(ROOT, "tests", "golden", "disc_ckpt_inventory.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
print({k: (v["n_variables"], v["n_params"]) for k, v in out.items()})
