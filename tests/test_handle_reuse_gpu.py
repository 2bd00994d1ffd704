"""-m gpu: one handle across shape changes inside the same allocation, every variant and mode.

make_plan (csrc/bsr_api.hip) states the invariant: a new shape moves every buffer of the workspace, and every buffer is fully rewritten
by its producer each forward except the channel-pad lanes of the listed 1/8-resolution buffers, which ensure_workspace clears.  A fresh
allocation is zero everywhere, so only a REUSED handle can show a violation: a pad lane left with an earlier shape's data (it is the K
pad of a 1x1 layer and feeds the residuals), or a forward that reads a slot its own launches did not write.  Each forward of the
sequence must equal, bit for bit, the same call on a fresh handle — the outputs, and the probes whose buffers carry pad lanes.

The sequences shrink, change W, change H and grow back, all within the first shape's allocation.  TSM (square images, whole frame groups)
alternates share=True / share=False: a share=False forward leaves the `share` slot holding the previous shape's data, and the next
share=True forward must not read it.  GSC alternates bsr_forward and bsr_forward_packed (two sets of output pointers into forward_impl)."""

import pytest
import torch

from blindshadowremoval_amd.weights import init_weights

pytestmark = pytest.mark.gpu

SEQ = ((8, 256, 256), (2, 256, 256), (1, 256, 512), (3, 288, 256), (8, 256, 256))
SEQ_TSM = ((8, 256, 256), (2, 256, 256), (2, 512, 512), (4, 256, 256), (8, 256, 256))
PAD_LANE_PROBES = ["x0", "xh"] + ["res%d" % i for i in range(6)]
CASES = [("gsc", d) for d in ("f32", "f32x3", "f16")] + [("tsm", d) for d in ("f32", "f32x3", "f16")] + [("rgb", "f32")]


def _make(variant: str, dtype: str, w):
    from blindshadowremoval_amd import Generator, GeneratorRGB, GeneratorTSM
    return {"gsc": Generator, "tsm": GeneratorTSM, "rgb": GeneratorRGB}[variant](dtype=dtype).load_weights(w)


def _forward(gen, variant: str, step: int, inp, uv, reg):
    """The step's call: outputs as a list, then the pad-lane probes."""
    if variant == "tsm":
        out = list(gen(inp, uv, reg, 2, step % 2 == 0))
    elif variant == "rgb":
        out = [gen(inp, uv)]
    elif step % 2:
        out = list(gen(inp, uv, packed_out=torch.empty(*inp.shape[:3], 4, device=inp.device)))
    else:
        out = list(gen(inp, uv))
    names = ["x0", "res0", "res1", "res2"] if variant == "rgb" else PAD_LANE_PROBES
    return [t.clone() for t in out], {k: gen.probe(k) for k in names}


@pytest.mark.parametrize("variant,dtype", CASES)
def test_handle_is_reusable_across_shapes(variant, dtype):
    from stage_parity import smooth_reg
    w = init_weights(1, variant=variant)
    gen = _make(variant, dtype, w)
    g = torch.Generator().manual_seed(51)
    seq = SEQ_TSM if variant == "tsm" else SEQ
    assert gen._lib.bsr_handle_workspace_bytes(gen._handle, *seq[0]) >= max(gen._lib.bsr_handle_workspace_bytes(gen._handle, *s) for s in seq), \
        "every later shape must fit the first one's allocation, or the later forwards would run on fresh memory"
    for step, (B, H, W) in enumerate(seq):
        inp, uv = torch.rand(B, H, W, 3, generator=g).cuda(), torch.rand(B, H, W, 3, generator=g).cuda()
        reg = smooth_reg(B, H, g).cuda() if variant == "tsm" else None
        a_out, a_pr = _forward(gen, variant, step, inp, uv, reg)
        fresh = _make(variant, dtype, w)
        b_out, b_pr = _forward(fresh, variant, step, inp, uv, reg)
        for i, (x, y) in enumerate(zip(a_out, b_out)):
            assert not torch.isnan(y).any() and torch.equal(x, y), (variant, dtype, step, (B, H, W), "output %d" % i)
        for k in a_pr:
            assert torch.equal(a_pr[k], b_pr[k]), (variant, dtype, step, (B, H, W), k)
        fresh.close()
    gen.close()
