"""What the host tests (test_colour_trunk_grad_cpu.py) and the device tests (test_colour_trunk_grad_gpu.py) of the backward of
res_stack/4, res_stack/3 and the hole share: seeded weights and inputs, the torch autograd restatement the statement is held to, the
scaled difference over the 45 outputs, the bounds, and constructed cases with closed-form answers.  Every `check_*` takes
`run(weights, x, bmask, uv, d_xin, d_x)` -> dict(`d_res2`, the 44 variables by name, `a1_<b>`, `a2_<b>` and the intermediate data
gradients `d_y3_<b>`, `d_skip_<b>`, `d_xin4`, `d_xin3` as kept, the chain's inputs `xh`, `y3_<b>`, `res<b>` as used, and `dtype`: the
arithmetic's type); `d_x` may be None.  Grids are (h, w, B) on the 1/8 grid."""
import numpy as np

from blindshadowremoval_amd import generator_grad as host
from blindshadowremoval_amd.weights import generator_bottleneck_trainable_names, generator_colour_trunk_trainable_names, generator_nonlocal_trainable_names

import block_chain_cases as chain
from block_chain_cases import autograd_block

f32 = np.float32
NAMES = tuple(generator_colour_trunk_trainable_names())
OUTPUTS = ("d_res2",) + NAMES
BLOCKS = (4, 3)
AUTOGRAD_SIZES = ((1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 32, 1))
# the largest scaled difference between the statement and autograd over AUTOGRAD_SIZES, measured on the CPU (test_colour_trunk_grad_cpu.py
# prints each figure)
AUTOGRAD_MEASURED = 1.11e-14            # res_stack/4/non_local/theta/bias at (4, 32, 1); 3.07e-15, 4.25e-15, 7.23e-15 at the other sizes
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                # the project's fp32-class stage budget (tests/stage_parity.py)
GPU_SIZES = ((4, 32, 1), (8, 32, 2), (12, 32, 3), (4, 64, 1))
# the largest scaled error of an output of the device chain against colour_trunk_grad(acts = the device's own a1, a2 of both blocks),
# measured on an MI355X over GPU_SIZES (tools/colour_trunk_bench.py --parity, profiles/colour_trunk_grad_bench.json)
E2E_MEASURED = 4.08e-6        # res_stack/3/non_local/theta/bias at (12, 32, 3); 3.03e-6, 3.38e-6, 3.4e-6 at (4, 32, 1), (8, 32, 2), (4, 64, 1)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)
# block_chain_cases.device_digest of the device's keep=True result on device_results' inputs at two of GPU_SIZES, recorded on an MI355X from
# commit 7a2e835 ("Run the fp32 colour tail's clr_conv1 in Winograd form, V in registers"), the last before the two trunk stages shared one
# statement of the chain: a call repeats its bits, so a mismatch means that what runs has changed
PARENT_DEVICE_DIGESTS = {(4, 32, 1): "f87bd706c5f8971e", (12, 32, 3): "09c619f87a1fdad8"}
# the same of `d_res2` and the 44 variables at the end of both branches chained on one forward at (32, 256), B = 2: the five table stages,
# GreyDecoder and ColourTrunk against the host statements chained on the device's own activations
CHAINED_MEASURED = 2.39e-6    # res_stack/3/non_local/phi/kernel; d_res2 9.1e-7
CHAINED_BOUND = min(4 * CHAINED_MEASURED, 1e-3)

_cases = {}
ct_weights = chain.weights          # init_weights(3) by default, cached: treat as read-only


def check_inputs(fw, bmask):
    """Both signs are present in each block's a1, a2 and output, and the hole covers between a quarter and three quarters of the pixels."""
    for b in (3, 4):
        for k in ("a1_%d", "a2_%d", "pre_%d"):
            frac = float((fw[k % b] > 0).mean())
            assert 0.02 < frac < 0.98, (k % b, frac)
    share = float(np.asarray(bmask).mean())
    assert 0.25 <= share <= 0.75, share


def case(h, w, B, seed=0):
    """(weights, x, bmask, uv, d_xin, d_x) at a coarse size, with check_inputs' conditions asserted.  Cached: treat as read-only."""
    if (h, w, B, seed) not in _cases:
        wt = ct_weights()
        x, bmask, uv, d_xin, d_x = host.colour_trunk_example_inputs(h, w, B, seed)
        check_inputs(host.trunk_forward(wt, x, bmask, uv), bmask)
        _cases[(h, w, B, seed)] = (wt, x, bmask, uv, d_xin, d_x)
    return _cases[(h, w, B, seed)]


def host_run(wt, x, bmask, uv, d_xin, d_x):
    """The `run` of check_* on the host: the statement in float64 on trunk_forward's own float64 tensors."""
    fw = host.trunk_forward(wt, x, bmask, uv)
    out = host.colour_trunk_grad(wt, fw["xh"], fw["y3_3"], fw["res3"], fw["y3_4"], fw["res4"], d_xin, d_x)
    out.update({k: fw[k] for k in ("xh", "y3_3", "res3", "y3_4", "res4")})
    out["dtype"] = np.float64
    return out


def device_inputs(wt, x, bmask, uv):
    """((y3x4, out4, y3x3, out3, xh) float32 as the device chain takes them, (y3_4, y3_3) as it will form them): trunk_forward in float64
    rounded once, y3x = y3 + pad(xin) rounded once as the forward stores it, y3' = y3x - pad(xin), one float32 subtraction."""
    fw = host.trunk_forward(wt, x, bmask, uv)
    xh, res3, res4 = (np.ascontiguousarray(fw[k], f32) for k in ("xh", "res3", "res4"))
    y3x3 = (fw["y3_3"].astype(f32) + xh[..., :257]).astype(f32)
    y3x4 = (fw["y3_4"].astype(f32) + res3[..., :257]).astype(f32)
    return (y3x4, res4, y3x3, res3, xh), ((y3x4 - res3[..., :257]).astype(f32), (y3x3 - xh[..., :257]).astype(f32))


def worst_scaled_diff(got, ref, names=OUTPUTS):
    """block_chain_cases.worst_scaled_diff, over the 45 outputs unless `names` says otherwise."""
    return chain.worst_scaled_diff(got, ref, names)


# ---- torch autograd in float64: block_chain_cases.autograd_block per block; the hole with bmask and uv constants (model.py:256-262).  The
# 44 variables and x are leaves
def autograd_grads(weights, x, bmask, uv, d_xin, d_x=None):
    """d (<d_xin, res4> + <d_x, x>) / d each of the 44 variables and x by torch autograd in float64 from the float32 variables: name ->
    float64 array in the variable's shape, `d_res2` [B,h,w,257]."""
    import torch
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    leaves = {n: t64(weights[n]).requires_grad_(True) for n in NAMES}
    xt = t64(x).requires_grad_(True)
    hole = t64(bmask)
    xh = torch.cat([xt * (1 - hole), hole, t64(uv)], dim=3)
    obj = (autograd_block(autograd_block(xh, 3, leaves, weights), 4, leaves, weights) * t64(d_xin)).sum()
    if d_x is not None:
        obj = obj + (xt * t64(d_x)).sum()
    obj.backward()
    res = {k: v.grad.numpy() for k, v in leaves.items()}
    res["d_res2"] = xt.grad.numpy()
    return res


# ---- constructed cases
def _tol(r):
    return AUTOGRAD_BOUND if r["dtype"] is np.float64 else E2E_BOUND


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def _hole(r, d_x):
    """d_res2 is the hole's arithmetic on the kept d_xin3 in the run's own type, bit for bit."""
    T = r["dtype"]
    _same("d_res2", np.asarray(r["d_res2"], T), host.hole_grad(np.asarray(r["xh"], T), np.asarray(r["d_xin3"], T), d_x, dtype=T))


def check_zero_d_xin(run, h=4, w=32, B=1):
    """d_xin = 0: all 44 gradients are exactly 0 and d_res2 is d_x bit for bit."""
    wt, x, bmask, uv, d_xin, d_x = case(h, w, B, 5)
    r = run(wt, x, bmask, uv, np.zeros_like(d_xin), d_x)
    for name in NAMES:
        assert np.asarray(r[name]).shape == wt[name].shape and not np.asarray(r[name]).any(), name
    _same("d_res2", np.asarray(r["d_res2"], f32), d_x)


def check_hole_everywhere(run, h=4, w=32, B=1):
    """bmask all ones: nothing of the colour branch reaches res_stack/2 — d_res2 is d_x bit for bit, and exactly zero with d_x None —
    while the variable gradients are not all zero."""
    wt, x, _, uv, d_xin, d_x = case(h, w, B, 6)
    ones = np.ones((B, h, w, 1), f32)
    r = run(wt, x, ones, uv, d_xin, d_x)
    _same("d_res2", np.asarray(r["d_res2"], f32), d_x)
    assert all(np.asarray(r[name]).any() for name in NAMES)
    r = run(wt, x, ones, uv, d_xin, None)
    assert not np.asarray(r["d_res2"]).any() and np.asarray(r["d_xin3"])[..., :257].any()


def check_no_hole(run, h=4, w=32, B=1):
    """bmask all zeros: d_res2 = d_xin3[..., :257] + d_x in the run's type, bit for bit, with d_xin3 the kept map."""
    wt, x, _, uv, d_xin, d_x = case(h, w, B, 7)
    r = run(wt, x, np.zeros((B, h, w, 1), f32), uv, d_xin, d_x)
    T = r["dtype"]
    _same("d_res2", np.asarray(r["d_res2"], T), np.asarray(r["d_xin3"], T)[..., :257] + np.asarray(d_x, T))
    _hole(r, d_x)


def check_random_hole(run, h=8, w=32, B=2):
    """A random bmask: the same per pixel — pixels in the hole carry d_x alone, the others d_xin3[..., :257] + d_x."""
    wt, x, bmask, uv, d_xin, d_x = case(h, w, B, 8)
    r = run(wt, x, bmask, uv, d_xin, d_x)
    T = r["dtype"]
    inside = bmask[..., 0] == 1
    assert inside.any() and not inside.all()
    got = np.asarray(r["d_res2"], T)
    _same("in the hole", got[inside], np.asarray(d_x, T)[inside])
    _same("outside", got[~inside], np.asarray(r["d_xin3"], T)[..., :257][~inside] + np.asarray(d_x, T)[~inside])
    _hole(r, d_x)
    r0 = run(wt, x, bmask, uv, d_xin, None)
    _hole(r0, None)
    assert not np.asarray(r0["d_res2"])[inside].any()


def check_the_skips_own_channels_reach_nothing(run, h=4, w=32, B=1):
    """d_xin changed in channels 257..260 only: they travel the skips down to d_xin3[..., 257:], which the hole drops — nothing in d_res2
    or in any of the 44 gradients changes by a bit."""
    wt, x, bmask, uv, d_xin, d_x = case(h, w, B, 9)
    r = run(wt, x, bmask, uv, d_xin, d_x)
    moved = d_xin.copy()
    moved[..., 257:] = -2 * moved[..., 257:] + f32(1e-3)
    r2 = run(wt, x, bmask, uv, moved, d_x)
    assert not np.array_equal(np.asarray(r2["d_xin3"])[..., 257:], np.asarray(r["d_xin3"])[..., 257:])
    for name in OUTPUTS:
        np.testing.assert_array_equal(np.asarray(r2[name]), np.asarray(r[name]), err_msg=name)


def check_the_blocks_take_their_own_weights(run, h=4, w=32, B=1):
    """res_stack/<b>'s gradients agree with the single-block statements of block b on the run's own tensors, and differ from the
    statements of the other block on the same tensors by more than 1e-2 scaled; for b = 3 and b = 4."""
    wt, x, bmask, uv, d_xin, d_x = case(h, w, B, 10)
    r = run(wt, x, bmask, uv, d_xin, d_x)
    feeds = {4: (r["y3_4"], r["res3"], r["res4"], d_xin), 3: (r["y3_3"], r["xh"], r["res3"], r["d_xin4"])}
    for b, (y3, xin, out, d_out) in feeds.items():
        own = tuple(generator_bottleneck_trainable_names(b)) + tuple(generator_nonlocal_trainable_names(b))
        for other in (3, 4):
            n = host.nonlocal_grad(wt, y3, xin, d_out, block=other, acts={"out": out})
            t = host.bottleneck_grad(wt, xin, n["d_y3"], n["d_skip"], block=other,
                                     acts={"a1": r["a1_%d" % b], "a2": r["a2_%d" % b]} if other == b else None)
            st = {name.replace("res_stack/%d/" % other, "res_stack/%d/" % b): v for name, v in list(n.items()) + list(t.items())}
            d, at = worst_scaled_diff(r, st, own)
            print("colour trunk: res_stack/%d's gradients against the statements of block %d: worst scaled difference %.3g at %s" % (b, other, d, at))
            assert (d <= _tol(r)) if other == b else (d > 1e-2), (b, other, d, at)


CONSTRUCTED = (check_zero_d_xin, check_hole_everywhere, check_no_hole, check_random_hole, check_the_skips_own_channels_reach_nothing,
               check_the_blocks_take_their_own_weights)
