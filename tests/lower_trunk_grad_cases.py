"""What the host tests (test_lower_trunk_grad_cpu.py) and the device tests (test_lower_trunk_grad_gpu.py) of the backward of
res_stack/2, res_stack/1 and res_stack/0 share: seeded weights and inputs, the torch autograd restatement the statement is held to, the
scaled difference over the 67 outputs, the bounds, and constructed cases.  Every `check_*` takes `run(weights, x0, d_res2)` ->
dict(`d_x0`, the 66 variables by name, `a1_<b>`, `a2_<b>` and the intermediate data gradients `d_y3_<b>`, `d_skip_<b>`, `d_xin2`,
`d_xin1` as kept, the chain's inputs `y3_<b>`, `res<b>` as used, and `dtype`: the arithmetic's type).  `x0` may be a view of a wider
array: [B,h,w,99] with more than 99 floats between pixels, as the generator keeps it.  Grids are (h, w, B) on the 1/8 grid."""
import hashlib

import numpy as np

from blindshadowremoval_amd import generator_grad as host, pack
from blindshadowremoval_amd.weights import (BN_EPS, LRELU_ALPHA, generator_bottleneck_trainable_names, generator_lower_trunk_trainable_names,
                                            generator_nonlocal_trainable_names, init_weights)

import block_chain_cases as chain
from block_chain_cases import autograd_block, to_dev, to_host      # noqa: F401

f32 = np.float32
NAMES = tuple(generator_lower_trunk_trainable_names())
OUTPUTS = ("d_x0",) + NAMES
BLOCKS = (2, 1, 0)                  # in the chain's order
WIDTHS = {0: 99, 1: 257, 2: 257}    # the blocks' input widths
WEIGHTS_SEED = 3                    # under init_weights(3) and the example inputs every a1, a2 and relu3 input of the float64 forward has both signs (check_inputs)
AUTOGRAD_SIZES = ((1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 32, 1))
# the largest scaled difference between the statement and autograd over AUTOGRAD_SIZES, measured on the CPU (test_lower_trunk_grad_cpu.py
# prints each figure)
AUTOGRAD_MEASURED = 1.99e-14        # res_stack/0/non_local/theta/bias at (4, 32, 1); 6.35e-15, 4.31e-15, 6.61e-15 at the other sizes
AUTOGRAD_CAP = 1e-9
AUTOGRAD_BOUND = min(4 * AUTOGRAD_MEASURED, AUTOGRAD_CAP)
STAGE_BUDGET = 1e-5                 # the project's fp32-class stage budget (tests/stage_parity.py)
GPU_SIZES = ((4, 32, 1), (8, 32, 2), (12, 32, 3), (4, 64, 1))
# the largest scaled error of an output of the device chain against lower_trunk_grad(acts = the device's own a1, a2 of the three blocks),
# measured on an MI355X over GPU_SIZES (tools/lower_trunk_bench.py --parity, profiles/lower_trunk_grad_bench.json)
E2E_MEASURED = 6.41e-6        # res_stack/0/bnorm2/gamma at (12, 32, 3); 5.03e-6, 5.57e-6, 4.28e-6 at (4, 32, 1), (8, 32, 2), (4, 64, 1)
E2E_BOUND = min(4 * E2E_MEASURED, 1e-3)
# block_chain_cases.device_digest of the device's keep=True result on device_results' inputs at two of GPU_SIZES, recorded on an MI355X from
# commit 7a2e835 ("Run the fp32 colour tail's clr_conv1 in Winograd form, V in registers"), the last before the two trunk stages shared one
# statement of the chain: a call repeats its bits, so a mismatch means that what runs has changed
PARENT_DEVICE_DIGESTS = {(4, 32, 1): "5788f23824252ae4", (12, 32, 3): "a2d8d2c71151d0d3"}
# the same of `d_x0` and the 66 variables at the end of the whole backward chained on one forward at (32, 256), B = 2: the five table
# stages, GreyDecoder, ColourTrunk and LowerTrunk against the eight host statements chained on the device's own activations
CHAINED_MEASURED = 4.76e-6    # res_stack/2/non_local/phi/kernel; d_x0 1.21e-6
CHAINED_BOUND = min(4 * CHAINED_MEASURED, 1e-3)

_cases = {}
lt_weights = chain.weights          # init_weights(3) by default, which is WEIGHTS_SEED; cached: treat as read-only


def check_inputs(fw):
    """Both signs are present in each block's a1, a2 and relu3 input: a share of positives in 0.02..0.98."""
    for b in (0, 1, 2):
        for k in ("a1_%d", "a2_%d", "pre_%d"):
            frac = float((fw[k % b] > 0).mean())
            assert 0.02 < frac < 0.98, (k % b, frac)


def case(h, w, B, seed=0):
    """(weights, x0, d_res2) at a coarse size, with check_inputs' conditions asserted on the float64 forward.  Cached: treat as
    read-only."""
    if (h, w, B, seed) not in _cases:
        wt = lt_weights()
        x0, d_res2 = host.lower_trunk_example_inputs(h, w, B, seed)
        check_inputs(host.lower_trunk_forward(wt, x0))
        _cases[(h, w, B, seed)] = (wt, x0, d_res2)
    return _cases[(h, w, B, seed)]


FORWARD_KEYS = ("y3_0", "res0", "y3_1", "res1", "y3_2", "res2")


def host_run(wt, x0, d_res2):
    """The `run` of check_* on the host: the statement in float64 on lower_trunk_forward's own float64 tensors."""
    fw = host.lower_trunk_forward(wt, x0)
    out = host.lower_trunk_grad(wt, x0, *(fw[k] for k in FORWARD_KEYS), d_res2)
    out.update({k: fw[k] for k in FORWARD_KEYS})
    out["dtype"] = np.float64
    return out


def pad257(x):
    """x [..., C <= 257] zero-padded to 257 channels."""
    x = np.asarray(x)
    return np.concatenate([x, np.zeros(x.shape[:-1] + (257 - x.shape[-1],), x.dtype)], axis=-1)


def device_inputs(wt, x0):
    """((y3x2, out2, y3x1, out1, y3x0, out0) float32 as the device chain takes them, {b: y3_<b> as it will form them}):
    lower_trunk_forward in float64 rounded once, y3x = y3 + pad_257(xin) rounded once as the forward stores it, y3' = y3x - pad_257(xin),
    one float32 subtraction."""
    fw = host.lower_trunk_forward(wt, x0)
    res = {b: np.ascontiguousarray(fw["res%d" % b], f32) for b in (0, 1, 2)}
    xin = {0: pad257(np.asarray(x0, f32)), 1: res[0], 2: res[1]}
    y3x = {b: (fw["y3_%d" % b].astype(f32) + xin[b]).astype(f32) for b in (0, 1, 2)}
    return (y3x[2], res[2], y3x[1], res[1], y3x[0], res[0]), {b: (y3x[b] - xin[b]).astype(f32) for b in (0, 1, 2)}


def worst_scaled_diff(got, ref, names=OUTPUTS):
    """block_chain_cases.worst_scaled_diff, over the 67 outputs unless `names` says otherwise."""
    return chain.worst_scaled_diff(got, ref, names)


# ---- torch autograd in float64: block_chain_cases.autograd_block per block.  The variables and the input are leaves
def autograd_grads(weights, x0, d_res2):
    """d <d_res2, res2> / d each of the 66 variables and x0 by torch autograd in float64 from the float32 variables: name -> float64
    array in the variable's shape, `d_x0` [B,h,w,99]."""
    import torch
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    leaves = {n: t64(weights[n]).requires_grad_(True) for n in NAMES}
    xt = t64(x0).requires_grad_(True)
    t = xt
    for b in (0, 1, 2):
        t = autograd_block(t, b, leaves, weights)
    (t * t64(d_res2)).sum().backward()
    res = {k: v.grad.numpy() for k, v in leaves.items()}
    res["d_x0"] = xt.grad.numpy()
    return res


def autograd_nonlocal(weights, y3, xin, d_out, block):
    """d <d_out, out> / d (y3, xin) of the upper half of res_stack/<block> alone, out = lrelu(pad(z) + pad(xin)), by torch autograd in
    float64: (d_y3, d_skip)."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    nl = "res_stack/%d/non_local/" % block
    y, t = t64(y3).requires_grad_(True), t64(xin).requires_grad_(True)
    B, h, w, n = y.shape
    C = t.shape[3]
    proj = lambda u, name: torch.matmul(u, t64(weights[nl + name + "/kernel"])[0, 0]) + t64(weights[nl + name + "/bias"])   # noqa: E731
    f = torch.softmax(torch.matmul(proj(y, "theta").reshape(B, h * w, -1), proj(y, "phi").reshape(B, h * w, -1).transpose(1, 2)), -1)
    c = proj(torch.matmul(f, proj(y, "g").reshape(B, h * w, -1)).reshape(B, h, w, -1), "w")
    mean, var, gamma, beta = (t64(weights[nl + "bnorm/" + p]) for p in ("moving_mean", "moving_variance", "gamma", "beta"))
    z = y + ((c - mean) / torch.sqrt(var + BN_EPS) * gamma + beta)
    tp = torch.cat([t, torch.zeros(B, h, w, max(n - C, 0), dtype=torch.float64)], dim=3)
    zp = torch.cat([z, torch.zeros(B, h, w, max(C - n, 0), dtype=torch.float64)], dim=3)
    (F.leaky_relu(tp + zp, LRELU_ALPHA) * t64(d_out)).sum().backward()
    return y.grad.numpy(), t.grad.numpy()


# ---- the statements as they stood before the skip could be narrower than the block: SHA-256 of their outputs' bytes on
# colour_trunk_grad_cases.case(4, 32, 1), computed from the parent commit
def statement_hashes():
    """name -> the first 16 hex digits of SHA-256 over the float64 bytes of every array nonlocal_forward, nonlocal_grad, bottleneck_grad
    (block 5, C = 261) and colour_trunk_grad return on colour_trunk_grad_cases.case(4, 32, 1), keys in sorted order; the same of
    lower_trunk_forward and lower_trunk_grad on case(4, 32, 1); and of the bytes of the two trunk stages' blobs."""
    import colour_trunk_grad_cases as ct

    def digest(d):
        h = hashlib.sha256()
        for k in sorted(d):
            a = np.ascontiguousarray(d[k])
            h.update(k.encode() + b"\0" + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
        return h.hexdigest()[:16]

    wt, x, bmask, uv, d_xin, d_x = ct.case(4, 32, 1)
    fw = host.trunk_forward(wt, x, bmask, uv)
    out = {"trunk_forward": digest(fw)}
    out["nonlocal_forward"] = digest(host.nonlocal_forward(wt, fw["y3_4"], fw["res3"], block=4))
    n = host.nonlocal_grad(wt, fw["y3_4"], fw["res3"], d_xin, block=4)
    out["nonlocal_grad"] = digest(n)
    out["bottleneck_grad"] = digest(host.bottleneck_grad(wt, fw["res3"], n["d_y3"], n["d_skip"], block=4))
    out["colour_trunk_grad"] = digest(host.colour_trunk_grad(wt, fw["xh"], fw["y3_3"], fw["res3"], fw["y3_4"], fw["res4"], d_xin, d_x))
    # what the two trunk stages stated before they shared blocks_forward, blocks_grad and pack_block_chain: lower_trunk_forward and
    # lower_trunk_grad on case(4, 32, 1), and the two blobs of init_weights(3)
    wt, x0, d_res2 = case(4, 32, 1)
    fw = host.lower_trunk_forward(wt, x0)
    out["lower_trunk_forward"] = digest(fw)
    out["lower_trunk_grad"] = digest(host.lower_trunk_grad(wt, x0, *(fw[k] for k in FORWARD_KEYS), d_res2))
    for pack_blob in (pack.pack_colour_trunk_grad, pack.pack_lower_trunk_grad):
        out[pack_blob.__name__] = hashlib.sha256(pack_blob(lt_weights(3))).hexdigest()[:16]
    return out


# statement_hashes() of the commit before this stage ("Backpropagate through res_stack/4, /3 and the hole to res_stack/2"); the last four
# of the commit before the two trunk stages shared one statement (7a2e835, "Run the fp32 colour tail's clr_conv1 in Winograd form, V in
# registers")
PARENT_HASHES = {"trunk_forward": "8c4ed034f8f80d1c", "nonlocal_forward": "97da193570627956", "nonlocal_grad": "b4128aacb455776f",
                 "bottleneck_grad": "1e2d9561be137e4a", "colour_trunk_grad": "67b35df3a6dcdb65", "lower_trunk_forward": "aef8a25568988b03",
                 "lower_trunk_grad": "fc38bec6559da48c", "pack_colour_trunk_grad": "9b219beb4fe1502a", "pack_lower_trunk_grad": "595933d59e055770"}


# ---- constructed cases
def _tol(r):
    return AUTOGRAD_BOUND if r["dtype"] is np.float64 else E2E_BOUND


def check_zero_d_res2(run, h=4, w=32, B=1):
    """d_res2 = 0: all 66 gradients, every intermediate data gradient and d_x0 are exactly 0."""
    wt, x0, d_res2 = case(h, w, B, 5)
    r = run(wt, x0, np.zeros_like(d_res2))
    for name in NAMES:
        assert np.asarray(r[name]).shape == wt[name].shape and not np.asarray(r[name]).any(), name
    assert np.asarray(r["d_x0"]).shape == (B, h, w, 99)
    for name in ("d_x0",) + host.LOWER_TRUNK_DATA:
        assert not np.asarray(r[name]).any(), name


def swapped_blocks(wt, a=1, b=2):
    """`wt` with res_stack/<a>'s and res_stack/<b>'s variables exchanged (their shapes are the same)."""
    out = dict(wt)
    sa, sb = "res_stack/%d/" % a, "res_stack/%d/" % b
    for n in wt:
        if n.startswith(sa):
            out[n], out[sb + n[len(sa):]] = wt[sb + n[len(sa):]], wt[n]
    return out


def check_the_blocks_take_their_own_weights(run, h=4, w=32, B=1):
    """res_stack/<b>'s gradients agree with the single-block statements of block b on the run's own tensors; for blocks 1 and 2, whose
    shapes are the same, they differ from the statements of the other block on the same tensors by more than 1e-2 scaled.  And with
    block 1's and block 2's weights exchanged the whole result changes: the gradients under res_stack/1's names are then those of the
    block that runs second."""
    wt, x0, d_res2 = case(h, w, B, 10)
    r = run(wt, x0, d_res2)
    feeds = {2: (r["y3_2"], r["res1"], r["res2"], d_res2), 1: (r["y3_1"], r["res0"], r["res1"], r["d_xin2"]),
             0: (r["y3_0"], np.asarray(x0), r["res0"], r["d_xin1"])}
    for b, (y3, xin, out, d_out) in feeds.items():
        own = tuple(generator_bottleneck_trainable_names(b)) + tuple(generator_nonlocal_trainable_names(b))
        for other in ((1, 2) if b else (0,)):
            n = host.nonlocal_grad(wt, y3, xin, d_out, block=other, acts={"out": out})
            t = host.bottleneck_grad(wt, xin, n["d_y3"], n["d_skip"], block=other,
                                     acts={"a1": r["a1_%d" % b], "a2": r["a2_%d" % b]} if other == b else None)
            st = {name.replace("res_stack/%d/" % other, "res_stack/%d/" % b): v for name, v in list(n.items()) + list(t.items())}
            d, at = worst_scaled_diff(r, st, own)
            print("lower trunk: res_stack/%d's gradients against the statements of block %d: worst scaled difference %.3g at %s" % (b, other, d, at))
            assert (d <= _tol(r)) if other == b else (d > 1e-2), (b, other, d, at)
    r2 = run(swapped_blocks(wt), x0, d_res2)
    d, at = worst_scaled_diff(r2, r)
    print("lower trunk: blocks 1 and 2 exchanged against the chain as it is: worst scaled difference %.3g at %s" % (d, at))
    assert d > 1e-2 and worst_scaled_diff(r2, r, ("d_x0",))[0] > 1e-3


def check_nan_in_the_pad_lanes_of_x0(run, h=4, w=32, B=1):
    """x0 as the generator keeps it, 99 channels at 120 floats between pixels, with lanes 99..119 filled with NaN: no output changes by a
    byte against the dense x0, and none holds a NaN.  It fails if anything reads x0 beyond channel 98."""
    wt, x0, d_res2 = case(h, w, B, 11)
    wide = np.full((B, h, w, 120), np.nan, f32)
    wide[..., :99] = x0
    view = wide[..., :99]
    assert view.strides[2] == 480 and not view.flags["C_CONTIGUOUS"] and np.isnan(wide[..., 99:]).all()
    r, rv = run(wt, x0, d_res2), run(wt, view, d_res2)
    for name in OUTPUTS + host.LOWER_TRUNK_DATA:
        a, b = np.asarray(r[name]), np.asarray(rv[name])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and not np.isnan(b).any(), name


CONSTRUCTED = (check_zero_d_res2, check_the_blocks_take_their_own_weights, check_nan_in_the_pad_lanes_of_x0)


# ---- on the device: what test_lower_trunk_grad_gpu.py and tools/lower_trunk_bench.py share
PROBES = ("y3x2", "res2", "y3x1", "res1", "y3x0", "res0", "x0")      # Generator.probe's names of LowerTrunk's strided inputs, in their order


def probe_copies(probes):
    """The seven probes as the tensors call takes them: the first 257 channels of the y3x slots."""
    return [probes[k][..., :257].contiguous() if k.startswith("y3x") else probes[k] for k in PROBES]


def statement_on_device_tensors(wt, p, d_res2, acts):
    """lower_trunk_grad on the device's own float32 tensors p[PROBES] (y3x 257 wide): y3_<b> = y3x<b> - pad_257(xin_b), one float32
    subtraction as the chain's entry forms it."""
    xin = {0: pad257(p["x0"]), 1: p["res0"], 2: p["res1"]}
    y3 = {b: (p["y3x%d" % b][..., :257] - xin[b]).astype(f32) for b in (0, 1, 2)}
    return host.lower_trunk_grad(wt, p["x0"], y3[0], p["res0"], y3[1], p["res1"], y3[2], p["res2"], d_res2, acts=acts)


def device_parity(runner, h, w, B):
    """One of GPU_SIZES through the tensors call -> (wt, arrays (the eight inputs), y3s, res, worst scaled error against the statement
    on the device's a1, a2, the output it occurred at, the statement)."""
    import torch
    wt, x0, d_res2 = case(h, w, B, 1)
    six, y3s = device_inputs(wt, x0)
    arrays = six + (x0, d_res2)
    runner.load_weights(wt)
    res = runner.lower_trunk_grad(*to_dev(*arrays), keep=True)
    torch.cuda.synchronize()
    got = to_host(res)
    st = host.lower_trunk_grad(wt, x0, y3s[0], six[5], y3s[1], six[3], y3s[2], six[1], d_res2, acts=got)
    worst, at = worst_scaled_diff(got, st)
    return wt, arrays, y3s, got, worst, at, st


def generated_forward():
    """A generator's forward at (32, 256), B = 2, with init_weights(1) and inputs from default_rng(21), as the colour trunk's chained test
    runs it -> (generator, weights, inputs, outputs, clones of the probes the backward's statements read)."""
    import torch
    from blindshadowremoval_amd import Generator
    w = init_weights(1)
    gen = Generator(device=0)
    gen.load_weights(w)
    rng = np.random.default_rng(21)
    inputs, uv = to_dev(rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32), rng.uniform(0, 1, (2, 32, 256, 3)).astype(f32))
    outs = gen(inputs, uv)
    torch.cuda.synchronize()
    names = PROBES + ("y3x3", "res3", "y3x4", "res4", "xh", "y3x5", "res5", "up1", "x3", "up2", "x2", "y", "f1", "f2", "f")
    return gen, w, inputs, outs, {k: gen.probe(k).clone() for k in names}


def whole_backward_chained(gen, w, inputs, outs, probes):
    """On that forward: the device walk over objective.BACKWARD's five stages, GreyDecoder.backward, ColourTrunk.backward and
    LowerTrunk.backward(gen, d_res2), against the eight host statements chained on the device's own activations -> (the device's result
    on the host, the statement, the hole's share of the pixels)."""
    import torch
    from blindshadowremoval_amd import ColourTrunk, GreyDecoder, LowerTrunk, objective
    gs, _, mask22, _ = outs
    _, _, g_con_a, g_gs_a = host.example_inputs(32, 256, 2, 9)
    g_con, g_gs = to_dev(g_con_a, g_gs_a)
    table = tuple(s.name for s in objective.BACKWARD)
    assert len(table) == 5
    walked = objective.device_walk(objective.device_runners(table, w), gen, dict(img=inputs, gs=gs, mask22=mask22, grad_con=g_con, grad_gs=g_gs),
                                   keep=("tail", "bottleneck", "heads"))
    grey, colour, lower = GreyDecoder(0), ColourTrunk(0), LowerTrunk(0)
    for stage in (grey, colour, lower):
        stage.load_weights(w)
    g = grey.backward(gen, walked["heads"]["d_y"])
    c = colour.backward(gen, walked["bottleneck"]["d_xin"], g["d_x"], keep=True)
    res = to_host(lower.backward(gen, c["d_res2"], keep=True))
    torch.cuda.synchronize()
    c = to_host(c)
    acts = lambda stage, keys: {k: walked[stage][k].cpu().numpy() for k in keys}            # noqa: E731
    p = {k: v.cpu().numpy() for k, v in probes.items()}
    st_t = host.tail_grad(w, gs.cpu().numpy(), p["f"], g_con_a, g_gs_a, acts=acts("tail", ("a1", "a2")))
    st_d = host.decoder_grad(w, p["res5"], st_t["d_f"], acts={"f1": p["f1"], "f2": p["f2"], "f": p["f"]})
    st_n = host.nonlocal_grad(w, (p["y3x5"][..., :257] - p["res4"][..., :257]).astype(f32), p["res4"], st_d["d_x"], acts={"out": p["res5"]})
    st_b = host.bottleneck_grad(w, p["res4"], st_n["d_y3"], st_n["d_skip"], acts=acts("bottleneck", ("a1", "a2")))
    st_h = host.heads_grad(w, inputs.cpu().numpy(), p["y"], st_t["d_gs"], acts=acts("heads", ("mask",)))
    st_g = host.grey_decoder_grad(w, p["res2"], p["x3"], p["x2"], st_h["d_y"], acts={"up1": p["up1"], "up2": p["up2"], "y": p["y"]})
    y3_4 = (p["y3x4"][..., :257] - p["res3"][..., :257]).astype(f32)
    y3_3 = (p["y3x3"][..., :257] - p["xh"][..., :257]).astype(f32)
    st_c = host.colour_trunk_grad(w, p["xh"], y3_3, p["res3"], y3_4, p["res4"], st_b["d_xin"], st_g["d_x"], acts=c)
    st_l = statement_on_device_tensors(w, p, st_c["d_res2"], res)
    return res, st_l, float(p["xh"][..., 257].mean())
