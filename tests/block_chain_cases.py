"""What the case modules (colour_trunk_grad_cases.py, lower_trunk_grad_cases.py) and the device tests (test_colour_trunk_grad_gpu.py,
test_lower_trunk_grad_gpu.py) of the two chains of residual blocks share: the weight cache, the scaled differences, the block in torch
autograd, host/device copies, the table of the launch that first writes each output, and the bodies of the device checks that read
the same for any chain."""
import hashlib

import numpy as np

from blindshadowremoval_amd.weights import BN_EPS, LRELU_ALPHA, generator_bottleneck_trainable_names, generator_nonlocal_trainable_names, init_weights

_weights = {}


def weights(seed=3, variant="gsc"):
    """init_weights(seed): non-trivial BN statistics.  Cached: treat as read-only."""
    if (seed, variant) not in _weights:
        _weights[(seed, variant)] = init_weights(seed, variant=variant)
    return _weights[(seed, variant)]


def worst_scaled_diff(got, ref, names):
    """The largest of max |got[v] - ref[v]| / max |ref[v]| over `names` (an output whose reference is all 0 must be all 0), and the name
    it occurred at.  A block's d phi/bias is identically zero in exact arithmetic (the rows of dS sum to 0), so it is held as an absolute
    bound on the scale of max |d theta/bias| of that block, as nonlocal_grad_cases does."""
    worst, at = 0.0, ""
    for name in names:
        a, b = np.asarray(got[name], np.float64), np.asarray(ref[name], np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        scale = np.abs(b).max()
        if name.endswith("non_local/phi/bias"):
            scale = np.abs(np.asarray(ref[name.replace("phi/bias", "theta/bias")], np.float64)).max()
        d = float(np.abs(a - b).max() / scale) if scale > 0 else (0.0 if not a.any() else np.inf)
        if d > worst:
            worst, at = d, name
    return worst, at


def scaled_error(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ---- torch autograd in float64, written from the reference's semantics (model.py:23-61, 81-113): conv2d with padding 1, inference BN,
# leaky_relu 0.3, the non-local block, and the skip zero-padded to the wider of the two
def autograd_block(t, b, leaves, weights):
    """res_stack/<b> on t [B,h,w,C] in torch float64: `leaves` name -> tensor for the block's trainable variables."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.from_numpy(np.array(a, np.float64))                        # noqa: E731
    st = "res_stack/%d/" % b
    B, h, w, C = t.shape

    def bn(c, stem):
        mean, var = (t64(weights[stem + p]) for p in ("moving_mean", "moving_variance"))
        return (c - mean) / torch.sqrt(var + BN_EPS) * leaves[stem + "gamma"] + leaves[stem + "beta"]

    def conv(u, j, pad):
        k = leaves[st + "conv%d/kernel" % j].permute(3, 2, 0, 1)                     # HWIO -> OIHW
        c = F.conv2d(u.permute(0, 3, 1, 2), k, leaves[st + "conv%d/bias" % j], padding=pad).permute(0, 2, 3, 1)
        return bn(c, st + "bnorm%d/" % j)

    y = F.leaky_relu(conv(t, 1, 0), LRELU_ALPHA)
    y = F.leaky_relu(conv(y, 2, 1), LRELU_ALPHA)
    y = conv(y, 3, 0)
    nl = st + "non_local/"
    proj = lambda u, name: torch.matmul(u, leaves[nl + name + "/kernel"][0, 0]) + leaves[nl + name + "/bias"]   # noqa: E731
    g_x = proj(y, "g").reshape(B, h * w, -1)
    phi_x = proj(y, "phi").reshape(B, h * w, -1).transpose(1, 2)
    theta_x = proj(y, "theta").reshape(B, h * w, -1)
    f = torch.softmax(torch.matmul(theta_x, phi_x), -1)
    z = y + bn(proj(torch.matmul(f, g_x).reshape(B, h, w, -1), "w"), nl + "bnorm/")
    n = z.shape[3]
    if C < n:                                                                        # model.py:105-113: the narrower of the two is padded
        t = torch.cat([t, torch.zeros(B, h, w, n - C, dtype=torch.float64)], dim=3)
    elif C > n:
        z = torch.cat([z, torch.zeros(B, h, w, C - n, dtype=torch.float64)], dim=3)
    return F.leaky_relu(t + z, LRELU_ALPHA)


# ---- on the device
def to_dev(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def flat_bytes(res, keys):
    return [res[k].cpu().numpy().tobytes() for k in keys]


# the launch (1..12) of its chain that first writes each map, from the two chains' own tables (test_nonlocal_grad_gpu.py,
# test_bottleneck_grad_gpu.py)
NL_FIRST = {"y3": 1, "dz": 1, "theta": 2, "phi": 2, "g": 2, "m": 3, "r": 3, "A": 3, "dA": 4, "D": 4, "d_phi": 5, "d_g": 5, "d_theta": 6, "Wgd": 11, "Sz": 12}
BN_FIRST = {"xp": 1, "dyp": 1, "a1": 2, "a2": 3, "gz2": 4, "gz1": 5, "Wg1": 11, "Wg2": 11, "Wg3": 11, "S1": 12, "S2": 12, "S3": 12}


def first_table(blocks, output, tail):
    """name -> the launch (1..) of the chain over `blocks` that first writes it: the maps, the data gradients and the variables of every
    block.  With a `tail` launch the stage's `output` is the tail's and every block's d_xin has its own name; without one, `output` is
    the last block's d_xin."""
    first = {}
    for k, b in enumerate(blocks):
        last = not tail and k == len(blocks) - 1
        first.update(("nl%d.%s" % (b, n), 24 * k + at) for n, at in NL_FIRST.items())
        first.update(("bn%d.%s" % (b, n), 24 * k + 12 + at) for n, at in BN_FIRST.items())
        first.update({"d_skip_%d" % b: 24 * k + 1, "d_y3_%d" % b: 24 * k + 10, output if last else "d_xin%d" % b: 24 * k + 21})
        first.update((n, 24 * k + (11 if n.endswith("/kernel") else 12)) for n in generator_nonlocal_trainable_names(b))
        first.update((n, 24 * k + 12 + (11 if n.endswith("/kernel") else 12)) for n in generator_bottleneck_trainable_names(b))
    if tail:
        first[output] = 24 * len(blocks) + 1
    return first


def as_block5(wt, res, b):
    """Block b's variables, and its gradients out of `res`, under res_stack/5's names: what the single-block tests read."""
    import bottleneck_grad_cases
    moved = bottleneck_grad_cases.with_block5(wt, b)
    src = "res_stack/%d/" % b
    return moved, {"res_stack/5/" + n[len(src):]: v for n, v in res.items() if n.startswith(src)}


def check_every_stop(runner, arrays, first, output):
    """stages(..., n) for every n: what launches 1..n write is the complete call's, byte for byte, and the outputs of the launches that
    did not run are zero."""
    import pytest
    import torch
    n = len(runner.LAUNCHES)
    t = to_dev(*arrays)
    whole = runner.stages(*t, n)
    whole.update(type(runner).split_grads(whole[""]))
    assert set(first) <= set(whole)
    for stop in range(1, n + 1):
        runner._scratch.zero_()                # what a stop leaves was written by this call, not by the one before
        got = runner.stages(*t, stop)
        got.update(type(runner).split_grads(got[""]))
        for name, at in first.items():
            if stop >= at:
                assert torch.equal(got[name], whole[name]), (stop, name)
            elif "/" in name or name == output:
                assert not bool(got[name].any()), (stop, name)
    with pytest.raises(ValueError, match="stop_after"):
        runner.stages(*t, n + 1)


def check_a_repeated_call_and_two_sizes_on_one_scratch(runner, call, wt, large, small, keys):
    """`large`, `small`: (arrays, the first result on the host) at two sizes; `call`: the name of the runner's tensors call."""
    (arrays3, res3), (arrays1, res1) = large, small
    t3, t1 = to_dev(*arrays3), to_dev(*arrays1)
    run = getattr(runner, call)
    first3 = flat_bytes(run(*t3), keys)
    first1 = flat_bytes(run(*t1), keys)                        # the larger size, then the smaller on the larger call's scratch
    assert first3 == [res3[k].tobytes() for k in keys] and first1 == [res1[k].tobytes() for k in keys]
    assert flat_bytes(run(*t3), keys) == first3
    assert flat_bytes(run(*t1), keys) == first1
    kept = run(*t1, keep=True)
    assert flat_bytes(kept, keys) == first1 and all(k in kept for k in type(runner).KEPT)   # keeping the maps changes no output
    for t, a in zip(t1, arrays1):
        assert t.cpu().numpy().tobytes() == a.tobytes()                     # no input is ever written
    fresh = type(runner)(0)
    fresh.load_weights(wt)
    assert flat_bytes(getattr(fresh, call)(*t1), keys) == first1   # a scratch of its own size gives the same bytes


def check_graph_capture(runner, call, arrays, keys):
    """Stream capture refuses a host synchronisation and work on another stream that is not joined: a call that is captured, replayed
    and gives the eager call's bytes has neither."""
    import torch
    run = getattr(runner, call)
    t = to_dev(*arrays)
    eager = flat_bytes(run(*t), keys)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*t)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            res = run(*t)
    torch.cuda.current_stream().wait_stream(side)
    for k in keys:
        res[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flat_bytes(res, keys) == eager


def device_digest(res, output, kept):
    """The first 16 hex digits of SHA-256 over the bytes of the flat gradient buffer, the stage's output and every keep=True entry in
    sorted key order, of a result on the host."""
    h = hashlib.sha256()
    for k in ("", output) + tuple(sorted(kept)):
        h.update(np.ascontiguousarray(res[k]).tobytes())
    return h.hexdigest()[:16]
