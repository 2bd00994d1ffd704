"""Generate tests/golden/shadow_synth_*.npz — the reference's OWN `process_mask` (train_test_GSC.py:81-105) and the utils.py functions it
calls (utils.py:438-900), executed from their source over a numpy TensorFlow stand-in, plus its tone-curve / colour-matrix functions
(pure numpy in the reference) on a small image.

Runs on the machine that holds the reference only (REF below); nothing of the reference's text is stored in the repository or read by
a test — only the arrays are.  utils.py is imported whole (cv2, skimage, matplotlib, scipy.misc are stubbed where absent: this path
never executes them); `process_mask` is cut out of train_test_GSC.py by its `def` line and executed in a namespace that holds the
stand-in and utils' functions, because importing that file whole would import the model, the loaders and sklearn.

THE TAPE.  `tf.random.uniform` is replaced by a tape: each call is served from a numpy Generator by its own signature (shape, minval,
maxval, dtype), except the range-less scalar calls — those are the branch uniforms of process_mask and render_shadow_from_mask, and the
tape serves the values that force the case's branches.  Every call is logged; `record_from_log` reads the log in the reference's call
order into a ShadowDraws record (angles become float32 (cos, sin) pairs, computed as the stand-in computes them), and fills the draws
the taken branches never made from `shadow_synth.draw`.  So the host statement sees exactly the draws the reference's functions saw.

WHAT THIS PINS: the reference's control flow, call order, operand order, dtype flow, the meshgrid / transpose of utils.py:809-812, the
lerp order, the disc's pad / crop offsets, the level weights — everything its text states.
WHAT STAYS UNPINNED: TensorFlow's own arithmetic, as in DESIGN.md section 2.  The stand-in's op semantics are float32 and are ours:
  tf.linspace(a, b, n)            a + i * ((b - a) / (n - 1)) in float32 (a TensorFlow that stores `b` itself as the last sample puts the
                                  last row and column on a lattice point exactly; i * step may fall one ulp short of it)
  tf.image.resize NEAREST         half-pixel centres, floor((i + 0.5) * n_in / n_out)
  tf.signal.fft2d / ifft2d        np.fft in double precision, rounded to complex64 after each transform and product
  tf.nn.depthwise_conv2d VALID    tap by tap in filter order, float32 accumulation
  tf.reduce_sum / max / min       numpy's reductions on float32
  tf.exp / cos / sin / sqrt / pow numpy's float32 functions
A binary operation between a stand-in tensor and a numpy float64 scalar (the reference multiplies by rows of a float64 table) is done
in the tensor's dtype, as TensorFlow converts the constant.

Cases: the 16 branch combinations at S = 64 and three of them at S = 128, a few per file so that every file stays under the
repository's 1 MiB limit; the inputs are shadow_synth.example_inputs(S, 1, seed) and only the seed is stored.
For every case the tool asserts that no pixel of the Perlin map lies within 1e-5 of 0.15 (it moves to the next seed otherwise), so the thresholded mask is comparable exactly.  It then runs the host
statement on the same inputs and draws and records the largest difference of img / mask_sv / mask_edge in `measured_max_diff`; the
tests allow 4 x that, never above 1e-4.

Usage:  python tools/make_shadow_synth_fixture.py
"""
import contextlib
import importlib.util
import itertools
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from blindshadowremoval_amd import shadow_synth as host            # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ tensors
class Shape(tuple):
    def assert_has_rank(self, n):
        assert len(self) == n, (self, n)


class T(np.ndarray):
    """numpy array with TensorFlow's dtype rule for constants: a float64 operand that is no tensor is converted to the tensor's
    float32."""

    @property
    def shape(self):
        return Shape(np.ndarray.shape.__get__(self))

    def set_shape(self, shape):
        assert tuple(self.shape) == tuple(shape)

    def numpy(self):
        return np.asarray(self)

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kw):
        has_f32 = any(isinstance(a, T) and a.dtype == np.float32 for a in inputs)
        args = []
        for a in inputs:
            if isinstance(a, T):
                a = a.view(np.ndarray)
            elif has_f32 and isinstance(a, (np.floating, np.ndarray, float)) and np.asarray(a).dtype == np.float64:
                a = np.asarray(a).astype(np.float32)
            args.append(a)
        if out is not None:
            kw["out"] = tuple(o.view(np.ndarray) if isinstance(o, T) else o for o in out)
        res = getattr(ufunc, method)(*args, **kw)
        if out is not None:
            return out[0]
        return t(res) if isinstance(res, (np.ndarray, np.generic)) else res


def t(a, dtype=None):
    return np.asarray(a, dtype=dtype).view(T)


def _as(x):
    """An operand as the stand-in sees it: python floats and float64 arrays become float32, integers stay."""
    a = np.asarray(x)
    if a.dtype == np.float64:
        a = a.astype(np.float32)
    return a


_DT = {"float32": np.float32, "int32": np.int32, "complex64": np.complex64}


class Tape:
    def __init__(self, rng, branch_uniforms):
        self.rng, self.branch, self.log = rng, list(branch_uniforms), []

    def uniform(self, shape=(), minval=None, maxval=None, dtype="float32"):
        shape = tuple(int(s) for s in shape)
        if dtype == "int32":
            v = np.int32(self.rng.integers(int(minval), int(maxval)))
            assert shape == ()
            kind = ("int", int(minval), int(maxval))
        elif minval is None and shape == ():
            v = f32(self.branch.pop(0))
            kind = ("branch",)
        elif minval is None:
            v = self.rng.random(shape, dtype=np.float32)
            kind = ("angles", shape[0])
        else:
            v = f32(f32(minval) + self.rng.random(dtype=np.float32) * f32(maxval - minval))
            kind = ("range", float(minval), float(maxval))
        self.log.append((kind, v))
        return t(v)


def _pad(x, paddings, mode="constant"):
    pads = [(int(a), int(b)) for a, b in paddings]
    return t(np.pad(np.asarray(x), pads, mode={"constant": "constant", "reflect": "reflect"}[mode.lower()]))


def _depthwise(x, k, strides, padding, name=None):
    x, k = np.asarray(x, np.float32), np.asarray(k, np.float32)
    assert padding == "VALID" and tuple(strides) == (1, 1, 1, 1) and k.shape[3] == 1 and k.shape[2] == x.shape[3]
    ho, wo = x.shape[1] - k.shape[0] + 1, x.shape[2] - k.shape[1] + 1
    acc = np.zeros((x.shape[0], ho, wo, x.shape[3]), np.float32)
    for i in range(k.shape[0]):
        for j in range(k.shape[1]):
            acc = acc + k[i, j, :, 0] * x[:, i:i + ho, j:j + wo, :]
    return t(acc)


def _resize(x, size, method=None):
    assert method == "nearest"
    x = np.asarray(x)
    iy = np.floor((np.arange(int(size[0]), dtype=np.float32) + f32(0.5)) * (f32(x.shape[0]) / f32(int(size[0])))).astype(np.int64)
    ix = np.floor((np.arange(int(size[1]), dtype=np.float32) + f32(0.5)) * (f32(x.shape[1]) / f32(int(size[1])))).astype(np.int64)
    return t(x[np.minimum(iy, x.shape[0] - 1)][:, np.minimum(ix, x.shape[1] - 1)])


def _linspace(start, stop, num):
    num = int(num)
    start, stop = f32(start), f32(stop)
    step = f32((stop - start) / f32(num - 1))
    return t((start + np.arange(num, dtype=np.float32) * step).astype(np.float32))


def _range(a, b=None):
    a, b = (0, a) if b is None else (a, b)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return t(np.arange(float(a), float(b), dtype=np.float32))
    return t(np.arange(int(a), int(b), dtype=np.int32))


def _cast(x, dtype):
    return t(np.asarray(x).astype(_DT[dtype]))


def _fft(fn):
    return lambda x: t(fn(np.asarray(x).astype(np.complex128)).astype(np.complex64))


def make_tf(tape):
    tf = types.ModuleType("tensorflow")
    tf.float32, tf.int32, tf.complex64, tf.newaxis = "float32", "int32", "complex64", None
    tf.name_scope = lambda name: contextlib.nullcontext()
    tf.constant = lambda v: t(_as(v))
    tf.cond = lambda pred, a, b: a() if bool(pred) else b()
    tf.greater = lambda a, b: t(_as(a) > _as(b))
    tf.less_equal = lambda a, b: t(_as(a) <= _as(b))
    tf.unstack = lambda x, axis=0: [t(p) for p in np.moveaxis(np.asarray(x), axis, 0)]
    tf.stack = lambda xs, axis=0: t(np.stack([_as(x) for x in xs], axis=axis))
    tf.concat = lambda xs, axis: t(np.concatenate([_as(x) for x in xs], axis=axis))
    tf.expand_dims = lambda x, axis: t(np.expand_dims(_as(x), axis))
    tf.reshape = lambda x, shape: t(np.reshape(_as(x), [int(s) for s in shape]))
    tf.transpose = lambda x, perm: t(np.transpose(_as(x), perm))
    tf.tile = lambda x, reps: t(np.tile(_as(x), [int(r) for r in reps]))
    tf.clip_by_value = lambda x, lo, hi: t(np.clip(_as(x), _as(lo).astype(_as(x).dtype), _as(hi).astype(_as(x).dtype)))
    tf.abs = lambda x: t(np.abs(np.asarray(x)))
    tf.multiply = lambda a, b: t((np.asarray(a) * np.asarray(b)).astype(np.asarray(a).dtype))
    tf.divide = lambda a, b: t(_as(a) / _as(b))
    tf.minimum = lambda a, b: t(np.minimum(_as(a), _as(b)).astype(np.float32))
    tf.pow = lambda a, b: t(np.power(_as(a), b))
    tf.sqrt = lambda a: t(np.sqrt(_as(a)))
    tf.exp = lambda a: t(np.exp(_as(a)))
    tf.cos = lambda a: t(np.cos(_as(a)))
    tf.sin = lambda a: t(np.sin(_as(a)))
    tf.reduce_sum = lambda x, axis=None: t(np.sum(_as(x), axis=axis))
    tf.reduce_max = lambda x, axis=None: t(np.max(_as(x), axis=axis))
    tf.reduce_min = lambda x, axis=None: t(np.min(_as(x), axis=axis))
    tf.zeros = lambda shape: t(np.zeros([int(s) for s in shape], np.float32))
    tf.shape = lambda x: tuple(np.ndarray.shape.__get__(np.asarray(x)))
    tf.cast, tf.pad, tf.range, tf.linspace = _cast, _pad, _range, _linspace
    tf.meshgrid = lambda a, b: [t(m) for m in np.meshgrid(np.asarray(a), np.asarray(b))]
    tf.math = types.SimpleNamespace(ceil=lambda x: t(np.ceil(_as(x))), floormod=lambda x, y: t(_as(x) - np.floor(_as(x) / f32(y)) * f32(y)))
    tf.signal = types.SimpleNamespace(fft2d=_fft(np.fft.fft2), ifft2d=_fft(np.fft.ifft2))
    tf.nn = types.SimpleNamespace(depthwise_conv2d=_depthwise)
    tf.image = types.SimpleNamespace(resize=_resize, ResizeMethod=types.SimpleNamespace(NEAREST_NEIGHBOR="nearest"),
                                     grayscale_to_rgb=lambda x: t(np.repeat(_as(x), 3, axis=-1)))
    tf.random = types.SimpleNamespace(uniform=tape.uniform)
    return tf


class _Stub(types.ModuleType):          # imported by utils.py at top level, never executed on this path
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(self.__name__ + "." + name)


def import_reference(tf):
    """-> (utils module, process_mask) executed from the reference's files over `tf`."""
    mods = {"tensorflow": tf, "tensorflow.keras": _Stub("tensorflow.keras"), "tensorflow.keras.layers": _Stub("tensorflow.keras.layers")}
    for name in ("cv2", "skimage", "skimage.draw", "matplotlib", "matplotlib.tri", "scipy.misc"):
        try:
            importlib.import_module(name)
        except Exception:
            mods[name] = _Stub(name)
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    if "scipy.misc" in mods:
        import scipy
        scipy.misc = mods["scipy.misc"]
    try:
        spec = importlib.util.spec_from_file_location("ref_utils", os.path.join(REF, "utils.py"))
        utils = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(utils)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    lines = open(os.path.join(REF, "train_test_GSC.py")).read().split("\n")
    lo = next(i for i, l in enumerate(lines) if l.startswith("def process_mask("))
    hi = next(i for i in range(lo + 1, len(lines)) if lines[i].startswith("def ") or lines[i].startswith("class "))
    ns = {"tf": tf, "np": np}
    ns.update({k: getattr(utils, k) for k in ("apply_ss_shadow_map", "get_brightness_mask", "render_perlin_mask")})
    exec(compile("\n".join(lines[lo:hi]), "process_mask", "exec"), ns)
    return utils, ns["process_mask"]


def grads_of(u):
    a = f32(2.0 * np.pi) * np.asarray(u, np.float32)
    return np.stack([np.cos(a), np.sin(a)], axis=2).astype(np.float32)


def record_from_log(log, S, fill):
    """The tape's log of one item, in the reference's call order, -> ShadowDraws; `fill` supplies what no call drew."""
    d = fill
    it = iter(log)

    def nxt(kind0):
        kind, v = next(it)
        assert kind[0] == kind0, (kind, kind0)
        return v

    def lattices(cells):
        out = []
        for n in cells:
            u = nxt("angles")
            assert u.shape == (n + 1, n + 1)
            out.append(grads_of(u))
        return out
    d.u_mask = nxt("branch")
    if not d.u_mask > f32(0.4):
        d.p_shadow = nxt("range")
        d.g_shadow = lattices(host.SHADOW_CELLS)
        d.disc_sz = nxt("int")
        d.u_sv = nxt("branch")
        if d.u_sv > f32(0.5):
            d.blur_size = nxt("int")
            d.p_guide = nxt("range")
            d.g_guide = lattices(host.GUIDE_CELLS)
    d.u_ss = nxt("branch")
    if d.u_ss > f32(0.25):
        d.r = nxt("range")
        d.gains = np.array([nxt("range") for _ in range(6)], np.float32)
    d.u_bright = nxt("branch")
    d.p_bright = nxt("range")
    d.g_bright = lattices(host.BRIGHT_CELLS)
    assert next(it, None) is None
    return d


def inputs(S, seed):
    return tuple(a[0] for a in host.example_inputs(S, 1, seed))


class ScaledTape(Tape):
    """The SS scale is drawn from [1, 15) by the reference; below S = 256 rule 2 admits less, so that one call is served from the
    admitted range (the value is logged and replayed like every other)."""

    def __init__(self, rng, branch_uniforms, S):
        super().__init__(rng, branch_uniforms)
        self.S = S

    def uniform(self, shape=(), minval=None, maxval=None, dtype="float32"):
        if dtype == "float32" and minval == 1 and maxval == host.MAX_SS_SIGMA:
            v = host.draw(self.rng, self.S).r
            self.log.append((("range", 1.0, float(maxval)), v))
            return t(v)
        return super().uniform(shape, minval, maxval, dtype)


def run_case(S, combo, seed):
    """One item through the reference's process_mask -> dict of arrays, or None where a Perlin pixel lies within 1e-5 of 0.15."""
    perlin, ss, low, sv = combo
    branch = [0.2 if perlin else 0.7] + ([0.9 if sv else 0.2] if perlin else []) + [0.6 if ss else 0.1, 0.8 if low else 0.3]
    rng = np.random.default_rng(seed)
    tape = ScaledTape(rng, branch, S)
    tf = make_tf(tape)
    utils, process_mask = import_reference(tf)
    captured = {}
    real = utils.perlin_collection

    def spy(size, reso, octaves, persistence):
        out = real(size, reso, octaves, persistence)
        if octaves == 4:
            captured["perlin_map"] = np.asarray(out).copy()
        return out
    utils.perlin_collection = spy
    mask, gt, dark, face = inputs(S, seed)
    with np.errstate(all="ignore"):
        img, mask_sv, mask_edge = process_mask(t(mask[None]), S, t(gt[None]), t(dark[None]), t(np.zeros((1, S, S, 3), np.float32)), t(face[None]))
    assert not tape.branch
    d = record_from_log(tape.log, S, host.draw(np.random.default_rng(seed + 10 ** 6), S))
    pmap = captured.get("perlin_map", np.zeros((S, S), np.float32))
    if perlin and np.abs(pmap.astype(np.float64) - 0.15).min() <= 1e-5:
        return None
    out = {"seed": np.int64(seed), "perlin_map": pmap, "img": np.asarray(img)[0], "mask_sv": np.asarray(mask_sv)[0],
           "mask_edge": np.asarray(mask_edge)[0], "draws": host.pack_draws([d], S)[0], "combo": np.array(combo, np.int32)}
    for k in ("img", "mask_sv", "mask_edge", "perlin_map"):
        assert out[k].dtype == np.float32 and np.isfinite(out[k]).all(), k
    return out, d


def tone_case(utils_mod, seed=5, S=16):
    rng = np.random.default_rng(seed)
    img = rng.random((S, S, 3)).astype(np.float32)
    gain = 0.5 + rng.uniform(-0.3, 0.3, 3)
    tone = utils_mod.apply_tone_curve(img, gain=gain, is_rgb=True)
    ctm = utils_mod.get_ctm_ls(img, tone)
    return {"tone_in": img, "tone_gain": gain, "tone_out": np.asarray(tone), "tone_ctm": np.asarray(ctm), "tone_applied": np.asarray(utils_mod.apply_ctm(img, ctm))}


CASES = {64: list(itertools.product((True, False), repeat=4)),                               # (Perlin mask, SS, low floor, SV blur): all 16
         128: [(True, True, True, True), (True, True, False, False), (False, True, True, False)]}
PER_FILE = {64: 4, 128: 1}          # cases per file: every file stays under the repository's limit for a committed file


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    tone = tone_case(import_reference(make_tf(Tape(np.random.default_rng(0), [])))[0])
    for S, combos in CASES.items():
        done, worst = [], 0.0
        for ci, combo in enumerate(combos):
            seed = 1000 * S + 10 * ci
            while True:
                got = run_case(S, combo, seed)
                if got is not None:
                    break
                seed += 1
            case, d = got
            ref = host.process_item(*inputs(S, seed), d)
            assert ref["status"] == 0
            for k in ("img", "mask_sv", "mask_edge"):
                worst = max(worst, float(np.abs(ref[k].astype(np.float64) - case[k].astype(np.float64)).max()))
            print("S=%d case %2d %s seed %d: |host - reference| perlin %.3g, outputs so far %.3g" % (
                S, ci, combo, seed, float(np.abs(ref["perlin_map"] - case["perlin_map"]).max()), worst))
            done.append(case)
        for fi in range(0, len(done), PER_FILE[S]):
            arrays = {"measured_max_diff": np.float64(worst), "backend": np.array("numpy stand-in"), "S": np.int64(S)}
            for ci, case in enumerate(done[fi:fi + PER_FILE[S]]):
                arrays.update({"c%d_%s" % (ci, k): v for k, v in case.items()})
            if S == 64 and fi == 0:
                arrays.update(tone)
            path = os.path.join(golden, "shadow_synth_%d_%d.npz" % (S, fi // PER_FILE[S]))
            np.savez_compressed(path, **arrays)
            print("wrote %s (%d bytes), measured_max_diff %.3g" % (path, os.path.getsize(path), worst))
            assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
