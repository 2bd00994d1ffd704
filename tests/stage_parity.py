"""Teacher-forced stage table of the generator forward (helper of tests/test_stage_parity_*.py).

Each stage takes the probes that are its inputs (``bsr_probe`` names, csrc/bsr_api.hip), upcast to fp64, runs the fp64 oracle
(``GeneratorOracle(dtype=torch.float64)``) for that stage alone, and compares the result with the probe(s) that are its output:

    err = max|got - ref64| / max|ref64|        over the rows given

Feeding a stage the GPU's own inputs isolates its error from everything upstream, so each stage can be held to a budget of its
own; the GPU's ``bmask`` is an input of ``res3_input``, so a threshold flip (model.py:256) needs no special protocol here.

``probes`` is a dict of NHWC tensors named as ``Generator.probe`` names them, plus ``inputs``, ``uv`` (and ``reg`` for TSM) and
the four outputs under ``gs``, ``con_rgb``, ``mask22``, ``dif`` (``dif`` is the 4th output, model.py:288).  ``oracle_probes``
builds the same dict from an oracle forward (the wiring check of the CPU tests).
"""
from typing import Dict, List, Optional, Tuple

import torch

from oracle.gsc_oracle import GeneratorOracle, GeneratorTSMOracle, conv2d_same, leaky_relu, resize_bilinear, share_layer

N_RES = 6
BLOCK_IN = {0: "x0", 1: "res0", 2: "res1", 3: "xh", 4: "res3", 5: "res4"}   # input of res block i (model.py:239-240,259-262)
Y3X_CS = 288          # the y3x probe keeps 9 channel tiles of 32 (bsr_api.hip CS_Y3X)

# the stage kinds, in forward order; every res block i gives res_head (-> y3x<i>), res_att (-> att<i>) and res_block (-> res<i>)
GSC_STAGES = ("stem", "down1", "down2", "down3_uv", "res_head", "res_att", "res_block", "up1", "up2", "up3", "heads",
              "res3_input", "clr_up1", "clr_up2", "clr_up3", "colour_tail")
TSM_STAGES = ("tsm_down3_share",)
# The whole TSM forward (model_with_TSM.py:261-325): the GSC kinds where the stage is the same function of wider tensors, and
#   tsm_res_tail     channels [288, C) of res<i> = leaky_relu(x[..., 288:]) (model.py:105-113: the wider of x / y is kept), normalised by
#                    that slice's own maximum — small next to the GEMM channels, so a block-wide maximum would hide them;
#   tsm_res3_select  the lanes of xh that are a select or a copy: [0, 291) = res2 * (1 - bmask), 291 = bmask, the last 3 = the uv slot of x0;
#   tsm_share2       lanes [292, 874) of xh = ShareLayer(xh[..., :291]) from the GPU's own x_hole lanes, normalised by its own slice.
#                    With share=False both ShareLayers are copies: the share lanes of x0 are listed under this kind too (stage "share1"),
#                    and every tsm_share2 line must then be exactly 0 (the tests assert that apart from the budget).
TSM_FULL_STAGES = ("stem", "down1", "down2", "tsm_down3_share", "res_head", "res_att", "res_block", "tsm_res_tail", "up1", "up2", "up3",
                   "heads", "tsm_res3_select", "tsm_share2", "clr_up1", "clr_up2", "clr_up3", "colour_tail")
EXACT_STAGES = ("res3_input", "tsm_res3_select")     # a select, not arithmetic: compared as max|got - ref|, must be 0
WEIGHTLESS_STAGES = ("tsm_res_tail", "tsm_share2")   # arithmetic without a weight: rounding the weights to fp16 cannot move them
C_X, C_R_TSM = 96, 291        # down3's channels; TSM x0 = cat[x 96 | x_share 192 | uv 3] = 291, and res0..2 keep that width


def smooth_reg(B: int, S: int, g: torch.Generator) -> torch.Tensor:
    """The [B,S,S,6] offset fields of the TSM tests: smooth, a few cells in amplitude, some leaving the map so that the clamp is hit."""
    reg = torch.nn.functional.interpolate((torch.rand(B, 6, 9, 9, generator=g) - 0.5) * 0.3, size=(S, S), mode="bicubic",
                                          align_corners=True).permute(0, 2, 3, 1).contiguous()
    reg[..., 2] = 0
    reg[..., 5] = 0
    return reg


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    scale = float(ref.abs().max())
    diff = float((got.double() - ref).abs().max())
    return diff / scale if scale > 0 else diff


def y3x_ref(y3: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """y3 + pad(x) over max(C_y3, C_x) channels (model.py:105-113 before the `w` term), cut at the probe's 288."""
    c = max(y3.shape[-1], x.shape[-1])
    out = y3.new_zeros(*y3.shape[:3], c)
    out[..., :y3.shape[-1]] += y3
    out[..., :x.shape[-1]] += x
    return out[..., :Y3X_CS]


def _cat(*ts):
    return torch.cat(ts, dim=3)


class Result:
    """errs[(stage kind, stage name, output)] = error;  info: free-form lines for the log (attention logit scale)."""

    def __init__(self, keep_refs: bool = False):
        self.errs: Dict[Tuple[str, str, str], float] = {}
        self.info: List[str] = []
        self.refs: Optional[Dict[Tuple[str, str, str], torch.Tensor]] = {} if keep_refs else None   # what each stage computed (tools/f16_stage_emulation.py)

    def add(self, kind, stage, name, got, ref):
        if self.refs is not None:
            self.refs[(kind, stage, name)] = ref
        if kind in EXACT_STAGES:
            assert got.shape == ref.shape, (stage, name)
            self.errs[(kind, stage, name)] = float((got.double() - ref).abs().max())
        else:
            self.errs[(kind, stage, name)] = rel_err(got, ref)

    def by_kind(self) -> Dict[str, float]:
        out: Dict[str, float] = {}
        for (kind, _, _), e in self.errs.items():
            out[kind] = max(out.get(kind, 0.0), e)
        return out

    def lines(self, tag: str) -> List[str]:
        return ["%s %-16s %-12s %-8s %.3e" % (tag, k, s, n, e) for (k, s, n), e in self.errs.items()] + \
               ["%s %s" % (tag, l) for l in self.info]


def run_gsc_stages(oracle64: GeneratorOracle, p: Dict[str, torch.Tensor], keep_refs: bool = False) -> Result:
    """Every GSC stage whose input and output probes are in ``p`` (att<i> only when present: fused attention + `w` keeps it in LDS)."""
    return _run_stages(oracle64, p, None, keep_refs)


def run_tsm_full_stages(oracle64: GeneratorTSMOracle, p: Dict[str, torch.Tensor], frame: int, share: bool = True, keep_refs: bool = False) -> Result:
    """Every stage of the TSM forward (TSM_FULL_STAGES).  ``p`` also holds ``reg``; its rows must be whole frame groups, because the
    ShareLayer mixes the rows of a group."""
    assert p["x3"].shape[0] % frame == 0, "the rows handed to the TSM table must be whole frame groups"
    return _run_stages(oracle64, p, (frame, share), keep_refs)


def _run_stages(o: GeneratorOracle, p: Dict[str, torch.Tensor], tsm: Optional[Tuple[int, bool]], keep_refs: bool = False) -> Result:
    """The forward, stage by stage.  ``tsm``: None for the GSC generator, (frame, share) for the TSM one — the same stage code on
    wider tensors, plus the stages only that forward has."""
    r = Result(keep_refs)
    assert o.dtype == torch.float64
    p = {k: v.detach().cpu().to(torch.float64) for k, v in p.items()}
    r.add("stem", "stem", "x1", p["x1"], o.conv_block(p["inputs"], "conv1"))
    r.add("down1", "down1", "x2", p["x2"], o.conv_block(p["x1"], "down1", 2))
    r.add("down2", "down2", "x3", p["x3"], o.conv_block(p["x2"], "down2", 2))
    x = o.conv_block(p["x3"], "down3", 2)
    uv_s = resize_bilinear(p["uv"], x.shape[1:3])
    if tsm is None:
        r.add("down3_uv", "down3_uv", "x0", p["x0"], _cat(x, uv_s))
    else:
        _tsm_down3_share(r, p, x, uv_s, *tsm)
    for i in range(N_RES):
        if i == 3:
            _res3_input(r, p) if tsm is None else _tsm_res3_input(r, p, *tsm)
        xin, pr = p[BLOCK_IN[i]], {}
        res = o.res_bottleneck(xin, i, pr)
        y3 = pr["res_stack/%d/y3" % i]
        ref = y3x_ref(y3, xin)
        r.add("res_head", "res%d" % i, "y3x", p["y3x%d" % i][..., :ref.shape[-1]], ref)
        if "att%d" % i in p:
            r.add("res_att", "res%d" % i, "att", p["att%d" % i], pr["res_stack/%d/non_local/att" % i])
            r.info.append("res%d attention logits max|theta.phi| %.1f" % (i, _logit_max(o, y3, i)))
        r.add("res_block", "res%d" % i, "res", p["res%d" % i], res)
        if tsm is not None:
            assert res.shape[-1] == xin.shape[-1] > Y3X_CS
            r.add("tsm_res_tail", "res%d" % i, "tail", p["res%d" % i][..., Y3X_CS:], leaky_relu(xin[..., Y3X_CS:]))
        if i == 2:
            r.add("up1", "up1", "up1", p["up1"], o.convt_block(p["res2"], "up1"))
            r.add("up2", "up2", "up2", p["up2"], o.convt_block(_cat(p["up1"], p["x3"]), "up2"))
            r.add("up3", "up3", "y", p["y"], o.convt_block(_cat(p["up2"], p["x2"]), "up3"))
            gs, mask22, _, d32 = o.heads(p["y"], p["inputs"])
            r.add("heads", "heads", "gs", p["gs"], gs)
            r.add("heads", "heads", "mask22", p["mask22"], mask22)
            r.add("heads", "heads", "d32", p["d32"], d32)
    f1 = o.convt_block(p["res5"], "clr_up1")
    r.add("clr_up1", "clr_up1", "f1", p["f1"], f1)
    r.add("clr_up2", "clr_up2", "f2", p["f2"], o.convt_block(p["f1"], "clr_up2"))
    r.add("clr_up3", "clr_up3", "f", p["f"], o.convt_block(p["f2"], "clr_up3"))
    con_rgb, dif2 = o.colour_tail(p["gs"], p["f"], p["inputs"])
    r.add("colour_tail", "colour_tail", "con_rgb", p["con_rgb"], con_rgb)
    r.add("colour_tail", "colour_tail", "dif", p["dif"], dif2)
    return r


def _res3_input(r: Result, p):
    """xh = cat[res2 * (1 - bmask), bmask, uv_s] (model.py:258-259), uv_s from the uv slot of x0: exact."""
    bm = p["bmask"]
    assert set(bm.unique().tolist()) <= {0.0, 1.0}
    r.add("res3_input", "res3_input", "xh", p["xh"], _cat(p["res2"] * (1 - bm), bm, p["x0"][..., -3:]))


def _logit_max(o: GeneratorOracle, y3: torch.Tensor, i: int) -> float:
    """max |theta_x . phi_x| of block i (model.py:51, no 1/sqrt(d)): the scale the softmax amplifies errors by."""
    st = "res_stack/%d/non_local/" % i
    t = y3.shape[1] * y3.shape[2]
    th = conv2d_same(y3, o.w[st + "theta/kernel"], o.w[st + "theta/bias"]).reshape(y3.shape[0], t, -1)
    ph = conv2d_same(y3, o.w[st + "phi/kernel"], o.w[st + "phi/bias"]).reshape(y3.shape[0], t, -1)
    return float(torch.matmul(th, ph.transpose(1, 2)).abs().max())


def _tsm_down3_share(r: Result, p, x, uv_s, frame: int, share: bool):
    """x0 = cat[x, ShareLayer(x), uv_s] (model_with_TSM.py:268-272) from x3, uv, reg.  share=False: the ShareLayer is cat[x, x], a copy
    of the GPU's own down3 lanes, listed on its own so that it is held to 0 and not to the conv's budget."""
    r.add("tsm_down3_share", "tsm_down3_share", "x0", p["x0"], _cat(x, share_layer(x, p["reg"], frame, share), uv_s))
    if not share:
        own = p["x0"][..., :C_X]
        r.add("tsm_share2", "share1", "x0", p["x0"][..., C_X:3 * C_X], _cat(own, own))


def _tsm_res3_input(r: Result, p, frame: int, share: bool):
    """xh = cat[x_hole 291, bmask, ShareLayer(x_hole) 582, uv_s] (model_with_TSM.py:291-293): the select / copy lanes exactly, the
    ShareLayer lanes from the x_hole lanes ``xh`` itself holds."""
    bm, xh, c = p["bmask"], p["xh"], C_R_TSM
    assert set(bm.unique().tolist()) <= {0.0, 1.0}
    assert xh.shape[-1] == 3 * c + 4 and p["res2"].shape[-1] == c
    r.add("tsm_res3_select", "res3_input", "xh", _cat(xh[..., :c + 1], xh[..., -3:]), _cat(p["res2"] * (1 - bm), bm, p["x0"][..., -3:]))
    r.add("tsm_share2", "share2", "xh", xh[..., c + 1:3 * c + 1], share_layer(xh[..., :c], p["reg"], frame, share))


def run_tsm_stages(oracle64: GeneratorTSMOracle, p: Dict[str, torch.Tensor], frame: int) -> Result:
    """TSM down3 + first ShareLayer alone: x3, uv, reg -> x0 = cat[x, x_share, uv_s].  The rows of ``p`` must be whole frame groups."""
    o, r = oracle64, Result()
    assert o.dtype == torch.float64 and p["x3"].shape[0] % frame == 0
    p = {k: v.detach().cpu().to(torch.float64) for k, v in p.items()}
    x = o.conv_block(p["x3"], "down3", 2)
    _tsm_down3_share(r, p, x, resize_bilinear(p["uv"], x.shape[1:3]), frame, True)
    return r


GSC_PROBES = ["x1", "x2", "x3", "x0", "up1", "up2", "y", "d32", "bmask", "xh", "f1", "f2", "f"] + \
             ["y3x%d" % i for i in range(N_RES)] + ["res%d" % i for i in range(N_RES)]


def gpu_probes(gen, inputs, uv, outputs, rows: List[int], att: bool, reg: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The probe dict of the last forward of ``gen`` (a Generator or, with ``reg``, a GeneratorTSM), rows ``rows`` only, on the CPU."""
    names = GSC_PROBES + (["att%d" % i for i in range(N_RES)] if att else [])
    p = {k: gen.probe(k)[rows].cpu() for k in names}
    p.update(inputs=inputs[rows].cpu(), uv=uv[rows].cpu())
    if reg is not None:
        p.update(reg=reg[rows].cpu())
    p.update({k: t[rows].cpu() for k, t in zip(("gs", "con_rgb", "mask22", "dif"), outputs)})
    return p


def oracle_probes(oracle: GeneratorOracle, inputs, uv, bmask_override: Optional[torch.Tensor] = None, reg=None, frame: int = 0,
                  share: bool = True) -> Dict[str, torch.Tensor]:
    """The same dict from one oracle forward (any dtype): what a GPU forward would hand ``run_gsc_stages`` or, with ``reg`` and
    ``frame`` (a GeneratorTSMOracle), ``run_tsm_full_stages``."""
    pr = {}
    if reg is None:
        gs, con_rgb, mask22, dif = oracle(inputs, uv, probes=pr, bmask_override=bmask_override)
    else:
        gs, con_rgb, mask22, dif = oracle(inputs, uv, reg, frame, share, probes=pr, bmask_override=bmask_override)
    p = {k: pr[k] for k in GSC_PROBES if not k.startswith("y3x")}
    for i in range(N_RES):
        p["y3x%d" % i] = y3x_ref(pr["res_stack/%d/y3" % i], p[BLOCK_IN[i]])
        p["att%d" % i] = pr["res_stack/%d/non_local/att" % i]
    if bmask_override is not None:
        p["bmask"] = bmask_override.to(p["d32"].dtype).reshape(p["d32"].shape)
    p.update(inputs=torch.as_tensor(inputs), uv=torch.as_tensor(uv), gs=gs, con_rgb=con_rgb, mask22=mask22, dif=dif)
    if reg is not None:
        p.update(reg=torch.as_tensor(reg))
    return p
