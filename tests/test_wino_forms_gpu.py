"""-m gpu: the fp32 forward with res*.conv2 in Winograd form (the default) against the same forward with the direct implicit-GEMM
kernel (BSR_WINO_CONV2=0), GSC and TSM.

The two forms round differently, so they agree to the stage ceiling of tests/test_stage_parity_gpu.py, not to the bit: every y3x<i> and
res<i> probe and every output within 1e-5 of the probe's largest magnitude.  The threshold decisions (bmask, model.py:256) must be the
same, or differ only where d32 is within 2e-5 of the threshold (FLIP_TOL of parity_util.py); the probes behind a differing bmask
(res3..5, the colour outputs) are then compared on the images whose bmask agrees."""
import pytest
import torch

from blindshadowremoval_amd.weights import init_weights

CEILING = 1e-5
FLIP_TOL = 2e-5
THRESHOLD = 0.1


def _rel(a, b) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _pair(cls, w, monkeypatch):
    new = cls(dtype="f32").load_weights(w)
    monkeypatch.setenv("BSR_WINO_CONV2", "0")
    old = cls(dtype="f32").load_weights(w)
    monkeypatch.delenv("BSR_WINO_CONV2")
    return new, old


def _compare(new, old, run, tag):
    a = [t.clone() for t in run(new)]
    pa = {n: new.probe(n).clone() for n in ["y3x%d" % i for i in range(6)] + ["res%d" % i for i in range(6)] + ["bmask", "d32"]}
    b = [t.clone() for t in run(old)]
    pb = {n: old.probe(n).clone() for n in pa}
    differ = (pa["bmask"] != pb["bmask"])
    if differ.any():
        assert float((pb["d32"][differ] - THRESHOLD).abs().max()) < FLIP_TOL, tag
    same = ~differ.flatten(1).any(dim=1)                         # images whose threshold decisions agree
    assert same.any(), tag
    worst = 0.0
    for n in pa:
        if n in ("bmask", "d32"):
            continue
        rows = same if n in ("y3x3", "y3x4", "y3x5", "res3", "res4", "res5") else torch.ones_like(same)
        e = _rel(pa[n][rows], pb[n][rows])
        worst = max(worst, e)
        assert e <= CEILING, (tag, n, e)
    for x, y, name in zip(a, b, ("gs", "con_rgb", "mask22", "dif")):
        rows = torch.ones_like(same) if name in ("gs", "mask22") else same
        e = _rel(x[rows], y[rows])
        worst = max(worst, e)
        assert e <= CEILING, (tag, name, e)
    assert not torch.equal(pa["y3x0"], pb["y3x0"]), "the switch selected the same kernel twice"
    print("wino vs direct %s: worst rel diff %.3e, bmask cells differing %d" % (tag, worst, int(differ.sum())))


@pytest.mark.gpu
def test_gsc_forward_agrees_in_both_forms_and_keeps_its_launch_name(monkeypatch):
    from blindshadowremoval_amd import Generator
    new, old = _pair(Generator, init_weights(1), monkeypatch)
    g = torch.Generator().manual_seed(91)
    for (B, H, W) in ((32, 256, 256), (3, 256, 256), (16, 288, 256), (2, 256, 512)):
        inp, uv = torch.rand(B, H, W, 3, generator=g).cuda(), torch.rand(B, H, W, 3, generator=g).cuda()
        _compare(new, old, lambda gen: gen(inp, uv), "gsc %dx%dx%d" % (B, H, W))
    new.set_timing(True)
    new(inp, uv)
    torch.cuda.synchronize()
    names = [n for n, _, _ in new.get_launch_timing()]
    new.set_timing(False)
    assert all("res%d.conv2" % i in names for i in range(6))
    new.close()
    old.close()


@pytest.mark.gpu
def test_tsm_forward_agrees_in_both_forms(monkeypatch):
    from blindshadowremoval_amd import GeneratorTSM
    new, old = _pair(GeneratorTSM, init_weights(1, variant="tsm"), monkeypatch)
    g = torch.Generator().manual_seed(92)
    inp, uv = torch.rand(4, 256, 256, 3, generator=g).cuda(), torch.rand(4, 256, 256, 3, generator=g).cuda()
    reg = ((torch.rand(4, 256, 256, 6, generator=g) - 0.5) * 0.2).cuda()
    _compare(new, old, lambda gen: gen(inp, uv, reg, 2, True), "tsm 4x256x256")
    new.close()
    old.close()
