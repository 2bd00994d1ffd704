"""-m gpu: the three attention kernels alone (csrc/attention.h through bsr_debug_attention_qw, csrc/attention_h16.h through
bsr_debug_split_qkv + bsr_debug_attention_split, csrc/attention256.h through bsr_debug_attention_rgb) against fp64
softmax(theta phi^T) g on the constructed cases of tests/attention_cases.py, over token counts from one loop trip up.

Budget of a (kernel, case): 3 x the error of the kernel's arithmetic emulated in float32 on the CPU (tools/attention_error.py; table in
attention_cases.EMULATED), by the per-query metric of attention_cases.py; one_hot on the fp32 kernels: 1e-6.  Every launch writes into
a NaN-filled buffer with one extra block of T rows behind it: the real rows must come out finite, the extra block untouched.

Each test prints a line per (kernel, case, T, B) — profiles/attention_edges_gpu.txt holds them as measured on an MI355X beside the
emulated column.  Measured there: every error inside its budget (closest: h16 staircase_under at T = 1152, 7.3e-6 of 1.5e-5); the spike cases
bit-exact on the fp32 kernels (their emulated error, hence their budget, is 0); all four fp32 workgroup shapes and repeated runs
bit-identical on every case; the one_hot rows equal to the bits of g[perm] except the one element per image where g is 0."""
import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu

ERR_ARG = 1


def _lib():
    from blindshadowremoval_amd import _lib as L
    return L, L.load()


def _note(line: str) -> None:
    """One line per (kernel, case, T, B) on the test's output (run with -s to keep them: tools/attention_error.py --merge reads that log)."""
    print(line)


def _sync() -> None:
    """A device error ends the session: nothing more is launched on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def _guarded(B: int, T: int, D: int) -> torch.Tensor:
    """The output buffer: B images and one extra block of T rows, all NaN."""
    return torch.full((B + 1, T, D), float("nan"), device="cuda")


def _check_guard(buf: torch.Tensor, B: int, what) -> torch.Tensor:
    bad = (~torch.isfinite(buf[:B])).any(dim=2).nonzero()
    assert bad.numel() == 0, ("rows left unwritten or not finite (image, query)", what, bad[:8].tolist())
    assert bool(torch.isnan(buf[B]).all()), ("rows behind the output were written", what)
    return buf[:B]


def _run_f32(x: torch.Tensor, qw: int) -> torch.Tensor:
    L, lib = _lib()
    B, T, _ = x.shape
    buf = _guarded(B, T, 128)
    L.check(lib.bsr_debug_attention_qw(x.data_ptr(), buf.data_ptr(), B, T, qw, None), "bsr_debug_attention_qw")
    _sync()
    return _check_guard(buf, B, ("f32", qw, B, T))


def _split(x: torch.Tensor) -> torch.Tensor:
    L, lib = _lib()
    B, T, _ = x.shape
    xs = torch.empty_like(x)                                    # the split layout has the size of the fp32 one
    L.check(lib.bsr_debug_split_qkv(x.data_ptr(), xs.data_ptr(), B, T, None), "bsr_debug_split_qkv")
    return xs


def _run_h16(xs: torch.Tensor, pv1: int) -> torch.Tensor:
    L, lib = _lib()
    B, T, _ = xs.shape
    buf = _guarded(B, T, 128)
    L.check(lib.bsr_debug_attention_split(xs.data_ptr(), buf.data_ptr(), B, T, pv1, None), "bsr_debug_attention_split")
    _sync()
    return _check_guard(buf, B, ("h16", pv1, B, T))


def _run_d256(x: torch.Tensor) -> torch.Tensor:
    L, lib = _lib()
    B, T, _ = x.shape
    buf = _guarded(B, T, 256)
    L.check(lib.bsr_debug_attention_rgb(x.data_ptr(), buf.data_ptr(), B, T, None), "bsr_debug_attention_rgb")
    _sync()
    return _check_guard(buf, B, ("d256", B, T))


def _hold(kernel: str, case: str, B: int, T: int, got: torch.Tensor, ref, scale, extra: str = "") -> float:
    err, img, q = ac.case_error(got.cpu(), ref, scale)
    bud = ac.budget(kernel, case)
    _note("%-8s %-17s T %5d  B %2d  err %.3e  budget %.3e  at (image %d, query %d)%s" % (kernel, case, T, B, err, bud, img, q, extra))
    assert err <= bud, (kernel, case, B, T, err, bud, img, q)
    return err


def _one_hot_bits(got: torch.Tensor, B: int, T: int, D: int) -> str:
    """Whether the one_hot rows came back as the bits of g[perm]; if not, how many elements differ and by how much."""
    want = torch.stack([ac.one_hot_expected(T, D, b) for b in range(B)])
    diff = got.cpu() != want
    if not bool(diff.any()):
        return "  one_hot rows bit-equal to g[perm]: True"
    return "  one_hot rows bit-equal to g[perm]: False (%d of %d elements, max |diff| %.1e)" % (int(diff.sum()), diff.numel(), float((got.cpu() - want).abs().max()))


F32_PLAN = [(c, ac.B_128, T) for T in ac.T_128 for c in ac.CASES] + [(c, 1, ac.T_128_BIG) for c in ac.BIG_CASES]


@pytest.mark.parametrize("case,B,T", F32_PLAN)
def test_fp32_kernel_every_workgroup_shape(case, B, T):
    """Within budget; qw = 4 / 2 / 1 and the automatic choice give the same bits on every case, and so do two runs."""
    qkv, ref, scale = ac.reference(case, B, T, 128)
    x = qkv.cuda()
    got = _run_f32(x, 4)
    same = all(torch.equal(_run_f32(x, qw), got) for qw in (2, 1, 0))
    again = torch.equal(_run_f32(x, 4), got)
    extra = "  qw 4/2/1/0 bit-identical: %s  rerun: %s" % (same, again)
    if case == "one_hot":
        extra += _one_hot_bits(got, B, T, 128)
    _hold("f32", case, B, T, got, ref, scale, extra)
    assert same and again, (case, B, T, same, again)


MAP_PLAN = [(128, 8), (128, 16), (128, 3), (256, 8)]      # XCD-congruent one round / two rounds, linear, XCD-congruent with two query blocks


@pytest.mark.parametrize("T,B", MAP_PLAN)
@pytest.mark.parametrize("case", ["one_hot", "benign"])
def test_workgroup_to_image_and_query_block_map(case, T, B):
    """Both branches of the map nblk % (8 qblocks), in the fp32 kernel at qw = 4 and in the h16 kernel's own copy: every image compared."""
    qkv, ref, scale = ac.reference(case, B, T, 128)
    x = qkv.cuda()
    _hold("f32", case, B, T, _run_f32(x, 4), ref, scale, "  map")
    xs = _split(x)
    _hold("h16", case, B, T, _run_h16(xs, 0), ref, scale, "  map")
    _hold("h16_pv1", case, B, T, _run_h16(xs, 1), ref, scale, "  map")


@pytest.mark.parametrize("case,B,T", F32_PLAN)
def test_h16_kernel_both_pv_forms(case, B, T):
    """pv1 = 0 (three products) and pv1 = 1 (hi planes only in P.V: the f16 mode's form), each within its own budget; on benign the
    switch must select the other kernel: pv1 = 1 is measurably the less accurate."""
    qkv, ref, scale = ac.reference(case, B, T, 128)
    xs = _split(qkv.cuda())
    got0, got1 = _run_h16(xs, 0), _run_h16(xs, 1)
    assert torch.equal(_run_h16(xs, 0), got0) and torch.equal(_run_h16(xs, 1), got1), (case, B, T)
    e0 = _hold("h16", case, B, T, got0, ref, scale, _one_hot_bits(got0, B, T, 128) if case == "one_hot" else "")
    e1 = _hold("h16_pv1", case, B, T, got1, ref, scale)
    if case == "benign":
        assert e1 > e0, (B, T, e0, e1)


@pytest.mark.parametrize("case,T", [(c, T) for T in ac.T_256 for c in ac.CASES])
def test_d256_kernel(case, T):
    B = ac.B_256
    qkv, ref, scale = ac.reference(case, B, T, 256)
    x = qkv.cuda()
    got = _run_d256(x)
    again = torch.equal(_run_d256(x), got)
    _hold("d256", case, B, T, got, ref, scale, "  rerun: %s" % again + (_one_hot_bits(got, B, T, 256) if case == "one_hot" else ""))
    assert again


def test_bad_token_counts_batches_and_pointers_are_refused_before_any_launch():
    """tokens 0 / 64 / 192 (not a multiple of 128), B = 0 and null pointers: non-zero with a message, the output untouched."""
    L, lib = _lib()
    x = torch.zeros(2, 256, 384, device="cuda")
    y = torch.full((2, 256, 128), float("nan"), device="cuda")
    xp, yp = x.data_ptr(), y.data_ptr()
    entries = {
        "bsr_debug_attention_qw": lambda a, b, B, T: lib.bsr_debug_attention_qw(a, b, B, T, 4, None),
        "bsr_debug_attention": lambda a, b, B, T: lib.bsr_debug_attention_dtype(a, b, B, T, 0, None),
        "bsr_debug_split_qkv": lambda a, b, B, T: lib.bsr_debug_split_qkv(a, b, B, T, None),
        "bsr_debug_attention_split": lambda a, b, B, T: lib.bsr_debug_attention_split(a, b, B, T, 0, None),
    }
    for name, call in entries.items():
        for B, T in ((1, 0), (1, 64), (2, 64), (1, 192), (0, 128), (0, 0), (-1, 128)):
            assert call(xp, yp, B, T) == ERR_ARG, (name, B, T)
            assert name.encode() in lib.bsr_last_error() and b"multiple of 128" in lib.bsr_last_error(), (name, B, T)
        for a, b in ((None, yp), (xp, None), (None, None)):
            assert call(a, b, 1, 128) == ERR_ARG, (name, a, b)
            assert name.encode() in lib.bsr_last_error() and b"null" in lib.bsr_last_error(), name
    assert lib.bsr_debug_attention_split(xp, yp, 1, 64, 1, None) == ERR_ARG
    for B, T in ((1, 0), (0, 32), (1, 48)):
        assert lib.bsr_debug_attention_rgb(xp, yp, B, T, None) == ERR_ARG and b"bsr_debug_attention_rgb" in lib.bsr_last_error()
    assert lib.bsr_debug_attention_rgb(None, yp, 1, 32, None) == ERR_ARG and lib.bsr_debug_attention_rgb(xp, None, 1, 32, None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and float(x.abs().max()) == 0.0


@pytest.mark.parametrize("H,W", [(32, 256), (288, 256)])
@pytest.mark.parametrize("dtype", ["f32x3", "f16"])
def test_fused_attention_w_tail_agrees_with_the_two_launch_form_at_other_maps(dtype, H, W, monkeypatch):
    """The comparison of test_gpu_parity.py's test_fused_attention_w_tail_agrees_with_the_two_launch_form_in_the_16_bit_modes, with its
    criterion unchanged, at B = 2 and T = 128 (32x256: the tail's weight-tile requests occupy every iteration of the key loop — only the
    four peeled ones run) and T = 1152 (288x256)."""
    from blindshadowremoval_amd import Generator
    from blindshadowremoval_amd.weights import init_weights
    from test_gpu_parity import F16_TOL
    w = init_weights(1)
    fused = Generator(dtype=dtype).load_weights(w)
    monkeypatch.setenv("BSR_FUSE_ATTW", "0")
    plain = Generator(dtype=dtype).load_weights(w)
    monkeypatch.delenv("BSR_FUSE_ATTW")
    g = torch.Generator().manual_seed(73 + H)

    def close(x, y, tol):
        return float((x.double() - y.double()).abs().max()) <= tol
    tol_blk, tol_blk2, tol_out = (2e-5, 5e-5, 1e-4) if dtype == "f32x3" else (5e-4, 1e-3, F16_TOL)

    B = 2
    inp, uv = torch.rand(B, H, W, 3, generator=g).cuda(), torch.rand(B, H, W, 3, generator=g).cuda()
    fused.set_timing(True)
    a = [t.clone() for t in fused(inp, uv)]
    torch.cuda.synchronize()
    names = [n for n, _, _ in fused.get_launch_timing()]
    fused.set_timing(False)
    assert "res0.attw" in names and "res5.attw" in names and "res0.w" not in names and "res0.attention" not in names, (B, H, W)
    fa = {pr: fused.probe(pr).clone() for pr in ("res0", "res2", "res3", "res5", "bmask")}
    plain.set_timing(True)
    b = plain(inp, uv)
    torch.cuda.synchronize()
    names_p = [n for n, _, _ in plain.get_launch_timing()]
    plain.set_timing(False)
    assert "res0.attention" in names_p and "res0.w" in names_p and "res0.attw" not in names_p
    fused.check_range()
    for pr in ("res0", "res2"):
        assert close(fa[pr], plain.probe(pr), tol_blk), (dtype, B, H, W, pr, float((fa[pr] - plain.probe(pr)).abs().max()))
    if torch.equal(fa["bmask"], plain.probe("bmask")):
        for pr in ("res3", "res5"):
            assert close(fa[pr], plain.probe(pr), tol_blk2), (dtype, B, H, W, pr, float((fa[pr] - plain.probe(pr)).abs().max()))
        for x, y, name in zip(a, b, ("gs", "con_rgb", "mask22", "dif")):
            assert close(x, y, tol_out), (dtype, B, H, W, name, float((x - y).abs().max()))
    with pytest.raises(RuntimeError, match="never left LDS"):
        fused.probe("att0")
    assert plain.probe("att0").shape == (B, H // 8, W // 8, 128)
    fused.close()
    plain.close()
