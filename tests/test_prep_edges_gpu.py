"""prep_rows_kernel, prep_groups_kernel<6|7>, their shared prep_meshes and prep_blur_kernel (csrc/prep_kernels.h,
csrc/prep_group_kernels.h) held to what their headers promise — float64 in the host's operation order, contraction off: "the same winner,
the same bits" — on the constructed parts of tests/prep_cases.py and on the golden UCB items: every float32 the device writes has the
bits of the numpy statement (statement_rows / statement_groups), NaN where the statement is NaN.  tests/test_prep_cases_cpu.py holds
that statement to matplotlib, resize_linear, gaussian_blur5 and build_row, and shows that float32 arithmetic in the kernel would fail
here on most elements while passing the 1e-6 of tests/test_prep_gpu.py."""
import os

import numpy as np
import pytest

from blindshadowremoval_amd import prep
import prep_cases as C
from tsm_group_cases import ucb_items

pytestmark = pytest.mark.gpu

MESH = C.mesh_cases()
CROP = C.crop_cases()
ROW_CASES = {**{n: (c.part, c.S) for n, c in MESH.items()}, **CROP}
_DP = {}


def _dp(S, planes=None):
    if (S, planes) not in _DP:
        _DP[(S, planes)] = prep.DevicePrep(0, S, planes=planes)
    return _DP[(S, planes)]


def _run(parts, S, planes=None, dp=None):
    import torch
    out, boxes = (dp or _dp(S, planes)).rows(parts)
    torch.cuda.synchronize()
    assert np.array_equal(boxes, np.stack([np.asarray(p.box, np.float32) for p in parts]))
    return out.cpu().numpy()


def _assert_bits(got, want, what):
    n = C.same_bits(got, want)
    if n:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        per_channel = bad.reshape(-1, bad.shape[-1]).sum(0)
        worst = np.nanmax(np.where(bad, np.abs(got.astype(np.float64) - want.astype(np.float64)), 0.0))
        print("%s: %d of %d elements differ from the statement; per channel %s; largest difference %.3e (NaN against a number not counted)"
              % (what, n, got.size, per_channel.tolist(), worst))
    else:
        print("%s: all %d elements have the statement's bits" % (what, got.size))
    assert n == 0, (what, n)


@pytest.mark.parametrize("name", sorted(ROW_CASES))
def test_row_kernel_on_constructed_parts(name):
    part, S = ROW_CASES[name]
    got = _run([part], S)
    assert got.shape == (1, S, S, 16)
    _assert_bits(got, C.statement_rows([part], S), name)


@pytest.mark.parametrize("S", [16, 32, 48, 64])
@pytest.mark.parametrize("name", ["full256", "inset"])
def test_row_kernel_block_mapping_at_every_size(name, S):
    """One block (16), three blocks per row (48: no power of two), and the sizes between."""
    part = MESH[name].part
    _assert_bits(_run([part], S), C.statement_rows([part], S), "%s at S = %d" % (name, S))


def _group_parts():
    return {n: C.as_group(ROW_CASES[n][0]) for n in ("full256", "on_edges_32", "inset", "right_bottom", "n_0")}


@pytest.mark.parametrize("S", [32, 48])
@pytest.mark.parametrize("name", ["full256", "on_edges_32", "inset", "right_bottom", "n_0"])
def test_group_kernel_on_constructed_parts(name, S):
    """The mirror slots carry another, asymmetric mesh: a block box taken for the wrong side of row 1 culls triangles its pixels need."""
    part = _group_parts()[name]
    got = _run([part], S, 6)
    assert got.shape == (1, 2, S, S, 16)
    _assert_bits(got, C.statement_groups([part], S, 6), "%s group at S = %d" % (name, S))
    rows = _run([part._replace(tabs=part.tabs[:4])], S)
    assert C.same_bits(got[0, 0], rows[0]) == 0                                  # row 0: the row kernel's bits
    assert np.array_equal(got[0, 1, :, :, :6].view(np.uint32), got[0, 0, :, ::-1, :6].view(np.uint32))      # row 1's crop planes: row 0's, flipped
    mirror = _run([part._replace(tabs=part.tabs[4:])], S)
    assert C.same_bits(got[0, 1, :, :, 6:], mirror[0, :, :, 6:]) == 0            # row 1's meshes: what the row kernel makes of tables 4..7
    if name == "n_0":
        assert not got[0, :, :, :, :6].any()


@pytest.mark.parametrize("S", [32, 48])
def test_group_kernel_with_a_grey_label_plane(S):
    parts = [C.as_group(CROP[n][0], C.grey_label(*CROP[n][0].img.shape[:2], seed=61 + i)) for i, n in enumerate(("right_bottom", "with_gt"))]
    got = _run(parts, S, 7)
    assert got.shape == (2, 2, S, S, 17)
    want = C.statement_groups(parts, S, 7)
    _assert_bits(got, want, "label groups at S = %d" % S)
    assert got[:, :, :, :, 6].max() > 1.0 and got[:, :, :, :, 6].max() <= 2.0                                # grey levels as they are
    assert np.array_equal(got[:, 1, :, :, :7].view(np.uint32), got[:, 0, :, ::-1, :7].view(np.uint32))


def test_mixed_batch_equals_its_items_alone():
    parts = C.mixed_batch()
    got = _run(parts, 32)
    _assert_bits(got, C.statement_rows(parts, 32), "mixed batch")
    for i, p in enumerate(parts):
        assert np.array_equal(got[i].view(np.uint32), _run([p], 32)[0].view(np.uint32)), p.name


def test_mixed_group_batch_equals_its_items_alone():
    parts = [C.as_group(p) for p in C.mixed_batch()[:7]]
    got = _run(parts, 32, 6)
    _assert_bits(got, C.statement_groups(parts, 32, 6), "mixed group batch")
    for i, p in enumerate(parts):
        assert np.array_equal(got[i].view(np.uint32), _run([p], 32, 6)[0].view(np.uint32)), p.name


def test_a_reused_object_gives_the_same_bits():
    """Both staging buffers of one DevicePrep, and the first one again: a later batch with other items around the shared ones."""
    dp = prep.DevicePrep(0, 32)
    parts = C.mixed_batch()
    first = _run(parts, 32, dp=dp)
    second = _run([CROP["up_9"][0]] + parts[::-1][:5] + [MESH["border_hull"].part], 32, dp=dp)
    third = _run(parts[3:] + parts[:2], 32, dp=dp)
    for j, i in enumerate(range(len(parts) - 1, len(parts) - 6, -1)):
        assert np.array_equal(second[1 + j].view(np.uint32), first[i].view(np.uint32)), i
    for j, i in enumerate(list(range(3, len(parts))) + [0, 1]):
        assert np.array_equal(third[j].view(np.uint32), first[i].view(np.uint32)), i
    _assert_bits(second[[0, -1]], C.statement_rows([CROP["up_9"][0], MESH["border_hull"].part], 32), "second call's own items")


@pytest.mark.parametrize("k", range(25))
def test_device_rows_have_the_statement_bits_on_the_golden_items(k):
    """The 25 UCB items of tests/test_prep_gpu.py::test_device_rows_match_the_reference_fixture_and_the_host_path (every fourth of
    the 100): the bit-level check on real faces that the 1e-6 comparisons cannot give."""
    lm, gt = ucb_items()[4 * k]
    part = prep.host_part((lm, gt, 256))
    _assert_bits(_run([part], 256), C.statement_rows([part], 256), os.path.basename(lm))


@pytest.mark.parametrize("k", range(4))
def test_device_groups_have_the_statement_bits_on_golden_items(k):
    lm, gt = ucb_items()[11 + 25 * k]
    part = prep.host_part_group((lm, gt, 256))
    _assert_bits(_run([part], 256, 6), C.statement_groups([part], 256, 6), os.path.basename(lm) + " group")
