"""ctypes binding of libbsr_hip.so (C ABI: include/bsr_hip.h).  There is NO CPU fallback: if the
library is missing the import of the HIP path fails loudly."""
from __future__ import annotations

import ctypes
import os
from typing import Optional

from . import build as _build
from .build import LIB_PATH

ABI_VERSION = 8
NUM_CLASSES = 7
CLASS_NAMES = ("conv3x3", "convT3x3", "conv1x1", "attention", "conv7", "glue", "convT3x3_ni2")

_lib: Optional[ctypes.CDLL] = None

c_i, c_v, c_sz, c_s = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
_BS = [c_i, c_i]                                # a size query's (B, S)
_BLOBS = [c_v, c_sz, c_v, c_sz]                 # a weighted term's forward and gradient blobs, each with its bytes

# name -> (restype, argtypes) of every symbol the binding calls; argtypes None leaves a symbol without arguments undeclared
SIGNATURES = {
    "bsr_abi_version": (c_i, None),
    "bsr_last_error": (c_s, None),
    "bsr_source_sha": (c_s, None),
    "bsr_create": (c_i, [ctypes.POINTER(c_v), c_i, c_v, c_sz, c_i]),
    "bsr_destroy": (None, [c_v]),
    "bsr_forward": (c_i, [c_v, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_v]),
    "bsr_forward_packed": (c_i, [c_v, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_forward_tsm": (c_i, [c_v, c_v, c_v, c_v, c_i, c_i, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_v]),
    "bsr_forward_rgb": (c_i, [c_v, c_v, c_v, c_i, c_i, c_i, c_v, c_v]),
    "bsr_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_handle_workspace_bytes": (c_sz, [c_v, c_i, c_i, c_i]),
    "bsr_reserve": (c_i, [c_v, c_i, c_i, c_i]),
    "bsr_probe": (c_i, [c_v, c_s, c_v, c_sz, ctypes.POINTER(c_i * 4), c_v]),
    "bsr_set_timing": (c_i, [c_v, c_i]),
    "bsr_get_timing": (c_i, [c_v, ctypes.POINTER(ctypes.c_float * NUM_CLASSES), ctypes.POINTER(c_i * NUM_CLASSES)]),
    "bsr_timing_launches": (c_i, [c_v]),
    "bsr_timing_entry": (c_i, [c_v, c_i, c_s, c_sz, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(c_i)]),
    "bsr_clock_trace": (c_i, [c_i, c_v, c_i, c_i, c_v, c_v, c_v]),
    "bsr_check_range": (c_i, [c_v, c_v]),
    "bsr_peek_range": (c_i, [c_v]),
    "bsr_debug_attention": (c_i, [c_v, c_v, c_i, c_i, c_v]),
    "bsr_debug_attention_rgb": (c_i, [c_v, c_v, c_i, c_i, c_v]),
    "bsr_debug_attention_dtype": (c_i, [c_v, c_v, c_i, c_i, c_i, c_v]),
    "bsr_debug_attention_qw": (c_i, [c_v, c_v, c_i, c_i, c_i, c_v]),
    "bsr_debug_attention_split": (c_i, [c_v, c_v, c_i, c_i, c_i, c_v]),
    "bsr_debug_attention_kv1": (c_i, [c_v, c_v, c_i, c_i, c_i, c_v]),
    "bsr_debug_split_qkv": (c_i, [c_v, c_v, c_i, c_i, c_v]),
    "bsr_debug_wino_conv": (c_i, [c_v, c_v, c_v, c_v, c_i, c_i, c_i, c_i, c_v]),
    "bsr_debug_wino_filter": (c_i, [c_v, c_v]),
    "bsr_debug_wino_convt": (c_i, [c_v, c_v, c_v, c_v, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_v]),
    "bsr_debug_wino_convt_filter": (c_i, [c_v, c_v, c_i]),
    "bsr_debug_wino_clr": (c_i, [c_v, c_v, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v, c_v, c_i, c_i, c_i, c_i, c_v]),
    "bsr_debug_wino_clr_filter": (c_i, [c_v, c_v, c_v]),
    "bsr_debug_keys_compose": (c_i, [c_v, c_v, c_v, c_v]),
    "bsr_debug_values_compose": (c_i, [c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_prep_rows": (c_i, [c_i, c_v, c_sz, c_sz, c_sz, c_i, c_i, c_v, c_v, c_v]),
    "bsr_prep_groups": (c_i, [c_i, c_v, c_sz, c_sz, c_sz, c_i, c_i, c_i, c_v, c_v, c_v]),
    "bsr_png_unfilter": (c_i, [c_i, c_v, c_sz, c_sz, c_i, c_v]),
    "bsr_png_unfilter_tall": (c_i, [c_i, c_v, c_sz, c_sz, c_i, c_v]),
    "bsr_png_file_bytes": (c_sz, [c_i, c_i]),
    "bsr_png_scratch_bytes": (c_sz, [c_i]),
    "bsr_png_encode": (c_i, [c_i, c_v, c_i, c_i, c_i, c_v, c_sz, c_v, c_v]),
    "bsr_png_encode_figs": (c_i, [c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_i, c_i, c_i, c_v, c_sz, c_v, c_v]),
    "bsr_crop_faces": (c_i, [c_i, c_v, c_sz, c_sz, c_i, c_i, c_v]),
    "bsr_paste_faces": (c_i, [c_i, c_v, c_sz, c_sz, c_i, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_v]),
    "bsr_ucb_post_scratch_bytes": (c_sz, _BS),
    "bsr_ucb_post": (c_i, [c_i, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_ucb_post_rgb_scratch_bytes": (c_sz, _BS),
    "bsr_ucb_post_rgb": (c_i, [c_i, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_ucb_post_tsm_scratch_bytes": (c_sz, _BS),
    "bsr_ucb_post_tsm": (c_i, [c_i, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_sfw_score_scratch_bytes": (c_sz, _BS),
    "bsr_sfw_score": (c_i, [c_i, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_shadow_synth_scratch_bytes": (c_sz, _BS),
    "bsr_shadow_synth": (c_i, [c_i, c_v, c_v, c_v, c_v, c_v, c_sz, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_train_losses_scratch_bytes": (c_sz, _BS),
    "bsr_train_losses": (c_i, [c_i, c_v, c_v, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_train_losses_grad_scratch_bytes": (c_sz, _BS),
    "bsr_train_losses_grad_offset": (c_sz, [c_i, c_i, c_i]),
    "bsr_train_losses_grad": (c_i, [c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_disc_blob_bytes": (c_sz, []),
    "bsr_disc_losses_scratch_bytes": (c_sz, _BS),
    "bsr_disc_act_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_disc_losses": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v]),
    "bsr_disc_dgrad_blob_bytes": (c_sz, []),
    "bsr_disc_grad_scratch_bytes": (c_sz, _BS),
    "bsr_disc_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_disc_gen_grad": (c_i, [c_i] + _BLOBS + [c_v, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_debug_disc_gen_grad": (c_i, [c_i] + _BLOBS + [c_v, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_i, c_v]),
    "bsr_disc_wgrad_blob_bytes": (c_sz, []),
    "bsr_disc_wgrad_scratch_bytes": (c_sz, _BS),
    "bsr_disc_wgrad_floats": (c_sz, []),
    "bsr_disc_wgrad_var_offset": (c_sz, [c_i]),
    "bsr_disc_wgrad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_disc_wgrad": (c_i, [c_i] + _BLOBS + [c_v, c_sz, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_v]),
    "bsr_debug_disc_wgrad": (c_i, [c_i] + _BLOBS + [c_v, c_sz, c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v, c_i, c_v]),
    "bsr_clr_tail_grad_blob_bytes": (c_sz, []),
    "bsr_clr_tail_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_clr_tail_grad_floats": (c_sz, []),
    "bsr_clr_tail_grad_var_offset": (c_sz, [c_i]),
    "bsr_clr_tail_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_clr_tail_grad_partials": (c_i, [c_i, c_i, c_i]),
    "bsr_clr_tail_grad": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v, c_v]),
    "bsr_debug_clr_tail_grad": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v, c_i, c_v]),
    "bsr_last_f": (c_i, [c_v, ctypes.POINTER(c_v), ctypes.POINTER(c_i), ctypes.POINTER(c_i * 4)]),
    "bsr_clr_decoder_grad_blob_bytes": (c_sz, []),
    "bsr_clr_decoder_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_clr_decoder_grad_floats": (c_sz, []),
    "bsr_clr_decoder_grad_var_offset": (c_sz, [c_i]),
    "bsr_clr_decoder_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_clr_decoder_grad_partials": (c_i, [c_i, c_i, c_i, c_i]),
    "bsr_clr_decoder_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_i, c_v, c_v]),
    "bsr_debug_clr_decoder_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_i, c_v, c_i, c_v]),
    "bsr_last_decoder": (c_i, [c_v, ctypes.POINTER(c_v), ctypes.POINTER(c_i), ctypes.POINTER(c_v), ctypes.POINTER(c_v), ctypes.POINTER(c_v),
                               ctypes.POINTER(c_i * 4)]),
    "bsr_last_block5": (c_i, [c_v, ctypes.POINTER(c_v), ctypes.POINTER(c_i), ctypes.POINTER(c_v), ctypes.POINTER(c_v), ctypes.POINTER(c_i),
                              ctypes.POINTER(c_i * 4)]),
    "bsr_nonlocal_grad_blob_bytes": (c_sz, []),
    "bsr_nonlocal_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_nonlocal_grad_floats": (c_sz, []),
    "bsr_nonlocal_grad_var_offset": (c_sz, [c_i]),
    "bsr_nonlocal_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_nonlocal_grad_partials": (c_i, [c_i, c_i, c_i]),
    "bsr_nonlocal_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_v]),
    "bsr_debug_nonlocal_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_i, c_v]),
    "bsr_bottleneck_grad_blob_bytes": (c_sz, []),
    "bsr_bottleneck_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_bottleneck_grad_floats": (c_sz, []),
    "bsr_bottleneck_grad_var_offset": (c_sz, [c_i]),
    "bsr_bottleneck_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_bottleneck_grad_partials": (c_i, [c_i, c_i, c_i]),
    "bsr_bottleneck_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_debug_bottleneck_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v]),
    "bsr_last_block": (c_i, [c_v, c_i, ctypes.POINTER(c_v), ctypes.POINTER(c_i), ctypes.POINTER(c_v), ctypes.POINTER(c_v), ctypes.POINTER(c_i),
                             ctypes.POINTER(c_i * 4)]),
    "bsr_colour_trunk_grad_blob_bytes": (c_sz, []),
    "bsr_colour_trunk_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_colour_trunk_grad_floats": (c_sz, []),
    "bsr_colour_trunk_grad_var_offset": (c_sz, [c_i]),
    "bsr_colour_trunk_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_colour_trunk_grad": (c_i, [c_i, c_v, c_sz] + [c_v, c_i] * 5 + [c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_debug_colour_trunk_grad": (c_i, [c_i, c_v, c_sz] + [c_v, c_i] * 5 + [c_v, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v]),
    "bsr_debug_hole_grad": (c_i, [c_i, c_v, c_i, c_v, c_v, c_i, c_i, c_i, c_v, c_v]),
    "bsr_last_lower_trunk": (c_i, [c_v, ctypes.POINTER(c_v * 7), ctypes.POINTER(c_i * 7), ctypes.POINTER(c_i * 4)]),
    "bsr_lower_trunk_grad_blob_bytes": (c_sz, []),
    "bsr_lower_trunk_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_lower_trunk_grad_floats": (c_sz, []),
    "bsr_lower_trunk_grad_var_offset": (c_sz, [c_i]),
    "bsr_lower_trunk_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_lower_trunk_grad": (c_i, [c_i, c_v, c_sz] + [c_v, c_i] * 7 + [c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_debug_lower_trunk_grad": (c_i, [c_i, c_v, c_sz] + [c_v, c_i] * 7 + [c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v]),
    "bsr_heads_grad_blob_bytes": (c_sz, []),
    "bsr_heads_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "bsr_heads_grad_floats": (c_sz, []),
    "bsr_heads_grad_var_offset": (c_sz, [c_i]),
    "bsr_heads_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_heads_grad_partials": (c_i, [c_i, c_i, c_i]),
    "bsr_heads_grad": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_debug_heads_grad": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_i, c_v]),
    "bsr_last_y": (c_i, [c_v, ctypes.POINTER(c_v), ctypes.POINTER(c_i), ctypes.POINTER(c_i * 4)]),
    "bsr_grey_decoder_grad_blob_bytes": (c_sz, []),
    "bsr_grey_decoder_grad_scratch_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_grey_decoder_grad_floats": (c_sz, []),
    "bsr_grey_decoder_grad_var_offset": (c_sz, [c_i]),
    "bsr_grey_decoder_grad_offset": (c_sz, [c_i, c_i, c_i, c_i]),
    "bsr_grey_decoder_grad_partials": (c_i, [c_i, c_i, c_i, c_i]),
    "bsr_grey_decoder_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_i, c_v, c_v]),
    "bsr_debug_grey_decoder_grad": (c_i, [c_i, c_v, c_sz, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_v, c_i, c_i, c_i, c_v, c_v, c_v, c_v, c_i, c_v, c_i,
                                          c_v]),
    "bsr_last_grey_decoder": (c_i, [c_v] + [ctypes.POINTER(c_v), ctypes.POINTER(c_i)] * 4 + [ctypes.POINTER(c_i * 4)]),
    "bsr_vgg_blob_bytes": (c_sz, []),
    "bsr_vgg_scratch_bytes": (c_sz, _BS),
    "bsr_vgg_act_offset": (c_sz, [c_i, c_i, c_i]),
    "bsr_vgg_per_loss": (c_i, [c_i, c_v, c_sz, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v]),
    "bsr_vgg_dgrad_blob_bytes": (c_sz, []),
    "bsr_vgg_grad_scratch_bytes": (c_sz, _BS),
    "bsr_vgg_grad_offset": (c_sz, [c_i, c_i, c_i]),
    "bsr_vgg_per_loss_grad": (c_i, [c_i] + _BLOBS + [c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_v]),
    "bsr_debug_vgg_per_loss_grad": (c_i, [c_i] + _BLOBS + [c_v, c_v, c_v, c_i, c_i, c_v, c_v, c_v, c_v, c_i, c_v]),
}

# every symbol include/bsr_hip.h declares: all of the above but bsr_debug_attention_kv1 and bsr_last_block5, which tests/test_cabi.py's
# header scan (names without digits) cannot see
EXPORTS = tuple(name for name in SIGNATURES if name not in ("bsr_debug_attention_kv1", "bsr_last_block5"))


def load() -> ctypes.CDLL:
    """Load the in-tree library (after torch, so both share one HIP runtime) and declare signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError("libbsr_hip.so is not built (%s missing): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "— the HIP path has no fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  (loads libamdhip64 first; our DT_NEEDED then resolves to the same runtime)
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    # The binary is bound to its sources: build.py compiles the hash of csrc/* + include/bsr_hip.h into it.  A library built from
    # other sources than this tree holds (the .so is git-ignored and travels as a built artefact) is refused — tests and bench lines
    # can then only ever describe the kernels that are in the tree.
    try:
        lib.bsr_source_sha.restype = ctypes.c_char_p
        built = (lib.bsr_source_sha() or b"").decode()
    except AttributeError:
        built = "<none: built before the hash was embedded>"
    want = _build.source_sha16()
    if built != want:
        raise RuntimeError("libbsr_hip.so is STALE: it was compiled from kernel sources %s, the tree holds %s — rebuild "
                           "(`python -c 'import __graft_entry__ as g; g.build()'`); there is no fallback" % (built, want))
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError("libbsr_hip.so has no %s: rebuild (`python -c 'import __graft_entry__ as g; g.build()'`); there is no "
                               "fallback" % name) from None
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    if lib.bsr_abi_version() != ABI_VERSION:
        raise RuntimeError("libbsr_hip.so ABI %d != binding ABI %d: rebuild" % (lib.bsr_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def source_sha() -> str:
    """The source hash the LOADED library carries (== build.source_sha16(), or load() would have refused it)."""
    return (load().bsr_source_sha() or b"").decode()


class RangeError(RuntimeError):
    """BSR_ERR_RANGE: an activation did not fit fp16 in a forward of a 16-bit-mode handle (include/bsr_hip.h, bsr_check_range)."""


ERR_RANGE = 5


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().bsr_last_error()
        raise (RangeError if rc == ERR_RANGE else RuntimeError)("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))
