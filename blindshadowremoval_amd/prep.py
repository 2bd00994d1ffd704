"""Device-side input preparation (round 3): the reference's per-sample loader work — `parse_fn_test_FFHQ` / `parse_fn_test`
(/root/reference/dataset.py:619-638, 148-170) — split so that only what is tiny and irregular stays on the host.

host (`host_part`, runs in the loader's worker processes): PNG decode, `face_crop_and_resize`'s crop box and landmark
    normalisation (utils.py:366-433, the float32 / float64 dtype flow of dataset.face_crop_and_resize), the Delaunay
    triangulations (matplotlib.tri.Triangulation = qhull, exactly the reference's call, <= 101 points each) and
    `Triangulation.calculate_plane_coefficients` — the numbers LinearTriInterpolator evaluates;
device (`device_rows` -> bsr_prep_rows, csrc/prep_kernels.h): the bilinear crop-resize of image + ground truth, the seven
    interpolated channels (uv map, reg_in, reg_out), the face-hull mask and its 5x5 Gaussian, all in float64 in the reference's
    operation order, written as the packed `[B,S,S,16]` float32 tensor directly in HBM.

Pinned by the same fixtures as the host path (tests/test_prep_gpu.py: tests/golden/sample_02165.npz — made by the reference's OWN
functions — and the host `build_row` on the UCB items, 1e-6)."""
from __future__ import annotations

import os
from typing import Any, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import dataset as D


# What the loaders' workers send to the loop's thread, one record per item.  Plain NamedTuples at module level: the workers import this
# module without torch and pickle the records; the field order is the order the tuples always had.
class HostPart(NamedTuple):
    """The host half of one row (host_part) or of one TSM group (host_part_group: eight tables), the bytes travelling with it."""
    img: Any                          # uint8 [h,w,3], or pngio.RawScanlines (inflated, still filtered)
    gt: Any                           # like img | None (an SFW group: the cmap)
    box: np.ndarray                   # int32 [4]
    tabs: list                        # 4 | 8 triangle tables, float64 [ntri, TRI_DOUBLES]
    name: bytes
    masks: Optional[tuple] = None     # pack_masks' (kind, data, S)
    label: Optional[np.ndarray] = None          # the SFW label plane, uint8 [h,w]


class CropGeometry(NamedTuple):
    """wild_crop.crop_geometry's crop of a photograph."""
    box: np.ndarray                   # int32 [4]
    preset_x: int
    preset_y: int


class UncroppedPart(NamedTuple):
    """The host half of one uncropped photograph (host_part_uncropped)."""
    img: Any
    gt: None                          # kept for the field order HostPart has
    box: np.ndarray                   # of the row, in the crop's coordinates
    tabs: list
    name: bytes
    crop: CropGeometry


class RingMasks(NamedTuple):
    """Where the seven masks of a ring item lie in its slot."""
    kind: str                         # "bits" | "u8" | "raw8"
    S: int
    off: int
    nbytes: int


class RingPart(NamedTuple):
    """An item whose bytes lie in a slot of the loaders' ring (host_part_ring)."""
    tag: str                          # "ring", kept for the field order
    slot: int
    hw: Tuple[int, int]
    has_gt: bool
    img_offs: Tuple[int, ...]         # the image's offset in the slot, then the ground truth's
    tab_offs: Tuple[int, ...]
    ntri: Tuple[int, ...]
    box: np.ndarray
    name: bytes
    masks: Optional[RingMasks]
    used: int                         # bytes of the slot
    rawc: Tuple[int, ...]             # per image: channels per filtered pixel, 0 = decoded RGB

    def __reduce_ex__(self, protocol):
        # one record per item crosses the workers' pipes and is loaded on the loop's own thread.  Its own pickle would go through a
        # NamedTuple's Python-level __new__ (once more for the nested RingMasks) and numpy's for the four ints of the box, which alone
        # is half the time of the whole record: the fields travel as one list of plain values instead.  The box is int32 [4] by
        # construction (host_part_ring) and comes back as that; _ring_part fills the list it is given, always pickle's own fresh one
        f = list(self)
        f[_RING_BOX], f[_RING_MASKS] = np.asarray(self.box).tolist(), self.masks and tuple(self.masks)
        return _ring_part, (f,)


_RING_BOX, _RING_MASKS = RingPart._fields.index("box"), RingPart._fields.index("masks")


def _ring_part(f: list) -> RingPart:
    """A RingPart back from its pickle."""
    f[_RING_BOX], f[_RING_MASKS] = np.array(f[_RING_BOX], np.int32), f[_RING_MASKS] and tuple.__new__(RingMasks, f[_RING_MASKS])
    return tuple.__new__(RingPart, f)


class UnfilterTable(NamedTuple):
    """The unfilter records of a blob: their offset, their number, and per item with "raw8" masks (output offset, S)."""
    off: int
    n: int
    mask_out: dict


class BlobLayout(NamedTuple):
    """_layout_ex's result."""
    total: int
    rows_off: int
    grid_off: int
    pieces: list                      # [(offset, array)]: what pack_into copies
    head: int                         # bytes staged on the host; behind them the ring cells and the device-only areas
    cells: list                       # [(part index, slot, cell offset)]
    unf: UnfilterTable


class UncroppedLayout(NamedTuple):
    """_layout_uncropped's result."""
    total: int
    head: int
    rows_off: int
    grid_off: int
    crop_off: int
    tall_off: int
    n_tall: int
    pieces: list
    paste_off: Optional[int]          # keep_photo: the batch's PASTE_DTYPE records
    photo_offs: Optional[List[int]]   # keep_photo: per item its reconstructed photograph


class _Cursor:
    """Hands out consecutive 8-byte aligned areas of a blob."""

    def __init__(self):
        self.off = 0

    def take(self, nbytes: int) -> int:
        o = self.off
        self.off += (int(nbytes) + 7) & ~7
        return o


TRI_DOUBLES = 18          # csrc/prep_kernels.h kPrepTriDoubles
MAX_TRI = 256
ROW_DTYPE = np.dtype([("img_off", "<i8"), ("gt_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("box", "<i4", (4,)),
                      ("tri_off", "<i8", (4,)), ("ntri", "<i4", (4,))], align=True)
assert ROW_DTYPE.itemsize == 88
# a TSM loader's group of two rows (csrc/prep_group_kernels.h PrepGroup): two RGB8 images, one grey8 plane (the SFW label; unread with
# six planes), the box, the four meshes of the item's landmarks and the four of the mirror landmarks
GROUP_DTYPE = np.dtype([("img_off", "<i8"), ("gt_off", "<i8"), ("aux_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("box", "<i4", (4,)),
                        ("tri_off", "<i8", (8,)), ("ntri", "<i4", (8,))], align=True)
assert GROUP_DTYPE.itemsize == 144


def _imread_u8(path: str) -> np.ndarray:
    from .pngio import read_rgb_u8            # round 5: plain 8-bit PNG files bypass PIL's decoder (4x faster; pngio.read_rgb_u8)
    return read_rgb_u8(path)


def _imread_raw(path: str):
    from .pngio import read_rgb_raw           # round 6: the worker stops after the inflate, the scanlines are reconstructed on the device
    return read_rgb_raw(path)


UNFILTER_DTYPE = np.dtype([("raw_off", "<i8"), ("out_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("c", "<i4"), ("grey_out", "<i4")], align=True)
assert UNFILTER_DTYPE.itemsize == 32          # csrc/prep_kernels.h UnfilterItem
UNFILTER_MAX_ROWS = 256                       # csrc/prep_kernels.h kUnfilterMaxRows: one workgroup, one thread per row


# in-the-wild photographs (csrc/wild_crop_kernels.h): the tall reconstruction's record (UNFILTER_DTYPE + rows_needed) and the crop's
UNFILTER_TALL_DTYPE = np.dtype([("raw_off", "<i8"), ("out_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("c", "<i4"), ("grey_out", "<i4"),
                                ("rows_needed", "<i4"), ("pad", "<i4")], align=True)
assert UNFILTER_TALL_DTYPE.itemsize == 40     # UnfilterTallItem
CROP_DTYPE = np.dtype([("src_off", "<i8"), ("out_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("box", "<i4", (4,)), ("preset_x", "<i4"),
                       ("preset_y", "<i4")], align=True)
assert CROP_DTYPE.itemsize == 48              # CropItem
# the way back (csrc/wild_paste_kernels.h): the photograph to rewrite in place, the crop's geometry, the item's row of im / con / face
PASTE_DTYPE = np.dtype([("photo_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("box", "<i4", (4,)), ("preset_x", "<i4"), ("preset_y", "<i4"),
                        ("row", "<i4"), ("pad", "<i4")], align=True)
assert PASTE_DTYPE.itemsize == 48             # PasteItem
UNFILTER_SLACK = 16                           # csrc/prep_kernels.h kUnfilterSlack: readable bytes around filtered scanlines


def _tri_table(tri, zs: Sequence[np.ndarray]) -> np.ndarray:
    """[ntri, 18] float64: three edge functions (normalised barycentrics l_i = A_i x + B_i y + C_i) + up to three channels of
    plane coefficients (a, b, c), the latter from matplotlib's own `calculate_plane_coefficients` (what LinearTriInterpolator uses)."""
    t = tri.triangles
    x, y = np.asarray(tri.x, np.float64), np.asarray(tri.y, np.float64)
    x0, y0, x1, y1, x2, y2 = x[t[:, 0]], y[t[:, 0]], x[t[:, 1]], y[t[:, 1]], x[t[:, 2]], y[t[:, 2]]
    d = (y1 - y2) * (x0 - x2) + (x2 - x1) * (y0 - y2)
    a0, b0 = (y1 - y2) / d, (x2 - x1) / d
    a1, b1 = (y2 - y0) / d, (x0 - x2) / d
    c0, c1 = -(a0 * x2 + b0 * y2), -(a1 * x2 + b1 * y2)
    out = np.zeros((t.shape[0], TRI_DOUBLES), np.float64)
    out[:, 0:9] = np.stack([a0, b0, c0, a1, b1, c1, -(a0 + a1), -(b0 + b1), 1.0 - c0 - c1], axis=1)
    for k, z in enumerate(zs):
        out[:, 9 + 3 * k:12 + 3 * k] = tri.calculate_plane_coefficients(np.asarray(z, np.float64))
    if t.shape[0] > MAX_TRI:
        raise ValueError("a mesh has %d triangles (> %d)" % (t.shape[0], MAX_TRI))
    return out


_REF_TRI: dict = {}      # the Delaunay mesh of the canonical landmarks (one per process: matplotlib / qhull take ~0.4 ms to rebuild it per item)


def meshes(lm: np.ndarray) -> List[np.ndarray]:
    """The four triangle tables of one set of normalised landmarks, with the reference's vertex sets and dtype flow
    (dataset.generate_uv_map / generate_offset_map / generate_face_region = warp.py:194-232, utils.py:255-276)."""
    import matplotlib.tri as mtri
    uv, lm_ref = D._face_model()
    tabs = [_tri_table(mtri.Triangulation(lm[:, 0], lm[:, 1]), [uv[:, 1], uv[:, 0], uv[:, 2]])]          # stacked [y, x, z] (warp.py:228-230)
    for k, (source, target) in enumerate(((lm, lm_ref), (lm_ref, lm))):                                   # reg_in, reg_out
        s = np.concatenate([source, D._ANCHORS], axis=0).astype(np.float32)
        t = np.concatenate([target, D._ANCHORS], axis=0).astype(np.float32)
        off = s - t
        if k == 0:          # reg_in triangulates the TARGET points = the canonical landmarks + anchors: the same mesh for every item
            tri = _REF_TRI.get("t")
            if tri is None or not np.array_equal(_REF_TRI["pts"], t):
                tri = mtri.Triangulation(t[:, 0], t[:, 1])
                _REF_TRI["t"], _REF_TRI["pts"] = tri, t.copy()
        else:
            tri = mtri.Triangulation(t[:, 0], t[:, 1])
        tabs.append(_tri_table(tri, [off[:, 1], off[:, 0]]))                                              # [my, mx] (warp.py:210-213)
    more = np.copy(lm[0:17, :])
    more[:, 1] = more[0, 1] - (more[:, 1] - more[0, 1]) * 0.8
    src = np.concatenate([lm, more], axis=0)
    tabs.append(_tri_table(mtri.Triangulation(src[:, 0], src[:, 1]), [src[:, 0]]))                         # hull: interpolated x > 0
    return tabs


def crop_box(lm0: np.ndarray) -> Tuple[List[int], np.ndarray]:
    """Crop box and normalised landmarks of dataset.face_crop_and_resize (aug=False), without touching pixels."""
    lm = np.array(lm0, np.float32)
    two = np.float32(2)
    center = [(lm[:, 0].min() + lm[:, 0].max()) / two, (lm[:, 1].min() + lm[:, 1].max()) / two]
    length = float(max((lm[:, 0].max() - lm[:, 0].min()) / two, (lm[:, 1].max() - lm[:, 1].min()) / two)) * 1.4
    box = [int(center[0]) - int(length), int(center[1]) - int(length * 1.2),
           int(center[0]) + int(length), int(center[1]) + int(length) + int(length) - int(length * 1.2)]
    lm[:, 0] = lm[:, 0] - np.float32(box[0])
    lm[:, 1] = lm[:, 1] - np.float32(box[1])
    return box, lm / np.float32(length * 2)


def crop_box_pair(lm0: np.ndarray, w: int) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """Crop box, normalised landmarks and normalised MIRROR landmarks of dataset.face_crop_and_resize(with_mirror=True) for an image
    `w` pixels wide, without touching pixels: the same float32 statements in the same order."""
    raw = np.array(lm0, np.float32)
    box, lm = crop_box(raw)
    lm_m = np.array(raw, np.float32)
    lm_m[:, 0] = np.float32(w) - lm_m[:, 0]
    lm_m = lm_m[D.LM_REVERSE, :]
    lm_m[:, 0] = lm_m[:, 0] - np.float32(w - box[2])
    lm_m[:, 1] = lm_m[:, 1] - np.float32(box[1])
    return box, lm, lm_m / np.float32(_box_length(raw) * 2)


def _box_length(lm: np.ndarray) -> float:
    """face_crop_and_resize's half-length of the crop (float64 after the `* 1.4`)."""
    two = np.float32(2)
    return float(max((lm[:, 0].max() - lm[:, 0].min()) / two, (lm[:, 1].max() - lm[:, 1].min()) / two)) * 1.4


MASK_ORDER = ("face_hair", "face", "mouth", "nose", "eyebrow", "eye", "glasses")      # train_test_GSC.py:386-392 (= the keys of ucb_post.MASK_DIRS)


def read_masks_u8(paths) -> np.ndarray:
    """The seven mask images of one item as grey levels, [7,S,S] uint8 in MASK_ORDER: cv2.imread(...) of the reference (:386-393) returns
    three equal channels of exactly these values; the / 255.0 happens on the device.  (Lives here, not in ucb_post_gpu: the loaders'
    worker processes call it and must not pay for an `import torch`.)"""
    from .pngio import read_grey_u8
    return np.stack([read_grey_u8(paths[k]) for k in MASK_ORDER], axis=0)


def _masks_raw(paths):
    """("raw8", the seven masks' inflated, still filtered scanlines back to back, S) when every mask is a plain 8-bit grey S x S PNG
    the device kernel takes (bsr_png_unfilter, grey output), else None: the worker then neither reconstructs, compares nor packs."""
    from . import pngio
    raws, S = [], None
    try:
        pngio._host_lib()
        for k in MASK_ORDER:
            with open(paths[k], "rb") as f:
                w, h, c, raw = pngio._parse_8bit(f.read())
            if c != 1 or w != h or h > UNFILTER_MAX_ROWS or w < 4 or (S is not None and h != S):
                return None
            if raw[::1 + w].max() > 4:             # an undefined filter type: the host readers refuse the file (PIL raises), so does this path
                return None
            S = h
            raws.append(raw)
    except (ValueError, TypeError, KeyError, OSError, __import__("struct").error, __import__("zlib").error):
        return None
    return ("raw8", np.concatenate(raws), S)


def masks_from_raw(packed: tuple) -> tuple:
    """A "raw8" record decoded on the host into the form pack_masks gives without `raw` (an item that went through the pipe after all)."""
    from .pngio import unfilter_host
    _, raw, S = packed
    n = S * (1 + S)
    return _pack_levels(np.stack([unfilter_host(raw[i * n:(i + 1) * n], S, S, 1)[:, :, 0] for i in range(7)], axis=0))


def pack_masks(paths, raw: bool = False) -> tuple:
    """The seven UCB segmentation masks of one item (dict in MASK_ORDER -> path) as grey levels, for the device post-processing
    (ucb_post_gpu): ("bits", [7, S*S/8] uint8) when every level is 0 or 255 — what the reference's masks are; an eighth of the bytes
    through the worker's pipe — else ("u8", [7,S,S] uint8).  raw = True (the ring path with the reconstruction on the device, round 6):
    ("raw8", ...) of _masks_raw where the files allow it."""
    if raw:
        r = _masks_raw(paths)
        if r is not None:
            return r
    m = read_masks_u8(paths)
    return _pack_levels(m)


def _pack_levels(m: np.ndarray) -> tuple:
    if m.shape[1] * m.shape[2] % 8 == 0 and bool(np.all((m == 0) | (m == 255))):
        return ("bits", np.packbits((m != 0).reshape(7, -1), axis=1), m.shape[1])
    return ("u8", m, m.shape[1])


def unpack_masks(packed: Sequence[tuple], device):
    """[pack_masks(...)] of a batch -> uint8 [B,7,S,S] grey levels on `device` (bit-packed items are expanded there)."""
    import torch
    S = packed[0][2]
    if any(p[0].startswith("dev_") for p in packed):           # ring items: the bytes are already in HBM (views of the batch's blob)
        shifts = torch.arange(7, -1, -1, device=device, dtype=torch.uint8)

        def full(p):
            t = p[1] if p[0].startswith("dev_") else torch.from_numpy(p[1]).to(device, non_blocking=True)
            return (((t[..., None] >> shifts) & 1) * 255).to(torch.uint8).reshape(7, S, S) if p[0].endswith("bits") else t.reshape(7, S, S)
        if all(p[0] == "dev_bits" for p in packed):
            return (((torch.stack([p[1] for p in packed], dim=0)[..., None] >> shifts) & 1) * 255).to(torch.uint8).reshape(len(packed), 7, S, S)
        return torch.stack([full(p) for p in packed], dim=0)
    if all(p[0] == "bits" for p in packed):
        bits = torch.from_numpy(np.stack([p[1] for p in packed], axis=0)).to(device, non_blocking=True)          # [B,7,S*S/8]
        shifts = torch.arange(7, -1, -1, device=bits.device, dtype=torch.uint8)
        return (((bits[..., None] >> shifts) & 1) * 255).to(torch.uint8).reshape(len(packed), 7, S, S)
    full = [np.unpackbits(p[1], axis=1).reshape(7, S, S) * np.uint8(255) if p[0] == "bits" else p[1] for p in packed]
    return torch.from_numpy(np.stack(full, axis=0)).to(device, non_blocking=True)


def _read_item(job, raw: bool):
    """The head host_part and host_part_group share: (lm_path, gt_path, size[, mask paths]) -> (lm_path, img, gt | None, name, packed
    masks | None), the mask paths split off the job, image and ground truth read by the raw or the decoding reader and of one size; the
    name is the ground truth's path or, without one, the image's."""
    masks = pack_masks(job[3], raw=raw) if len(job) > 3 else None
    lm_path, gt_path, _ = job[:3]
    img_path = os.path.splitext(lm_path)[0] + ".png"
    read = _imread_raw if raw else _imread_u8
    img = read(img_path)
    gt = read(gt_path) if gt_path else None
    if gt is not None and gt.shape != img.shape:
        raise ValueError("ground truth %s and image %s differ in size" % (gt_path, img_path))
    return lm_path, img, gt, (gt_path or img_path).encode(), masks


def host_part(job, raw: bool = False) -> HostPart:
    """(lm_path, gt_path, size[, mask paths]) -> the host half of one row: HostPart(img u8, gt u8 | None, box, [4 triangle tables], name,
    packed masks | None).  raw = True (the ring path, round 6): img / gt may be pngio.RawScanlines — inflated, still filtered; the device
    reconstructs them."""
    lm_path, img, gt, name, masks = _read_item(job, raw)
    box, lm = crop_box(np.load(lm_path))
    return HostPart(img, gt, np.asarray(box, np.int32), meshes(lm), name, masks)


def host_part_group(job, raw: bool = False) -> HostPart:
    """The host half of one TSM group (an item and its mirror image, csrc/prep_group_kernels.h), in host_part's form with EIGHT triangle
    tables — meshes(lm) + meshes(lm_m) of face_crop_and_resize(with_mirror=True) — so that the ring and the blob code carry it like a row:
    (lm_path, gt_path, size[, mask paths]) -> HostPart(img, gt, box, [8 tables], name, packed masks | None): dataset.build_ucb_tsm_pair's group;
    (label_path, "<sfw>", size)            -> HostPart(img, cmap, box, [8 tables], name, None, label u8 [h,w]): dataset.build_sfw_pair's group
    (decoded in the worker: the label is a palette or grey file whose levels travel as they are).
    The reg_in mesh of the canonical landmarks is the one cached triangulation (_REF_TRI) for both rows and every item."""
    if job[1] == "<sfw>":
        from .pngio import read_grey_u8
        lm_path = job[0]
        stem = lm_path.rsplit(".", 1)[0]
        frame = stem[:-6]                                                 # strips "_label"
        img, cmap, label = _imread_u8(frame + ".png"), _imread_u8(stem + "_cmap.png"), np.ascontiguousarray(read_grey_u8(lm_path))
        if cmap.shape != img.shape or label.shape != img.shape[:2]:
            raise ValueError("the planes of SFW frame %s differ in size" % frame)
        box, lm, lm_m = crop_box_pair(np.load(frame + ".npy"), img.shape[1])
        return HostPart(img, cmap, np.asarray(box, np.int32), meshes(lm) + meshes(lm_m), (frame + ".png").encode(), None, label)
    lm_path, img, gt, name, masks = _read_item(job, raw)
    if gt is None:
        raise ValueError("a TSM group needs the ground truth of %s" % lm_path)
    box, lm, lm_m = crop_box_pair(np.load(lm_path), img.shape[1])
    return HostPart(img, gt, np.asarray(box, np.int32), meshes(lm) + meshes(lm_m), name, masks)


def host_part_uncropped(job, raw: bool = True) -> Optional[UncroppedPart]:
    """The host half of one UNCROPPED photograph (dataset.Dataset(uncropped=True, device_prep=gpu)): (png_path, size) -> UncroppedPart(img,
    None, box of the row, [4 triangle tables], name, CropGeometry(crop box, preset_x, preset_y)) or None where dataprocess.py skips the
    photograph.  Everything but `img` comes from the landmarks alone: wild_crop.crop_geometry (the script's box, presets and landmarks in
    the crop's coordinates), then — as the FFHQ loader does with the folder the script wrote — crop_box and meshes of those landmarks.
    img: the file's inflated, still filtered scanlines (pngio.RawScanlines: the device reconstructs and crops them) or, for a file that
    is no plain 8-bit PNG, the decoded photograph."""
    from . import wild_crop
    img_path, size = job
    img = (_imread_raw if raw else _imread_u8)(img_path)
    if hasattr(img, "raw") and img.w * img.c < 4:
        img = img.decode()
    geo = wild_crop.crop_geometry(np.load(os.path.splitext(img_path)[0] + ".npy"), img.shape[0], img.shape[1])
    if geo is None:
        return None
    cbox, preset_x, preset_y, lm256 = geo
    box, lm = crop_box(lm256)
    return UncroppedPart(img, None, np.asarray(box, np.int32), meshes(lm), img_path.encode(),
                         CropGeometry(np.asarray(cbox, np.int32), preset_x, preset_y))


class WildPhoto:
    """The photograph an element of Dataset(uncropped=True, keep_photo=True) was cropped from, with the crop's geometry (wild_crop.
    crop_geometry): what wild_paste / bsr_paste_faces need to write the network's change back.  Host route: `array` is the uint8
    [h,w,3] photograph.  Device route: `blob` is the batch's uint8 device blob — every WildPhoto of a batch holds the same tensor, and
    with it the blob's memory — the photograph's RGB8 area lies at `off`, and `paste_off` is the blob's area for the batch's
    PASTE_DTYPE records."""
    __slots__ = ("array", "blob", "off", "paste_off", "h", "w", "box", "preset_x", "preset_y")

    def __init__(self, h, w, box, preset_x, preset_y, array=None, blob=None, off=0, paste_off=0):
        self.h, self.w, self.box, self.preset_x, self.preset_y = int(h), int(w), [int(v) for v in box], int(preset_x), int(preset_y)
        self.array, self.blob, self.off, self.paste_off = array, blob, int(off), int(paste_off)

    @property
    def view(self):
        """The photograph as a uint8 [h,w,3] view of the device blob (device route)."""
        return self.blob[self.off:self.off + self.h * self.w * 3].view(self.h, self.w, 3)


def _layout_uncropped(parts, size: int, keep_photo: bool = False) -> UncroppedLayout:
    """The blob of a batch of host_part_uncropped results: [row records | grid | crop records | tall records | per item: scanlines with
    their slack (or the decoded photograph) and the four tables] — the `head`, staged by the caller — then, device only, the
    reconstructed photographs and the S x S crops the row records point to.  keep_photo: every row of every photograph is reconstructed
    (rows_needed = 0) and the device part ends with room for the batch's paste records (paste_off; photo_offs: the photograph of each
    item)."""
    B = len(parts)
    rows, crops = np.zeros(B, ROW_DTYPE), np.zeros(B, CROP_DTYPE)
    n_tall = sum(1 for p in parts if hasattr(p.img, "raw"))
    talls = np.zeros(n_tall, UNFILTER_TALL_DTYPE)
    pieces, cur = [], _Cursor()
    take = cur.take
    rows_off, grid_off, crop_off, tall_off = take(rows.nbytes), take(size * 8), take(crops.nbytes), take(max(n_tall, 1) * UNFILTER_TALL_DTYPE.itemsize)
    pieces.append((grid_off, np.linspace(0, 1, size).astype("<f8")))
    k = 0
    for i, part in enumerate(parts):
        img, box, tabs = part.img, part.box, part.tabs
        cbox, preset_x, preset_y = part.crop
        if len(tabs) != 4:
            raise ValueError("prep blob: item %d carries %d triangle tables, the record takes 4" % (i, len(tabs)))
        c = crops[i]
        c["h"], c["w"], c["box"], c["preset_x"], c["preset_y"] = img.shape[0], img.shape[1], cbox, preset_x, preset_y
        if hasattr(img, "raw"):
            t = talls[k]
            k += 1
            take(UNFILTER_SLACK)
            t["raw_off"] = take(img.raw.nbytes)
            take(UNFILTER_SLACK)
            pieces.append((int(t["raw_off"]), img.raw))
            t["h"], t["w"], t["c"] = img.h, img.w, img.c
            # the lowest photograph row a tap of the crop can touch is the box's last one
            t["rows_needed"] = 0 if keep_photo else min(max(int(cbox[3]) - int(preset_y), 1), img.h)
        else:
            c["src_off"] = take(img.nbytes)
            pieces.append((int(c["src_off"]), img))
        r = rows[i]
        r["h"] = r["w"] = size
        r["box"] = box
        for m, tab in enumerate(tabs):
            if tab.shape[0] > MAX_TRI:
                raise ValueError("a mesh has %d triangles (> %d)" % (tab.shape[0], MAX_TRI))
            r["tri_off"][m] = take(tab.nbytes)
            r["ntri"][m] = tab.shape[0]
            pieces.append((int(r["tri_off"][m]), tab))
    head = cur.off
    k = 0
    for i, part in enumerate(parts):
        if hasattr(part.img, "raw"):
            talls[k]["out_off"] = crops[i]["src_off"] = take(part.img.h * part.img.w * 3 + UNFILTER_SLACK)
            k += 1
    for i in range(B):
        crops[i]["out_off"] = rows[i]["img_off"] = rows[i]["gt_off"] = take(size * size * 3)
    pieces += [(rows_off, rows), (crop_off, crops)] + ([(tall_off, talls)] if n_tall else [])
    paste_off = take(B * PASTE_DTYPE.itemsize) if keep_photo else None
    photo_offs = [int(c["src_off"]) for c in crops] if keep_photo else None
    return UncroppedLayout(cur.off, head, rows_off, grid_off, crop_off, tall_off, n_tall, pieces, paste_off, photo_offs)


RING_CAP = 1 << 20        # bytes of one slot of the loaders' shared-memory ring (a 256x256 UCB item with ground truth, tables and masks: ~0.55 MB)
_RING_VIEWS: dict = {}


def _is_ring(part) -> bool:
    return isinstance(part, RingPart)


def host_part_ring(job, ring, group: bool = False):
    """`host_part(job)` (group: `host_part_group(job)`, eight tables instead of four) written INTO slot `slot` of the shared-memory ring the parent page-locked (SlotRing) instead of pickled through
    the worker's pipe: -> RingPart("ring", slot, (h, w), has_gt, image offsets, table offsets, table lengths, box, name, RingMasks | None,
    bytes used, rawc) — a few hundred bytes.  The loop's own thread then neither reads, unpickles nor repacks the ~0.5 MB of an item (0.1 ms
    per item of the one thread every batch goes through): the slot goes to the device as it lies, by one copy per batch.  An item that
    does not fit a slot comes back the old way, as a HostPart.  Round 6: images that are plain 8-bit PNG files lie in the slot as their
    inflated, still FILTERED scanlines (rawc: channels per image, 0 = decoded RGB) and are reconstructed on the device
    (bsr_png_unfilter) when the job's ring tuple says so (its 4th element: dataset.Dataset.device_unfilter)."""
    path, slot, cap = ring[:3]
    use_raw = bool(ring[3]) if len(ring) > 3 else False       # dataset.Dataset.device_unfilter decides
    part = (host_part_group if group else host_part)(job, raw=use_raw)
    img, gt, tabs, masks = part.img, part.gt, part.tabs, part.masks
    nt = len(tabs)
    # the device kernel takes images of at most UNFILTER_MAX_ROWS rows whose scanlines hold at least one dword; anything else is decoded
    # here.  "raw8" masks stay as they are: _masks_raw only made them for S x S grey files the kernel takes, whatever the images are
    fits = lambda a: not hasattr(a, "raw") or (a.h <= UNFILTER_MAX_ROWS and a.w * a.c >= 4)
    if not (fits(img) and (gt is None or fits(gt))):
        img, gt = (img.decode() if hasattr(img, "raw") else img), (gt.decode() if gt is not None and hasattr(gt, "raw") else gt)
    rawc = tuple(int(getattr(a, "c", 0)) if hasattr(a, "raw") else 0 for a in ([img] + ([gt] if gt is not None else [])))
    arrays = [getattr(a, "raw", a) for a in ([img] + ([gt] if gt is not None else []))] + list(tabs) + ([masks[1]] if masks is not None else [])
    offs, off = [], 0
    for a in arrays:
        offs.append(off)
        off = (off + a.nbytes + 7) & ~7
    if off > cap:                                  # through the pipe after all: decoded here
        dec = lambda a: a.decode() if hasattr(a, "raw") else a
        return part._replace(img=dec(img), gt=dec(gt) if gt is not None else None,
                             masks=masks_from_raw(masks) if masks is not None and masks[0] == "raw8" else masks)
    view = _RING_VIEWS.get(path)
    if view is None:
        view = _RING_VIEWS[path] = np.memmap(path, np.uint8, "r+")
    base = int(slot) * int(cap)
    for o, a in zip(offs, arrays):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        view[base + o:base + o + raw.size] = raw
    k = 2 if gt is not None else 1
    mrec = None if masks is None else RingMasks(masks[0], int(masks[2]), offs[k + nt], int(masks[1].nbytes))
    return RingPart("ring", int(slot), (int(img.shape[0]), int(img.shape[1])), gt is not None, tuple(offs[:k]), tuple(offs[k:k + nt]),
                    tuple(int(t.shape[0]) for t in tabs), np.asarray(part.box, np.int32), part.name, mrec, off, rawc)


class SlotRing:
    """Parent side of the ring: `nslots` x `cap` bytes of shared memory (a file under /dev/shm, unlinked as soon as every worker has
    mapped it), page-locked with hipHostRegister so that the copy engine reads the workers' bytes where they wrote them."""

    def __init__(self, nslots: int, cap: int = RING_CAP):
        import mmap
        import tempfile
        import torch
        self.nslots, self.cap = int(nslots), int(cap)
        d = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
        if d is not None:
            # a tmpfs smaller than the ring would let ftruncate succeed and kill a worker with SIGBUS at its first write beyond the limit
            # (containers often mount 64 MB there): the ring is only built where twice its size is free
            st = os.statvfs(d)
            if st.f_bavail * st.f_frsize < 2 * self.nslots * self.cap:
                raise OSError("/dev/shm has %d MB free, the loader ring needs %d MB" % (st.f_bavail * st.f_frsize >> 20, self.nslots * self.cap >> 20))
        fd, self.path = tempfile.mkstemp(prefix="bsr_ring_%d_" % os.getpid(), dir=d)
        try:
            os.ftruncate(fd, self.nslots * self.cap)
            self._mm = mmap.mmap(fd, self.nslots * self.cap)
        finally:
            os.close(fd)
        self.tensor = torch.frombuffer(self._mm, dtype=torch.uint8)
        self._torch = torch
        self.pinned = False
        if torch.cuda.is_available():
            rc = torch.cuda.cudart().cudaHostRegister(self.tensor.data_ptr(), self.nslots * self.cap, 0)
            self.pinned = int(rc) == 0 and bool(self.tensor.is_pinned())

    def unlink(self) -> None:
        path, self.path = self.path, None
        if path:
            try:
                os.unlink(path)
            except OSError:
                pass

    def close(self) -> None:
        self.unlink()
        t, self.tensor = self.tensor, None
        if t is not None and self.pinned:
            try:
                self._torch.cuda.cudart().cudaHostUnregister(t.data_ptr())
            except Exception:
                pass
        self.pinned = False
        del t
        mm, self._mm = getattr(self, "_mm", None), None
        if mm is not None:
            try:
                mm.close()                       # refused (BufferError) while a view of the mapping is still alive somewhere: the GC takes it then
            except (BufferError, ValueError):
                pass


def _layout(parts, size: int):
    """The blob of a batch of `host_part` results that all came through the pipe: see _layout_ex."""
    lay = _layout_ex(parts, size, RING_CAP)
    if lay.cells:
        raise ValueError("_layout: ring items need DevicePrep.rows_ex")
    return lay.total, lay.rows_off, lay.grid_off, lay.pieces


def _layout_ex(parts, size: int, cap: int, group: bool = False) -> BlobLayout:
    """group = True: the parts are host_part_group's and the records GROUP_DTYPE (eight tables, the label plane).  Offsets of every section
    of the blob (all 8-byte aligned).  Items that came through the pipe are packed behind the records (the `head`, staged
    by the caller); every ring item gets one `cap`-byte cell behind the head, in batch order — cells = [(part index, slot, cell
    offset)] — which the caller fills with the slot's bytes.  Ring images that lie in their slot as filtered scanlines (round 6) get
    a record in the unfilter table (in the head) and an output area behind the cells, where the row records then point."""
    B = len(parts)
    dtype, nt = (GROUP_DTYPE, 8) if group else (ROW_DTYPE, 4)
    rows = np.zeros(B, dtype)
    pieces = []
    cur = _Cursor()
    take = cur.take
    rows_off = take(B * dtype.itemsize)
    grid_off = take(size * 8)
    pieces.append((grid_off, np.linspace(0, 1, size).astype("<f8")))
    for i, part in enumerate(parts):
        if _is_ring(part):
            continue
        img, gt, box, tabs = part.img, part.gt, part.box, part.tabs
        r = rows[i]
        r["h"], r["w"] = img.shape[0], img.shape[1]
        r["img_off"] = take(img.nbytes)
        pieces.append((int(r["img_off"]), img))
        if gt is not None:
            r["gt_off"] = take(gt.nbytes)
            pieces.append((int(r["gt_off"]), gt))
        else:
            r["gt_off"] = r["img_off"]
        r["box"] = box
        if len(tabs) != nt:
            raise ValueError("prep blob: item %d carries %d triangle tables, the record takes %d" % (i, len(tabs), nt))
        if group:
            if part.label is not None:         # the SFW label plane
                r["aux_off"] = take(part.label.nbytes)
                pieces.append((int(r["aux_off"]), part.label))
            else:
                r["aux_off"] = r["img_off"]
        for m, t in enumerate(tabs):
            r["tri_off"][m] = take(t.nbytes)
            r["ntri"][m] = t.shape[0]
            pieces.append((int(r["tri_off"][m]), t))
    pieces.append((rows_off, rows))
    ring_idx = [i for i, part in enumerate(parts) if _is_ring(part)]
    rp = [parts[i] for i in ring_idx]
    raw_masks = [j for j, p in enumerate(rp) if p.masks is not None and p.masks.kind == "raw8"]
    n_unf = sum(sum(1 for c in p.rawc if c) for p in rp) + 7 * len(raw_masks)
    unf = np.zeros(n_unf, UNFILTER_DTYPE)
    unf_off = take(max(n_unf, 1) * UNFILTER_DTYPE.itemsize)
    if n_unf:
        pieces.append((unf_off, unf))
    head = off = cur.off
    cells, mask_out = [], {}
    if ring_idx:
        # the records of the ring items in whole columns (per-field assignments on a structured array cost ~15 us each: 0.3 ms per batch
        # of the loop's own thread when done item by item)
        n = len(rp)
        bases = off + cap * np.arange(n, dtype=np.int64)
        off += cap * n
        hw = np.array([p.hw for p in rp], np.int64).reshape(n, 2)
        has_gt = np.array([p.has_gt for p in rp], bool)
        io0 = np.array([p.img_offs[0] for p in rp], np.int64)
        io1 = np.where(has_gt, np.array([p.img_offs[-1] for p in rp], np.int64), io0)
        toff = np.array([p.tab_offs for p in rp], np.int64).reshape(n, nt)
        ntri = np.array([p.ntri for p in rp], np.int64).reshape(n, nt)
        used = np.array([p.used for p in rp], np.int64)
        rawc = np.array([(tuple(p.rawc) + (0, 0))[:2] for p in rp], np.int64).reshape(n, 2)
        rawc[:, 1] = np.where(has_gt, rawc[:, 1], rawc[:, 0])
        if ((rawc != 0) & (rawc != 1) & (rawc != 3) & (rawc != 4)).any():
            raise ValueError("prep blob: a ring item names %s channels per filtered pixel" % sorted(set(rawc.reshape(-1).tolist())))
        if ((rawc > 0) & ((hw[:, :1] > UNFILTER_MAX_ROWS) | (hw[:, 1:2] * rawc < 4))).any():
            raise ValueError("prep blob: a filtered ring image has more than %d rows or scanlines under 4 bytes" % UNFILTER_MAX_ROWS)
        nb = np.where(rawc > 0, hw[:, :1] * (1 + hw[:, 1:2] * rawc), hw[:, :1] * hw[:, 1:2] * 3)      # bytes of each image as it lies in the slot
        npx = hw[:, 0] * hw[:, 1] * 3
        ends = np.maximum(np.maximum(io0 + nb[:, 0], io1 + nb[:, 1]), (toff + ntri * (TRI_DOUBLES * 8)).max(axis=1))
        bad = (used > cap) | (np.minimum(np.minimum(io0, io1), toff.min(axis=1)) < 0) | (ends > cap) | (hw.min(axis=1) < 0) | (ntri.min(axis=1) < 0)
        if bad.any():
            raise ValueError("prep blob: ring item %d points outside its slot (%d-byte slots)" % (ring_idx[int(np.argmax(bad))], cap))
        sel = np.array(ring_idx)
        rows["h"][sel], rows["w"][sel] = hw[:, 0], hw[:, 1]
        img_at, gt_at = bases + io0, bases + io1
        if n_unf:
            # filtered images: reconstructed into their own area behind the cells (bsr_png_unfilter), the row record points there.  Whole
            # columns again (a Python loop over the images of a batch of 32 cost the loop's thread ~1 ms per batch)
            sel01 = np.stack([rawc[:, 0] > 0, has_gt & (rawc[:, 1] > 0)], axis=1).reshape(-1)
            jj, ww = np.repeat(np.arange(n), 2)[sel01], np.tile(np.array([0, 1]), n)[sel01]
            sizes = (npx[jj] + 7) & ~7
            outs = off + np.cumsum(sizes) - sizes
            off += int(sizes.sum())
            ni = len(jj)
            unf["raw_off"][:ni] = np.where(ww == 0, img_at[jj], gt_at[jj])
            unf["out_off"][:ni], unf["h"][:ni], unf["w"][:ni], unf["c"][:ni] = outs, hw[jj, 0], hw[jj, 1], rawc[jj, ww]
            img_at[jj[ww == 0]] = outs[ww == 0]
            gt_at[jj[ww == 1]] = outs[ww == 1]
            gt_at = np.where(has_gt, gt_at, img_at)
            # the seven masks of an item that lie in its slot as filtered scanlines ("raw8"): seven records, grey output, one area
            if raw_masks:
                mj = np.array(raw_masks)
                mS = np.array([rp[j].masks.S for j in mj], np.int64)
                moff = np.array([rp[j].masks.off for j in mj], np.int64)
                mlen = np.array([rp[j].masks.nbytes for j in mj], np.int64)
                if ((mS < 4) | (mS > UNFILTER_MAX_ROWS) | (mlen != 7 * mS * (1 + mS)) | (moff < 0) | (moff + mlen > cap)).any():
                    raise ValueError("prep blob: a ring item's filtered masks do not fit its slot")
                area = (7 * mS * mS + 7) & ~7
                mout = off + np.cumsum(area) - area
                off += int(area.sum())
                seven = np.arange(7, dtype=np.int64)[None, :]
                sl = slice(ni, ni + 7 * len(mj))
                unf["raw_off"][sl] = (bases[mj][:, None] + moff[:, None] + seven * (mS * (1 + mS))[:, None]).reshape(-1)
                unf["out_off"][sl] = (mout[:, None] + seven * (mS * mS)[:, None]).reshape(-1)
                unf["h"][sl] = unf["w"][sl] = np.repeat(mS, 7)
                unf["c"][sl], unf["grey_out"][sl] = 1, 1
                mask_out = {ring_idx[int(j)]: (int(o), int(S_)) for j, o, S_ in zip(mj, mout, mS)}
        rows["img_off"][sel] = img_at
        rows["gt_off"][sel] = gt_at
        if group:
            rows["aux_off"][sel] = img_at      # ring groups are UCB items: six planes, the label plane is not read
        rows["box"][sel] = np.stack([np.asarray(p.box, np.int32).reshape(4) for p in rp])
        rows["tri_off"][sel] = bases[:, None] + toff
        rows["ntri"][sel] = ntri
        cells = [(i, int(p.slot), int(bs)) for i, p, bs in zip(ring_idx, rp, bases)]
    # the kernel dereferences these offsets on the device without bounds information: every record is checked against the blob here
    h64, w64 = rows["h"].astype(np.int64), rows["w"].astype(np.int64)
    ends = np.maximum(np.maximum(rows["img_off"], rows["gt_off"]) + h64 * w64 * 3, (rows["tri_off"] + rows["ntri"].astype(np.int64) * (TRI_DOUBLES * 8)).max(axis=1))
    lows = np.minimum(np.minimum(rows["img_off"], rows["gt_off"]), rows["tri_off"].min(axis=1))
    if group:
        ends, lows = np.maximum(ends, rows["aux_off"] + h64 * w64), np.minimum(lows, rows["aux_off"])
    bad = (lows < 0) | (ends > off) | (rows["ntri"].max(axis=1) > MAX_TRI) | (rows["ntri"].min(axis=1) < 0) | (h64 < 0) | (w64 < 0)
    if bad.any():
        raise ValueError("prep blob: row %d points outside the %d-byte blob" % (int(np.argmax(bad)), off))
    return BlobLayout(off, rows_off, grid_off, pieces, head, cells, UnfilterTable(unf_off, n_unf, mask_out))


def pack_into(buf: np.ndarray, pieces) -> None:
    """Copy every section into `buf` (a uint8 view of the staging memory)."""
    for off, arr in pieces:
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf[off:off + raw.size] = raw


def pack_batch(parts, size: int):
    """One blob for bsr_prep_rows: [row records | grid | images | triangle tables], every section 8-byte aligned."""
    total, rows_off, grid_off, pieces = _layout(parts, size)
    buf = np.zeros(total, np.uint8)
    pack_into(buf, pieces)
    return buf.tobytes(), rows_off, grid_off


def pack_group_batch(parts, size: int):
    """One blob for bsr_prep_groups: [group records | grid | images | triangle tables], every section 8-byte aligned."""
    lay = _layout_ex(parts, size, RING_CAP, group=True)
    if lay.cells:
        raise ValueError("pack_group_batch: ring items need DevicePrep.rows_ex")
    buf = np.zeros(lay.total, np.uint8)
    pack_into(buf, lay.pieces)
    return buf.tobytes(), lay.rows_off, lay.grid_off


class DevicePrep:
    """`rows(parts)` -> packed `[B,S,S,16]` float32 CUDA tensor (+ the crop boxes) for a list of `host_part` results.
    `planes` = 6 | 7: the parts are `host_part_group` results and the tensor is `[B,2,S,S,planes+10]` (bsr_prep_groups)."""

    def __init__(self, device: int = 0, size: int = 256, planes: Optional[int] = None):
        if planes not in (None, 6, 7):
            raise ValueError("DevicePrep: planes is None (rows), 6 (UCB groups) or 7 (SFW groups), got %r" % (planes,))
        self.planes = planes
        import torch
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError("DevicePrep needs a ROCm GPU: the host path is blindshadowremoval_amd.dataset.build_row")
        self._torch, self._lib, self._check = torch, _lib.load(), _lib.check
        self.device, self.size = int(device), int(size)
        self._stage, self._copied, self._turn = [None, None], [None, None], 0
        self.ring = None              # the loaders' SlotRing (set by the Dataset that owns it): where the bytes of RingPart records lie
        self._h2d = None              # the side stream of the uploads, made by the first batch
        self.last_copy = None         # the event behind the last batch's host-to-device copies

    def warm(self, nbytes: int = 8 << 20) -> None:
        """Page-lock the two staging buffers now (~60 ms each) instead of inside the first two batches of a timed loop."""
        for k in (0, 1):
            if self._stage[k] is None or self._stage[k].numel() < nbytes:
                self._stage[k] = self._torch.empty(nbytes, dtype=self._torch.uint8).pin_memory()

    def _staged(self, head: int, pieces):
        """The host side of a batch's upload: `pieces` packed into the first `head` bytes of a pinned buffer, which is returned.  Two
        buffers are used alternately (self._turn): the sections are copied straight into page-locked memory and go to the device in one
        asynchronous copy; a buffer is reused only after the copy that read it (self._copied) has finished."""
        k = self._turn = (self._turn + 1) & 1
        stage = self._stage[k]
        if stage is None or stage.numel() < head:
            stage = self._stage[k] = self._torch.empty(max(head, 1 << 22) * 5 // 4, dtype=self._torch.uint8).pin_memory()
        if self._copied[k] is not None:
            self._copied[k].synchronize()
        pack_into(stage.numpy(), pieces)
        return stage

    def _side_stream(self):
        """The uploads' OWN stream: the copy engine moves batch k + 1 while the compute stream is still in batch k's forward (on one
        stream the ~16 MB of a batch sat between two forwards: ~0.4 ms of a 4 ms step)."""
        if self._h2d is None:
            self._h2d = self._torch.cuda.Stream(device=self.device)
        return self._h2d

    def rows(self, parts):
        out, boxes, _, _ = self.rows_ex(parts)
        return out, boxes

    def rows_ex(self, parts):
        """-> (rows [B,S,S,16] float32 on the device, boxes [B,4], per item its masks as device views | None, per item its name).
        `parts`: `host_part` results (pickled through a worker's pipe) and / or `host_part_ring` records (the bytes lie in self.ring)."""
        torch = self._torch
        B, S = len(parts), self.size
        ring = self.ring
        cap = ring.cap if ring is not None else RING_CAP
        lay = _layout_ex(parts, S, cap, group=self.planes is not None)
        total, rows_off, grid_off, head, cells, unf = lay.total, lay.rows_off, lay.grid_off, lay.head, lay.cells, lay.unf

        def launch(stream):
            """the preparation kernels on `stream`: -> (out, return code)"""
            if self.planes is None:
                out = torch.empty((B, S, S, 16), dtype=torch.float32, device=dev)
                tmp = torch.empty((B, S, S), dtype=torch.float32, device=dev)
                return out, self._lib.bsr_prep_rows(self.device, d_blob.data_ptr(), total, rows_off, grid_off, B, S, out.data_ptr(), tmp.data_ptr(), stream)
            out = torch.empty((B, 2, S, S, self.planes + 10), dtype=torch.float32, device=dev)
            tmp = torch.empty((2 * B, S, S), dtype=torch.float32, device=dev)
            return out, self._lib.bsr_prep_groups(self.device, d_blob.data_ptr(), total, rows_off, grid_off, B, S, self.planes, out.data_ptr(),
                                                  tmp.data_ptr(), stream)
        if cells and ring is None:
            raise RuntimeError("DevicePrep.rows_ex: ring records without a ring")
        if cells and self.planes == 7:           # a ring record has no label plane: its aux_off points at the photograph
            raise ValueError("DevicePrep.rows_ex: SFW groups (planes=7) do not travel through the ring")
        dev = "cuda:%d" % self.device
        with torch.cuda.device(self.device):
            stage = self._staged(head, lay.pieces)
            main = torch.cuda.current_stream()
            h2d = self._side_stream()
            with torch.cuda.stream(h2d):
                d_blob = torch.empty(total, dtype=torch.uint8, device=dev)
                d_blob[:head].copy_(stage[:head], non_blocking=True)
                # ring items: consecutive slots of consecutive cells go in ONE copy (the usual case: the whole batch), whole slots as they lie
                c = 0
                while c < len(cells):
                    e = c + 1
                    while e < len(cells) and cells[e][1] == cells[e - 1][1] + 1:
                        e += 1
                    src = ring.tensor[cells[c][1] * cap:(cells[e - 1][1] + 1) * cap]
                    d_blob[cells[c][2]:cells[c][2] + (e - c) * cap].copy_(src, non_blocking=True)
                    c = e
                ev = self._copied[self._turn] = self.last_copy = torch.cuda.Event()
                ev.record()
                # the preparation kernel follows its input on the same side stream (BSR_PREP_SIDE=0: on the compute stream): a short
                # bandwidth-bound kernel that shares the chip with the previous batch's forward instead of standing in line behind it
                side = os.environ.get("BSR_PREP_SIDE", "1") != "0"
                if side:
                    if unf.n:                      # the filtered images of the ring items become RGB8 where their row records point
                        self._check(self._lib.bsr_png_unfilter(self.device, d_blob.data_ptr(), total, unf.off, unf.n, h2d.cuda_stream), "bsr_png_unfilter")
                    out, rc = launch(h2d.cuda_stream)
                    done = torch.cuda.Event()
                    done.record()
            if side:
                main.wait_event(done)
                out.record_stream(main)
            else:
                main.wait_event(ev)
            d_blob.record_stream(main)             # allocated on the side stream, read by the compute stream (the mask views; the kernel when it runs there)
            if not side:
                if unf.n:
                    self._check(self._lib.bsr_png_unfilter(self.device, d_blob.data_ptr(), total, unf.off, unf.n, main.cuda_stream), "bsr_png_unfilter")
                out, rc = launch(main.cuda_stream)
        self._check(rc, "bsr_prep_rows" if self.planes is None else "bsr_prep_groups")
        boxes = np.stack([np.asarray(p.box, np.float32) for p in parts], axis=0)
        names = [p.name for p in parts]
        masks = [None if _is_ring(p) else p.masks for p in parts]
        for i, _, base in cells:
            m = parts[i].masks
            if m is not None:
                if m.kind == "raw8":               # reconstructed by bsr_png_unfilter into their own area: grey levels [7,S,S]
                    o = unf.mask_out[i][0]
                    masks[i] = ("dev_u8", d_blob[o:o + 7 * m.S * m.S].view(7, m.S, m.S), m.S)
                    continue
                v = d_blob[base + m.off:base + m.off + m.nbytes]
                masks[i] = ("dev_" + m.kind, v.view(7, -1) if m.kind == "bits" else v.view(7, m.S, m.S), m.S)
        return out, boxes, masks, names

    def rows_uncropped(self, parts, keep_photo: bool = False):
        """rows_ex for host_part_uncropped results (they come through the workers' pipes: a 1024 x 1024 photograph is three ring slots):
        the scanlines go to the device as they were inflated, and bsr_png_unfilter_tall -> bsr_crop_faces -> bsr_prep_rows run behind the
        copy in one stream; the crop's output is the row record's image.  -> (rows [B,S,S,16], boxes, [None] * B, names).  keep_photo:
        the third entry holds a WildPhoto per item instead — the whole photograph, reconstructed in the blob, and its geometry; the
        rows are the same bits."""
        if self.planes is not None:
            raise ValueError("DevicePrep.rows_uncropped prepares rows (planes=None)")
        torch = self._torch
        B, S = len(parts), self.size
        lay = _layout_uncropped(parts, S, keep_photo)
        total, head = lay.total, lay.head
        dev = "cuda:%d" % self.device
        with torch.cuda.device(self.device):
            stage = self._staged(head, lay.pieces)
            main = torch.cuda.current_stream()
            h2d = self._side_stream()
            with torch.cuda.stream(h2d):
                st = h2d.cuda_stream
                d_blob = torch.empty(total, dtype=torch.uint8, device=dev)
                d_blob[:head].copy_(stage[:head], non_blocking=True)
                ev = self._copied[self._turn] = self.last_copy = torch.cuda.Event()
                ev.record()
                if lay.n_tall:
                    self._check(self._lib.bsr_png_unfilter_tall(self.device, d_blob.data_ptr(), total, lay.tall_off, lay.n_tall, st), "bsr_png_unfilter_tall")
                self._check(self._lib.bsr_crop_faces(self.device, d_blob.data_ptr(), total, lay.crop_off, B, S, st), "bsr_crop_faces")
                out = torch.empty((B, S, S, 16), dtype=torch.float32, device=dev)
                tmp = torch.empty((B, S, S), dtype=torch.float32, device=dev)
                rc = self._lib.bsr_prep_rows(self.device, d_blob.data_ptr(), total, lay.rows_off, lay.grid_off, B, S, out.data_ptr(), tmp.data_ptr(), st)
                done = torch.cuda.Event()
                done.record()
            main.wait_event(done)
            out.record_stream(main)
            tmp.record_stream(main)
            d_blob.record_stream(main)
        self._check(rc, "bsr_prep_rows")
        boxes = np.stack([np.asarray(p.box, np.float32) for p in parts], axis=0)
        photos = [None] * B
        if keep_photo:
            photos = [WildPhoto(p.img.shape[0], p.img.shape[1], p.crop.box, p.crop.preset_x, p.crop.preset_y, blob=d_blob, off=o,
                                paste_off=lay.paste_off) for p, o in zip(parts, lay.photo_offs)]
        return out, boxes, photos, [p.name for p in parts]
