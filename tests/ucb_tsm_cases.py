"""Inputs of the TSM UCB post-processing cases shared by tools/make_ucb_post_tsm_fixture.py (which runs the reference's code on them)
and the tests (which run ours): the ten cases of tests/ucb_cases.py, each with a seeded second prediction for the mirror row
(con1 = flip(gt) + noise), plus constructed cases whose kept shadow covers a chosen share of the nose, so that every nose window of
train_with_TSM.py:556 is reached, on a normal and on a darkened input (the two reaches of :561-565).

A case is (key, row, box, masks, con0, con1, dif0)."""
import numpy as np

from ucb_cases import build_item, cases as gsc_cases, load_masks

NOSE_TARGETS = (("w0", 0.424), ("w1", 0.545), ("w2", 0.365), ("w3", 0.5925), ("miss", 0.47))


def second_prediction(row, noise, seed):
    gt = row[..., 3:6]
    return (gt[:, ::-1] + np.random.RandomState(seed).randn(*gt.shape).astype(np.float32) * np.float32(max(noise, 0.01))).astype(np.float32)


def nose_dif(masks, share):
    """dif0 = 0.5 on the first round(share * n) nose pixels in raster order (one component inside the face), 0 elsewhere."""
    nose = masks["nose"][:, :, 0] == 1
    ys, xs = np.nonzero(nose)
    n = int(round(share * ys.size))
    dif = np.zeros(nose.shape + (1,), np.float32)
    dif[ys[:n], xs[:n], 0] = 0.5
    return dif


def cases():
    for i, (key, row, box, masks, con, dif) in enumerate(gsc_cases()):
        yield key, row, box, masks, con, second_prediction(row, 0.02, 100 + i), dif
    item = "9156-004"
    row, box = build_item(item)
    masks = load_masks(item)
    for j, (tag, share) in enumerate(NOSE_TARGETS):
        for dark in (False, True):
            r = row.copy()
            if dark:
                r[..., 0:3] *= np.float32(0.2)
            con0 = (r[..., 3:6] + np.float32(0.05)).astype(np.float32)
            yield ("nose_%s%s" % (tag, "_dark" if dark else "")), r, box, masks, con0, second_prediction(r, 0.02, 200 + 2 * j + dark), nose_dif(masks, share)


def edge_cases():
    """Where the reference would raise or produce NaN: (key, row, box, masks, con0, con1, dif0, what)."""
    item = "9156-004"
    row, box = build_item(item)
    masks = load_masks(item)
    con0 = row[..., 3:6].copy()
    con1 = second_prediction(row, 0.02, 300)
    yield "no_component", row, box, masks, con0, con1, np.zeros(row.shape[:2] + (1,), np.float32), "no_component"
    hair = (masks["face_hair"][:, :, 0] - masks["face"][:, :, 0]) == 1
    dif = np.where(hair[..., None], np.float32(0.5), np.float32(0)).astype(np.float32)
    yield "hair_only", row, box, masks, con0, con1, dif, "empty_keep"
    m = dict(masks)
    m["nose"] = np.zeros_like(masks["nose"])
    yield "no_nose", row, box, m, con0, con1, nose_dif(masks, 0.5), "empty_nose"
