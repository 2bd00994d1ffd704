"""CPU oracle of the single-stage RGB baseline generator (/root/reference/model_RGB.py:198-266) — test infrastructure.

Built on oracle.gsc_oracle's primitives (``conv_block``, ``convt_block``, ``res_bottleneck``, ``non_local``), which restate the blocks
model_RGB.py shares with model.py (:6-177).  ``dtype=torch.float64`` runs every statement in double precision (the reference of the
stage table in tests/test_rgb_gpu.py).

Probes (named as ``GeneratorRGB.probe`` names them): x1 x2 x3 x0 res0-2 (plus the ``res_stack/<i>/y3`` / ``.../non_local/att``
intermediates of ``res_bottleneck``) up1 up2 up3 y con.
"""
from typing import Dict, Optional

import numpy as np
import torch

from oracle.gsc_oracle import GeneratorOracle, _t, resize_bilinear


class GeneratorRGBOracle(GeneratorOracle):
    """Restatement of the RGB baseline's ``Generator.call`` (model_RGB.py:228-266) at ``training=False``."""

    def __init__(self, weights: Dict[str, np.ndarray], n_res: int = 6, dtype: torch.dtype = torch.float32):
        super().__init__(weights, n_res, dtype)

    def head(self, y):
        """conv2 'tconv3' then conv3 'tconv4' (:253-254): 7x7 convs, no BN, no activation.  Returns (y_head, con)."""
        yh = self.conv_block(y, "conv2", bn=False, act=False)
        return yh, self.conv_block(yh, "conv3", bn=False, act=False)

    def forward(self, inputs, uv, reg=None, chuck=1, training=False, probes: Optional[dict] = None):
        assert not training, "the oracle restates the inference path only"
        inputs, uv = _t(inputs, self.dtype), _t(uv, self.dtype)
        x1 = self.conv_block(inputs, "conv1")                     # :230
        x2 = self.conv_block(x1, "down1", 2)                      # :231
        x3 = self.conv_block(x2, "down2", 2)                      # :232
        x = self.conv_block(x3, "down3", 2)                       # :233
        uv_s = resize_bilinear(uv, (x.shape[1], x.shape[2]))      # :237
        x = torch.cat([x, uv_s], dim=3)                           # :238
        if probes is not None:
            probes.update(x1=x1, x2=x2, x3=x3, x0=x)
        for i in range(self.n_res // 2):                          # :239-240
            x = self.res_bottleneck(x, i, probes)
            if probes is not None:
                probes["res%d" % i] = x
        y = self.convt_block(x, "up1")                            # :250
        if probes is not None:
            probes["up1"] = y
        y = self.convt_block(torch.cat([y, x3], dim=3), "up2")    # :251
        if probes is not None:
            probes["up2"] = y
        y = self.convt_block(torch.cat([y, x2], dim=3), "up3")    # :252
        yh, con = self.head(y)                                    # :253-254
        if probes is not None:
            probes.update(up3=y, y=yh, con=con)
        return con                                                # :266

    __call__ = forward


def load_fixture(path):
    """tests/golden/model_py_rgb_*.npz (tools/make_model_rgb_fixture.py) -> (inputs, uv float32 tensors, con [B, H/s, W/s, 3] numpy, s):
    the reference's con is stored on every s-th row and column; compare it with ``out[:, ::s, ::s]``."""
    z = np.load(path)
    inp = torch.from_numpy(z["inputs_u8"].astype(np.float32) / np.float32(255.0))
    uv = torch.from_numpy(z["uv_u8"].astype(np.float32) / np.float32(255.0))
    return inp, uv, z["con"], int(z["con_stride"])
