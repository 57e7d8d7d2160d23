#!/usr/bin/env python3
"""The reference's depth losses (utils.py:301-342) on the cases of tests/helpers/depth_loss_ref.py, by IMPORTING the reference on CPU
(stubs as in make_golden.py) and running its OWN functions on float64 tensors under autograd: the goldens are the reference itself,
not a restatement. Writes tests/golden/depth_loss.npz (outputs only: the inputs are rebuilt from seeds by the case builder) and
tests/golden/depth_loss_signatures.json (parameter names, kinds and defaults of the four functions).

    python tests/golden/make_golden_depth_loss.py

statsmodels is not installed here. scale_shift_invariant_loss calls `sm.add_constant(x)` and `sm.WLS(y, X, weights=w).fit().params`;
the stand-in below gives them statsmodels' documented default arithmetic — a column of ones in front, and the pseudo-inverse of the
sqrt(w)-whitened design applied to the whitened target (WLS.fit(method="pinv")) in float64 — like the kornia stand-in of
make_golden.py. `s` and `t` from the real package have NOT been compared.
"""
import inspect
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
for name in ["cv2", "imageio", "imageio.v2", "configargparse", "torchvision", "torchvision.transforms", "statsmodels",
             "statsmodels.api", "lpips", "plyfile", "skimage", "skimage.io", "skimage.metrics", "skimage.measure", "scripts.Warper",
             "scipy", "scipy.signal"]:
    sys.modules.setdefault(name, MagicMock())
kornia = types.ModuleType("kornia")
kornia.create_meshgrid = lambda *a, **k: None      # imported by name only; never called here
sys.modules["kornia"] = kornia

import utils as ref_utils  # noqa: E402

from tests.helpers import depth_loss_ref as D  # noqa: E402


class _WLS:
    def __init__(self, endog, exog, weights):
        sw = np.sqrt(np.asarray(weights, np.float64))
        self.y, self.x = np.asarray(endog, np.float64) * sw, np.asarray(exog, np.float64) * sw[:, None]

    def fit(self):
        return types.SimpleNamespace(params=np.linalg.pinv(self.x) @ self.y)


ref_utils.sm = types.SimpleNamespace(add_constant=lambda x: np.stack([np.ones(len(x)), np.asarray(x, np.float64)], 1), WLS=_WLS)


def describe(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(grad)


def grad_of(t):
    return np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()


def main():
    out = {}
    for cid, c in D.all_cases().items():
        y = t64(c["depth_t"])
        # gnll (the directed cases exist for it; the ssi specials have no guarantees about its branches)
        if not cid.startswith("ssi-"):
            mu, w, z = t64(c["depth_fin"], True), t64(c["w"], True), t64(c["z"])
            loss = ref_utils.compute_depth_loss(mu, z, w, y, target_std=D.SIGMA)
            out[f"{cid}/gnll_shape"] = np.array(loss.shape, np.int64)
            loss.sum().backward()
            out[f"{cid}/gnll_loss"], out[f"{cid}/gnll_d_depth"], out[f"{cid}/gnll_d_w"] = loss.detach().numpy().reshape(-1)[0], grad_of(mu), grad_of(w)
            var = ((z - mu.detach()[:, None]) ** 2 * w.detach()).sum(-1) + 1e-8
            out[f"{cid}/gnll_apply"] = ref_utils.is_not_in_expected_distribution(mu.detach(), var, y, D.SIGMA).numpy()
        if cid.startswith(("rand-", "narrow-")):
            mu = t64(c["depth_fin"], True)
            loss = ref_utils.compute_depth_loss_scale_invariant(mu, y)
            loss.backward()
            out[f"{cid}/si_loss"], out[f"{cid}/si_d_depth"] = loss.detach().numpy(), grad_of(mu)
        if not cid.startswith("directed-"):
            w, z = t64(c["w"], True), t64(c["z"])
            loss, s, t = ref_utils.scale_shift_invariant_loss(z, w, y)
            loss.backward()
            out[f"{cid}/ssi_loss"], out[f"{cid}/ssi_st"], out[f"{cid}/ssi_d_w"] = loss.detach().numpy(), np.array([s, t], np.float64), grad_of(w)
    np.savez_compressed(os.path.join(HERE, "depth_loss.npz"), **out)
    print("depth_loss.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "depth_loss.npz")), "bytes")
    path = os.path.join(HERE, "depth_loss_signatures.json")
    with open(path, "w") as fh:
        json.dump({n: describe(getattr(ref_utils, n)) for n in ("is_not_in_expected_distribution", "compute_depth_loss",
                                                                 "compute_depth_loss_scale_invariant", "scale_shift_invariant_loss")},
                  fh, indent=1, sort_keys=True)
    print(open(path).read())


if __name__ == "__main__":
    main()
