#!/usr/bin/env python3
"""Writes tests/golden/g20_dfv_head.npz: what the reference's own code computes between a decoder level's cost volume and DFVNet's
outputs, recorded as data.  DFVNet itself needs torchvision for its feature extractor and is not built; the head is
`disparityregression` of DFV_models/submodule.py (that file imports only torch and numpy and is loaded by path) applied to
`F.softmax(F.interpolate(...), 1)` exactly as DFV_models/DFFNet.py:94-95 (bilinear, levels 1 and 2) and :107-108 (trilinear over
[S, H, W] with the depth unchanged, levels 3 and 4) do.  Run once, on the CPU, where a checkout of the reference is at hand; the tests
only read the file.

    python tests/golden/make_dfv_head_golden.py --reference /path/to/reference [--out tests/golden/g20_dfv_head.npz]

Cases, each with B = 2, S = 5, two different rows of focus distances (the second descending) and costs spanning about +-6:
    bilinear 8 x 12 -> 32 x 48 (ratio 4 exactly), bilinear 9 x 13 -> 37 x 54 (ratio about 4.1 on both axes), trilinear 4 x 5 -> 32 x 40.
Recorded per case: cost, foc_dists, g_pred, pred, std and the autograd gradient of <g_pred, pred> to the cost and the focus distances."""
import argparse
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("bilinear", 8, 12, 32, 48), ("bilinear", 9, 13, 37, 54), ("trilinear", 4, 5, 32, 40)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "g20_dfv_head.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_dfv_submodule", os.path.join(a.reference, "DFV_models", "submodule.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    disp_reg = ref.disparityregression(1)

    g = torch.Generator().manual_seed(20)
    B, S = 2, 5
    foc = torch.tensor([[0.6, 1.0, 1.5, 2.1, 2.9], [2.8, 2.2, 1.7, 1.1, 0.7]])
    data = {"foc_dists": foc.numpy(), "cases": np.array([f"{m}|{h}|{w}|{H}|{W}" for m, h, w, H, W in CASES])}
    for i, (mode, h, w, H, W) in enumerate(CASES):
        cost = 2.0 * torch.randn(B, S, h, w, generator=g)
        g_pred = torch.randn(B, 1, H, W, generator=g)
        c, u = cost.clone().requires_grad_(True), foc.clone().requires_grad_(True)
        if mode == "bilinear":
            up = F.interpolate(c, [H, W], mode="bilinear")
        else:
            up = F.interpolate(c.unsqueeze(1), [u.shape[1], H, W], mode="trilinear").squeeze(1)
        pred, std = disp_reg(F.softmax(up, 1), u, uncertainty=True)
        assert not std.requires_grad and pred.shape == std.shape == (B, 1, H, W)
        (pred * g_pred).sum().backward()
        tag = f"case{i}_"
        data.update({tag + "cost": cost.numpy(), tag + "g_pred": g_pred.numpy(), tag + "pred": pred.detach().numpy(), tag + "std": std.numpy(),
                     tag + "d_cost": c.grad.numpy(), tag + "d_foc_dists": u.grad.numpy()})
        print(f"case {i}: {mode} {h} x {w} -> {H} x {W}: cost {float(cost.min()):.2f} .. {float(cost.max()):.2f}, "
              f"pred {float(pred.detach().min()):.3f} .. {float(pred.detach().max()):.3f}, std up to {float(std.max()):.3f}")
    np.savez_compressed(a.out, **data)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
