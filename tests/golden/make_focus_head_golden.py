#!/usr/bin/env python3
"""Writes tests/golden/g18_focus_head.npz: what the reference's own AiFDepthNet (dff/AiFNet.py of the reference project; it imports only
torch and numpy) computes in its attention stage and its loss, recorded as data.  Run once, on the CPU, where a checkout of the reference
is at hand; the tests only read the file.

    python tests/golden/make_focus_head_golden.py --reference /path/to/reference [--out tests/golden/g18_focus_head.npz]

Per net AiFDepthNet(n_classes K, normalize_attention, n_stack 4), K in {1, 2}: `fit` on one seeded stack [2,3,4,32,32] with two different
rows of focus distances; the logits are taken with a forward hook on `net.out`, whose weight and bias are first rescaled so that the
logits span [-6, 6] (at initialisation they span a few hundredths, where every attention is flat) and, in the normalised-softplus net
with K = 2, [-24, 24], past softplus's threshold of 20.  Recorded: logits, pred_depth, pred_AiF_img and the autograd gradient of
<g_depth, pred_depth> + <g_aif, pred_AiF_img> with respect to the logits.  For the loss: `compute_loss` on the first net's predictions
for D_FS, A_FS and DA_FS with mask_range False and True (weights 1, 0.7, 0.3), its dict and the gradients of 'total' with respect to
d_out and AiF, plus one crop case (DA_FS, gt_depth 30 x 31 under the 32 x 32 prediction)."""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = dict(disp_w=1.0, aif_w=0.7, smooth_w=0.3)
NETS = [(1, False, 6.0), (1, True, 6.0), (2, False, 6.0), (2, True, 24.0)]      # K, normalize_attention, half-span of the logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "g18_focus_head.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_aifnet", os.path.join(a.reference, "dff", "AiFNet.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    g = torch.Generator().manual_seed(18)
    N, S, H, W = 2, 4, 32, 32
    stack = torch.rand(N, 3, S, H, W, generator=g)
    foc = torch.tensor([[0.6, 1.0, 1.6, 2.4], [2.8, 1.9, 1.2, 0.7]])
    g_depth, g_aif = torch.randn(N, 1, H, W, generator=g), torch.randn(N, 3, H, W, generator=g)
    args = {"device": "cpu"}
    data = {"stack": stack.numpy(), "foc_dists": foc.numpy(), "g_depth": g_depth.numpy(), "g_aif": g_aif.numpy(),
            "nets": np.array([(k, int(nz)) for k, nz, _ in NETS], np.int32), "weights": np.array([WEIGHTS[k] for k in ("disp_w", "aif_w", "smooth_w")])}
    first = None
    for i, (K, norm, span) in enumerate(NETS):
        torch.manual_seed(100 + i)
        net = ref.AiFDepthNet(n_channels=3, n_classes=K, n_stack=S, normalize_attention=norm, **WEIGHTS).eval()
        net.d_layers = foc
        seen = {}
        hook = net.out.register_forward_hook(lambda m, inp, out: seen.__setitem__("z", out))
        with torch.no_grad():
            net.fit(stack, args)
            lo, hi = float(seen["z"].min()), float(seen["z"].max())
            f = 2.0 * span / (hi - lo)
            net.out.weight.mul_(f)
            net.out.bias.mul_(f).sub_(f * 0.5 * (hi + lo))
        out = net.fit(stack, args)
        z = seen["z"]
        z.retain_grad()
        hook.remove()
        assert float(z.detach().min()) < -0.9 * span and float(z.detach().max()) > 0.9 * span and z.shape == (N, K, S, H, W)
        depth, aif = out["pred_depth"], out["pred_AiF_img"]
        ((depth * g_depth).sum() + (aif * g_aif).sum()).backward()
        tag = f"net{i}_"
        data.update({tag + "logits": z.detach().numpy(), tag + "depth": depth.detach().numpy(), tag + "aif": aif.detach().numpy(),
                     tag + "d_logits": z.grad.numpy()})
        print(f"net {i}: K {K} normalize {norm}: logits {float(z.detach().min()):.2f} .. {float(z.detach().max()):.2f}")
        if first is None:
            first = (net, depth.detach(), aif.detach())

    net, depth, aif = first
    gt_depth = 0.3 + 2.9 * torch.rand(N, 1, H, W, generator=g)
    gt_depth[torch.rand(N, 1, H, W, generator=g) < 0.1] = 0.0
    gt_aif = 0.5 + 0.004 * torch.randn(N, 3, H, W, generator=g)
    gt_aif[:, :, H // 2:, W // 3:] += 0.25
    data.update({"gt_depth": gt_depth.numpy(), "gt_aif": gt_aif.numpy()})
    cases = [(task, mr, (H, W)) for task in ("D_FS", "A_FS", "DA_FS") for mr in (False, True)] + [("DA_FS", False, (30, 31))]
    data["loss_cases"] = np.array([f"{t}|{int(mr)}|{h}|{w}" for t, mr, (h, w) in cases])
    for j, (task, mr, (h, w)) in enumerate(cases):
        net.MASK_RANGE = mr
        d, x = depth.clone().requires_grad_(True), aif.clone().requires_grad_(True)
        gd = gt_depth[:, :, :h, :w]
        ga = gt_aif[:, :, :h, :w] if task == "A_FS" else gt_aif          # DA_FS crops gt_AiF itself, by the amount gt_depth is smaller
        losses, _ = net.compute_loss({"pred_depth": d, "pred_AiF_img": x}, {"depth": gd, "AiF_img": ga}, {"task": task, "device": "cpu"})
        losses["total"].backward()
        tag = f"loss{j}_"
        data[tag + "keys"] = np.array(list(losses))
        data[tag + "values"] = np.array([float(v) for v in losses.values()], np.float32)
        data[tag + "d_depth"] = (torch.zeros_like(d) if d.grad is None else d.grad).numpy()
        data[tag + "d_aif"] = (torch.zeros_like(x) if x.grad is None else x.grad).numpy()
        print(f"loss {j}: {task} mask_range {mr} gt {h} x {w}: " + ", ".join(f"{k} {float(v):.6f}" for k, v in losses.items()))
    np.savez_compressed(a.out, **data)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
