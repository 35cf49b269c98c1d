"""Shared by tests/test_psfnet_grad_host.py and tests/test_gpu_psfnet_grad.py (not a test module): the cases of the PSF-network
gradient tests and their float64 comparator.

oracle/psfnet.py:psfnet_render casts its network input to float32, so the comparator composes oracle.psfnet.depth2z, mlp_forward
and oracle.conv.local_psf_render itself, in the requested dtype.  The coordinate axes are the float32 linspace values the kernels
use, cast up: they are inputs, not results.

The gradient of a ReLU network jumps where a hidden pre-activation crosses 0, so a last-bit difference moves a few pixels' gradients
by percents.  The tests therefore zero the cotangent on every row (n, slice, y, x) whose smallest |hidden pre-activation|, computed
in float64, is below EPS = 1e-5 (20 x the ~5e-7 operand-split / fp32 error of a 256-term layer).  An output pixel depends on its own
row's PSF only, so such rows drop out of d_depth and d_foc completely.  The masked share must stay <= 5 % (MAX_MASKED)."""
import numpy as np
import torch
import torch.nn.functional as F

from aadff.synth import mlp_state_dict, synth_depth_mm, synth_rgb
from oracle import conv as oconv
from oracle import psfnet as opsf

EPS, MAX_MASKED, KS = 1e-5, 0.05, 11
G7_FDS = (-500.0, -800.0, -1500.0, -3000.0, -5000.0)

# name, N, C, S, H, W, weight seed, focus distances [N][S]
CASES = [
    ("1x3x64x64_S5", 1, 3, 5, 64, 64, 4321, [G7_FDS]),
    ("2x3x96x128_S3", 2, 3, 3, 96, 128, 4321, [(-600.0, -1200.0, -3000.0), (-800.0, -2000.0, -4500.0)]),
    ("1x1x67x131_S1", 1, 1, 1, 67, 131, 7, [(-1500.0,)]),
    ("1x3x240x320_S2", 1, 3, 2, 240, 320, 4321, [(-700.0, -2500.0)]),
]


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def state_dict(seed):
    return {k: tt(v) for k, v in mlp_state_dict(seed=seed).items()}


def case_inputs(case):
    """(sd, img [N,C,H,W], depth [N,1,H,W] mm < 0, fds [N,S], dy [N,C,S,H,W]) float32 on the CPU; G7's scene seeds for item 0."""
    name, N, C, S, H, W, wseed, fds = case
    img = torch.stack([tt(synth_rgb(H, W, seed=11 + 100 * n))[:C] for n in range(N)])
    depth = torch.stack([-tt(synth_depth_mm(H, W, seed=12 + 100 * n))[None] for n in range(N)])
    dy = torch.randn((N, C, S, H, W), generator=torch.Generator().manual_seed(31))
    return state_dict(wseed), img, depth, torch.tensor(fds, dtype=torch.float32), dy


def _rows(depth, fd, dtype):
    """Network input [N,H,W,4] of one slice: depth [N,1,H,W], fd [N] (deeplens/psfnet.py:424-437)."""
    N, _, H, W = depth.shape
    x, y = torch.meshgrid(torch.linspace(-1, 1, W).to(dtype), torch.linspace(1, -1, H).to(dtype), indexing="xy")
    z = opsf.depth2z(depth).squeeze(1)
    foc_z = opsf.depth2z(fd.reshape(N, 1, 1).expand(N, H, W))
    return torch.stack((x.unsqueeze(0).expand(N, H, W), y.unsqueeze(0).expand(N, H, W), z, foc_z), -1)


def oracle_stack(sd, img, depth, fds, dtype):
    """[N,C,S,H,W] in `dtype`, differentiable to img, depth and fds."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    N, C, H, W = img.shape
    sl = []
    for s in range(fds.shape[1]):
        psf = opsf.mlp_forward(sdd, _rows(depth, fds[:, s], dtype))
        sl.append(oconv.local_psf_render(img, psf.reshape(N, H, W, KS, KS), KS))
    return torch.stack(sl, dim=2)


def oracle_grads(sd, img, depth, fds, dy, dtype):
    """(out, d_img, d_depth, d_foc) of the oracle in `dtype`; one slice at a time (bounded memory), summed in slice order."""
    x = img.detach().to(dtype).requires_grad_(True)
    d = depth.detach().to(dtype).requires_grad_(True)
    f = fds.detach().to(dtype).requires_grad_(True)
    outs, gi, gd, gf = [], torch.zeros_like(x), torch.zeros_like(d), torch.zeros_like(f)
    for s in range(fds.shape[1]):
        out = oracle_stack(sd, x, d, f[:, s:s + 1], dtype)
        a, b, c = torch.autograd.grad(out, (x, d, f), dy[:, :, s:s + 1].to(dtype))
        gi, gd, gf = gi + a, gd + b, gf + c
        outs.append(out.detach())
    return torch.cat(outs, dim=2), gi, gd, gf


def keep_rows(sd, depth, fds):
    """[N,1,S,H,W] float32 mask: 1 where every hidden pre-activation of the row is at least EPS away from 0 (float64)."""
    sdd = {k: v.double() for k, v in sd.items()}
    n_lin = len([k for k in sdd if k.endswith(".weight")])
    keep = []
    with torch.no_grad():
        for s in range(fds.shape[1]):
            h = _rows(depth.double(), fds[:, s].double(), torch.float64)
            small = torch.full(h.shape[:-1], float("inf"), dtype=torch.float64)
            for i in range(n_lin - 1):
                a = F.linear(h, sdd[f"net.{2 * i}.weight"], sdd[f"net.{2 * i}.bias"])
                small = torch.minimum(small, a.abs().amin(-1))
                h = torch.relu(a)
            keep.append(small >= EPS)
    return torch.stack(keep, dim=1).unsqueeze(1).float()


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())
