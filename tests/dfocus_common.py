"""Shared by tests/test_dfocus_host.py, tests/test_gpu_dfocus.py and tools/dfocus_bench.py: the oracle of the classical depth-from-focus
estimator (csrc/dfocus.hip), written in torch from the specification of DESIGN.md 4.10, and the seeded inputs.

Oracle: gray and the modified Laplacian in float32 in the stated operation order (separate torch ops, each exactly rounded, so the ML
map is the kernel's bit for bit); window sum, peak and fit in `acc` (float64 in the tests; float32 on the GPU is the torch composition
tools/dfocus_bench.py times the kernel against).  It runs on the device of its inputs.
"""
import numpy as np
import torch
import torch.nn.functional as F

INTERPS = ("none", "parabola", "gaussian")


def focus_volume(stack, window, acc=torch.float64):
    """stack [N,C,S,H,W] -> (ML [N,S,H,W] float32, F [N,S,H,W] in `acc`): specification steps 1-3."""
    x = stack.to(torch.float32)
    C = x.shape[1]
    g = x[:, 0]
    for c in range(1, C):
        g = g + x[:, c]                                        # channel order
    g = g * torch.tensor(np.float32(1.0 / C), device=x.device)
    p = F.pad(g, (1, 1, 1, 1), mode="replicate")               # [N,S,H+2,W+2]: pads the last two dimensions
    c0, left, right, up, down = p[..., 1:-1, 1:-1], p[..., 1:-1, :-2], p[..., 1:-1, 2:], p[..., :-2, 1:-1], p[..., 2:, 1:-1]
    g2 = c0 * 2.0
    ml = ((g2 - left) - right).abs() + ((g2 - up) - down).abs()
    r = window // 2
    H, W = ml.shape[-2:]
    m = F.pad(ml.to(acc), (r, r, r, r), mode="replicate")
    rows = m[..., :, 0:W]
    for k in range(1, window):
        rows = rows + m[..., :, k:k + W]
    vol = rows[..., 0:H, :]
    for k in range(1, window):
        vol = vol + rows[..., k:k + H, :]
    return ml, vol


def first_argmax(vol):
    """Index of the first largest value along dim 1 (ascending scan with a strict >), [N,1,H,W]."""
    S = vol.shape[1]
    top = vol.max(dim=1, keepdim=True).values
    ar = torch.arange(S, device=vol.device).reshape(1, S, 1, 1)
    return torch.where(vol == top, ar, S).min(dim=1, keepdim=True).values


def peak_fit(vol, coords, interp, eps=1e-8, acc=torch.float64):
    """Specification steps 4-5 on a focus volume [N,S,H,W] and coords [N,S] -> dict(u, index, peak, hm, hp), all [N,1,H,W]."""
    assert interp in INTERPS
    v = vol.to(acc)
    N, S, H, W = v.shape
    u = coords.to(device=v.device, dtype=acc).reshape(N, S, 1, 1).expand(N, S, H, W)
    idx = first_argmax(v)
    im, ip = (idx - 1).clamp(min=0), (idx + 1).clamp(max=S - 1)
    f0, fm, fp = v.gather(1, idx), v.gather(1, im), v.gather(1, ip)
    u0, um, up = u.gather(1, idx), u.gather(1, im), u.gather(1, ip)
    hm, hp = u0 - um, up - u0
    if interp == "gaussian":
        e = float(np.float32(eps))                              # the kernel's eps is a float32
        a, b = torch.log1p((f0 - fm) / (fm + e)), torch.log1p((f0 - fp) / (fp + e))
    else:
        a, b = f0 - fm, f0 - fp
    den = 2.0 * (b * hm + a * hp)
    x = torch.where(den == 0, torch.zeros_like(den), (a * hp * hp - b * hm * hm) / torch.where(den == 0, torch.ones_like(den), den))
    x = torch.maximum(torch.minimum(x, torch.maximum(-hm, hp)), torch.minimum(-hm, hp))
    inner = (idx > 0) & (idx < S - 1)
    if interp == "none":
        inner = torch.zeros_like(inner)
    x = torch.where(inner, x, torch.zeros_like(x))
    return {"u": u0 + x, "index": idx.to(torch.int32), "peak": f0, "hm": hm, "hp": hp}


def gather_aif(stack, index):
    """stack [N,C,S,H,W], index [N,1,H,W] -> [N,C,H,W]: every pixel from its slice."""
    N, C, S, H, W = stack.shape
    return stack.gather(2, index.to(torch.int64).reshape(N, 1, 1, H, W).expand(N, C, 1, H, W)).squeeze(2)


def oracle(stack, coords, window, interp, eps=1e-8, acc=torch.float64):
    """The whole estimator: dict(u, index, peak, aif, volume, hm, hp)."""
    ml, vol = focus_volume(stack, window, acc)
    out = peak_fit(vol, coords, interp, eps, acc)
    out["volume"] = vol
    out["aif"] = gather_aif(stack.to(torch.float32), out["index"])
    return out


# ------------------------------------------------------------------ seeded inputs
def random_stack(N, C, S, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((N, C, S, H, W), generator=g, dtype=torch.float32)


def random_coords(N, S, seed):
    """[N,S] float32, non-uniform spacing; even rows increase, odd rows decrease (and are negative: the sign convention of the lenses)."""
    g = torch.Generator().manual_seed(seed)
    steps = 0.5 + torch.rand((N, S), generator=g, dtype=torch.float64)
    u = 1.0 / 3000.0 + torch.cumsum(steps, dim=1) * 2.0e-4
    for n in range(1, N, 2):
        u[n] = -u[n]
    return u.to(torch.float32)


BUILT = {"H": 48, "W": 64, "S": 8}
_BUILT = {}


def built_stack():
    """The recovery fixture (cached, treat as read-only): stack [1,3,8,48,64], coords [1,8] = linspace(1/600, 1/3000, 8) and the true
    depth [48,64] in mm - 1000 on the left half, 2000 on the right, plus 300 y / H.  Slice s is synth_rgb(48, 64, seed=3) under a
    per-pixel normalised 11 x 11 Gaussian of sigma = 0.3 + 2500 |1/depth - coords[s]| pixels, replicate padding."""
    if not _BUILT:
        from aadff.synth import synth_rgb
        H, W, S = BUILT["H"], BUILT["W"], BUILT["S"]
        img = torch.from_numpy(synth_rgb(H, W, seed=3)).to(torch.float64)
        coords = torch.linspace(1.0 / 600.0, 1.0 / 3000.0, S, dtype=torch.float64)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        depth = torch.where(xx < W // 2, 1000.0, 2000.0) + 300.0 * yy / H
        pad = F.pad(img[None], (5, 5, 5, 5), mode="replicate")[0]
        patches = pad.unfold(1, 11, 1).unfold(2, 11, 1)                                    # [3,H,W,11,11]
        k = torch.arange(-5, 6, dtype=torch.float64)
        rho = (k[:, None] ** 2 + k[None, :] ** 2).reshape(1, 1, 11, 11)
        slices = []
        for s in range(S):
            sigma = 0.3 + 2500.0 * (1.0 / depth - coords[s]).abs()
            w = torch.exp(-rho / (2.0 * sigma[..., None, None] ** 2))
            w = w / w.sum(dim=(-1, -2), keepdim=True)
            slices.append((patches * w[None]).sum(dim=(-1, -2)))
        _BUILT["v"] = (torch.stack(slices, dim=1)[None].to(torch.float32).contiguous(), coords.to(torch.float32)[None].contiguous(),
                       depth.to(torch.float32))
    return _BUILT["v"]


def recovery_error(u, peak, coords, depth):
    """|u* - 1/depth| in units of the slice spacing on the pixels with peak >= median(peak) -> (errors [K] float64, mask [H,W])."""
    spacing = float((coords[0, 1] - coords[0, 0]).abs())
    pk = peak.reshape(depth.shape).to(torch.float64)
    mask = pk >= pk.median()
    err = (u.reshape(depth.shape).to(torch.float64) - 1.0 / depth.to(torch.float64)).abs() / spacing
    return err[mask], mask


def nearest_slice(coords, depth):
    return (coords[0].to(torch.float64).reshape(-1, 1, 1) - 1.0 / depth.to(torch.float64)[None]).abs().argmin(dim=0)
