"""The oracle of the confidence-guided depth refinement (csrc/depth_refine.hip, aadff/refine.py): the specification as a
torch composition on the CPU, (2r+1)^2 shifted slices, in float64 or float32, built from differentiable torch ops so that autograd gives
the reference gradients.  Also the closed-form gather backward of the specification restated in torch, the seeded inputs of the GPU cases
and the recovery fixture.  Nothing here imports the code under test.

    c < 2^-30 counts as 0 (the threshold passes the gradient on: d_c is the formula at every pixel);
    w(p,q) = exp(max(-((dy^2 + dx^2) ks + sum_ch (g(p) - g(q))^2 kr), -64)) over the window clipped to the image;
    A = sum w c u,  D = sum w c  (a non-finite u under c = 0 is left out),  Wn = sum w;
    u' = A / D where D > 0, else u;   c' = D / Wn;   scale = sum w c |u| / D, the natural size of u'.
"""
import numpy as np
import torch
import torch.nn.functional as F

CMIN = 2.0 ** -30


def constants(channels, sigma_space, sigma_range):
    """(ks, kr): formed in float64, rounded to float32 (what the kernels are given), returned as Python floats."""
    return float(np.float32(1.0 / (2.0 * sigma_space ** 2))), float(np.float32(1.0 / (2.0 * sigma_range ** 2 * channels)))


def _shifts(H, W, r):
    """(dy, dx, the slices of p, the slices of q = p + (dy, dx), the padding that puts the p region back into H x W) of every tap."""
    for dy in range(-r, r + 1):
        y0, y1 = max(0, -dy), H - max(0, dy)
        if y1 <= y0:
            continue
        for dx in range(-r, r + 1):
            x0, x1 = max(0, -dx), W - max(0, dx)
            if x1 <= x0:
                continue
            yield (dy, dx, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx)), (x0, W - x1, y0, H - y1))


def _weight(g, dy, dx, P, Q, ks, kr):
    d = g[:, :, P[0], P[1]] - g[:, :, Q[0], Q[1]]
    return torch.exp((-((dy * dy + dx * dx) * ks + (d * d).sum(1, keepdim=True) * kr)).clamp_min(-64.0))


def effective(u, c):
    """(u, c) as the sums see them: c below the threshold is 0 (with the gradient passed on), a non-finite u under c = 0 is 0."""
    ce = c - (c * (c < CMIN)).detach()
    return torch.where((ce.detach() == 0) & ~torch.isfinite(u.detach()), torch.zeros_like(u), u), ce


def sums(u, c, g, radius, ks, kr):
    """A, D, Wn and sum w c |u| [N,1,H,W] of the specification in the dtype of the inputs."""
    H, W = u.shape[-2:]
    ue, ce = effective(u, c)
    cu, cabs = ce * ue, ce * ue.abs()
    A = D = Wn = S = 0
    for dy, dx, P, Q, pad in _shifts(H, W, radius):
        w = _weight(g, dy, dx, P, Q, ks, kr)
        A = A + F.pad(w * cu[:, :, Q[0], Q[1]], pad)
        D = D + F.pad(w * ce[:, :, Q[0], Q[1]], pad)
        S = S + F.pad(w * cabs[:, :, Q[0], Q[1]], pad)
        Wn = Wn + F.pad(w, pad)
    return A, D, Wn, S


def refine_step(u, c, g, radius, ks, kr, dtype=torch.float64):
    """One iteration -> dict(u, c, scale, some): u', c', sum w c |u| / D and the mask D > 0, in `dtype`."""
    u, c, g = (t.to(dtype) for t in (u, c, g))
    A, D, Wn, S = sums(u, c, g, radius, ks, kr)
    some = D.detach() > 0
    safe = torch.where(some, D, torch.ones_like(D))
    return {"u": torch.where(some, A / safe, u), "c": D / Wn, "scale": (S / safe).detach(), "some": some}


def refine(u, c, g, radius, sigma_space, sigma_range, iterations, dtype=torch.float64):
    ks, kr = constants(g.shape[1], sigma_space, sigma_range)
    for _ in range(iterations):
        o = refine_step(u, c, g, radius, ks, kr, dtype)
        u, c = o["u"], o["c"]
    return u, c


def grads(u, c, g, radius, ks, kr, g_u, g_c, dtype=torch.float64):
    """Autograd of refine_step for the cotangents g_u, g_c of u' and c' -> dict(d_u, d_c) in `dtype`."""
    uu, cc = u.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    o = refine_step(uu, cc, g, radius, ks, kr, dtype)
    d_u, d_c = torch.autograd.grad((o["u"], o["c"]), (uu, cc), (g_u.to(dtype), g_c.to(dtype)))
    return {"d_u": d_u, "d_c": d_c}


def closed_form_backward(u, c, g, radius, ks, kr, g_u, g_c, dtype=torch.float64):
    """The gather backward of the specification: alpha = gu' / D (0 where D = 0), beta = gc' / Wn,
    d_u(q) = c(q) sum_p w alpha(p) + [D(q) = 0] gu'(q),   d_c(q) = sum_p w (alpha(p) (u(q) - u'(p)) + beta(p)),   p over the window of q."""
    u, c, g, g_u, g_c = (t.to(dtype) for t in (u, c, g, g_u, g_c))
    H, W = u.shape[-2:]
    with torch.no_grad():
        A, D, Wn, _ = sums(u, c, g, radius, ks, kr)
        ue, ce = effective(u, c)
        some = D > 0
        safe = torch.where(some, D, torch.ones_like(D))
        alpha, beta = torch.where(some, g_u / safe, torch.zeros_like(D)), g_c / Wn
        uo = torch.where(some, A / safe, torch.zeros_like(D))
        S1 = S2 = 0
        for dy, dx, Q, Pp, pad in _shifts(H, W, radius):      # here the kept region is q and the shifted one p = q + (dy, dx)
            w = _weight(g, dy, dx, Q, Pp, ks, kr)
            al, up, be = (t[:, :, Pp[0], Pp[1]] for t in (alpha, uo, beta))
            S1 = S1 + F.pad(w * al, pad)
            S2 = S2 + F.pad(w * (al * (ue[:, :, Q[0], Q[1]] - up) + be), pad)
        return {"d_u": ce * S1 + torch.where(some, torch.zeros_like(D), g_u), "d_c": S2}


def case_inputs(N, C, H, W, radius, seed, nan=False, guide_scale=1.0):
    """Seeded float32 inputs of a case: signed u, a guide in [0, guide_scale), a confidence with about 30 % exact zeros, one value below
    the threshold and one block of zeros larger than the window (clipped to the image; it crosses a tile boundary of the kernel and
    touches the right border at the sizes the GPU tests use), with nan in u under a part of it when asked for; two cotangents."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(N, 1, H, W, generator=gen) * 0.7 + 0.3
    g = torch.rand(N, C, H, W, generator=gen) * guide_scale
    c = torch.rand(N, 1, H, W, generator=gen) + 0.01
    c = c * (torch.rand(N, 1, H, W, generator=gen) >= 0.3)
    b = 2 * radius + 4
    y0, x0 = min(10, H - b), W - b
    if y0 >= 0 and x0 >= 0:
        c[:, :, y0:y0 + b, x0:x0 + b] = 0
        if nan:
            u[:, :, y0:y0 + b // 2, x0:x0 + b] = float("nan")
    if H * W > 1:
        c[:, :, 0, 0] = 2.0 ** -31                           # below the threshold: zero
        if nan:
            u[:, :, 0, 0] = float("inf")
    else:
        c[0], c[1:] = 0.5, 0.0                               # one pixel: one image filters itself, the others pass through
    return {"u": u, "c": c, "g": g, "g_u": torch.randn(N, 1, H, W, generator=gen), "g_c": torch.randn(N, 1, H, W, generator=gen)}


def recovery_fixture():
    """48 x 64, seed 0, float64: a depth step of 1.0 at x = 32 on a ramp, a 3-channel guide with the same step, confidence 1 on the 8 x 8
    blocks with (x // 8 + y // 8) even and 0.01 elsewhere, input = truth + noise of 0.02 on the confident blocks and 0.5 elsewhere.
    -> dict(truth, guide, conf, inp, low, high, band) with the three masks [1,1,48,64]."""
    H, W = 48, 64
    gen = torch.Generator().manual_seed(0)
    x = torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, W).expand(1, 1, H, W)
    y = torch.arange(H, dtype=torch.float64).reshape(1, 1, H, 1).expand(1, 1, H, W)
    step = (x >= 32).to(torch.float64)
    truth = 1.0 + step + 0.2 * x / 64
    guide = 0.3 + 0.4 * step + 0.02 * (torch.rand(1, 3, H, W, generator=gen, dtype=torch.float64) - 0.5)
    high = ((x // 8 + y // 8) % 2) == 0
    conf = torch.where(high, 1.0, 0.01).to(torch.float64)
    inp = truth + torch.randn(1, 1, H, W, generator=gen, dtype=torch.float64) * torch.where(high, 0.02, 0.5)
    band = (x >= 30) & (x < 34)
    return {"truth": truth, "guide": guide, "conf": conf, "inp": inp, "low": ~high, "high": high, "band": band}


RECOVERY = dict(radius=4, sigma_space=3.0, sigma_range=0.1, iterations=2)


def recovery_errors(fx, out):
    """mean |error| of `out` on the low-confidence pixels, the confident ones and the four columns around the step."""
    e = (out.to(torch.float64) - fx["truth"]).abs()
    return float(e[fx["low"]].mean()), float(e[fx["high"]].mean()), float(e[fx["band"]].mean())


def check_recovery(fx, out, who):
    """The three conditions of the fixture; returns the figures."""
    raw = recovery_errors(fx, fx["inp"])
    got = recovery_errors(fx, out)
    print(f"{who}: raw low {raw[0]:.4f} high {raw[1]:.4f}; refined low {got[0]:.4f} high {got[1]:.4f} step band {got[2]:.4f}")
    assert got[0] <= 0.05 * raw[0], f"{who}: low-confidence error {got[0]:.4f} is above 0.05 x raw {raw[0]:.4f}"
    assert got[1] <= raw[1], f"{who}: confident error {got[1]:.4f} is above raw {raw[1]:.4f}"
    assert got[2] <= 0.02, f"{who}: step-band error {got[2]:.4f} is above 0.02"
    return raw, got
