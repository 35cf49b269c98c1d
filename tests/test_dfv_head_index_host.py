"""CPU: the index logic of the cost-volume head's backward (csrc/dfv_head.hip: axis_src, first_at_least, axis_range, axis_weight) restated
in float32 numpy, step for step, and held to two things the kernels rely on:

  * axis_range(j) is exactly the set of output indices whose axis_src reads cell j, at integer and odd ratios, and first_at_least needs
    at most two correcting steps from its estimate;
  * the two-stage gather through those ranges and weights (along x into [B,S,H,w], then along y) is the gradient torch's autograd gives
    for F.interpolate(..., mode='bilinear'): the remaining distance is the float32 rounding of the weights, bounded below.

This checks the algorithm the kernels implement, not their code; tests/test_gpu_dfv_head.py checks the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

f32 = np.float32
PAIRS = [(1, 1), (1, 7), (6, 23), (5, 19), (7, 10), (9, 37), (13, 54), (19, 76), (18, 18), (3, 96), (4, 128), (3, 1000), (40, 41), (23, 47),
         (29, 59), (120, 480), (160, 641), (15, 480)]


def axis_src(dst, scale, n):
    s = f32(f32(scale * f32(f32(dst) + f32(0.5))) - f32(0.5))
    s = f32(0) if s < 0 else s
    i0 = min(int(s), n - 1)
    return i0, min(i0 + 1, n - 1), f32(s - f32(i0))


def first_at_least(k, scale, n, out):
    if k <= 0:
        return 0, 0
    if k > n - 1:
        return out, 0
    guess = f32(f32(f32(f32(k) + f32(0.5)) / scale) - f32(0.5))
    x = 0 if guess < 0 else (int(guess) if guess < out else out)
    steps = 0
    while x > 0 and axis_src(x - 1, scale, n)[0] >= k:
        x, steps = x - 1, steps + 1
    while x < out and axis_src(x, scale, n)[0] < k:
        x, steps = x + 1, steps + 1
    return x, steps


def axis_range(j, scale, n, out):
    return first_at_least(j - 1, scale, n, out)[0], first_at_least(j + 1, scale, n, out)[0]


def axis_weight(i0, i1, lam, j):
    return f32((f32(1) - lam if i0 == j else f32(0)) + (lam if i1 == j else f32(0)))


@pytest.mark.parametrize("n,out", PAIRS, ids=["%d_to_%d" % p for p in PAIRS])
def test_ranges_invert_the_forward_index(n, out):
    scale = f32(f32(n) / f32(out))
    src = [axis_src(x, scale, n) for x in range(out)]
    assert all(a[0] <= b[0] for a, b in zip(src, src[1:])) and all(0 <= i0 <= i1 <= n - 1 and 0 <= lam <= 1 for i0, i1, lam in src)
    want = F.interpolate(torch.arange(n, dtype=torch.float32).reshape(1, 1, 1, n), [1, out], mode="bilinear").flatten()      # ATen's own indices
    got = torch.tensor([float((f32(1) - lam) * f32(i0) + lam * f32(i1)) for i0, i1, lam in src])
    assert float((got - want).abs().max()) <= 2.0 ** -22 * n
    for j in range(n):
        lo, hi = axis_range(j, scale, n, out)
        assert list(range(lo, hi)) == [x for x in range(out) if j in src[x][:2]], (j, lo, hi)
        assert hi > lo                                                     # upsampling: every cell is read
    assert max(first_at_least(k, scale, n, out)[1] for k in range(n + 1)) <= 2


@pytest.mark.parametrize("h,w,H,W", [(2, 3, 7, 1000), (5, 40, 7, 41), (9, 13, 37, 54), (23, 29, 47, 59), (3, 4, 96, 128), (1, 1, 5, 7)])
def test_two_stage_gather_is_the_gradient_of_the_interpolation(h, w, H, W):
    g = torch.Generator().manual_seed(h * 1000 + W)
    dz = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    c = torch.zeros(2, 3, h, w, dtype=torch.float64, requires_grad=True)
    (F.interpolate(c, [H, W], mode="bilinear") * dz).sum().backward()
    sh, sw = f32(f32(h) / f32(H)), f32(f32(w) / f32(W))
    t = np.zeros((2, 3, H, w))
    for j in range(w):
        for x in range(*axis_range(j, sw, w, W)):
            t[:, :, :, j] += float(axis_weight(*axis_src(x, sw, w), j)) * dz[:, :, :, x].numpy()
    d = np.zeros((2, 3, h, w))
    for i in range(h):
        for y in range(*axis_range(i, sh, h, H)):
            d[:, :, i, :] += float(axis_weight(*axis_src(y, sh, h), i)) * t[:, :, y, :]
    err = float(np.linalg.norm(d - c.grad.numpy()) / np.linalg.norm(c.grad.numpy()))
    # a float32 weight lambda = src - i0 carries the rounding of src, at most about 1.5 ulp of the largest source index, relative to
    # weights of order 1; the sums are float64 here
    assert err <= 2.0 * max(h, w) * 2.0 ** -24, err
