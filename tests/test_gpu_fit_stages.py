"""GPU tests (run with `-m gpu` on an MI355X): every stored stage of the bf16 fit step of the PSF network (csrc/mlp_train.hip through
aadff/mlp_fit.py: gemm_nt_tile with its four epilogues, fit_chain_kernel, fit_dw_all_kernel, fit_head_kernel, fit_adamw_kernel) and
the fp32 leg's kernels of csrc/optim.hip, against float64 on the CPU.

tests/fit_common.py has the reference, the bounds and the checkers (DESIGN.md §4.5.1 derives them); tests/test_fit_host.py shows on the
CPU that a float32 emulation passes them and that planted errors do not.  The kernels of mlp_train.hip are driven only through
`FusedFit`, with its own buffers and leading dimensions; every comparison starts from what the kernel itself stored for the stage
before; bf16 outputs are judged element by element by an interval that lets a rounding tie fall either way.  No number here comes
from the kernels under test.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fit_common as fc                                    # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff.mlp_fit import FusedFit, supported              # noqa: E402

DEV = "cuda:0"
LR0, T_MAX = 1e-3, 20
BETAS, EPS, WD = FusedFit.BETAS, FusedFit.EPS, FusedFit.WD


def _module(case):
    """A module with a `.net` Sequential: Linear + ReLU ... Linear + Sigmoid with the case's weights and biases."""
    mods = []
    for l, (W, b) in enumerate(zip(case.W, case.b)):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        mods += [lin, torch.nn.Sigmoid() if l == len(case.W) - 1 else torch.nn.ReLU()]
    m = torch.nn.Module()
    m.net = torch.nn.Sequential(*mods).to(DEV)
    return m


def _fit(case, chain_env, monkeypatch):
    net = _module(case)
    assert supported(net, case.B)
    monkeypatch.setenv("AADFF_FIT_CHAIN", chain_env)
    fit = FusedFit(net, LR0, T_MAX, case.B, torch.device(DEV))
    assert fit.chain == (chain_env == "1" and 2 <= fit.L <= _abi.FIT_MAX_LAYERS)
    return fit


def _snapshot(fit, case, grad, pred):
    """Everything the step stored, on the CPU.  Chain form: the scratch is cut at the descriptor's offsets, which must tile it."""
    cpu = lambda t: t.detach().cpu()
    L, ldb, widths = fit.L, fit.ldb, [fit.K[0]] + fit.N
    assert widths == case.widths and fit.bs == case.B
    if fit.chain:
        scr, d, used = cpu(fit.scratch16), fit.net_desc, 0
        XT, dZT = [], [None]
        for l in range(L):
            n = fc.up(widths[l], 4) * ldb
            XT.append(scr[d.off_xt[l]:d.off_xt[l] + n].view(-1, ldb))
            used += n
        for l in range(1, L + 1):
            n = fc.up(widths[l], 4) * ldb
            dZT.append(scr[d.off_dzt[l]:d.off_dzt[l] + n].view(-1, ldb))
            used += n
        assert used == scr.numel()
        X = dZ = None
    else:
        X, XT = [cpu(t) for t in fit.X], [cpu(t) for t in fit.XT[:L]]
        dZ, dZT = [None] + [cpu(t) for t in fit.dZ[1:]], [None] + [cpu(t) for t in fit.dZT[1:]]
        assert not bool(fc.bits(cpu(fit.XT[L])).any())                  # the logits have no stored transpose: never written
    return fc.new_snap(chain=fit.chain, B=fit.bs, widths=widths, inp=cpu(fit.inp), target=cpu(fit.psf), pred=cpu(pred), flat=cpu(fit.flat),
                       grad=cpu(grad), w_off=fit.w_off, b_off=fit.b_off, p16=cpu(fit.p16), dst=cpu(fit.dst), dst_t=cpu(fit.dst_t),
                       XT=XT, dZT=dZT, X=X, dZ=dZ)


def _step(fit, case):
    grad, pred = fit.gradients(case.inp.to(DEV), case.target.to(DEV))
    torch.cuda.synchronize()
    snap = _snapshot(fit, case, grad, pred)
    assert torch.equal(snap.inp, case.inp) and torch.equal(snap.target, case.target)
    assert torch.equal(snap.flat, torch.cat([t.reshape(-1) for W, b in zip(case.W, case.b) for t in (W, b)]))
    return snap


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("name", list(fc.CASES) + ["one_layer"])
def test_fit_stages_against_float64(name, chain, monkeypatch, margin):
    """Cases A-G of DESIGN.md §4.5.1 and the one-layer network (Linear + Sigmoid: the layer form under either setting), both settings
    of AADFF_FIT_CHAIN: stages 1-5, then a second run that must repeat the first bit for bit except in the bias gradients."""
    widths, B = fc.CASES[name] if name in fc.CASES else fc.ONE_LAYER
    case = fc.make_case(widths, B)
    fit = _fit(case, chain, monkeypatch)
    snap = _step(fit, case)
    fc.check_all(snap, margin, tag=f"fit {name} AADFF_FIT_CHAIN={chain} ({'chain' if fit.chain else 'layers'}): ")
    assert fc.same_but_bias_gradients(snap, _step(fit, case)) == []


@pytest.mark.parametrize("chain", ["1", "0"])
def test_saturated_head_gives_exact_zeros(chain, monkeypatch):
    """Case B with the last bias at -100: every logit is below -89 (by the float64 reference), where exp(-z) overflows fp32, so the
    sigmoid is 0, the row sum is clamped at 1e-12 and prediction and gradients are exactly 0 and finite, as F.normalize gives."""
    widths, B = fc.CASES["B"]
    case = fc.make_case(widths, B)
    case.b[-1].fill_(-100.0)
    snap = _step(_fit(case, chain, monkeypatch), case)
    fc.check_input(snap)
    _, (z_lo, z_hi, z) = fc.check_forward(snap)
    assert float(z_hi.max()) <= -89.0
    assert torch.isfinite(snap.pred).all() and torch.isfinite(snap.grad).all()
    assert not bool(snap.pred.ne(0).any())
    for l in range(1, snap.L + 1):
        assert not bool(fc.dz(snap, l).ne(0).any()), l
    assert not bool(snap.grad.ne(0).any())


@pytest.mark.parametrize("chain", ["1", "0"])
def test_schedule_scalars_after_a_whole_step(chain, monkeypatch):
    """`scal` and `step_dev` after forward + backward + optimiser with the device counter at t: the float64 closed form within 1 ulp."""
    widths, B = fc.CASES["D"]
    case = fc.make_case(widths, B)
    fit = _fit(case, chain, monkeypatch)
    fit.inp.copy_(case.inp)
    fit.psf.copy_(case.target)
    for t in (0, 1, T_MAX - 1, T_MAX, T_MAX + 5):
        fit.step_dev.fill_(t)
        fit._body()
        torch.cuda.synchronize()
        assert int(fit.step_dev.item()) == t + 1
        fc.check_scal(fit.scal.cpu().numpy(), t, LR0, T_MAX, *BETAS, WD)
        assert not bool(fit.grad.ne(0).any())


def _moments(n, seed):
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(n, generator=g) * 1e-3
    grad[::7] = 0.0
    return grad, torch.randn(n, generator=g) * 1e-3, (torch.randn(n, generator=g) * 1e-3) ** 2


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("t", [3, T_MAX])
def test_fit_adamw_kernel_in_isolation(t, chain, monkeypatch, margin):
    """fit_adamw_kernel through FusedFit._adamw on case B's parameters, with grad, m, v, flat and scal set here: p, m, v within
    4 x d32 of float64, grad cleared, both bf16 copies refreshed from the kernel's own p; at t >= T no parameter moves by a bit."""
    widths, B = fc.CASES["B"]
    case = fc.make_case(widths, B)
    fit = _fit(case, chain, monkeypatch)
    grad, m, v = _moments(fit.n, 11)
    p = fit.flat.cpu().clone()
    scal = fc.scal_closed_form(t, LR0, T_MAX, *BETAS, WD).astype(np.float32)
    fit.grad.copy_(grad)
    fit.m.copy_(m)
    fit.v.copy_(v)
    fit.scal.copy_(torch.from_numpy(scal))
    fit._adamw(_abi.stream_ptr(fit.dev))
    torch.cuda.synchronize()
    after = (fit.flat.cpu(), fit.grad.cpu(), fit.m.cpu(), fit.v.cpu())
    fc.check_adamw((p, grad, m, v), after, scal, *BETAS, EPS, margin, tag=f"fit_adamw t={t} AADFF_FIT_CHAIN={chain}: ")
    assert not bool(after[1].view(torch.int32).any())
    if t >= T_MAX:
        assert torch.equal(after[0].view(torch.int32), p.view(torch.int32))
    h, p16, dst_t = after[0].to(torch.bfloat16), fit.p16.cpu(), fit.dst_t.cpu()
    assert torch.equal(fc.bits(p16[fit.dst.cpu().long()]), fc.bits(h))
    assert torch.equal(fc.bits(p16[dst_t[dst_t >= 0].long()]), fc.bits(h[dst_t >= 0]))


# ---------------------------------------------------------------------------------------------------------------------
# csrc/optim.hip: plain dense tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_relu_bwd_bias_against_float64(bf16, margin):
    """aadff_relu_bwd_bias: dz = dy where y > 0 (0, -0.0 and negatives are masked) exactly; db = column sums within M u sum |dz|
    (fp32) or by the interval rule (bf16, share pooled over the shapes)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    pool, worst = fc._Pool(), 0.0
    for M in (1, 63, 65, 200):
        for N in (1, 3, 5, 121, 256):
            g = torch.Generator().manual_seed(M * 1000 + N)
            dy = torch.randn(M, N, generator=g).to(dt)
            y = torch.randn(M, N, generator=g).to(dt)
            y.view(-1)[0::5] = 0.0
            y.view(-1)[1::5] = -0.0
            dz = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            db = torch.full((N,), float("nan"), dtype=dt, device=DEV)
            d_dy, d_y = dy.to(DEV), y.to(DEV)
            _abi.call("aadff_relu_bwd_bias", _abi.ptr(d_dy), _abi.ptr(d_y), _abi.ptr(dz), _abi.ptr(db), M, N, int(bf16), _abi.stream_ptr())
            torch.cuda.synchronize()
            want = torch.where(y.double() > 0, dy.double(), torch.zeros((), dtype=torch.float64))
            assert torch.equal(dz.cpu().double(), want), (M, N)
            v, d = want.sum(0), M * fc.U * want.abs().sum(0)
            if bf16:
                fc.interval("dw", f"db of relu_bwd_bias M={M} N={N}", db.cpu().double(), v, d, pool)
            else:
                assert torch.isfinite(db).all()
                worst = max(worst, fc.ratio((db.cpu().double() - v).abs(), d))
    if bf16:
        margin("relu_bwd_bias bf16: db share", pool.share(), fc.SHARE_CAP)
    else:
        margin("relu_bwd_bias fp32: db err/bound", worst, 1.0)


def _head_inputs(B, N):
    g = torch.Generator().manual_seed(B * 1000 + N)
    z = (torch.rand(B, N, generator=g) * 2 - 1) * 6
    t = torch.rand(B, N, generator=g)
    return z, t / t.sum(-1, keepdim=True)


def _head(z, t):
    B, N = z.shape
    pred = torch.full((B, N), float("nan"), device=DEV)
    dz = torch.full((B, N), float("nan"), dtype=z.dtype, device=DEV)
    d_z, d_t = z.to(DEV), t.to(DEV)
    _abi.call("aadff_psfnet_head_loss_grad", _abi.ptr(d_z), _abi.ptr(d_t), _abi.ptr(pred), _abi.ptr(dz), B, N,
              int(z.dtype == torch.bfloat16), _abi.stream_ptr())
    torch.cuda.synchronize()
    return pred.cpu(), dz.cpu()


def test_head_loss_grad_bf16_against_float64(margin):
    """aadff_psfnet_head_loss_grad, bf16: stage 3 on dense tensors, shares pooled over the shapes; then B = 3 with a middle row of
    logits -100, which must give exact zeros and leave its neighbours inside the bounds."""
    pools = {"sigmoid": fc._Pool(), "dz": fc._Pool()}
    for B in (1, 3):
        for N in (1, 64, 65, 121, 128):
            z, t = _head_inputs(B, N)
            z = z.to(torch.bfloat16)
            pred, dz = _head(z, t)
            fc.check_head_values(z.double(), z.double(), z.double(), pred.double(), t.double(), dz.double(), B, True, margin,
                                 tag=f"head_loss_grad bf16 B={B} N={N}: ", pools=pools)
    z, t = _head_inputs(3, 121)
    z = z.to(torch.bfloat16)
    z[1] = -100.0
    pred, dz = _head(z, t)
    assert not bool(pred[1].ne(0).any()) and not bool(dz[1].ne(0).any())
    keep = [0, 2]
    fc.check_head_values(z[keep].double(), z[keep].double(), z[keep].double(), pred[keep].double(), t[keep].double(), dz[keep].double(), 3, True,
                         margin, tag="head_loss_grad bf16 beside a saturated row: ", pools=pools)
    fc.judge_head_pools(pools, margin, tag="head_loss_grad bf16: ")


def _head64(z, t, B):
    s = torch.sigmoid(z.double())
    S = s.sum(-1, keepdim=True).clamp_min(1e-12)
    pred = s / S
    g = 2.0 * (pred - t.double()) / (B * z.shape[1])
    return pred, (g - (g * pred).sum(-1, keepdim=True)) / S * s * (1 - s)


def test_head_loss_grad_fp32_against_float64(margin):
    """aadff_psfnet_head_loss_grad, fp32 (the sigmoid is not rounded): pred and dz within 4 x d32 + 2^-20 of float64 in relative L2,
    d32 being the same arithmetic in float32 on the CPU and 2^-20 the derived error of the hardware exponential for |z| <= 16.
    N = 1 has pred = 1 and a gradient that is exactly 0 in float64, so no relative measure: there |dz| stays within stage 3's
    elementwise bound (N + 8) u (|g| + sum |g pred|) s (1 - s) / S.  Then B = 3 with a row of logits -100: exact zeros."""
    for B in (1, 3):
        for N in (1, 64, 65, 121, 128):
            z, t = _head_inputs(B, N)
            pred, dz = _head(z, t)
            p64, dz64 = _head64(z, t, B)
            p32, dz32 = fc.head32(z, t, B, rounded=False)
            assert torch.isfinite(pred).all() and torch.isfinite(dz).all()
            tag = f"head_loss_grad fp32 B={B} N={N}: "
            margin(tag + "pred rel_l2", fc.rel_l2(pred, p64), 4 * fc.rel_l2(p32, p64) + 2.0 ** -20)
            if N == 1:
                _, d = fc.head_terms(pred.double(), t.double(), torch.sigmoid(z.double()), B)
                margin(tag + "|dz| / bound", fc.ratio(dz.double().abs(), d), 1.0)
            else:
                margin(tag + "dz rel_l2", fc.rel_l2(dz, dz64), 4 * fc.rel_l2(dz32, dz64) + 2.0 ** -20)
    z, t = _head_inputs(3, 121)
    z[1] = -100.0
    pred, dz = _head(z, t)
    assert not bool(pred[1].ne(0).any()) and not bool(dz[1].ne(0).any())
    p64, dz64 = _head64(z, t, 3)
    p32, dz32 = fc.head32(z, t, 3, rounded=False)
    for k in (0, 2):
        margin(f"head_loss_grad fp32 beside a saturated row: pred[{k}] rel_l2", fc.rel_l2(pred[k], p64[k]), 4 * fc.rel_l2(p32[k], p64[k]) + 2.0 ** -20)
        margin(f"head_loss_grad fp32 beside a saturated row: dz[{k}] rel_l2", fc.rel_l2(dz[k], dz64[k]), 4 * fc.rel_l2(dz32[k], dz64[k]) + 2.0 ** -20)


@pytest.mark.parametrize("with_copy", [False, True], ids=["no-copy", "bf16-copy"])
@pytest.mark.parametrize("grad_bf16", [False, True], ids=["fp32-grad", "bf16-grad"])
@pytest.mark.parametrize("n", [1, 257, 1048579])
def test_adamw_step_against_float64(n, grad_bf16, with_copy, margin):
    """aadff_adamw_step: the schedule scalars within 1 ulp of the closed form, the counter advanced, p, m, v within 4 x d32 of float64
    from the kernel's own scalars, the bf16 copy the rounding of the kernel's own p.  n = 1 048 579 makes the grid, capped at 4096
    blocks of 256, stride a second time; t >= T leaves the parameters untouched."""
    for t in (3, T_MAX):
        grad, m, v = _moments(n, n + t)
        g = torch.Generator().manual_seed(n)
        p = torch.randn(n, generator=g)
        if grad_bf16:
            grad = grad.to(torch.bfloat16)
        dp, dg, dm, dv = (x.to(DEV) for x in (p, grad, m, v))
        p16 = torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV) if with_copy else None
        step = torch.full((1,), t, dtype=torch.int32, device=DEV)
        scal = torch.zeros(4, device=DEV)
        _abi.call("aadff_adamw_step", _abi.ptr(dp), _abi.ptr(dg), int(grad_bf16), _abi.ptr(dm), _abi.ptr(dv), _abi.ptr(p16), n, _abi.ptr(step),
                  _abi.ptr(scal), C.c_float(LR0), T_MAX, C.c_float(BETAS[0]), C.c_float(BETAS[1]), C.c_float(EPS), C.c_float(WD), _abi.stream_ptr())
        torch.cuda.synchronize()
        assert int(step.item()) == t + 1
        fc.check_scal(scal.cpu().numpy(), t, LR0, T_MAX, *BETAS, WD)
        fc.check_adamw((p, grad, m, v), (dp.cpu(), None, dm.cpu(), dv.cpu()), scal.cpu().numpy(), *BETAS, EPS, margin,
                       tag=f"adamw_step n={n} t={t} {'bf16' if grad_bf16 else 'fp32'} grad{' + copy' if with_copy else ''}: ")
        assert torch.equal(dg.cpu().view(torch.int16), grad.view(torch.int16))                      # the gradient is only read
        if t >= T_MAX:
            assert torch.equal(dp.cpu().view(torch.int32), p.view(torch.int32))
        if with_copy:
            assert torch.equal(fc.bits(p16.cpu()), fc.bits(dp.cpu().to(torch.bfloat16)))
