"""GPU tests (run with `-m gpu` on an MI355X): the forward values of the per-pixel PSF gather (aadff_local_psf_render: the LDS-DMA, the
direct and the generic kernels of csrc/gather.hip) and of the thin-lens forward (csrc/thinlens.hip) against float64 on the CPU.  The gather is the yardstick of the
thin-lens and the fused PSF-network gather tests of tests/test_gpu_parity.py; here it is anchored itself.

tests/local_gather_common.py has the cases, the comparator (oracle.conv.local_psf_render in float64), the float32 restatement in the
kernels' order and the derived elementwise bound; tests/test_local_gather_host.py shows on the CPU that the comparators meet their own
conditions.  Every case asserts
  (a) every element within elementwise_bound = ks^2 * 2^-24 * sum|x w| + 2^-24 |out64| of float64, no element excluded;
  (b) rel_l2(got, oracle64) <= 4 x d32seq (4: the project's allowance for another order of the same float32 terms), through `margin`;
  (c) shape, dtype, finiteness.
No number here comes from the kernels under test.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import local_gather_common as lg                           # noqa: E402
import thinlens_grad_common as tc                          # noqa: E402
from aadff import ops                                      # noqa: E402,F401  (registers torch.ops.aadff)
from deeplens.psfnet import ThinLens                       # noqa: E402

DEV = "cuda:0"


def _run(img, psf, ks):
    out = torch.ops.aadff.local_psf_render(img.to(DEV), psf.to(DEV), ks)
    torch.cuda.synchronize()
    return out


def _misaligned(psf):
    """The same values on the device in storage that starts one float past a 16-byte boundary: a contiguous view, so the op keeps the
    pointer and the host code takes the direct form also where W % 4 == 0."""
    n = psf.numel()
    flat = torch.empty(n + 8, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + n].view(psf.shape)
    view.copy_(psf)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _check(tag, got, case, signed, margin):
    B, C, H, W, ks = case
    img, psf, out64, A, d32seq = lg.reference(case, signed)
    assert got.shape == (B, C, H, W) and got.dtype == torch.float32 and got.is_cuda                                  # (c)
    g = got.cpu()
    assert torch.isfinite(g).all()
    err = (g.double() - out64).abs()
    use = err / lg.elementwise_bound(ks * ks, A, out64)
    worst = int(use.argmax())
    e = lg.rel_l2(g, out64)
    print(f"\n{tag}: rel_l2 {e:.3e} d32seq {d32seq:.3e}; largest use of the elementwise bound {float(use.max()):.3f}")
    assert float(use.max()) <= 1.0, f"{tag}: element {worst} of {tuple(g.shape)} is {float(err.flatten()[worst]):.3e} from float64"  # (a)
    margin(f"local_gather {tag}", e, 4.0 * d32seq)                                                                    # (b)


@pytest.mark.parametrize("case", lg.CASES, ids=[lg.case_id(c) for c in lg.CASES])
def test_templated_kernels_against_float64(case, margin):
    img, psf = lg.reference(case)[:2]
    _check(lg.case_id(case), _run(img, psf, case[4]), case, False, margin)


@pytest.mark.parametrize("case", lg.GENERIC_CASES, ids=[lg.case_id(c) for c in lg.GENERIC_CASES])
def test_generic_kernel_against_float64(case, margin):
    B, C, H, W, ks = case
    img, psf, out64, A, d32seq = lg.reference(case)
    got = _run(img, psf, ks)
    if ks == 1:                                           # one fma with a zero accumulator: the rounded product, bit for bit
        assert torch.equal(got.cpu(), img * psf[..., 0, 0][:, None])
        w = torch.rand(psf.shape, generator=torch.Generator().manual_seed(3)) * 2.0 - 0.5          # not normalised: out != img
        assert torch.equal(_run(img, w, 1).cpu(), img * w[..., 0, 0][:, None])
        assert got.shape == (B, C, H, W) and got.dtype == torch.float32
        return
    _check(lg.case_id(case), got, case, False, margin)


def test_signed_psfs(margin):
    img, psf = lg.reference(lg.SIGNED_CASE, True)[:2]
    _check(lg.case_id(lg.SIGNED_CASE, True), _run(img, psf, lg.SIGNED_CASE[4]), lg.SIGNED_CASE, True, margin)


def test_lds_admission_rule_refuses_and_leaves_the_device_usable(margin):
    for case in lg.REFUSED_CASES:
        B, C, H, W, ks = case
        img = torch.zeros((B, C, H, W), device=DEV)
        psf = torch.zeros((B, H, W, ks, ks), device=DEV)
        with pytest.raises(RuntimeError, match="LDS"):
            torch.ops.aadff.local_psf_render(img, psf, ks)
        torch.cuda.synchronize()
        ok = (1, 3, 5, 20, 31)                            # a passing case right after the refusal
        _check(f"{lg.case_id(ok)} after refusing {lg.case_id(case)}", _run(*lg.reference(ok)[:2], ok[4]), ok, False, margin)


@pytest.mark.parametrize("ks", [5, 11])
def test_both_forms_on_the_same_inputs(ks, margin):
    """W % 4 == 0: the aligned call takes the LDS-DMA form, the misaligned PSF pointer the direct form.  Both meet (a) and (b); they
    need not be equal (the waves of the DMA form split the tap rows)."""
    case = (2, 3, 9, 132, ks)
    img, psf = lg.reference(case)[:2]
    a = _run(img, psf, ks)
    b = torch.ops.aadff.local_psf_render(img.to(DEV), _misaligned(psf), ks)
    torch.cuda.synchronize()
    _check(f"{lg.case_id(case)} dma", a, case, False, margin)
    _check(f"{lg.case_id(case)} direct (misaligned)", b, case, False, margin)
    print(f"ks {ks}: {int((a != b).sum())} of {a.numel()} elements differ between the two forms")
    # The misaligned call really took the direct form: that is the fmaf chain of the sequential restatement, whose steps (a float64 sum
    # rounded again to float32) differ from an fma only when the float64 sum falls on a float32 tie, about 2^-29 per step - fewer than
    # one of the 9504 x ks^2 steps here, where another summation order would move a large share of the elements.
    differ = float((b.cpu() != lg.reference_seq(case)).float().mean())
    print(f"ks {ks}: share of the direct form's elements that differ from the sequential restatement {differ:.2e}")
    assert differ <= 1e-3


def test_direct_form_equals_the_generic_kernel_bit_for_bit():
    """Direct and generic kernel are the same fmaf chain in the same tap order and nothing in the build allows reassociation: the first
    four channels of a five-channel image through the generic kernel equal the run-time-C direct form on img[:, :4], and the C = 3 and
    C = 1 instantiations on the matching slices."""
    case = (1, 5, 6, 70, 11)
    img, psf = lg.reference(case)[:2]
    x, p = img.to(DEV), psf.to(DEV)
    gen = _run(x, p, 11)
    assert torch.equal(gen[:, :4], _run(x[:, :4].contiguous(), p, 11))                 # W = 70: direct form, CN = 0
    assert torch.equal(gen[:, 1:4], _run(x[:, 1:4].contiguous(), p, 11))               # CN = 3
    assert torch.equal(gen[:, 4:5], _run(x[:, 4:5].contiguous(), p, 11))               # CN = 1
    assert torch.equal(gen[:, 0:2], _run(x[:, 0:2].contiguous(), p, 11))               # CN = 0 with C = 2


def test_repeatability():
    for case in ((2, 3, 9, 132, 11), (2, 3, 5, 40, 21)):
        img, psf = lg.reference(case)[:2]
        x, p = img.to(DEV), psf.to(DEV)
        assert torch.equal(_run(x, p, case[4]), _run(x, p, case[4])), case


# ---------------------------------------------------------------------------------------------------------------- thin lens
def _lens(case):
    foc_len, fnum, ks, ssize, sres = tc.lens_args(case)
    return ThinLens(foc_len=foc_len, fnum=fnum, kernel_size=ks, sensor_size=ssize, sensor_res=sres)


@pytest.mark.parametrize("case", lg.THIN_CASES, ids=[c[0] for c in lg.THIN_CASES])
def test_thinlens_forward_against_float64(case, margin):
    """thinlens_kernel (csrc/thinlens.hip), slice by slice, against the float64 oracle on every pixel that tc.keep_rows keeps (next to a jump of the
    cut or a kink a last-bit difference moves a whole ring of taps; nothing else is excluded): rel_l2 <= 4 x d32seq of thin_sequential32 on
    the same pixels."""
    img, depth, fds, keep, share, out64, seq, d32seq = lg.thin_reference(case)
    assert share <= tc.MAX_MASKED
    lens = _lens(case)
    x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
    got = torch.stack([lens.render(x, d, f[:, i]) for i in range(f.shape[1])], dim=2)
    torch.cuda.synchronize()
    assert got.shape == out64.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    g = got.cpu()
    e = lg.rel_l2(g[keep], out64[keep])
    print(f"\n{case[0]}: e_fwd {e:.3e} d32seq {d32seq:.3e}; distance from the float32 restatement {lg.rel_l2(g[keep], seq[keep]):.3e}; "
          f"excluded share {share:.5%}")
    margin(f"thinlens_forward {case[0]}", e, 4.0 * d32seq)


@pytest.mark.parametrize("shape", [(1, 3, 5, 131), (2, 4, 5, 68)], ids=["1x3x5x131", "2x4x5x68"])
def test_thinlens_in_focus_is_the_identity(shape):
    """Exactly in focus: coc 0 -> floor 0.1 px -> only the centre tap survives the cut -> out == img bit for bit."""
    N, C, H, W = shape
    img = torch.rand(shape, generator=torch.Generator().manual_seed(9)) * 4.0 - 1.0
    for ks in (11, 5):
        lens = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=ks, sensor_size=[24.0, 24.0], sensor_res=(64, 64))
        for sign in (-1.0, 1.0):
            depth = torch.full((N, 1, H, W), sign * 1500.0, device=DEV)
            out = lens.render(img.to(DEV), depth, torch.full((N,), sign * 1500.0, device=DEV))
            assert torch.equal(out.cpu(), img), (shape, ks, sign)
