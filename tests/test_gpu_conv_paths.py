"""GPU tests (run with `-m gpu` on an MI355X): every instantiation of the patch convolution (csrc/conv.hip: conv_psf_map_kernel,
_generic_kernel, _mfma_kernel, _toeplitz_wide_kernel, _sbatch_kernel, _blk_kernel, _blkw_kernel) that an argument or a switch can reach,
against float64 on the CPU.

tests/conv_paths_common.py has the case table (each case built for one instantiation, named by `dispatch`, an independent restatement
of the rule of conv_plan, csrc/conv_plan.cpp), the comparator (oracle.conv.render_psf_map in float64, slice by slice) and the derived
bounds; tests/test_conv_paths_host.py shows on the CPU that the bounds are attainable and reject planted errors, that the table reaches
all 96 instantiations that are not TIMED, and that the library's own plan (aadff_conv_plan_describe) names the instantiation `dispatch`
names, for every case here and on a sweep of the rule's thresholds.  profiles/conv_paths_coverage.md is the kernel trace of this module.
Every case asserts
  (a) every element within the elementwise bound of its family (plain fp32 or matrix cores), no element excluded;
  (b) plain-fp32 kernels: rel_l2(got, oracle64) <= 4 x d32seq, through `margin`; matrix-core kernels report it;
  (c) every pixel written: the call goes through _abi.call into an output pre-filled with a sentinel, none survives;
  (d) shape, dtype, finiteness.
The switches are set with monkeypatch.setenv: the library reads them at every launch.  No number here comes from the kernels under test.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_paths_common as cp                             # noqa: E402
from aadff import _abi                                     # noqa: E402

DEV = "cuda:0"


def _run(c, r, monkeypatch):
    """The case through its entry point: float32 [B,C,S,H,W] on the CPU, after the sentinel check."""
    for k in cp.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    st = _abi.stream_ptr(torch.device(DEV))
    img, maps = r.img.to(DEV), r.maps.to(DEV)
    B, Cn, S, H, W, g, ks = c.B, c.C, c.S, c.H, c.W, c.grid, c.ks
    if c.entry == "strided":                               # slices as every k-th [C,H,W] unit of a larger buffer, one unit in
        assert B == 1
        k = 2
        units = torch.full((S * k + 2, Cn, H, W), cp.SENTINEL, device=DEV)
        _abi.call("aadff_render_psf_map_stack_strided", _abi.ptr(img), _abi.ptr(maps), C.c_void_p(units.data_ptr() + 4 * Cn * H * W),
                  H * W, k * Cn * H * W, 1, Cn, S, H, W, g, ks, st)
        torch.cuda.synchronize()
        keep = torch.ones(units.shape[0], dtype=torch.bool)
        keep[1:1 + S * k:k] = False
        assert bool((units[keep.to(DEV)] == cp.SENTINEL).all()), "wrote outside its planes"
        out = units[1:1 + S * k:k].permute(1, 0, 2, 3)[None].contiguous()
    else:
        out = torch.full((B, Cn, S, H, W), cp.SENTINEL, device=DEV)
        if c.entry == "stack":
            _abi.call("aadff_render_psf_map_stack", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), B, Cn, S, H, W, g, ks, st)
        elif c.entry == "map":
            _abi.call("aadff_render_psf_map", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), B, Cn, H, W, g, ks, st)
        elif c.entry == "psf":
            _abi.call("aadff_render_psf", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), B, Cn, H, W, ks, st)
        else:
            assert c.entry == "layered"
            _abi.call("aadff_render_psf_map_stack_layered", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(r.lidx.to(DEV)), _abi.ptr(out), B, Cn, S, c.L,
                      H, W, g, ks, st)
        torch.cuda.synchronize()
    for k in c.env:
        monkeypatch.delenv(k)
    got = out.cpu()
    left = int((got == cp.SENTINEL).sum())
    assert left == 0, f"{c.id}: {left} of {got.numel()} elements were never written"                                   # (c)
    return got


def _check(c, got, r, margin):
    name, family = cp.dispatch(c)
    use, worst, rel = cp.compare(c, got, r)                                                                             # (d) inside
    print(f"\n{c.id} [{name}]: largest use of the elementwise bound {use:.3f}; rel_l2 {rel:.2f} x d32seq ({r.d32seq:.3e})")
    err = float((got.double() - r.out64).abs().flatten()[worst])
    assert use <= 1.0, f"{c.id} [{name}]: element {worst} of {tuple(got.shape)} is {err:.3e} from float64, {use:.2f} x its bound"   # (a)
    if family in cp.PLAIN:
        margin(f"conv_paths {c.id}", rel * r.d32seq, 4.0 * r.d32seq)                                                    # (b)


@pytest.mark.parametrize("c", cp.TABLE, ids=[c.id for c in cp.TABLE])
def test_instantiation_against_float64(c, margin, monkeypatch):
    r = cp.reference(c)
    _check(c, _run(c, r, monkeypatch), r, margin)


def test_out_of_range_wave_counts_are_ignored(margin, monkeypatch):
    """AADFF_CONV_NW = 9 and = x are not wave counts: the default pick (4 waves for 7 slices) comes back bit for bit."""
    r = cp.reference(cp.NW_DEFAULT)
    want = _run(cp.NW_DEFAULT, r, monkeypatch)
    _check(cp.NW_DEFAULT, want, r, margin)
    for c in cp.NW_IGNORED:
        assert torch.equal(_run(c, cp.reference(c), monkeypatch), want), c.id


def test_ks1_is_the_rounded_product(monkeypatch):
    """ks 1 (generic kernel): one fma with a zero accumulator."""
    for c in (c for c in cp.TABLE if c.ks == 1):
        r = cp.reference(c)
        hb, wb = cp._bounds(c.H, c.grid), cp._bounds(c.W, c.grid)
        w = r.maps[:, :, [max(i for i in range(c.grid) if hb[i] <= y) for y in range(c.H)]][:, :, :, [max(j for j in range(c.grid) if wb[j] <= x) for x in range(c.W)]]
        assert torch.equal(_run(c, r, monkeypatch), r.img[:, :, None] * w.permute(1, 0, 2, 3)[None])
