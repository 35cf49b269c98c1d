"""CPU: the backward entry points of the image-space operators (csrc/conv_bwd.hip, csrc/gather.hip) validate their arguments before any HIP
call, the workspace query is host arithmetic, and aadff.diffrender imports without a GPU."""
import ctypes as C

import pytest
import torch

from aadff import _abi

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first


def _err(lib):
    return lib.aadff_last_error()


def test_map_bwd_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_render_psf_map_stack_bwd
    big = C.c_size_t(1 << 40)
    assert f(None, P8, P8, P8, P8, P8, big, 1, 3, 1, 64, 64, 2, 3, None) == -1 and b"NULL" in _err(lib)
    assert f(P8, P8, None, P8, P8, P8, big, 1, 3, 1, 64, 64, 2, 3, None) == -1 and b"NULL" in _err(lib)
    assert f(P8, P8, P8, None, None, P8, big, 1, 3, 1, 64, 64, 2, 3, None) == -1 and b"d_img" in _err(lib) and b"d_psf" in _err(lib)
    assert f(P8, P8, P8, P8, P8, P8, big, 1, 3, 1, 64, 64, 2, 4, None) == -1 and b"odd" in _err(lib)
    assert f(P8, P8, P8, P8, P8, P8, big, 1, 3, 1, 640, 640, 100, 3, None) == -1 and b"grid" in _err(lib)
    assert f(P8, P8, P8, P8, P8, P8, big, 1, 3, 1, 64, 64, 2, 53, None) == -1 and b"ks" in _err(lib)
    assert f(P8, P8, P8, P8, P8, P8, big, 1, 3, 1, 4, 64, 2, 11, None) == -1 and b"pad" in _err(lib)       # the forward's reflect-padding condition
    assert f(P8, P8, P8, P8, P8, P8, big, 1, 3, 0, 64, 64, 2, 3, None) == -1 and b"empty" in _err(lib)
    # d_psf asked for: the workspace must be there and large enough
    need = C.c_size_t(0)
    assert lib.aadff_render_psf_map_stack_bwd_workspace(1, 3, 1, 64, 64, 2, 3, C.byref(need)) == 0 and need.value > 0
    assert f(P8, P8, P8, P8, P8, P8, C.c_size_t(need.value - 4), 1, 3, 1, 64, 64, 2, 3, None) == -1 and b"workspace" in _err(lib)
    assert f(P8, P8, P8, P8, P8, None, C.c_size_t(need.value), 1, 3, 1, 64, 64, 2, 3, None) == -1 and b"workspace" in _err(lib)


def test_local_bwd_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_local_psf_render_bwd
    assert f(P8, None, P8, P8, P8, 1, 3, 16, 16, 5, None) == -1 and b"NULL" in _err(lib)
    assert f(P8, P8, P8, None, None, 1, 3, 16, 16, 5, None) == -1 and b"d_img" in _err(lib) and b"d_psf" in _err(lib)
    assert f(P8, P8, P8, P8, P8, 1, 3, 16, 16, 4, None) == -1 and b"ks" in _err(lib)
    assert f(P8, P8, P8, P8, P8, 1, 3, 16, 16, 53, None) == -1 and b"ks" in _err(lib)
    assert f(P8, P8, P8, P8, P8, 0, 3, 16, 16, 5, None) == -1 and b"empty" in _err(lib)
    # what the forward rejects, the backward rejects the same way: same return code and message
    g = lib.aadff_local_psf_render
    for args in ((1, 3, 16, 16, 51), (1, 3, 70000, 16, 5)):
        rc_f = g(P8, P8, P8, *args, None)
        msg_f = _err(lib)
        rc_b = f(P8, P8, P8, P8, P8, *args, None)
        assert rc_f == rc_b == -1 and _err(lib) == msg_f


def test_workspace_query():
    lib = _abi.load_library()
    q = lib.aadff_render_psf_map_stack_bwd_workspace

    def ws(B, S, H=256, W=256, grid=11, ks=11):
        n = C.c_size_t(0)
        assert q(B, 3, S, H, W, grid, ks, C.byref(n)) == 0
        return n.value

    assert ws(1, 1) > 0
    assert ws(1, 1) <= ws(1, 2) <= ws(1, 10) and ws(1, 1) < ws(1, 10)
    assert ws(1, 3) <= ws(2, 3) <= ws(5, 3) and ws(1, 3) < ws(5, 3)
    # one slab of S * C * (grid ks)^2 floats per 32 x 32 tile of a patch and batch item: 1024^2 at grid 11 has 94-pixel patches -> 3 x 3 tiles
    assert ws(1, 10, 1024, 1024) == 9 * 10 * 3 * 121 * 121 * 4
    n = C.c_size_t(0)
    assert q(1, 3, 1, 64, 64, 2, 4, C.byref(n)) == -1 and b"odd" in _err(lib)
    assert q(1, 3, 1, 64, 64, 2, 3, None) == -1 and b"bytes" in _err(lib)


def test_diffrender_imports_without_gpu():
    import aadff.diffrender as dr
    for name in ("render_psf", "render_psf_map", "render_psf_map_stack", "local_psf_render", "local_psf_render_high_res"):
        assert callable(getattr(dr, name))
    for op in ("render_psf_map_stack_bwd", "local_psf_render_bwd", "render_psf_map_stack_diff", "local_psf_render_diff"):
        assert hasattr(torch.ops.aadff, op)


def test_empty_inputs_stay_differentiable():
    """An empty batch / an empty slice loop needs no kernel (and no GPU): empty output, zero gradients of the inputs' shapes."""
    import aadff.diffrender as dr
    x, m = torch.rand(0, 3, 16, 16, requires_grad=True), torch.rand(3, 6, 6, requires_grad=True)
    out = dr.render_psf_map(x, m, 2)
    assert out.shape == (0, 3, 16, 16) and out.requires_grad
    out.sum().backward()
    assert x.grad.shape == x.shape and m.grad.shape == m.shape and m.grad.abs().max().item() == 0
    x, ms = torch.rand(2, 3, 16, 16, requires_grad=True), torch.rand(0, 3, 6, 6, requires_grad=True)
    out = dr.render_psf_map_stack(x, ms, 2)
    assert out.shape == (2, 3, 0, 16, 16)
    out.sum().backward()
    assert x.grad.abs().max().item() == 0 and ms.grad.shape == ms.shape
    x, p = torch.rand(0, 3, 8, 8, requires_grad=True), torch.rand(0, 8, 8, 3, 3, requires_grad=True)
    out = dr.local_psf_render(x, p, kernel_size=3)
    out.sum().backward()
    assert out.shape == x.shape and x.grad.shape == x.shape and p.grad.shape == p.shape


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is visible: the no-GPU refusal cannot be seen (tests/test_gpu_diffrender.py runs the functions)")
def test_diffrender_refuses_without_gpu():
    import aadff.diffrender as dr
    img = torch.rand(1, 3, 16, 16)
    for rg in (False, True):
        x = img.clone().requires_grad_(rg)
        with pytest.raises(RuntimeError, match="no HIP device"):
            dr.render_psf_map(x, torch.rand(3, 6, 6), 2)
        with pytest.raises(RuntimeError, match="no HIP device"):
            dr.render_psf(x, torch.rand(3, 3, 3))
        with pytest.raises(RuntimeError, match="no HIP device"):
            dr.render_psf_map_stack(x, torch.rand(2, 3, 6, 6), 2)
        with pytest.raises(RuntimeError, match="no HIP device"):
            dr.local_psf_render(x, torch.rand(1, 16, 16, 3, 3), kernel_size=3)
        with pytest.raises(RuntimeError, match="no HIP device"):
            dr.local_psf_render_high_res(x, torch.rand(1, 16, 16, 3, 3), patch_size=[8, 8], kernel_size=3)
