"""CPU: the host side of the differentiable thin-lens renderer (csrc/thinlens.hip, aadff/ops.py, aadff/diffrender.py): exported
symbols, argument errors of the new C entries without a GPU, fake-tensor shapes of the new ops, the workspace formula, the conditions on
every GPU test case (excluded share, the oracle's own float32 distance), and the closed forms of DESIGN.md 4.9 restated in float64
torch against the oracle's float64 autograd (tests/thinlens_grad_common.py)."""
import ctypes as C

import pytest
import torch

import thinlens_grad_common as tc
from aadff import _abi, ops

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
F = C.c_float
LENS = (F(50.0 / 1.8), F(50.0), F(1.0 / 0.09375), F(200.0), F(20000.0))


def _err(lib):
    return lib.aadff_last_error()


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("aadff_thinlens_render_stack", "aadff_thinlens_render_stack_bwd", "aadff_thinlens_render_stack_bwd_workspace"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9           # additions only


def test_new_entries_are_importable_without_gpu():
    import aadff.diffrender as dr
    from deeplens.psfnet import ThinLens
    assert callable(dr.thinlens_render) and callable(dr.thinlens_render_stack) and callable(ThinLens.render_stack)
    for op in ("thinlens_render_stack", "thinlens_render_stack_bwd", "thinlens_render_stack_diff"):
        assert hasattr(torch.ops.aadff, op)
    assert "thinlens_render" not in dr.__doc__.split("Not covered:")[1]


def test_stack_forward_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_thinlens_render_stack

    def call(img=P8, depth=P8, fd=P8, out=P8, B=1, Cn=3, S=2, H=32, W=48, ks=11):
        return f(img, depth, fd, None, out, B, Cn, S, H, W, ks, *LENS, None)

    assert call(img=None) == -1 and b"NULL" in _err(lib)
    assert call(fd=None) == -1 and b"NULL" in _err(lib)
    assert call(out=None) == -1 and b"NULL" in _err(lib)
    assert call(S=0) == -1 and b"empty" in _err(lib)
    assert call(B=0) == -1 and b"empty" in _err(lib)
    assert call(Cn=5) == -1 and b"channels" in _err(lib)
    assert call(ks=15) == -1 and b"ks" in _err(lib)
    assert call(ks=4) == -1 and b"ks" in _err(lib)
    assert call(H=70000) == -1 and b"too large" in _err(lib)


def test_bwd_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_thinlens_render_stack_bwd
    big = C.c_size_t(1 << 40)

    def call(img=P8, depth=P8, fd=P8, dy=P8, d_img=P8, d_depth=P8, d_foc=P8, ws=P8, nbytes=big, B=1, Cn=3, S=2, H=32, W=48, ks=11):
        return f(img, depth, fd, None, dy, d_img, d_depth, d_foc, ws, nbytes, B, Cn, S, H, W, ks, *LENS, None)

    assert call(img=None) == -1 and b"NULL" in _err(lib)
    assert call(depth=None) == -1 and b"NULL" in _err(lib)
    assert call(dy=None) == -1 and b"NULL" in _err(lib)
    assert call(d_img=None, d_depth=None, d_foc=None) == -1 and b"d_img" in _err(lib) and b"d_depth" in _err(lib) and b"d_foc" in _err(lib)
    assert call(S=0) == -1 and b"empty" in _err(lib)
    assert call(W=0) == -1 and b"empty" in _err(lib)
    assert call(Cn=5) == -1 and b"channels" in _err(lib)
    assert call(ks=15) == -1 and b"ks" in _err(lib)
    assert call(ks=6) == -1 and b"ks" in _err(lib)
    need = ops.thinlens_bwd_workspace_bytes(1, 3, 2, 32, 48, 11, True, True)
    assert call(nbytes=C.c_size_t(need - 4)) == -1 and b"workspace" in _err(lib)
    assert call(ws=None) == -1 and b"workspace" in _err(lib)
    # only d_foc: the partials are needed, the per-row floats of the image gradient are not
    need_foc = ops.thinlens_bwd_workspace_bytes(1, 3, 2, 32, 48, 11, False, True)
    assert need_foc < need and call(d_img=None, d_depth=None, nbytes=C.c_size_t(need_foc - 4)) == -1 and b"workspace" in _err(lib)


def test_workspace_query():
    ws = ops.thinlens_bwd_workspace_bytes
    hw = 480 * 640
    rows = 2 * 8 * hw
    # image gradient: r^2 and 1/Z of every row (n, slice, pixel), 8 bytes - against the 484 bytes of one 11 x 11 PSF
    assert ws(2, 3, 8, 480, 640, 11, True, False) == 4 * 2 * rows
    # focus gradient: one partial per workgroup (a 64-pixel run of a row) and slice
    assert ws(2, 3, 8, 480, 640, 11, False, True) == 4 * 2 * 8 * 480 * 10
    assert ws(2, 3, 8, 480, 640, 11, True, True) == ws(2, 3, 8, 480, 640, 11, True, False) + ws(2, 3, 8, 480, 640, 11, False, True)
    assert ws(1, 1, 1, 67, 131, 13, True, True) == 4 * (2 * 67 * 131 + 67 * 3)            # ragged last workgroup of a row
    assert ws(1, 3, 5, 64, 64, 11, False, False) == 0                                    # d_depth alone lives in registers
    assert ws(2, 3, 8, 480, 640, 7, True, True) == ws(2, 1, 8, 480, 640, 13, True, True)  # independent of C and ks
    lib = _abi.load_library()
    n = C.c_size_t(0)
    assert lib.aadff_thinlens_render_stack_bwd_workspace(1, 3, 1, 64, 64, 11, 1, 1, None) == -1 and b"bytes" in _err(lib)
    assert lib.aadff_thinlens_render_stack_bwd_workspace(1, 3, 1, 64, 64, 4, 1, 1, C.byref(n)) == -1 and b"ks" in _err(lib)
    assert lib.aadff_thinlens_render_stack_bwd_workspace(0, 3, 1, 64, 64, 11, 1, 1, C.byref(n)) == -1 and b"empty" in _err(lib)


def test_fake_tensor_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    consts = (11, 50.0, 1.8, 0.09375, 200.0, 20000.0)
    with FakeTensorMode():
        img, depth, fd = torch.empty(2, 3, 40, 56, device="cuda"), torch.empty(2, 1, 40, 56, device="cuda"), torch.empty(2, 5, device="cuda")
        for op in (torch.ops.aadff.thinlens_render_stack, torch.ops.aadff.thinlens_render_stack_diff):
            out = op(img, depth, fd, *consts)
            assert out.shape == (2, 3, 5, 40, 56) and out.dtype == torch.float32
        dy = torch.empty(2, 3, 5, 40, 56, device="cuda")
        gi, gd, gf = torch.ops.aadff.thinlens_render_stack_bwd(img, depth, fd, dy, *consts, True, True, True)
        assert gi.shape == img.shape and gd.shape == depth.shape and gf.shape == fd.shape
        gi, gd, gf = torch.ops.aadff.thinlens_render_stack_bwd(img, depth, fd, dy, *consts, False, True, False)
        assert gi.numel() == 0 and gd.shape == depth.shape and gf.numel() == 0
        x = torch.empty(2, 3, 40, 56, device="cuda", requires_grad=True)
        assert torch.ops.aadff.thinlens_render_stack_diff(x, depth, fd, *consts).requires_grad


def test_no_grad_call_is_the_forward_and_needs_a_gpu(monkeypatch):
    """Without a GPU the forward-only renderer raises its 'no HIP device' error; under no_grad diffrender raises the same one, and the 3-D
    branch raises ThinLens.render's ValueError whether or not a gradient is asked for."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    import aadff.diffrender as dr
    from deeplens.psfnet import ThinLens
    thin = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=11, sensor_size=[24.0, 24.0], sensor_res=(64, 64))
    img, depth, fd = torch.rand(1, 3, 16, 16), torch.full((1, 1, 16, 16), -900.0), torch.tensor([-1500.0])
    with pytest.raises(RuntimeError) as e0:
        thin.render(img, depth, fd)
    with torch.no_grad(), pytest.raises(RuntimeError) as e1:
        dr.thinlens_render(thin, img.clone().requires_grad_(True), depth, fd)
    assert str(e0.value) == str(e1.value) and "no HIP device" in str(e1.value)
    with pytest.raises(RuntimeError, match="no HIP device"):
        dr.thinlens_render_stack(thin, img, depth, fd.reshape(1, 1))
    with pytest.raises(ValueError) as v0:
        thin.render(img[0], depth[0, 0], -1500.0)
    with pytest.raises(ValueError) as v1:
        dr.thinlens_render(thin, img[0].clone().requires_grad_(True), depth[0, 0], -1500.0)
    with torch.no_grad(), pytest.raises(ValueError) as v2:
        dr.thinlens_render(thin, img[0], depth[0, 0], -1500.0)
    assert str(v0.value) == str(v1.value) == str(v2.value)


_REF = {}


def _reference(case):
    if case[0] not in _REF:
        img, depth, fds, dy = tc.case_inputs(case)
        keep = tc.keep_rows(case, depth, fds)
        dym = dy * keep
        o64 = tc.oracle_grads(case, img, depth, fds, dym, torch.float64)
        _REF[case[0]] = (img, depth, fds, dym, 1.0 - float(keep.mean()), o64)
    return _REF[case[0]]


@pytest.mark.parametrize("case", tc.CASES, ids=[c[0] for c in tc.CASES])
def test_conditions_of_every_gpu_case(case):
    """Excluded share <= 0.5 % and the oracle's own float32 distance <= 5e-5 for every gradient: the case measures the kernel."""
    img, depth, fds, dym, share, o64 = _reference(case)
    o32 = tc.oracle_grads(case, img, depth, fds, dym, torch.float32)
    d32 = [tc.rel_l2(a, b) for a, b in zip(o32, o64)]
    print(f"{case[0]}: excluded share {share:.5%}; d32 out {d32[0]:.2e} d_img {d32[1]:.2e} d_depth {d32[2]:.2e} d_foc {d32[3]:.2e}")
    assert share <= tc.MAX_MASKED
    assert all(0.0 < v <= tc.MAX_D32 for v in d32[1:]), d32


def test_cases_span_what_they_should():
    cs = tc.CASES
    assert {c[1] for c in cs} >= {1, 2} and {c[2] for c in cs} >= {1, 3} and {c[6] for c in cs} >= {7, 11, 13} and {c[3] for c in cs} >= {1, 3, 5}
    assert any(c[5] % 64 for c in cs) and {c[10] for c in cs} == {-1, 1} and {c[7] for c in cs} >= {(256, 256), (480, 640)}
    lo, hi, out = [], [], False
    for c in cs:
        img, depth, fds, dy = tc.case_inputs(c)
        sg, d, f, dc, K, cp, r = tc.coc_chain(c, depth, fds)
        lo.append(float(cp.min()))
        hi.append(float(cp.max()))
        out |= bool(((d < tc.D_MIN) | (d > tc.D_MAX)).any())
    assert min(lo) < 0.1 and 20.0 <= max(hi) <= 60.0 and out        # the floor, large discs and the depth clamp all occur


@pytest.mark.parametrize("case", tc.CASES, ids=[c[0] for c in tc.CASES])
def test_closed_forms_agree_with_float64_autograd(case):
    """The formulas the kernels implement (radius gradient in the centred form, the coc chain, the clamp and floor rules, the adjoint
    gather with border clamping), in float64 torch without autograd, against torch.autograd through the oracle: <= 1e-10."""
    img, depth, fds, dym, share, o64 = _reference(case)
    got = tc.closed_form_grads(case, img, depth, fds, dym)
    for name, g, ref in zip(("d_img", "d_depth", "d_foc"), got, o64[1:]):
        err = tc.rel_l2(g, ref)
        print(f"{case[0]}: closed form {name} {err:.2e}")
        assert err <= 1e-10, (name, err)
    sg, d, f, dc, K, cp, r = tc.coc_chain(case, depth, fds)
    outside = ((d < tc.D_MIN) | (d > tc.D_MAX))[:, :, 0]
    assert (o64[2][outside] == 0).all() and (got[1][outside] == 0).all()
