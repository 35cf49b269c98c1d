"""CPU: the host side of the classical depth-from-focus estimator (csrc/dfocus.hip, aadff/ops.py, aadff/dfocus.py): the exported
symbol, every argument error of the C entry without a GPU, the fake-tensor shapes of the op, the wrapper's errors and empty results,
and the oracle of tests/dfocus_common.py itself - against a literal per-pixel restatement of the specification and on the recovery
fixture (depth recovered to a fraction of the slice spacing; the log-domain fit beats the plain parabola)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dfocus_common as dc
from aadff import _abi, dfocus

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
F = C.c_float


def _err(lib):
    return lib.aadff_last_error()


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "aadff_depth_from_stack") and "aadff_depth_from_stack" in _abi.PROTOTYPES
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9           # an addition only
    assert _abi.DFOCUS_INTERP == {"none": 0, "parabola": 1, "gaussian": 2}


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_depth_from_stack

    def call(stack=P8, coords=P8, depth=P8, index=P8, peak=P8, aif=P8, volume=P8, N=1, Cn=3, S=4, H=16, W=16, window=9, interp=2, eps=1e-8):
        return f(stack, coords, depth, index, peak, aif, volume, N, Cn, S, H, W, window, interp, F(eps), None)

    for name in ("stack", "coords", "depth", "index", "peak"):
        assert call(**{name: None}) == -1 and b": %s is NULL" % name.encode() in _err(lib)
    assert call(Cn=0) == -1 and b"C = 0" in _err(lib)
    assert call(Cn=5) == -1 and b"C = 5" in _err(lib)
    assert call(S=0) == -1 and b"S = 0" in _err(lib)
    assert call(N=0) == -1 and b"N = 0" in _err(lib)
    assert call(H=0) == -1 and b"H = 0" in _err(lib)
    assert call(W=-3) == -1 and b"W = -3" in _err(lib)
    for w in (0, 2, 4, 8, 11, -1):
        assert call(window=w) == -1 and b"window = %d" % w in _err(lib)
    for i in (-1, 3):
        assert call(interp=i) == -1 and b"interp = %d" % i in _err(lib)
    assert call(eps=0.0) == -1 and b"eps" in _err(lib)
    assert call(eps=-1e-8) == -1 and b"eps" in _err(lib)
    assert call(eps=float("nan")) == -1 and b"eps" in _err(lib)
    assert call(N=70000, H=70000, W=70000) == -1 and b"too large" in _err(lib)


def test_op_and_fake_shapes():
    from aadff import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.aadff, "depth_from_stack")
    with FakeTensorMode():
        stack, coords = torch.empty(2, 3, 5, 40, 56, device="cuda"), torch.empty(2, 5, device="cuda")
        d, i, p, a, v = torch.ops.aadff.depth_from_stack(stack, coords, 9, "gaussian", 1e-8, True, True)
        assert d.shape == i.shape == p.shape == (2, 1, 40, 56) and a.shape == (2, 3, 40, 56) and v.shape == (2, 5, 40, 56)
        assert (d.dtype, i.dtype, p.dtype, a.dtype, v.dtype) == (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32)
        assert not d.requires_grad
        d, i, p, a, v = torch.ops.aadff.depth_from_stack(stack, coords, 3, "none", 1e-8, False, False)
        assert d.shape == (2, 1, 40, 56) and a.shape == (0,) and v.shape == (0,) and a.dtype == v.dtype == torch.float32
        d, i, p, a, v = torch.ops.aadff.depth_from_stack(stack, coords, 1, "parabola", 1e-8, True, False)
        assert a.shape == (2, 3, 40, 56) and v.shape == (0,)


def test_wrapper_value_errors():
    from aadff.dfocus import depth_from_stack
    st, fd = torch.rand(2, 3, 4, 8, 8), torch.tensor([[-600.0, -900.0, -1500.0, -3000.0]] * 2)
    with pytest.raises(ValueError, match="N,C,S,H,W"):
        depth_from_stack(st[0], fd)
    with pytest.raises(ValueError, match="foc_dists"):
        depth_from_stack(st, fd[:, :3])
    with pytest.raises(ValueError, match="foc_dists"):
        depth_from_stack(st, fd[0])                                                # [S] is accepted for N == 1 only
    with pytest.raises(ValueError, match="foc_dists"):
        depth_from_stack(st, fd.reshape(2, 2, 2))
    with pytest.raises(ValueError, match="no slices"):
        depth_from_stack(st[:, :, :0], fd[:, :0])
    with pytest.raises(ValueError, match="monotone"):
        depth_from_stack(st, torch.tensor([[-600.0, -900.0, -1500.0, -3000.0], [-600.0, -1500.0, -900.0, -3000.0]]))
    with pytest.raises(ValueError, match="monotone"):
        depth_from_stack(st, torch.tensor([[600.0, 900.0, 900.0, 3000.0]] * 2), space="linear")
    with pytest.raises(ValueError, match="zero"):
        depth_from_stack(st, torch.tensor([[0.0, 900.0, 1500.0, 3000.0]] * 2))
    for w in (0, 2, 11, 3.5):
        with pytest.raises(ValueError, match="window"):
            depth_from_stack(st, fd, window=w)
    with pytest.raises(ValueError, match="interp"):
        depth_from_stack(st, fd, interp="cubic")
    with pytest.raises(ValueError, match="space"):
        depth_from_stack(st, fd, space="log")
    with pytest.raises(ValueError, match="eps"):
        depth_from_stack(st, fd, eps=0.0)


def test_wrapper_empty_inputs_need_no_gpu():
    from aadff.dfocus import DepthFromStack, depth_from_stack
    fd = torch.tensor([[-600.0, -900.0, -1500.0]])
    out = depth_from_stack(torch.rand(0, 3, 3, 8, 8), fd[:0], return_volume=True)
    assert isinstance(out, DepthFromStack) and out._fields == ("depth", "index", "peak", "aif", "volume")
    assert out.depth.shape == out.index.shape == out.peak.shape == (0, 1, 8, 8) and out.aif.shape == (0, 3, 8, 8) and out.volume.shape == (0, 3, 8, 8)
    assert out.index.dtype == torch.int32 and out.depth.dtype == torch.float32
    out = depth_from_stack(torch.rand(1, 2, 3, 0, 8), fd[0])
    assert out.depth.shape == (1, 1, 0, 8) and out.aif.shape == (1, 2, 0, 8) and out.volume.shape == (0,)
    out = depth_from_stack(torch.rand(1, 2, 3, 8, 0), fd, return_volume=True)
    assert out.peak.shape == (1, 1, 8, 0) and out.volume.shape == (1, 3, 8, 0)


def test_wrapper_has_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    from aadff.dfocus import depth_from_stack
    with pytest.raises(RuntimeError, match="no HIP device"):
        depth_from_stack(torch.rand(1, 3, 3, 8, 8), torch.tensor([-600.0, -900.0, -1500.0]))


def _literal(stack, coords, window, interp, eps):
    """The specification pixel by pixel (numpy; float32 gray and ML, float64 beyond), for tiny inputs."""
    x = stack.numpy()
    N, Cn, S, H, W = x.shape
    r = window // 2
    cl = lambda v, n: min(max(v, 0), n - 1)                                       # noqa: E731
    vol = np.zeros((N, S, H, W))
    for n in range(N):
        for s in range(S):
            g = x[n, 0, s].copy()
            for c in range(1, Cn):
                g = g + x[n, c, s]
            g = (g * np.float32(1.0 / Cn)).astype(np.float32)
            ml = np.zeros((H, W), np.float32)
            for y in range(H):
                for xx in range(W):
                    g2 = np.float32(2) * g[y, xx]
                    ml[y, xx] = abs((g2 - g[y, cl(xx - 1, W)]) - g[y, cl(xx + 1, W)]) + abs((g2 - g[cl(y - 1, H), xx]) - g[cl(y + 1, H), xx])
            for y in range(H):
                for xx in range(W):
                    vol[n, s, y, xx] = sum(float(ml[cl(y + dy, H), cl(xx + dx, W)]) for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    u = coords.numpy().astype(np.float64)
    out, idx = np.zeros((N, 1, H, W)), np.zeros((N, 1, H, W), np.int32)
    for n in range(N):
        for y in range(H):
            for xx in range(W):
                f = vol[n, :, y, xx]
                k = 0
                for s in range(1, S):
                    if f[s] > f[k]:
                        k = s
                d = 0.0
                if 0 < k < S - 1 and interp != "none":
                    hm, hp = u[n, k] - u[n, k - 1], u[n, k + 1] - u[n, k]
                    if interp == "parabola":
                        a, b = f[k] - f[k - 1], f[k] - f[k + 1]
                    else:
                        e = float(np.float32(eps))
                        a, b = np.log1p((f[k] - f[k - 1]) / (f[k - 1] + e)), np.log1p((f[k] - f[k + 1]) / (f[k + 1] + e))
                    den = 2.0 * (b * hm + a * hp)
                    d = 0.0 if den == 0 else (a * hp * hp - b * hm * hm) / den
                    d = min(max(d, min(-hm, hp)), max(-hm, hp))
                out[n, 0, y, xx], idx[n, 0, y, xx] = u[n, k] + d, k
    return vol, idx, out


@pytest.mark.parametrize("shape,window", [((2, 3, 5, 6, 7), 3), ((1, 1, 4, 3, 3), 9), ((2, 4, 1, 1, 5), 5), ((1, 2, 2, 5, 1), 1)])
def test_oracle_is_the_specification(shape, window):
    stack, coords = dc.random_stack(*shape, seed=11), dc.random_coords(shape[0], shape[2], seed=12)
    assert dc.INTERPS == dfocus.INTERPS and window in dfocus.WINDOWS                # the oracle covers what the package offers
    for interp in dc.INTERPS:
        got = dc.oracle(stack, coords, window, interp)
        vol, idx, u = _literal(stack, coords, window, interp, 1e-8)
        assert np.allclose(got["volume"].numpy(), vol, rtol=1e-14, atol=0) and np.array_equal(got["index"].numpy(), idx)
        assert np.allclose(got["u"].numpy(), u, rtol=1e-12, atol=0)
        assert torch.equal(got["aif"], dc.gather_aif(stack, got["index"]))


def test_oracle_constant_image_and_ties():
    stack = torch.full((2, 3, 4, 5, 6), 0.3)
    coords = dc.random_coords(2, 4, seed=1)
    for interp in dc.INTERPS:
        o = dc.oracle(stack, coords, 5, interp)
        assert (o["volume"] == 0).all() and (o["index"] == 0).all() and (o["peak"] == 0).all()
        assert torch.equal(o["u"].float(), coords[:, 0].reshape(2, 1, 1, 1).expand(2, 1, 5, 6))
    vol = torch.tensor([1.0, 3.0, 3.0, 2.0]).reshape(1, 4, 1, 1)                   # the first of equal maxima
    assert int(dc.first_argmax(vol)) == 1
    o = dc.peak_fit(vol, torch.tensor([[1.0, 2.0, 3.0, 4.0]]), "parabola")         # a = 2, b = 0: vertex half a step towards the tie
    assert float(o["u"]) == 2.5


_REC = {}


def _recovery(window, interp):
    if (window, interp) not in _REC:
        stack, coords, depth = dc.built_stack()
        o = dc.oracle(stack, coords, window, interp)
        err, mask = dc.recovery_error(o["u"], o["peak"], coords, depth)
        near = (o["index"].reshape(depth.shape).to(torch.int64) - dc.nearest_slice(coords, depth)).abs()[mask]
        _REC[(window, interp)] = (float(err.median()), float(err.quantile(0.9)), float((near <= 1).double().mean()))
    return _REC[(window, interp)]


@pytest.mark.parametrize("window", [5, 9])
def test_oracle_recovers_the_built_depth(window):
    """Median |u* - 1/depth| <= 0.5 slice spacings on the pixels with peak >= median(peak), for both fits; gaussian below parabola."""
    stack, coords, depth = dc.built_stack()
    assert stack.shape == (1, 3, 8, 48, 64) and coords.shape == (1, 8) and depth.shape == (48, 64)
    med = {}
    for interp in ("parabola", "gaussian"):
        med[interp], p90, near = _recovery(window, interp)
        print(f"window {window} {interp}: median {med[interp]:.3f} p90 {p90:.3f} spacings; index within one of the nearest slice on {near:.1%}")
        assert med[interp] <= 0.5
        assert near == 1.0
    assert med["gaussian"] < med["parabola"]
