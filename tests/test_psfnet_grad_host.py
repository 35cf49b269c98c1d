"""CPU: the host side of the PSF-network renderer's backward (csrc/psfnet_bwd.hip, aadff/psfnet_pack.py, aadff/ops.py): the
transposed weight pack against a numpy restatement of the fragment order, fake-tensor shapes of the new ops, the workspace query,
argument errors of the C entry without a GPU, and the masked-share condition of every GPU test case (tests/psfnet_grad_common.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import psfnet_grad_common as pc
from aadff import _abi, ops, psfnet_pack

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first


class _Net:
    """What psfnet_pack reads of deeplens.psfnet_arch.MLP: `.net`, Linear + ReLU ..., Linear + Sigmoid."""

    def __init__(self, widths, seed):
        g = torch.Generator().manual_seed(seed)
        mods = []
        for i, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
            lin = torch.nn.Linear(k, n)
            with torch.no_grad():
                lin.weight.copy_((torch.rand((n, k), generator=g) * 2 - 1) * (6.0 / k) ** 0.5)
            mods += [lin, torch.nn.ReLU() if i < len(widths) - 2 else torch.nn.Sigmoid()]
        self.net = torch.nn.Sequential(*mods)


def _unpack(flat, n, k):
    """numpy restatement of the fragment order: flat fp16 [tile][step][plane][lane = kg * 16 + m][8] -> (hi, lo) [n pad 16][k pad 32]
    with element (16 tile + m, 32 step + 8 kg + e) at [tile][step][plane][kg * 16 + m][e]."""
    npad, kpad = (n + 15) // 16 * 16, (k + 31) // 32 * 32
    a = flat.reshape(npad // 16, kpad // 32, 2, 64, 8)
    out = np.zeros((2, npad, kpad), np.float16)
    for tile in range(npad // 16):
        for step in range(kpad // 32):
            for lane in range(64):
                m, kg = lane & 15, lane >> 4
                out[:, 16 * tile + m, 32 * step + 8 * kg:32 * step + 8 * kg + 8] = a[tile, step, :, lane, :]
    return out[0], out[1]


@pytest.mark.parametrize("widths", [(4, 64, 256, 256, 256, 256, 256, 256, 256, 256, 256, 121), (4, 50, 70, 33, 81)], ids=["psfnet", "odd_widths"])
def test_transposed_pack_is_w_transposed_hi_lo(widths):
    net = _Net(widths, seed=3)
    assert psfnet_pack.supported(net)
    flat, exps = psfnet_pack.pack_transposed(net, torch.device("cpu"))
    flat, off = flat.numpy(), 0
    assert len(exps) == len(widths) - 1
    for lin, e in zip(psfnet_pack.linears_of(net), exps):
        n, k = lin.in_features, lin.out_features                    # the transpose maps out_features -> in_features
        npad, kpad = (n + 15) // 16 * 16, (k + 31) // 32 * 32
        size = npad * kpad * 2
        hi, lo = _unpack(flat[off:off + size], n, k)
        off += size
        wt = lin.weight.detach().numpy().T.astype(np.float32) * np.float32(2.0 ** e)
        assert 512.0 <= np.abs(wt).max() < 1024.0                   # the layer's power-of-two scale
        want = np.zeros((npad, kpad), np.float32)
        want[:n, :k] = wt
        whi = want.astype(np.float16)
        wlo = (want - whi.astype(np.float32)).astype(np.float16)
        assert np.array_equal(hi, whi) and np.array_equal(lo, wlo)
        # what the split leaves of a weight: 2^-22 relative for every weight above max / 2^13
        resid = np.abs(want.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
        big = np.abs(want) >= 2.0 ** -3
        assert (resid[big] <= np.abs(want[big]) * 2.0 ** -21).all() and resid.max() <= 2.0 ** -12
    assert off == flat.size


def test_transposed_pack_is_cached_with_the_pack():
    net = _Net((4, 64, 121), seed=5)
    packed = psfnet_pack.PackedMLP(net, torch.device("cpu"))
    assert packed.wtpack is None
    wt, exps = psfnet_pack.transposed(packed, net)
    assert psfnet_pack.transposed(packed, net)[0] is wt and packed.wt_exp == exps
    with torch.no_grad():
        net.net[0].weight.mul_(2.0)                                  # bumps the version counter: the pack's key no longer matches
    with pytest.raises(ValueError, match="stale"):
        psfnet_pack.transposed(packed, net)


def test_fake_tensor_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img, depth, fz = torch.empty(2, 3, 40, 56, device="cuda"), torch.empty(2, 40, 56, device="cuda"), torch.empty(2, 5, device="cuda")
        xs, ys = torch.empty(56, device="cuda"), torch.empty(40, device="cuda")
        wp, b, wt = (torch.empty(64, dtype=torch.float16, device="cuda"), torch.empty(64, device="cuda"),
                     torch.empty(64, dtype=torch.float16, device="cuda"))
        out, flags = torch.ops.aadff.psfnet_render_rgbd_diff(img, depth, xs, ys, fz, -200.0, -5e-5, wp, b, wt, [0, 0], [4, 64], [64, 121], 11)
        assert out.shape == (2, 3, 5, 40, 56) and out.dtype == torch.float32 and flags.shape == (1,) and flags.dtype == torch.int32
        dy = torch.empty(2, 3, 5, 40, 56, device="cuda")
        gi, gd, gf = torch.ops.aadff.psfnet_render_rgbd_bwd(img, depth, xs, ys, fz, dy, -200.0, -5e-5, wp, b, wt, [0, 0], [4, 64], [64, 121], 11,
                                                            True, True, True)
        assert gi.shape == img.shape and gd.shape == depth.shape and gf.shape == fz.shape
        gi, gd, gf = torch.ops.aadff.psfnet_render_rgbd_bwd(img, depth, xs, ys, fz, dy, -200.0, -5e-5, wp, b, wt, [0, 0], [4, 64], [64, 121], 11,
                                                            False, True, False)
        assert gi.numel() == 0 and gd.shape == depth.shape and gf.numel() == 0


def test_workspace_query():
    ws = ops.psfnet_bwd_workspace_bytes
    hw = 480 * 640
    rows = 2 * 8 * hw
    # depth / focus gradients: one float per row (n, slice, y, x) and one per workgroup of 64 rows; nothing of the PSFs' size
    assert ws(2, 8, 3, 480, 640, 11, True, False) == 4 * (rows + rows // 64)
    # image gradient: the network input and the PSFs of ONE slice, whatever N and S
    assert ws(2, 8, 3, 480, 640, 11, False, True) == ws(1, 1, 3, 480, 640, 11, False, True) == 4 * hw * (4 + 121)
    assert ws(2, 8, 3, 480, 640, 11, True, True) == ws(2, 8, 3, 480, 640, 11, True, False) + ws(2, 8, 3, 480, 640, 11, False, True)
    assert ws(1, 1, 1, 67, 131, 11, True, False) == 4 * ((67 * 131 + (67 * 131 + 63) // 64 + 3) // 4 * 4)        # ragged last workgroup
    assert ws(1, 1, 3, 64, 64, 11, False, False) == 0
    lib = _abi.load_library()
    n = C.c_size_t(0)
    assert lib.aadff_psfnet_render_rgbd_bwd_workspace(1, 1, 3, 64, 64, 11, 1, 1, None) == -1 and b"bytes" in lib.aadff_last_error()
    assert lib.aadff_psfnet_render_rgbd_bwd_workspace(1, 1, 3, 64, 64, 4, 1, 1, C.byref(n)) == -1 and b"ks" in lib.aadff_last_error()
    assert lib.aadff_psfnet_render_rgbd_bwd_workspace(0, 1, 3, 64, 64, 11, 1, 1, C.byref(n)) == -1 and b"empty" in lib.aadff_last_error()


def test_bwd_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_psfnet_render_rgbd_bwd
    ins, outs = (C.c_int * 3)(4, 64, 256), (C.c_int * 3)(64, 256, 121)
    ex = (C.c_int * 3)(9, 11, 11)
    big = C.c_size_t(1 << 40)

    def call(depth=P8, wt=P8, wexp=ex, n_layers=3, ins=ins, outs=outs, img=P8, dy=P8, N=1, S=2, Cn=3, H=32, W=48, ks=11, d_img=P8, d_depth=P8,
             d_foc=P8, ws=P8, nbytes=big):
        return f(depth, P8, P8, P8, -200.0, -5e-5, N, S, P8, P8, wt, wexp, n_layers, ins, outs, img, dy, Cn, H, W, ks, d_img, d_depth, d_foc, ws,
                 nbytes, None)

    def err():
        return lib.aadff_last_error()

    assert call(depth=None) == -1 and b"NULL" in err()
    assert call(dy=None) == -1 and b"NULL" in err()
    assert call(img=None) == -1 and b"NULL" in err()
    assert call(d_img=None, d_depth=None, d_foc=None) == -1 and b"d_img" in err() and b"d_depth" in err() and b"d_foc_z" in err()
    assert call(wt=None) == -1 and b"transposed" in err()
    assert call(ks=4) == -1 and b"ks" in err()                       # even
    assert call(ks=13) == -1 and b"ks" in err()                      # ks^2 > 128 outputs
    assert call(ks=9) == -1 and b"ks" in err()                       # does not match the network's 121 outputs
    assert call(N=0) == -1 and b"empty" in err()
    assert call(S=0) == -1 and b"empty" in err()
    assert call(H=0) == -1 and b"empty" in err()
    assert call(n_layers=17) == -1 and b"layers" in err()
    assert call(ins=(C.c_int * 3)(4, 64, 255)) == -1 and b"chain" in err()
    assert call(outs=(C.c_int * 3)(64, 300, 121), ins=(C.c_int * 3)(4, 64, 300)) == -1 and b"256" in err()
    assert call(wexp=(C.c_int * 3)(9, 99, 11)) == -1 and b"exponent" in err()
    need = ops.psfnet_bwd_workspace_bytes(1, 2, 3, 32, 48, 11, True, True)
    assert call(nbytes=C.c_size_t(need - 4)) == -1 and b"workspace" in err()
    assert call(ws=None) == -1 and b"workspace" in err()
    # only d_img: neither the transposed pack nor the per-row workspace is needed, but one slice of PSFs is
    need_img = ops.psfnet_bwd_workspace_bytes(1, 2, 3, 32, 48, 11, False, True)
    assert call(wt=None, wexp=None, d_depth=None, d_foc=None, nbytes=C.c_size_t(need_img - 4)) == -1 and b"workspace" in err()


def test_new_entries_are_importable_without_gpu():
    import aadff.diffrender as dr
    assert callable(dr.psfnet_render) and callable(dr.psfnet_render_stack)
    for op in ("psfnet_render_rgbd_diff", "psfnet_render_rgbd_bwd"):
        assert hasattr(torch.ops.aadff, op)
    assert "WEIGHTS get no gradient" in " ".join(dr.psfnet_render_stack.__doc__.split())


CASES_3D = [("3d_3x64x64", 1, 3, 1, 64, 64, 4321, [(-1500.0,)])]


@pytest.mark.parametrize("case", [c for c in pc.CASES + CASES_3D], ids=[c[0] for c in pc.CASES + CASES_3D])
def test_masked_share_of_every_gpu_case(case):
    """The cotangent mask of the GPU parity tests (rows within 1e-5 of a ReLU kink, float64) must stay a small share of the rows."""
    sd, img, depth, fds, dy = pc.case_inputs(case)
    share = 1.0 - float(pc.keep_rows(sd, depth, fds).mean())
    print(f"{case[0]}: masked share {share:.4f}")
    assert 0.0 < share <= pc.MAX_MASKED
