"""GPU tests (run with `-m gpu` on an MI355X): torch.library.opcheck of the torch.ops.aadff.* ops that no other test file checks -
render_psf, psfnet_forward, psfnet_render_rgbd, psfnet_render_rgbd_bwd, psfnet_render_rgbd_diff, depth_metric_sums,
image_metric_sums, psf_points and psf_points_block.  `test_schema` runs the real op and checks that it mutates and aliases what its
schema says; `test_faketensor` checks that the op's fake implementation returns the real op's shapes, dtypes and strides - with every
"want" / "need" flag both ways, so the empty tensor that stands for an output that is not wanted is compared too.

The arguments are built the way the kernels' own tests build them (test_gpu_psfnet_grad.py, test_gpu_metrics.py, test_gpu_parity.py,
deeplens/optics.py:_psf_launch for the packed lens tables), at their smallest sizes; the PSF network is the shipped architecture."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_common as mc                                # noqa: E402
import psfnet_grad_common as pc                            # noqa: E402
from aadff import ops, psfnet_pack                         # noqa: E402
from deeplens.basics import DEFAULT_WAVE, GEO_SPP, WAVE_RGB  # noqa: E402
from deeplens.psfnet import PSFNet                         # noqa: E402

DEV = "cuda:0"
UTILS = ("test_schema", "test_faketensor")
N, CN, S, H, W = 2, 3, 2, 16, 20                           # RGB-D renderer: 1280 rows, a ragged last workgroup of 64
GRID, SPP = 3, 256                                         # ray-traced PSFs: 9 field points


def _check(op, args, test_utils=UTILS):
    torch.library.opcheck(op.default, args, test_utils=test_utils)


def _assert_unwanted_empty(outs, wanted):
    """An output that is not wanted is an empty tensor of its own; one that is wanted is not empty."""
    for o, w in zip(outs, wanted):
        assert (o.numel() > 0) == bool(w)
    unwanted = [o for o, w in zip(outs, wanted) if not w]
    assert all(a is not b for i, a in enumerate(unwanted) for b in unwanted[:i])


@pytest.fixture(scope="module")
def lens(repo_root):
    """The shipped lens with the shipped PSF-network architecture (seeded weights), focused at 2 m."""
    net = PSFNet(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(64, 64), kernel_size=pc.KS, device=DEV)
    net.psfnet.load_state_dict(pc.state_dict(4321))
    torch.manual_seed(0)
    net.refocus(-2000.0)
    return net


@pytest.fixture(scope="module")
def rgbd(lens):
    """The arguments of psfnet_render_rgbd as aadff.diffrender._psfnet_stack forms them, and a cotangent."""
    case = ("opcheck", N, CN, S, H, W, 4321, [(-600.0, -3000.0), (-800.0, -4500.0)])
    _, img, depth, fds, dy = pc.case_inputs(case)
    packed = lens._fused(torch.device(DEV))
    wt, wt_exp = psfnet_pack.transposed(packed, lens.psfnet)
    xs, ys = lens._field_axes(H, W, torch.device(DEV))
    inv_range = float(np.float32(1.0) / np.float32(lens.d_max - lens.d_min))
    return dict(img=img.to(DEV), depth=depth[:, 0].contiguous().to(DEV), xs=xs, ys=ys, foc_z=lens.depth2z(fds.to(DEV)), dy=dy.to(DEV),
                consts=(float(lens.d_min), inv_range), packed=packed, wt=wt, wt_exp=list(wt_exp), ins=list(packed.ins), outs=list(packed.outs))


def test_render_psf():
    rng = np.random.Generator(np.random.PCG64(9))
    img = torch.from_numpy(rng.random((1, 3, 48, 40), dtype=np.float32)).to(DEV)
    for ks in (5, 11):
        psf = torch.from_numpy(rng.random((3, ks, ks), dtype=np.float32)).to(DEV)
        _check(torch.ops.aadff.render_psf, (img, psf / psf.sum((-1, -2), keepdim=True)))


def test_psfnet_forward(lens, rgbd):
    p = rgbd["packed"]
    inp = torch.rand((200, 4), generator=torch.Generator().manual_seed(5)).to(DEV)          # 200 rows: ragged against every tile size
    for precision in (0, 1):
        _check(torch.ops.aadff.psfnet_forward, (inp, p.wpack, p.bias, rgbd["ins"], rgbd["outs"], p.flags, precision))
    _check(torch.ops.aadff.psfnet_forward, (inp.reshape(50, 4, 4), p.wpack, p.bias, rgbd["ins"], rgbd["outs"], p.flags))
    assert int(p.flags.item()) == 0


def test_psfnet_render_rgbd(rgbd):
    r, p = rgbd, rgbd["packed"]
    for precision in (0, 1):
        _check(torch.ops.aadff.psfnet_render_rgbd, (r["img"], r["depth"], r["xs"], r["ys"], r["foc_z"], *r["consts"], p.wpack, p.bias, r["ins"],
                                                    r["outs"], pc.KS, p.flags, precision))
    assert int(p.flags.item()) == 0


@pytest.mark.parametrize("need", [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)],
                         ids=lambda n: "".join("x" if b else "-" for b in n))
def test_psfnet_render_rgbd_bwd(rgbd, need):
    r, p = rgbd, rgbd["packed"]
    args = (r["img"], r["depth"], r["xs"], r["ys"], r["foc_z"], r["dy"], *r["consts"], p.wpack, p.bias, r["wt"], r["wt_exp"], r["ins"], r["outs"],
            pc.KS, *need)
    _check(torch.ops.aadff.psfnet_render_rgbd_bwd, args)
    outs = torch.ops.aadff.psfnet_render_rgbd_bwd(*args)
    _assert_unwanted_empty(outs, need)
    for o, shape, w in zip(outs, ((N, CN, H, W), (N, H, W), (N, S)), need):
        assert o.shape == (shape if w else (0,)) and o.dtype == torch.float32


def test_psfnet_render_rgbd_diff(rgbd):
    r, p = rgbd, rgbd["packed"]
    rg = lambda t: t.clone().requires_grad_(True)      # noqa: E731
    for img, depth, foc_z in ((rg(r["img"]), rg(r["depth"]), rg(r["foc_z"])), (r["img"], rg(r["depth"]), r["foc_z"])):
        _check(torch.ops.aadff.psfnet_render_rgbd_diff, (img, depth, r["xs"], r["ys"], foc_z, *r["consts"], p.wpack, p.bias, r["wt"], r["wt_exp"],
                                                         r["ins"], r["outs"], pc.KS), test_utils=(*UTILS, "test_autograd_registration"))


def test_depth_metric_sums():
    est, gt, mask, conf = (torch.from_numpy(a).to(DEV) for a in mc.depth_inputs(2, 16, 20, seed=3))
    none = torch.empty(0, device=DEV)
    for m, c, mode in ((mask, conf, "mask"), (mask, none, "mask"), (none, conf, "finite"), (none, none, "finite")):
        _check(torch.ops.aadff.depth_metric_sums, (est, gt, m, c, mode))


def test_image_metric_sums():
    pred, target = (t.to(DEV) for t in mc.image_inputs(2, 3, 16, 20, seed=4))
    for ssim in (True, False):
        _check(torch.ops.aadff.image_metric_sums, (pred, target, ssim))


def _trace_args(lens):
    """(points [N,3] normalised, the packed surface tables of the main and the chief wavelengths, lens constants, one lens state, flags)."""
    pts = lens.point_source_grid(depth=-2000.0, grid=GRID).reshape(-1, 3).float().contiguous().to(DEV)
    return (pts, lens._table(WAVE_RGB), lens._table([DEFAULT_WAVE]), ops.lens_const_to_list(lens._lens_const()), lens._state_device(),
            torch.zeros(1, dtype=torch.int32, device=DEV))


def test_psf_points(lens):
    pts, tab, tab_chief, lc, state, flags = _trace_args(lens)
    g = torch.Generator().manual_seed(6)
    L = len(WAVE_RGB)
    pts2, states = pts.unsqueeze(0).repeat(S, 1, 1), state.repeat(S)                          # the same focus state twice
    u_main, u_chief = torch.rand((S, L, 2, SPP), generator=g).to(DEV), torch.rand((S, L, 2, GEO_SPP), generator=g).to(DEV)
    no_chief = torch.empty((S, L, 2, 0), device=DEV)
    for uc, centre, map_layout in ((u_chief, True, True), (u_chief, True, False), (no_chief, False, True), (no_chief, False, False)):
        _check(torch.ops.aadff.psf_points, (pts2, tab, tab_chief, lc, states, u_main, uc, pc.KS, centre, map_layout, flags))
    assert int(flags.item()) == 0


def test_psf_points_block(lens):
    pts, tab, tab_chief, lc, state, flags = _trace_args(lens)
    g = torch.Generator().manual_seed(7)
    L = len(WAVE_RGB)
    for spc, map_layout, ks in ((GEO_SPP, True, 11), (GEO_SPP, False, 5), (0, True, 5), (0, False, 11)):
        u_block = torch.rand((L * (2 * SPP + 2 * spc),), generator=g).to(DEV)
        _check(torch.ops.aadff.psf_points_block, (pts, tab, tab_chief, lc, state, u_block, L, SPP, spc, ks, map_layout, flags))
    assert int(flags.item()) == 0
