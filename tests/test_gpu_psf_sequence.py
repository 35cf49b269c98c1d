"""The PSF-grid kernel's two traces (run with `-m gpu`): the straight-line trace compiled per surface-kind sequence
(SSSSSTSSAASS: rf50mm and its variants; SSSSSSTSSSS: 50mm_f2.8) against the run-time loop over the surface table, which
every other sequence takes and which AADFF_PSF_TRACE=loop forces (read per launch, so both run here on the same draws).

Shape: 3 x 3 field points (centre, edges, corners: the compaction sees ns = 2048 and ns < 1024), 2 focus states,
3 wavelengths, ks 11; spp 2048 and 300 (the second ray of a lane partly inactive).

Tolerances: chief-ray centres <= 2e-5 mm (the mean sensor-hit tolerance of tests/test_gpu_margins.py), PSFs <= 2e-3
rel-L2 (the project's PSF tolerance), every PSF sums to 1 within 1e-5.  Both traces run the same per-surface arithmetic in
the same order: on an MI355X the centres (a fixed-order sum) come out equal to the bit; the PSFs differ by 1.2e-7 .. 3.4e-7
rel-L2, which is what two launches of the SAME trace differ by - the histogram is summed with float atomics in LDS, in the order
the waves happen to arrive (measured alongside in the test: `again`)."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aadff import _abi                                   # noqa: E402
from aadff.focal_stack import StackPlan, render_focal_stack_m1   # noqa: E402
from aadff.synth import synth_rgb                         # noqa: E402
from deeplens.basics import GEO_SPP                       # noqa: E402
from deeplens.optics import Lensgroup                     # noqa: E402
from oracle.lens import OracleLens                        # noqa: E402

DEV = "cuda:0"
RES = (256, 256)
GRID, KS, FOCUS, PLANE = 3, 11, [-1000.0, -3000.0], -1500.0
CENTRE_TOL, PSF_TOL, SUM_TOL = 2e-5, 2e-3, 1e-5
# PSFs of one trace against the other, and of one trace launched twice: only the order of the float atomics differs.  A bin sums
# <= 2048 weights; fp32 sums of n terms in two random orders differ by about sqrt(n) x 2^-24 relative.  Observed: <= 3.4e-7 (8 x under).
ORDER_TOL = 2048 ** 0.5 * 2.0 ** -24                      # 2.7e-6
# flags bits under AADFF_PSF_TRACE=mark: which body the workgroups took (none: the loop)
SEQ_FLAG = {"rf50mm": 256, "rf50mm_k": 256, "50mm_f2.8": 512, "rf50mm_asph2": 0}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@contextlib.contextmanager
def trace_path(which):
    """'seq': the compiled sequence where the lens has one (the default); 'loop': the run-time loop for every lens; 'mark': as
    'seq', and the workgroups that take a compiled sequence say which in the flags word (SEQ_FLAG)."""
    old = os.environ.pop("AADFF_PSF_TRACE", None)
    if which != "seq":
        os.environ["AADFF_PSF_TRACE"] = which
    try:
        yield
    finally:
        os.environ.pop("AADFF_PSF_TRACE", None)
        if old is not None:
            os.environ["AADFF_PSF_TRACE"] = old


def lens_file(repo_root, tmp_path, name):
    """Shipped lenses by name; 'rf50mm_k': rf50mm with a conic constant on its first asphere (same kind sequence);
    'rf50mm_asph2': its third sphere turned into an asphere (a sequence that is not compiled: the loop)."""
    base = name if name in ("rf50mm", "50mm_f2.8") else "rf50mm"
    path = os.path.join(repo_root, "lenses", base, "lens.json")
    if name == base:
        return path
    d = json.load(open(path))
    if name == "rf50mm_k":
        d["surfaces"][8]["k"] = 0.35
    else:
        d["surfaces"][2].update({"type": "Aspheric", "k": -0.6, "ai": [0.0, 1.5e-6, -2e-9, 0.0, 0.0, 0.0]})
    path = str(tmp_path / f"{name}.json")
    json.dump(d, open(path, "w"))
    return path


def psf_grid_both_paths(path, spp, centre_mode=1):
    """One draw, one refocus of both focus states, then the fused PSF kernel on each trace: {which: (psf [S,N,L,ks,ks],
    centres [S,L,N,2]), "mark": the flags word of one more launch under AADFF_PSF_TRACE=mark}."""
    lens = Lensgroup(path, sensor_res=RES, device=DEV)
    S, N = len(FOCUS), GRID * GRID
    plan = StackPlan(lens, S, RES[0], RES[1], grid=GRID, ks=KS, spp=spp)
    torch.manual_seed(7)
    ub = plan.uniforms(lens.sampler).data_ptr()
    dep, pts = plan.geometry(FOCUS, PLANE)
    st = _abi.stream_ptr(torch.device(DEV))
    _abi.call("aadff_refocus", _abi.ptr(dep), S, C.c_void_p(ub), GEO_SPP, plan.per, _abi.ptr(plan.tab_green), plan.lc, _abi.ptr(plan.states), st)
    out = {}
    for which in ("seq", "loop", "again"):                # again: the first trace a second time
        psf = torch.full((S, N, 3, KS, KS), float("nan"), device=DEV)
        cen = torch.full((S, 3, N, 2), float("nan"), device=DEV)
        with trace_path("loop" if which == "loop" else "seq"):
            _abi.call("aadff_psf_points", _abi.ptr(pts), S, N, 3, _abi.ptr(plan.tab_rgb), _abi.ptr(plan.tab_green) if centre_mode else None,
                      plan.lc, _abi.ptr(plan.states), C.c_void_p(ub + 4 * plan.o_main), spp, plan.per, plan.per_l,
                      C.c_void_p(ub + 4 * plan.o_chief) if centre_mode else None, GEO_SPP if centre_mode else 0, plan.per, plan.per_l, KS,
                      centre_mode, 0, _abi.ptr(psf), _abi.ptr(cen), _abi.ptr(plan.flags), st)
        plan.check_flags()
        out[which] = (psf.cpu().numpy(), cen.cpu().numpy())
    mark = torch.zeros(1, dtype=torch.int32, device=DEV)  # a flags word of its own: the plan's is read by check_flags
    with trace_path("mark"):
        _abi.call("aadff_psf_points", _abi.ptr(pts), S, N, 3, _abi.ptr(plan.tab_rgb), _abi.ptr(plan.tab_green) if centre_mode else None,
                  plan.lc, _abi.ptr(plan.states), C.c_void_p(ub + 4 * plan.o_main), spp, plan.per, plan.per_l,
                  C.c_void_p(ub + 4 * plan.o_chief) if centre_mode else None, GEO_SPP if centre_mode else 0, plan.per, plan.per_l, KS,
                  centre_mode, 0, _abi.ptr(psf), _abi.ptr(cen), _abi.ptr(mark), st)
    out["mark"] = int(mark.item())
    return out


@pytest.mark.parametrize("spp", [2048, 300])
@pytest.mark.parametrize("name", ["rf50mm", "50mm_f2.8", "rf50mm_k"])
def test_sequence_trace_against_loop(repo_root, tmp_path, margin, name, spp):
    got = psf_grid_both_paths(lens_file(repo_root, tmp_path, name), spp)
    (psf, cen), (psf_l, cen_l) = got["seq"], got["loop"]
    assert got["mark"] == SEQ_FLAG[name]                  # the compiled body of this lens really ran, and only that one
    assert np.isfinite(psf).all() and np.isfinite(cen).all()
    d_cen, d_psf, d_again = float(np.abs(cen - cen_l).max()), rel(psf, psf_l), rel(got["again"][0], psf)
    print(f"{name} spp {spp}: centres max |d| {d_cen:.3e} mm, PSF rel-L2 {d_psf:.3e}, max |d| {np.abs(psf - psf_l).max():.3e}; same trace twice: rel-L2 {d_again:.3e}")
    margin(f"PSF sequence vs loop, {name} spp {spp}: chief-ray centres [mm]", d_cen, CENTRE_TOL)
    margin(f"PSF sequence vs loop, {name} spp {spp}: PSF rel-L2", d_psf, PSF_TOL)
    for p in (psf, psf_l):
        assert np.abs(p.sum((-1, -2)) - 1.0).max() <= SUM_TOL
    assert np.array_equal(cen, cen_l) and np.array_equal(got["again"][1], cen)       # observed: the same bits
    assert d_psf <= ORDER_TOL and d_again <= ORDER_TOL                   # observed: <= 3.4e-7 both


@pytest.mark.parametrize("name", ["rf50mm", "50mm_f2.8", "rf50mm_k", "rf50mm_asph2"])
def test_against_oracle(repo_root, tmp_path, margin, name):
    """Both focus states, the three wavelengths, against the oracle on the same host-RNG stream (a table entry read at the wrong
    index shows here, not between the two traces of one table); rf50mm_asph2 is the loop, by its sequence.
    (2048 rays: at 300 a single ray on a bin edge is 1/300 of a PSF, above the PSF tolerance by itself.)"""
    path = lens_file(repo_root, tmp_path, name)
    pts = OracleLens(path, sensor_res=RES).point_source_grid(PLANE, GRID).reshape(-1, 3).float()
    ora = OracleLens(path, sensor_res=RES)
    lens = Lensgroup(path, sensor_res=RES, device=DEV)
    for who in (ora, lens):
        torch.manual_seed(11)
        res = []
        for f in FOCUS:
            who.refocus(f)
            res.append(who.psf_rgb(pts, ks=KS, spp=2048))
        if who is ora:
            want = torch.stack(res).numpy()
        else:
            got = torch.stack(res).cpu().numpy()
    assert got.shape == want.shape == (2, GRID * GRID, 3, KS, KS)
    margin(f"PSF vs oracle, {name}: rel-L2", rel(got, want), PSF_TOL)
    assert np.abs(got.sum((-1, -2)) - 1.0).max() <= SUM_TOL
    if name == "rf50mm_asph2":                            # not a compiled sequence: the switch changes nothing (same code, atomics order)
        with trace_path("loop"):
            torch.manual_seed(11)
            again = []
            for f in FOCUS:
                lens.refocus(f)
                again.append(lens.psf_rgb(pts, ks=KS, spp=2048))
        assert rel(torch.stack(again).cpu().numpy(), got) <= ORDER_TOL


def test_pinhole_centre_through_the_sequence_trace(repo_root, tmp_path):
    """centre_mode 0: no chief pass and no chief table; the main pass alone picks the sequence."""
    got = psf_grid_both_paths(lens_file(repo_root, tmp_path, "rf50mm"), 2048, centre_mode=0)
    (psf, cen), (psf_l, cen_l) = got["seq"], got["loop"]
    assert got["mark"] == SEQ_FLAG["rf50mm"]
    assert np.isfinite(psf).all() and np.abs(psf.sum((-1, -2)) - 1.0).max() <= SUM_TOL
    assert np.array_equal(cen, cen_l) and rel(psf, psf_l) <= ORDER_TOL


def test_other_sequence_takes_the_loop(repo_root, tmp_path):
    """A kind sequence that is not compiled: no workgroup reports a compiled body, and the switch changes nothing - the centres
    to the bit, the PSFs up to the order of the float atomics (the same code ran three times)."""
    got = psf_grid_both_paths(lens_file(repo_root, tmp_path, "rf50mm_asph2"), 2048)
    (psf, cen), (psf_l, cen_l) = got["seq"], got["loop"]
    assert got["mark"] == SEQ_FLAG["rf50mm_asph2"] == 0
    assert np.isfinite(psf).all() and np.abs(psf.sum((-1, -2)) - 1.0).max() <= SUM_TOL
    assert np.array_equal(cen, cen_l) and np.array_equal(got["again"][1], cen)
    assert rel(psf, psf_l) <= ORDER_TOL and rel(got["again"][0], psf) <= ORDER_TOL


@pytest.mark.parametrize("S", [3, 5])
def test_staged_stack_on_both_traces(repo_root, margin, S):
    """The staged launch with a reused plan: a 64 x 64 stack from the same seed on each trace.  S = 3: every focus state's draws
    are uploaded by the refocus launch; S = 5: the last two by upload workgroups in front of the PSF workgroups."""
    H = W = 64
    lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(H, W), device=DEV)
    img = torch.from_numpy(synth_rgb(H, W))[None].to(DEV)
    fds = [-800.0, -1500.0, -3000.0, -1100.0, -5000.0][:S]
    plan = StackPlan(lens, len(fds), H, W, grid=GRID, ks=KS, spp=512)
    assert not lens.sampler.on_device and plan.per % 4 == 0               # the staged path
    out = {}
    for which in ("seq", "loop"):
        torch.manual_seed(3)
        with trace_path(which):
            out[which] = render_focal_stack_m1(lens, img, PLANE, fds, grid=GRID, ks=KS, spp=512, plan=plan).cpu().numpy()
        plan.check_flags()
    assert np.isfinite(out["seq"]).all()
    margin(f"M1 stack 64^2 x {S}, staged launch: sequence vs loop, image rel-L2", rel(out["seq"], out["loop"]), 1e-4)
