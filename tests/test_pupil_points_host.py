"""CPU: the layout of the pupil points of a stack (aadff_chief_fit_prologue) against the layout of the draws they are
made of (`stack_uniform_layout`), and the new entries' place in the ABI.  No compute calls (there is no GPU here)."""
import ctypes as C

import numpy as np
import pytest

from aadff import _abi
from aadff.focal_stack import GEO_SPP, pupil_xy_layout, stack_uniform_layout

L = 3


@pytest.mark.parametrize("spp", [300, 2048])
def test_layout_is_the_block_of_draws_without_the_focus_draws(spp):
    per, o_main, o_chief, per_l = stack_uniform_layout(spp, L)
    per_state, o_cx, block = pupil_xy_layout(spp, L)
    assert block == per_l == 2 * spp + 2 * GEO_SPP                   # one block per (state, wavelength), as many floats as its draws
    assert per_state == L * block == per - o_main                    # a state: its draws minus the focus draws in front of them
    assert o_cx == o_chief - o_main == 2 * spp                       # the chief rows where the chief draws are


@pytest.mark.parametrize("spp", [300, 2048])
def test_every_point_sits_where_its_draw_sits(spp):
    """Element by element: number every float of a flat block of draws of S states; the point made of draw (s, l, which, i) has, in
    pupil_xy [S][L][4][.], the offset of that draw's theta (x) or r (y) within the state, less the focus draws."""
    S = 2
    per, o_main, o_chief, per_l = stack_uniform_layout(spp, L)
    per_state, o_cx, block = pupil_xy_layout(spp, L)
    flat = np.arange(S * per).reshape(S, per)
    rest = flat[:, o_main:].reshape(S, L, per_l)
    u_main, u_chief = rest[:, :, :2 * spp].reshape(S, L, 2, spp), rest[:, :, 2 * spp:].reshape(S, L, 2, GEO_SPP)
    xy = np.arange(S * per_state).reshape(S, L, block)               # offsets into pupil_xy
    main_x, main_y = xy[:, :, :spp], xy[:, :, spp:2 * spp]
    chief_x, chief_y = xy[:, :, o_cx:o_cx + GEO_SPP], xy[:, :, o_cx + GEO_SPP:]
    assert chief_y.shape == (S, L, GEO_SPP)
    for s in range(S):
        for got, want in ((main_x, u_main[:, :, 0]), (main_y, u_main[:, :, 1]), (chief_x, u_chief[:, :, 0]), (chief_y, u_chief[:, :, 1])):
            assert np.array_equal(got[s] - s * per_state, want[s] - s * per - o_main)
    # what the PSF kernel of a launch with points does: the pointers and strides it reads draws through, on pupil_xy
    for s in range(S):
        for l in range(L):
            assert main_x[s, l, 0] == s * per_state + l * block and chief_x[s, l, 0] == o_cx + s * per_state + l * block


def test_entries_are_bound_and_check_their_arguments_without_a_gpu():
    lib = _abi.load_library()
    for name, nargs in (("aadff_chief_fit_prologue", 15), ("aadff_psf_points_fit_pts", 26), ("aadff_psf_points_staged_fit_pts", 27)):
        assert hasattr(lib, name) and len(_abi.PROTOTYPES[name]) == nargs
    # one argument more than the entries they extend (pupil_xy_or_null, in front of the stream)
    assert len(_abi.PROTOTYPES["aadff_psf_points_fit_pts"]) == len(_abi.PROTOTYPES["aadff_psf_points_fit"]) + 1
    assert len(_abi.PROTOTYPES["aadff_psf_points_staged_fit_pts"]) == len(_abi.PROTOTYPES["aadff_psf_points_staged_fit"]) + 1
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9                                      # additions only
    lc = _abi.LensConst()
    rc = lib.aadff_chief_fit_prologue(None, 2048, 0, 0, C.c_void_p(16), 1, L, GEO_SPP, 0, 0, lc, None, C.c_void_p(16), None, None)
    assert rc == -1 and b"chief_fit_prologue" in lib.aadff_last_error()
    rc = lib.aadff_chief_fit_prologue(C.c_void_p(16), 2048, 0, 0, None, 1, L, GEO_SPP, 0, 0, lc, None, None, C.c_void_p(16), None)
    assert rc == -1 and b"NULL" in lib.aadff_last_error()
