"""GPU: `refocus_kernel` (csrc/trace.hip) through aadff_refocus, aadff_refocus_staged and aadff_post_computation at ragged sizes - the
masked second ray of a lane, the multi-pass loop, the ragged and the empty quarters of the staged entry, the upload workgroups' tail -
against the float64 oracle on draws for which the count of valid rays is decidable (tests/focus_hist_common.py, part A; the inputs'
conditions, the tolerances and the mutated references they reject: tests/test_focus_hist_host.py).

n_focus_rays is compared exactly; d_sensor, hfov, tan_hfov, foclen and fnum within 4 x the float32 oracle's own distance from float64
(`tolerances`, at most 1e-5)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focus_hist_common as fh                            # noqa: E402
from aadff import _abi                                    # noqa: E402
from deeplens.optics import Lensgroup                     # noqa: E402

DEV = "cuda:0"
SENTINEL = -7.0
NB = C.sizeof(_abi.LensState)
PLAIN = [pytest.param(name, spp, id=f"{name}-spp{spp}") for name in fh.LENSES for spp in fh.PLAIN_SPP]
STAGED = [pytest.param(name, spp, S, id=f"{name}-spp{spp}-S{S}") for name in fh.LENSES for spp in fh.STAGED_SPP for S in fh.STAGED_S]


@functools.lru_cache(maxsize=None)
def lens_of(repo_root, name):
    return Lensgroup(os.path.join(repo_root, "lenses", name, "lens.json"), sensor_res=(64, 64), device=DEV)


def host_states(states, S):
    return (_abi.LensState * S).from_buffer_copy(states.cpu().numpy().tobytes())


def refocus(lens, block, depths, spp, stride):
    """aadff_refocus on a flat block of draws; the states start as 0xff bytes: every field has to be written"""
    S = len(depths)
    dep = torch.tensor(depths, dtype=torch.float32, device=DEV)
    u = torch.from_numpy(block).to(DEV)
    states = torch.full((S * NB,), 255, dtype=torch.uint8, device=DEV)
    _abi.call("aadff_refocus", _abi.ptr(dep), S, _abi.ptr(u), spp, stride, _abi.ptr(lens._table([0.589])), lens._lens_const(), _abi.ptr(states),
              _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return states


def refocus_staged(lens, block, depths, spp, stride, n_u, scratch):
    """aadff_refocus_staged reading `block` from pinned memory; returns (states, u_dev [n_u + 8] prefilled with SENTINEL)"""
    S = len(depths)
    dep = torch.tensor(depths, dtype=torch.float32, device=DEV)
    u_pin = torch.from_numpy(block).pin_memory()
    u_dev = torch.full((n_u + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    states = torch.full((S * NB,), 255, dtype=torch.uint8, device=DEV)
    _abi.call("aadff_refocus_staged", _abi.ptr(dep), S, C.c_void_p(u_pin.data_ptr()), _abi.ptr(u_dev), n_u, spp, stride, _abi.ptr(lens._table([0.589])),
              lens._lens_const(), _abi.ptr(states), _abi.ptr(scratch), _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return states, u_dev


def against_float64(margin, tag, d, got, S):
    """counts and flags exactly; d_sensor and the lens-state fields of every state within the tolerances; returns the d_sensor values"""
    tol = fh.tolerances()
    worst = {k: 0.0 for k in tol}
    for s in range(S):
        st = got[s]
        print(f"{tag} state {s}: n_focus_rays {st.n_focus_rays} (float64 {d.count[s]}), flags {st.flags}, d_sensor {st.d_sensor:.7f} (float64 {d.d_sensor[s]:.7f})")
        assert st.n_focus_rays == d.count[s], f"{tag} state {s}: {st.n_focus_rays} rays counted, float64 counts {d.count[s]}"
        assert st.flags == 0 and st.pad == 0
        worst["d_sensor"] = max(worst["d_sensor"], abs(st.d_sensor - d.d_sensor[s]) / d.d_sensor[s])
        for f in fh.FIELDS:
            worst[f] = max(worst[f], abs(getattr(st, f) - d.state[s][f]) / abs(d.state[s][f]))
    print(f"{tag}: relative distance from float64, worst state: " + ", ".join(f"{k} {v:.3e} (tol {tol[k]:.3e})" for k, v in worst.items()))
    margin(f"{tag}: d_sensor vs float64, worst state (rel)", worst["d_sensor"], tol["d_sensor"])
    for f in fh.FIELDS:
        margin(f"{tag}: {f} vs float64 calc_fov, worst state (rel)", worst[f], tol[f])


def fields_bits(states, S):
    return np.frombuffer(states.cpu().numpy().tobytes(), np.int32).reshape(S, NB // 4)


@pytest.mark.parametrize("name,spp", PLAIN)
def test_plain_entry_against_float64(repo_root, margin, name, spp):
    """aadff_refocus, one workgroup of 1024 lanes per state, S = 3: spp below, at and above one and two passes of 2 x 1024 rays; then
    aadff_post_computation on states that hold only that d_sensor gives the same hfov, tan_hfov, foclen and fnum to the bit"""
    lens, d = lens_of(repo_root, name), fh.draw_sets(name)[("plain", spp)]
    S = len(fh.DEPTHS)
    states = refocus(lens, d.block(), fh.DEPTHS, spp, d.stride)
    got = host_states(states, S)
    against_float64(margin, f"refocus {name} spp {spp}", d, got, S)
    preset = (_abi.LensState * S)()
    for s in range(S):
        preset[s].d_sensor, preset[s].n_focus_rays = got[s].d_sensor, got[s].n_focus_rays
    again = torch.frombuffer(bytearray(bytes(preset)), dtype=torch.uint8).to(DEV)
    _abi.call("aadff_post_computation", S, _abi.ptr(lens._table([0.589])), lens._lens_const(), _abi.ptr(again), _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert np.array_equal(fields_bits(again, S), fields_bits(states, S)), "post_computation at refocus' d_sensor: other bits"


@pytest.mark.parametrize("name,spp,S", STAGED)
def test_staged_entry_against_float64_and_the_plain_entry(repo_root, margin, name, spp, S):
    """aadff_refocus_staged, four workgroups of 256 lanes per state (ragged chunk = ceil(spp / 4); quarters without a ray at spp < 4),
    draws read from pinned memory and copied to the device by the upload workgroups; S = 1 runs the first state of the draw set"""
    lens, d = lens_of(repo_root, name), fh.draw_sets(name)[("staged", spp)]
    block = d.block()[:S * d.stride].copy()
    depths = fh.DEPTHS[:S]
    scratch = torch.zeros(S * 64, dtype=torch.uint8, device=DEV)
    states, u_dev = refocus_staged(lens, block, depths, spp, d.stride, len(block), scratch)
    got = host_states(states, S)
    tag = f"refocus_staged {name} spp {spp} S {S}"
    against_float64(margin, tag, d, got, S)
    # the upload: the whole block, bit for bit, and nothing behind it
    up = u_dev.cpu().numpy()
    assert np.array_equal(up[:len(block)].view(np.int32), block.view(np.int32)) and (up[len(block):] == SENTINEL).all()
    # the same scratch again: the counters reset themselves, the partial sums are added in a fixed order
    states2, _ = refocus_staged(lens, block, depths, spp, d.stride, len(block), scratch)
    assert np.array_equal(fields_bits(states2, S), fields_bits(states, S)), "second launch on the same scratch: other bits"
    assert not scratch.view(torch.int32).view(S, 16)[:, 8:].any(), "arrived / nan_seen / loaded / passed not back at 0"
    # the plain entry on the same draws: the same rays, another split of the sum
    plain = host_states(refocus(lens, block, depths, spp, d.stride), S)
    apart = 0.0
    for s in range(S):
        assert plain[s].n_focus_rays == got[s].n_focus_rays and plain[s].flags == 0
        apart = max(apart, abs(plain[s].d_sensor - got[s].d_sensor) / got[s].d_sensor)
    margin(f"{tag}: d_sensor, staged vs plain entry (rel)", apart, fh.tolerances()["d_sensor"])


@pytest.mark.parametrize("entry", ["plain", "staged"])
@pytest.mark.parametrize("name", fh.LENSES)
def test_a_state_without_a_valid_ray_leaves_its_neighbours_alone(repo_root, name, entry):
    """S = 3 with the middle state's object 1 mm in front of the lens: no ray passes, n_focus_rays 0, d_sensor 0/0, hfov 0.5 and flag
    bit 1 for that state; the states beside it have the bits of a launch without it"""
    lens, d = lens_of(repo_root, name), fh.draw_sets(name)[(entry, 1025)]
    S, block = len(fh.DEPTHS), d.block()
    dead = (fh.DEPTHS[0], -1.0, fh.DEPTHS[2])
    if entry == "plain":
        run = lambda dep: refocus(lens, block, dep, d.spp, d.stride)
    else:
        scratch = torch.zeros(S * 64, dtype=torch.uint8, device=DEV)
        run = lambda dep: refocus_staged(lens, block, dep, d.spp, d.stride, len(block), scratch)[0]
    healthy, hit = run(fh.DEPTHS), run(dead)
    st = host_states(hit, S)
    assert st[1].n_focus_rays == 0 and np.isnan(st[1].d_sensor) and st[1].hfov == 0.5 and st[1].flags & 2
    assert st[0].flags == 0 and st[2].flags == 0
    a, b = fields_bits(healthy, S), fields_bits(hit, S)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    if entry == "staged":                                   # and the scratch is fit for the next launch
        assert np.array_equal(fields_bits(run(fh.DEPTHS), S), a)


@pytest.mark.parametrize("n_u", fh.UPLOAD_N)
def test_upload_tail(repo_root, n_u):
    """the upload workgroups of aadff_refocus_staged at lengths that are no multiple of 4 floats, below one float4, and 0: the first n_u
    floats of the pinned block arrive bit for bit, the 8 floats behind them keep their fill, and the focus states do not care"""
    lens, d = lens_of(repo_root, "rf50mm"), fh.draw_sets("rf50mm")[("staged", 5)]
    draws = d.block()[:d.stride]
    block = np.random.default_rng(n_u).random(max(n_u, len(draws)) + 8, dtype=np.float32)
    block[:len(draws)] = draws
    scratch = torch.zeros(64, dtype=torch.uint8, device=DEV)
    states, u_dev = refocus_staged(lens, block, fh.DEPTHS[:1], d.spp, d.stride, n_u, scratch)
    up = u_dev.cpu().numpy()
    assert len(up) == n_u + 8 and np.array_equal(up[:n_u].view(np.int32), block[:n_u].view(np.int32)), "uploaded floats differ"
    assert (up[n_u:] == SENTINEL).all(), "written behind n_u"
    st = host_states(states, 1)[0]
    assert st.n_focus_rays == d.count[0] and st.flags == 0
    assert abs(st.d_sensor - d.d_sensor[0]) <= fh.tolerances()["d_sensor"] * d.d_sensor[0]
