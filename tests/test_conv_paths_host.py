"""CPU: the conditions on the comparators and the case table of tests/test_gpu_conv_paths.py, shown to hold before a kernel is involved
(tests/conv_paths_common.py has the table, the float64 comparator, the restatements and the derived bounds).
  * the float64 oracle equals an independent per-pixel loop of the definition on tiny cases (1e-12);
  * on every case of the table the oracle's own float32 result meets the plain-fp32 bound and a numpy restatement of the fp16 hi + lo
    split meets the matrix-core bound: both budgets are attainable by a correct implementation;
  * two planted errors - one tap dropped at one pixel, one image row read unreflected - fail the comparator under both bounds;
  * the table, read through the restated dispatch, reaches every instantiation of the library except the TIMED ones;
  * the library agrees with the restatement.  The rule itself lives in csrc/conv_plan.cpp (conv_plan: one host function without a HIP
    call, which every entry launches from); aadff_conv_plan_describe runs it and reports the instantiation's name, the workgroup
    count, the slices per workgroup of a wide Toeplitz launch and the timing flag.  Name, spw and workgroups equal what
    conv_paths_common.dispatch and its helpers say on every case of the table and on a sweep over the rule's thresholds; the timing
    flag is set for the slice-batched kernel of the stack entries only; refusals come back as the entries themselves give them; and
    a stand-alone program built from conv_plan.cpp with the address and undefined-behaviour sanitizers walks the corners of the domain.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest
import torch

import conv_paths_common as cp

IDS = [c.id for c in cp.TABLE]


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", cp.TINY, ids=[c.id for c in cp.TINY])
def test_oracle64_equals_a_per_pixel_loop(c):
    img, maps, _ = cp.inputs(c)
    a, b = cp.oracle64(img, maps, c.grid), cp.loop64(img, maps, c.grid)
    assert a.dtype == torch.float64 and a.shape == b.shape == (c.B, c.C, c.S, c.H, c.W)
    assert float((a - b).abs().max()) <= 1e-12
    assert float((cp.definition64(img, maps, c.grid) - b).abs().max()) <= 1e-12        # the tap iteration of the restatements is the same operation
    seq = cp.sums(img, maps, c.grid)[0]
    assert float((seq.double() - b).abs().max()) <= 25 * 2.0 ** -23 * 37.5


@pytest.mark.parametrize("c", cp.TABLE, ids=IDS)
def test_float32_oracle_and_split_restatement_meet_the_bounds(c):
    r = cp.reference(c)
    M = c.S * max(c.L, 1)
    assert r.img.shape == (c.B, c.C, c.H, c.W) and r.maps.shape == (M, c.C, c.grid * c.ks, c.grid * c.ks)
    assert float(r.img.min()) >= -3.0 and float(r.img.max()) < 34.5
    blocks = r.maps.double().reshape(M, c.C, c.grid, c.ks, c.grid, c.ks)
    if c.signed:
        assert bool((r.maps < 0).any()) and bool((r.maps > 0).any())
        norm = blocks.abs().sum((3, 5))
    else:
        assert bool((r.maps > 0).all())
        norm = blocks.sum((3, 5))
    assert bool((((norm - 1).abs() <= 1e-6) | ((norm - 1e-3).abs() <= 1e-9)).all())
    if M * c.C > 1:                                                                   # one slice (one channel of a lone slice) is 1e-3 of the others
        assert float(r.Wmax.min()) < 1e-2 * float(r.Wmax.max())
    o32, rest = cp.host_results(c)
    if c.L:
        idx = (torch.arange(c.S)[None, None, :, None, None] * c.L + r.lidx.long()[:, None, None]).expand(c.B, c.C, c.S, c.H, c.W)
        o32, rest = torch.gather(o32, 2, idx), torch.gather(rest, 2, idx)
        assert int(r.lidx.max()) == c.L - 1 and bool((r.lidx[:, :-1, :-1] != r.lidx[:, 1:, :-1]).all()) and bool((r.lidx[:, :, :-1] != r.lidx[:, :, 1:]).all())
    use32, _, rel32 = cp.compare(c, o32, r, plain=True)
    use_mc, _, rel_mc = cp.compare(c, rest, r, plain=False)
    use_seq, _, _ = cp.compare(c, r.seq, r, plain=True)
    print(f"{c.id}: d32seq {r.d32seq:.3e}; share of the plain bound used by the float32 oracle {use32:.3f} and by the sequential chain "
          f"{use_seq:.3f}; share of the matrix-core bound used by the split restatement {use_mc:.3f} (rel_l2 {rel_mc:.2f} x d32seq)")
    assert use32 <= 1.0 and use_seq <= 1.0 and use_mc <= 1.0
    assert rel32 <= 4.0 and r.d32seq > 0.0


# (one average tap at one pixel is x w ~ 16 / ks^2; the worst-case rounding term ks^2 U sum|x w| ~ 16 ks^2 2^-24 passes it from ks ~ 45 on,
# so the planted cases stop at ks 27; the unreflected row moves whole rows by far more at every ks)
PLANTED = [c for c in cp.TABLE if c.id.startswith(("signed-", "E-ks3-S2-", "F-ks13-S5-", "A-ks21-S2-2x2x82"))]


@pytest.mark.parametrize("c", PLANTED, ids=[c.id for c in PLANTED])
def test_planted_errors_fail_the_comparator(c):
    r = cp.reference(c)
    p = c.ks // 2
    y, x = c.H // 2, c.W // 3                                                         # interior of a patch: no reflection at this pixel
    hb, wb = cp._bounds(c.H, c.grid), cp._bounds(c.W, c.grid)
    pi, pj = max(i for i in range(c.grid) if hb[i] <= y), max(j for j in range(c.grid) if wb[j] <= x)
    u, v = p, p + 1
    drop = r.out64.clone()
    drop[0, -1, -1, y, x] -= r.img[0, -1, y - p + u, x - p + v].double() * r.maps[-1, -1, pi * c.ks + c.ks - 1 - u, pj * c.ks + c.ks - 1 - v].double()
    rowless = cp.definition64(r.img, r.maps, c.grid, clamp_row=True)
    assert float((cp.definition64(r.img, r.maps, c.grid) - r.out64).abs().max()) <= 1e-12
    assert bool((rowless[:, :, :, p:] == cp.definition64(r.img, r.maps, c.grid)[:, :, :, p:]).all())      # rows 0 .. p-1 only
    for name, wrong in (("one tap dropped at one pixel", drop), ("one row unreflected", rowless)):
        for plain in (True, False):
            use, worst, _ = cp.compare(c, wrong.float(), r, plain)
            clean, _, _ = cp.compare(c, r.out64.float(), r, plain)
            print(f"{c.id}: {name}, {'plain' if plain else 'matrix-core'} bound: {use:.1f} x the bound (the rounded oracle itself: {clean:.3f})")
            assert use > 1.0 and clean <= 1.0, (c.id, name, plain)


def test_table_reaches_every_instantiation():
    reached = {}
    for c in cp.TABLE:
        reached.setdefault(cp.dispatch(c)[0], []).append(c.id)
    want = cp.expected_instantiations()
    assert len(want) == 96 and set(reached) == want, sorted(set(reached) ^ want)
    # the names are the library's: its symbol table holds exactly these and the eight TIMED slice-batched ones
    from aadff import _abi
    syms = subprocess.run(["nm", "-C", _abi.LIB_PATH], capture_output=True, text=True).stdout
    have = set(re.findall(r"(conv_psf_map_[a-z_]*kernel(?:<[^>]*>)?)\(", syms))
    timed = {f"conv_psf_map_sbatch_kernel<24, {nc}, {p}, true, false>" for nc in range(1, 5) for p in ("false", "true")}
    assert have == want | timed, sorted(have ^ (want | timed))


def test_cases_are_what_their_comments_say():
    by = {c.id: c for c in cp.TABLE}
    d = lambda cid: cp.dispatch(by[cid])[0]
    args = lambda name: name[name.index("<"):]
    for ks in (21, 13):
        got = [d(f"A-ks{ks}-S1-1x2x{H}x50-g1") for H in (24, 25, 32, 33, 48, 49, 64, 65, 96, 97)]
        assert got == [f"conv_psf_map_blkw_kernel<{ks}, {rb}>" for rb in (24, 32, 32, 48, 48, 32, 32, 48, 48, 32)]
    assert d("A-ks5-S1-1x7x768x96-g8") == "conv_psf_map_blkw_kernel<5, 32>"
    big = [c for c in cp.TABLE if (c.B, c.C, c.grid) == (5, 13, 32)]
    assert len(big) == 4 and all(cp.workgroups_block_gemm(c) == 66560 for c in big)
    assert {cp.dispatch(c)[0] for c in big} == {"conv_psf_map_blkw_kernel<5, 24>", "conv_psf_map_blk_kernel<9, false>", "conv_psf_map_blk_kernel<11, false>"}
    assert d("B-ks11-S1-2x1x192x45-g2") == "conv_psf_map_blk_kernel<11, false>"
    whole = [c for c in cp.TABLE if c.group == "F" and c.grid == 16]
    assert [(cp.toeplitz_slices_per_workgroup(c), args(cp.dispatch(c)[0])) for c in whole] == [(8, "<1, false, 12, 5>"), (4, "<2, true, 20, 10>")]
    tails = [c for c in cp.TABLE if c.group == "F" and c.S in (5, 6)]
    assert len(tails) == 7 and all(cp.toeplitz_slices_per_workgroup(c) == 4 for c in tails)      # two chunks, the second one of 1 or 2 slices
    nw = {c.env["AADFF_CONV_NW"]: cp.dispatch(c)[0] for c in cp.TABLE + cp.NW_IGNORED if "AADFF_CONV_NW" in c.env}
    assert nw == {v: f"conv_psf_map_mfma_kernel<11, {v if v in '1235' else 4}, 1>" for v in ("1", "2", "3", "5", "9", "x")}
    assert cp.dispatch(cp.NW_DEFAULT)[0] == "conv_psf_map_mfma_kernel<11, 4, 1>"
    assert [args(cp.dispatch(c)[0]) for c in cp.TABLE if c.group == "D" and c.ks == 11 and "AADFF_CONV_NW" not in c.env] == [f"<11, {n}, 1>" for n in (1, 2, 3, 4, 5, 3)]
    for fam in cp.FAMILIES:
        assert any(c.signed and cp.dispatch(c)[1] == fam for c in cp.TABLE), fam
        assert any(c.entry == "strided" and cp.dispatch(c)[1] == fam for c in cp.TABLE), fam
        assert fam == "sbatch" or any(c.entry == "psf" and cp.dispatch(c)[1] == fam for c in cp.TABLE), fam


# ------------------------------------------------------------------------------------------------ the library against the restatement
@pytest.fixture(scope="module")
def lib():
    from aadff import _abi
    return _abi.load_library()


def _describe(lib, c, strides=None):
    """aadff_conv_plan_describe for a case under the CURRENT environment: (0, name, {workgroups, block, lds, spw, attach}) or
    (code, message, None) of a refusal.  strides: (stride_bc, stride_s) of the strided entry, default the contiguous stack's."""
    name, info = C.create_string_buffer(96), (C.c_longlong * 5)()
    sbc, ss = strides or (c.S * c.H * c.W, c.H * c.W)
    rc = lib.aadff_conv_plan_describe(c.entry.encode(), c.B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, sbc, ss, name, len(name), info)
    if rc != 0:
        return rc, lib.aadff_last_error().decode(), None
    return 0, name.value.decode(), dict(zip(("workgroups", "block", "lds", "spw", "attach"), info))


def _setenv(monkeypatch, env):
    for k in cp.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _agrees(lib, c):
    """The library's plan of an accepted case equals the restatement; returns False for a refusal (describe's own)."""
    rc, name, info = _describe(lib, c)
    if rc != 0:
        assert rc in (-1, -2) and name, (c.id, rc)
        return False
    want, family = cp.dispatch(c)
    assert name == want, (c.id, name, want)
    if family == "toeplitz_wide":
        assert info["spw"] == cp.toeplitz_slices_per_workgroup(c), c.id
    if family in ("blk", "blkw"):
        assert info["workgroups"] == cp.workgroups_block_gemm(c), c.id
    # the events of aadff_time_next_launch ride on the slice-batched kernel of the stack entries, and on nothing else
    assert info["attach"] == (name.startswith("conv_psf_map_sbatch_kernel<") and c.entry in ("stack", "strided")), (c.id, name)
    return True


ALL_CASES = cp.TABLE + cp.NW_IGNORED + [cp.NW_DEFAULT] + cp.TINY


@pytest.mark.parametrize("c", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_library_plan_equals_the_restated_dispatch(lib, monkeypatch, c):
    _setenv(monkeypatch, c.env)
    assert _agrees(lib, c), "a case of the table is refused"
    _, name, info = _describe(lib, c)
    assert info["workgroups"] >= 1 and info["block"] in (64, 128, 192, 256, 320) and 0 <= info["lds"] <= 64 * 1024 - 64
    assert (info["spw"] > 0) == ("toeplitz_wide" in name)


# The sweep: every odd ks, S across the chunking thresholds of every family (4 / 8 / 12 maps per slice-batched workgroup, the wave
# counts 1 - 5), the band-height thresholds of the block-GEMM rule and their neighbours, patches narrower and wider than a 96-column
# band.  Thinned so that it runs in seconds, every threshold kept: all H at W 50, the other widths at four heights; the switches
# that only some kernel sizes read (BLKW / BLKW_RB: 3..21, NW and PAIR: 11) at those sizes and their neighbours; four shapes where
# AADFF_CONV_PATH is set, which takes the block-GEMM rule - the only one that reads the patch height - out of the decision.
SWEEP_H = (24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 147, 768)
SWEEP_HW = [(H, 50) for H in SWEEP_H] + [(H, W) for H in (24, 97, 147, 768) for W in (96, 202)]
SWEEP_HW_PATH = [(24, 50), (97, 96), (147, 202), (768, 50)]
SWEEP_ENVS = [((), range(1, 52, 2), SWEEP_HW)] + [((("AADFF_CONV_PATH", v),), range(1, 52, 2), SWEEP_HW_PATH) for v in ("valu", "toeplitz")]
SWEEP_ENVS += [((("AADFF_CONV_BLKW", v),), range(1, 24, 2), SWEEP_HW) for v in ("0", "1")]
SWEEP_ENVS += [((("AADFF_CONV_BLKW", "1"), ("AADFF_CONV_BLKW_RB", rb)), range(1, 24, 2), SWEEP_HW) for rb in ("24", "32", "48")]
SWEEP_ENVS += [((("AADFF_CONV_PAIR", "1"),), (9, 11, 13), SWEEP_HW_PATH)] + [((("AADFF_CONV_NW", str(v)),), (9, 11, 13), SWEEP_HW_PATH) for v in range(1, 6)]


def test_library_plan_equals_the_restated_dispatch_on_a_sweep(lib, monkeypatch):
    done = refused = 0
    for env, sizes, shapes in SWEEP_ENVS:
        _setenv(monkeypatch, dict(env))
        for ks, S, grid, (H, W) in itertools.product(sizes, range(1, 18), (1, 2, 7, 11, 32), shapes):
            ok = _agrees(lib, cp._case("sweep", ks, S, dict(env), B=1, C=2, H=H, W=W, grid=grid))
            done += ok
            refused += not ok
    print(f"sweep: {done} plans equal the restated dispatch, {refused} shapes skipped because the library refuses them")
    assert done > 50000 and refused < done


def test_forced_block_gemm_of_a_ks11_stack_does_not_attach_the_events(lib, monkeypatch):
    c = cp._case("timing", 11, 5, B=1, C=3, H=256, W=256, grid=5)
    _setenv(monkeypatch, {})
    assert _describe(lib, c)[1:] == ("conv_psf_map_sbatch_kernel<24, 2, false, false, false>", dict(workgroups=5 * 1 * 5 * 3 * 3, block=128, lds=0, spw=0, attach=1))
    _setenv(monkeypatch, {"AADFF_CONV_BLKW": "1"})
    rc, name, info = _describe(lib, c)
    assert rc == 0 and name.startswith("conv_psf_map_blkw_kernel<11, ") and info["attach"] == 0
    _setenv(monkeypatch, {})
    assert _describe(lib, c._replace(entry="strided"))[2]["attach"] == 1
    assert _describe(lib, c._replace(entry="layered", L=2))[1:] == ("conv_psf_map_sbatch_kernel<24, 3, false, false, true>", dict(workgroups=5 * 1 * 5 * 3 * 3, block=192, lds=0, spw=0, attach=0))


def test_refusals_are_the_entries_own(lib, monkeypatch):
    """The refusals tests/test_gpu_parity.py and tests/test_abi_symbols.py pin on the entries (even ks, a grid above the image or above
    AADFF_MAX_GRID, strides below one plane, overlapping planes, the layered entry at another ks): describe returns the code and sets the
    message of the entry itself, which refuses before its first HIP call - so both run here, the entry with dummy pointers."""
    _setenv(monkeypatch, {})
    p = C.c_void_p(8)
    HW = 128 * 128
    cases = [
        (cp._case("r", 4, 1, B=1, C=3, H=32, W=32, grid=2), None, -1, "PSF kernel size should be odd"),
        (cp._case("r", 3, 1, B=1, C=3, H=32, W=32, grid=40), None, -1, "render_psf_map: grid 40 larger than image 32x32"),
        (cp._case("r", 3, 1, B=1, C=3, H=64, W=64, grid=100), None, -1, "render_psf_map: grid 100 outside [1,64]"),
        (cp._case("r", 11, 2, entry="strided", B=1, C=3, H=128, W=128, grid=2), (HW, HW), -1,
         "render_psf_map_stack_strided: planes overlap (stride_bc 16384, stride_s 16384, B*C 3, S 2)"),
        (cp._case("r", 11, 2, entry="strided", B=1, C=1, H=128, W=128, grid=2), (HW - 1, 2 * HW), -1,
         "render_psf_map_stack_strided: strides 16383 / 32768 below one plane (128 x 128)"),
        (cp._case("r", 9, 2, entry="layered", L=3, B=1, C=3, H=64, W=64, grid=2), None, -2,
         "render_psf_map_stack_layered: the fused form exists for ks 11 only (ks 9: compose aadff_render_psf_map_stack and a gather)"),
        (cp._case("r", 11, 2, entry="stack", B=1, C=3, H=5, W=64, grid=2), None, -1, "render_psf_map: reflect padding 5 needs H,W > pad"),
        (cp._case("r", 11, 4, entry="stack", B=1, C=1, H=8192, W=16385, grid=2), None, -1,
         "render_psf_map: image planes above 2^27 pixels / slice strides above 2^28 elements are not supported on the stack path"),
    ]
    for c, strides, code, msg in cases:
        assert _describe(lib, c, strides) == (code, msg, None), c.id
        sbc, ss = strides or (c.S * c.H * c.W, c.H * c.W)
        shape = (c.B, c.C, c.S, c.H, c.W, c.grid, c.ks, None)
        if c.entry == "map":
            rc = lib.aadff_render_psf_map(p, p, p, c.B, c.C, c.H, c.W, c.grid, c.ks, None)
        elif c.entry == "stack":
            rc = lib.aadff_render_psf_map_stack(p, p, p, *shape)
        elif c.entry == "strided":
            rc = lib.aadff_render_psf_map_stack_strided(p, p, p, sbc, ss, *shape)
        else:
            rc = lib.aadff_render_psf_map_stack_layered(p, p, p, p, c.B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, None)
        assert (rc, lib.aadff_last_error().decode()) == (code, msg), c.id
    assert lib.aadff_conv_plan_describe(b"stacked", 1, 1, 1, 1, 8, 8, 1, 3, 0, 0, C.create_string_buffer(8), 8, (C.c_longlong * 5)()) == -1


def test_sanitized_walk_of_the_plan(tmp_path, repo_root):
    """tests/conv_plan_walk.cpp + csrc/conv_plan.cpp as an ordinary executable under the address and undefined-behaviour sanitizers
    (runtimes linked statically: nothing is preloaded): grid = AADFF_MAX_GRID, ks = AADFF_MAX_KS, B*C = 65535, S up to 64, planes at
    and just past 2^27 and 2^30 pixels, H = W = grid, under every switch."""
    csrc = os.path.join(repo_root, "aberration-aware-depth-from-focus_amd", "csrc")
    exe = tmp_path / "conv_plan_walk"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(repo_root, "include"), "-I", csrc,
                           os.path.join(csrc, "conv_plan.cpp"), os.path.join(repo_root, "tests", "conv_plan_walk.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and re.fullmatch(r"conv_plan_walk: \d+ plans, \d+ refused\n", run.stdout) and not run.stderr
