"""CPU: the conditions on the comparators and the case table of tests/test_gpu_conv_paths.py, shown to hold before a kernel is involved
(tests/conv_paths_common.py has the table, the float64 comparator, the restatements and the derived bounds).
  * the float64 oracle equals an independent per-pixel loop of the definition on tiny cases (1e-12);
  * on every case of the table the oracle's own float32 result meets the plain-fp32 bound and a numpy restatement of the fp16 hi + lo
    split meets the matrix-core bound: both budgets are attainable by a correct implementation;
  * two planted errors - one tap dropped at one pixel, one image row read unreflected - fail the comparator under both bounds;
  * the table, read through the restated dispatch, reaches every instantiation of the library except the TIMED ones.
"""
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
