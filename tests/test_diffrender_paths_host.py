"""CPU: the conditions on the comparator, the bounds and the case table of tests/test_gpu_diffrender_paths.py, shown to hold before a kernel
is involved (tests/diffrender_paths_common.py has the table, the float64 comparator, the definitions, the restated summation tree and the
derived bounds).
  * the float64 autograd of the oracle equals the definition written as Python loops on the tiny cases and tap by tap in numpy on every
    case, to 1e-12 of the sum of the absolute values of an element's terms;
  * A > 0 and N >= 1 everywhere; N is what the kernels' comments say it is;
  * the oracle's own float32 autograd meets every bound, and a numpy float32 restatement of the summation tree of map_dpsf_partial_kernel /
    map_dpsf_sum_kernel meets the depth bound of d_psf: the bounds are attainable by a correct implementation;
  * eight planted errors (modified float64 references) fail their bound on every case on which they change anything;
  * the cases are what their reasons say.
"""
import pytest
import torch

import diffrender_paths_common as dp

IDS = [c.id for c in dp.CASES]


def test_the_table_is_the_one_that_was_set():
    assert len(set(IDS)) == len(IDS)
    assert [(c.B, c.C, c.S, c.H, c.W, c.grid, c.ks) for c in dp.MAP_CASES] == [
        (2, 2, 2, 6, 7, 1, 11), (1, 2, 2, 12, 13, 3, 11), (1, 1, 1, 23, 25, 11, 11), (2, 3, 2, 33, 97, 3, 11), (1, 1, 1, 96, 96, 2, 11),
        (1, 1, 1, 96, 96, 2, 5), (2, 2, 2, 4, 5, 1, 7), (1, 2, 1, 97, 33, 3, 5), (2, 1, 2, 27, 29, 2, 51), (1, 1, 1, 64, 65, 64, 3), (1, 2, 2, 5, 6, 2, 1)]
    assert [(c.B, c.C, c.H, c.W, c.ks) for c in dp.LOCAL_CASES] == [
        (2, 3, 3, 131, 11), (1, 3, 9, 70, 21), (1, 2, 1, 70, 5), (1, 1, 5, 1, 5), (1, 8, 2, 64, 5), (2, 5, 4, 66, 7), (1, 4, 3, 65, 3),
        (2, 3, 2, 3, 13), (1, 1, 1, 1, 13), (1, 2, 4, 9, 1), (1, 1, 5, 20, 47)]
    assert all(c.why for c in dp.CASES)


@pytest.mark.parametrize("c", dp.TINY, ids=[c.id for c in dp.TINY])
def test_comparator_equals_the_loop_definition(c):
    r = dp.reference(c)
    li, lp = dp.loop64(c, r.img, r.psf, r.dy)
    assert li.shape == r.gi.shape == r.img.shape and lp.shape == r.gp.shape == r.psf.shape and r.gi.dtype == r.gp.dtype == torch.float64
    assert bool(((li - r.gi).abs() <= 1e-12 * r.Ai).all()) and bool(((lp - r.gp).abs() <= 1e-12 * r.Ap).all())


@pytest.mark.parametrize("c", dp.CASES, ids=IDS)
def test_comparator_equals_the_tap_by_tap_definition(c):
    r = dp.reference(c)
    di, dpsf = dp.definition64(c, r.img, r.psf, r.dy)
    assert bool(((di - r.gi).abs() <= 1e-12 * r.Ai).all()) and bool(((dpsf - r.gp).abs() <= 1e-12 * r.Ap).all())
    # A and N are the same sums over |terms| and over ones
    ai, ap = dp.definition64(c, r.img.abs(), r.psf.abs(), r.dy.abs())
    ni, npsf = dp.definition64(c, torch.ones_like(r.img), torch.ones_like(r.psf), torch.ones_like(r.dy))
    assert bool(((ai - r.Ai).abs() <= 1e-12 * r.Ai).all()) and bool(((ap - r.Ap).abs() <= 1e-12 * r.Ap).all())
    assert torch.equal(ni.round(), r.Ni.round()) and torch.equal(npsf.round(), r.Np.round())


@pytest.mark.parametrize("c", dp.CASES, ids=IDS)
def test_inputs_and_term_counts(c):
    r = dp.reference(c)
    assert float(r.img.min()) >= -1.0 and float(r.img.max()) < 3.0
    assert bool((r.psf < 0).any()) and bool((r.psf > 0).any())
    if c.op == "map":
        norm = r.psf.double().reshape(c.S, c.C, c.grid, c.ks, c.grid, c.ks).abs().sum((3, 5))
    else:
        norm = r.psf.double().abs().sum((-1, -2))
    assert bool(((norm - 1).abs() <= 1e-6).all())
    assert bool((r.Ai > 0).all()) and bool((r.Ap > 0).all())
    assert bool(((r.Ni - r.Ni.round()).abs() <= 1e-9).all()) and bool(((r.Np - r.Np.round()).abs() <= 1e-9).all())
    assert float(r.Ni.min()) >= 1 - 1e-9 and float(r.Np.min()) >= 1 - 1e-9
    if c.op == "map":                                                        # d_psf: B x the pixels of the element's patch; d_img: S ks^2 on average
        hb, wb = dp.oconv.patch_bounds(c.H, c.grid), dp.oconv.patch_bounds(c.W, c.grid)
        for i in range(c.grid):
            for j in range(c.grid):
                blk = r.Np[:, :, i * c.ks:(i + 1) * c.ks, j * c.ks:(j + 1) * c.ks]
                assert bool((blk.round() == c.B * (hb[i + 1] - hb[i]) * (wb[j + 1] - wb[j])).all())
        assert round(float(r.Ni.sum())) == c.B * c.C * c.S * c.H * c.W * c.ks * c.ks
    else:
        assert bool((r.Np.round() == c.C).all())
        assert round(float(r.Ni.sum())) == c.B * c.C * c.H * c.W * c.ks * c.ks


@pytest.mark.parametrize("c", dp.CASES, ids=IDS)
def test_float32_oracle_meets_the_bounds(c):
    r = dp.reference(c)
    bi, bp = dp.bounds(c, r)
    ui, ii, _, _ = dp.share(r.gi32, r.gi, bi)
    up, ip, _, _ = dp.share(r.gp32, r.gp, bp)
    ri, rp = dp.share(r.gi.float(), r.gi, bi)[0], dp.share(r.gp.float(), r.gp, bp)[0]
    print(f"{c.id}: share of the bound used by the oracle's float32 autograd: d_img {ui:.4f} at {ii}, d_psf {up:.4f} at {ip}; by the rounded "
          f"float64 result {ri:.4f}, {rp:.4f}; in units of u A: d_img {float(((r.gi32.double() - r.gi).abs() / (dp.U * r.Ai)).max()):.2f}, "
          f"d_psf {float(((r.gp32.double() - r.gp).abs() / (dp.U * r.Ap)).max()):.2f}")
    assert ui <= 1.0 and up <= 1.0 and ri <= 1.0 and rp <= 1.0


@pytest.mark.parametrize("c", dp.MAP_CASES, ids=[c.id for c in dp.MAP_CASES])
def test_restated_summation_tree_meets_the_depth_bound(c):
    r = dp.reference(c)
    tree = dp.dpsf_tree32(c, r.img, r.dy)
    assert tree.dtype == torch.float32
    use, idx, err, b = dp.share(tree, r.gp, dp.bounds(c, r)[1])
    print(f"{c.id}: the float32 tree of map_dpsf_partial_kernel + map_dpsf_sum_kernel uses {use:.4f} of (min(D, N) + 2) u A (element {idx}: {err:.3e} of {b:.3e}); "
          f"D = {int(dp.dpsf_depth(c).min())} .. {int(dp.dpsf_depth(c).max())}")
    assert use <= 1.0


_PLANTED = {}


def _planted(c):
    """[(name, tensor, elements changed, largest share of the bound, its index, elements over their bound)] of a case, computed once."""
    if c.id not in _PLANTED:
        r = dp.reference(c)
        bi, bp = dp.bounds(c, r)
        rows = []
        for name, tensor in dp.plants(c).items():
            wi, wp = dp.definition64(c, r.img, r.psf, r.dy, plant=name)
            wrong, right, bound, a = (wi, r.gi, bi, r.Ai) if tensor == "d_img" else (wp, r.gp, bp, r.Ap)
            other, other_right, other_a = (wp, r.gp, r.Ap) if tensor == "d_img" else (wi, r.gi, r.Ai)
            assert bool(((other - other_right).abs() <= 1e-12 * other_a).all()), (c.id, name)       # a plant touches its own tensor only
            changed = int(((wrong - right).abs() > 1e-12 * a).sum())
            use, idx, _, _ = dp.share(wrong.float(), right, bound)
            over = int((((wrong.float().double() - right).abs() / bound) > 1.0).sum())
            rows.append((name, tensor, changed, use, idx, over))
        _PLANTED[c.id] = rows
    return _PLANTED[c.id]


@pytest.mark.parametrize("c", dp.CASES, ids=IDS)
def test_planted_errors_fail_their_bound(c):
    for name, tensor, changed, use, idx, over in _planted(c):
        print(f"{c.id}: {name}: {changed} elements of {tensor} change, {over} exceed their bound, the worst {use:.3g} x ({idx})")
        assert use > 1.0 if changed else use <= 1.0, (c.id, name, use)


def test_every_planted_error_changes_the_cases_it_should():
    by = {}
    for c in dp.CASES:
        for name, _, changed, _, _, _ in _planted(c):
            by.setdefault(name, set())
            if changed:
                by[name].add(c.id)
    assert set(by) == set(dp.MAP_PLANTS) | set(dp.LOCAL_PLANTS) and all(by.values())
    tallest = lambda c: max(b - a for a, b in zip(dp.oconv.patch_bounds(c.H, c.grid), dp.oconv.patch_bounds(c.H, c.grid)[1:]))      # noqa: E731
    # every case with ks > 1 has folded / clamped terms, every seam needs the right patch, every sum its last item
    assert by["corner mirror terms dropped"] == {c.id for c in dp.MAP_CASES if c.ks > 1}
    assert by["d_psf window replicated"] == {c.id for c in dp.MAP_CASES if c.ks > 1}
    assert by["PSF of the target pixel's patch"] == {c.id for c in dp.MAP_CASES if c.grid > 1 and c.ks > 1}
    assert by["slice 0's PSF for every slice"] == {c.id for c in dp.MAP_CASES if c.S > 1}
    assert by["d_psf over batch item 0 only"] == {c.id for c in dp.MAP_CASES if c.B > 1}
    assert by["last row of each 32-row tile dropped"] == {c.id for c in dp.MAP_CASES if tallest(c) >= 32}
    assert by["zero padding in d_img"] == {c.id for c in dp.LOCAL_CASES if c.ks > 1}
    assert by["d_psf over C - 1 channels"] == {c.id for c in dp.LOCAL_CASES}


def test_cases_are_what_their_reasons_say():
    by = {c.id: c for c in dp.CASES}
    widths = lambda n, g: [b - a for a, b in zip(dp.oconv.patch_bounds(n, g), dp.oconv.patch_bounds(n, g)[1:])]      # noqa: E731
    assert dp.oconv.patch_bounds(97, 3) == [0, 32, 64, 97] and widths(97, 3) == [32, 32, 33] and widths(33, 3) == [11, 11, 11]
    c = by["map-2x3x2x33x97-g3-ks11"]
    tyn, txn, nty, ntx = dp.tiles(c)
    assert (tyn, txn, nty, ntx) == ([1, 1, 1], [1, 1, 2], 1, 2)                    # the workspace holds 2 slabs per (b, patch row); two patch columns write one
    assert dp.workspace_bytes(c) == 2 * 2 * 1 * 2 * 3 * 9 * 121 * 4
    assert -(-c.H // dp.BT) == 2 and c.H - dp.BT == 1                             # d_img: a second tile row of one image row
    c = by["map-1x2x1x97x33-g3-ks5"]
    assert dp.tiles(c)[:2] == ([1, 1, 2], [1, 1, 1])
    for cid in ("map-2x2x2x6x7-g1-ks11", "map-2x2x2x4x5-g1-ks7"):                 # H = p + 1: rows 1 .. H - 2 are mirrored at both ends
        c = by[cid]
        p = c.ks // 2
        assert c.H == p + 1 and [y for y in range(c.H) if 1 <= y <= p and c.H - 1 - p <= y <= c.H - 2] == list(range(1, c.H - 1))
        assert [x for x in range(c.W) if 1 <= x <= p and c.W - 1 - p <= x <= c.W - 2] == list(range(1, c.W - 1))
        assert c.B > 1 and c.C > 1 and c.S > 1
    assert by["map-2x2x2x6x7-g1-ks11"].H <= 16                                    # waves 2 and 3 (rows 16 ..) have no row in the image
    assert sorted(set(widths(12, 3) + widths(13, 3))) == [4, 5] and sorted(set(widths(23, 11) + widths(25, 11))) == [2, 3]
    assert widths(96, 2) == [48, 48]                                               # tile (1, 1) = rows / columns 32 .. 63 straddles 48 and is >= 6 from every border
    assert widths(64, 64) == [1] * 64 and sorted(set(widths(65, 64))) == [1, 2]
    c = by["map-2x1x2x27x29-g2-ks51"]
    assert c.ks // 2 >= c.H - 1 - c.ks // 2 and float(dp.reference(c).Ni.max()) == 5618.0
    big = by["local-1x1x5x20-ks47"]                                               # (1 + u)^R - 1 <= (R + 2) u needs R <= 8192: N everywhere but here
    assert max(float(dp.reference(k).Ni.max()) for k in dp.CASES if k is not big) == 5618.0 <= 8192
    assert float(dp.reference(big).Ni.max()) == 31900.0 == float(dp.reference(big).Ni[0, 0, 0, 0]) == sum(24 - y for y in range(5)) * sum(24 - x for x in range(20))
    assert 24 * sum(24 - x for x in range(20)) + big.H == 6965 <= 8192            # the longest fmaf chain of gather_adjoint (dy row 0) and the row additions
    # the gather
    r = dp.reference(by["local-1x3x9x70-ks21"])
    assert float(r.Ni.max()) == 4158.0 == float(r.Ni[0, 0, 0, 0])
    assert float(dp.reference(by["local-1x1x1x1-ks13"]).Ni.max()) == 169.0
    assert by["local-1x8x2x64-ks5"].C == 2 * 4 and by["local-2x5x4x66-ks7"].C == 4 + 1 and by["local-1x8x2x64-ks5"].W == 64
    assert dp.lg.generic_lds_bytes((1, 1, 5, 20, 47)) <= 160 * 1024 < dp.lg.generic_lds_bytes((1, 2, 5, 20, 47))
    assert {dp.kernels(c)[t] for c in dp.CASES for t in ("d_img", "d_psf")} == {
        "map_dimg<11>", "map_dimg<0>", "map_dpsf<11>", "map_dpsf<1>", "local_dimg", "local_dpsf<11>", "local_dpsf<0>"}
