"""CPU: the conditions on the comparators of tests/test_gpu_local_gather.py, shown to hold before anything runs on a GPU
(tests/local_gather_common.py has the cases, the float64 comparator, the float32 restatements and the derived bound).
  * the sequential float32 restatement is within the derived elementwise bound of the float64 oracle on every element of every case,
    and d32seq, the unit of every relative-L2 budget, is > 0;
  * the float64 oracle equals an independent per-pixel double loop (it is not unfold arithmetic compared with itself);
  * the LDS requests the case list quotes are the ones the host code computes, and the admission rule refuses what it should;
  * thin-lens cases: the excluded share is <= 0.5 % and the restatement is finite (and has a d32seq > 0).
"""
import ctypes as C

import pytest
import torch

import local_gather_common as lg
import thinlens_grad_common as tc

IDS = [lg.case_id(c, s) for c, s in lg.ALL_CASES]


@pytest.mark.parametrize("case,signed", lg.ALL_CASES, ids=IDS)
def test_sequential32_is_within_the_derived_bound(case, signed):
    B, Cn, H, W, ks = case
    img, psf, out64, A, d32seq = lg.reference(case, signed)
    assert img.shape == (B, Cn, H, W) and psf.shape == (B, H, W, ks, ks) and img.dtype == psf.dtype == torch.float32
    assert float(img.min()) >= -1.0 and float(img.max()) < 3.0
    if signed:
        assert bool((psf < 0).any()) and bool((psf > 0).any())
    else:
        assert bool((psf > 0).all()) and float((psf.double().sum((-1, -2)) - 1).abs().max()) <= 1e-6
    seq = lg.reference_seq(case, signed)
    bound = lg.elementwise_bound(ks * ks, A, out64)
    use = float(((seq.double() - out64).abs() / bound).max())
    print(f"{lg.case_id(case, signed)}: d32seq {d32seq:.3e}, largest use of the elementwise bound {use:.3f}")
    assert torch.isfinite(seq).all() and use <= 1.0
    if ks > 1:
        assert d32seq > 0.0
    else:                                                                    # normalised 1 x 1 PSFs are 1.0: the gather is the identity
        assert torch.equal(seq, img)


@pytest.mark.parametrize("case,signed", [((2, 3, 2, 3, 3), False), ((1, 2, 4, 5, 5), True)], ids=["2x3x2x3_ks3", "1x2x4x5_ks5_signed"])
def test_oracle64_equals_a_per_pixel_loop(case, signed):
    img, psf = lg.inputs(case, 1, signed)
    a, b = lg.oracle64(img, psf, case[4]), lg.loop64(img, psf, case[4])
    assert a.dtype == torch.float64 and a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-14                               # |out| < 3, 25 terms: a few ulp of float64
    seq, A = lg.sequential32(img, psf, case[4])
    assert float((seq.double() - b).abs().max()) <= 1e-5                     # the restatement is the same operation
    x, w = img.double(), psf.double()
    p = case[4] // 2
    pad = torch.nn.functional.pad(x, (p, p, p, p), mode="replicate")
    want_A = sum((pad[:, :, u:u + case[2], v:v + case[3]] * w[:, None, :, :, u, v]).abs() for u in range(case[4]) for v in range(case[4]))
    assert float((A - want_A).abs().max()) <= 1e-14


def test_lds_requests_and_the_admission_rule():
    """The generic cases ask for the LDS the list says (one below and several above the 64 KB default, the last one just under the
    160 KB rule), and the rule itself is checked through the C entry without a GPU: validation comes before any launch."""
    want = {(1, 5, 6, 70, 11): 47256, (1, 1, 6, 70, 15): 62280, (1, 3, 6, 70, 15): 71640, (2, 3, 5, 40, 21): 37296, (1, 3, 5, 20, 31): 78616}
    for case, nbytes in want.items():
        assert lg.generic_lds_bytes(case) == nbytes, (case, lg.generic_lds_bytes(case))
    assert lg.generic_lds_bytes((1, 1, 6, 70, 15)) <= 64 * 1024 < lg.generic_lds_bytes((1, 3, 6, 70, 15))
    assert lg.generic_lds_bytes((1, 1, 5, 20, 47)) == 153032 <= 160 * 1024
    assert [lg.generic_lds_bytes(c) for c in lg.REFUSED_CASES] == [164688, 179928]
    from aadff import _abi
    lib = _abi.load_library()
    P8 = C.c_void_p(8)                                                       # never dereferenced: the shape check refuses first
    for (B, Cn, H, W, ks) in lg.REFUSED_CASES:
        assert lib.aadff_local_psf_render(P8, P8, P8, B, Cn, H, W, ks, None) == -1
        msg = lib.aadff_last_error()
        assert b"LDS" in msg and str(lg.generic_lds_bytes((B, Cn, H, W, ks))).encode() in msg, msg


def test_case_list_reaches_what_it_should():
    cs = lg.CASES
    for ks in lg.TEMPLATED_KS:
        assert (2, 3, 9, 132, ks) in cs and (2, 3, 9, 131, ks) in cs
    assert {c[1] for c in cs} == {1, 2, 3, 4}
    assert any(c[3] % 4 == 0 and c[3] > 128 for c in cs) and any(c[3] % 4 and c[3] > 128 for c in cs)
    # exactly one full run: the last 1 KiB piece of the 64 * ks^2 * 4 bytes is partial
    assert [(-(-64 * ks * ks * 4 // 1024), 64 * ks * ks * 4 % 1024 != 0) for ks in (5, 11, 13)] == [(7, True), (31, True), (43, True)]
    assert {c[4] for c in lg.GENERIC_CASES} == {1, 11, 15, 21, 31, 47} and any(c[1] > 4 for c in lg.GENERIC_CASES)


def test_sequential_chain_against_torch_float32():
    """Why d32seq and not the oracle's float32 distance is the unit: the ratio grows with ks (printed)."""
    ratios = {}
    for case in ((2, 3, 9, 131, 3), (2, 3, 9, 131, 7), (2, 3, 9, 131, 11), (2, 3, 9, 131, 13), (1, 3, 6, 70, 15), (2, 3, 5, 40, 21),
                 (1, 3, 5, 20, 31), (1, 1, 5, 20, 47)):
        ratios[case[4]] = lg.ratio_to_torch_float32(case)
    print("d32seq / d32 of oracle.conv.local_psf_render in float32: " + ", ".join(f"ks {k}: {v:.2f}" for k, v in ratios.items()))
    assert ratios[3] < 1.5 and ratios[31] > 4.0                              # 4 x d32 of the oracle cannot serve both ends


THIN_IDS = [c[0] for c in lg.THIN_CASES]


@pytest.mark.parametrize("case", lg.THIN_CASES, ids=THIN_IDS)
def test_thin_lens_conditions(case):
    img, depth, fds, keep, share, out64, seq, d32seq = lg.thin_reference(case)
    o32 = tc.oracle_grads(case, img, depth, fds, torch.zeros_like(out64, dtype=torch.float32), torch.float32)[0]
    d32 = lg.rel_l2(o32[keep], out64[keep])
    print(f"{case[0]}: excluded share {share:.5%}; d32seq {d32seq:.3e}; oracle float32 {d32:.3e}; ratio {d32seq / d32:.2f}")
    assert share <= tc.MAX_MASKED
    assert seq.shape == out64.shape and seq.dtype == torch.float32 and torch.isfinite(seq).all()
    assert 0.0 < d32seq <= 1e-6                                              # the restatement is the oracle's operation, at float32 accuracy


def test_thin_lens_cases_span_what_they_should():
    cs = lg.THIN_CASES
    assert len(cs) == 9 and {c[6] for c in cs} == {3, 5, 7, 9, 11, 13} and {c[2] for c in cs} == {1, 2, 3, 4}
    assert min(c[5] for c in cs) == 17 and max(c[5] for c in cs) == 131 and {c[10] for c in cs} == {-1, 1}
