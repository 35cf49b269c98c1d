"""CPU tests of tests/fit_common.py, the float64 reference and stage checkers of the bf16 fit step: a float32
emulation with the kernels' rounding points passes every stage on every case of tests/test_gpu_fit_stages.py, under the 1 % caps,
and each planted error is rejected by the stage it belongs to and by no earlier one.  That is the evidence that the GPU tests
would notice a subtly wrong kernel; nothing here touches a GPU."""
import numpy as np
import pytest
import torch

import fit_common as fc

FORMS = [pytest.param(True, id="chain"), pytest.param(False, id="layers")]
LR0, T_MAX, BETAS, EPS, WD = 1e-3, 20, (0.9, 0.999), 1e-8, 0.01


def test_bf_is_one_rounding_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-39, torch.randn(1024, generator=g) * 1e30,
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134])])
    assert torch.equal(fc.bf(x.double()), x.to(torch.bfloat16).double())
    # a float64 just above a tie rounds up although its float32 rounding sits ON the tie (which would then go to even)
    assert float(fc.bf(torch.tensor(1.00390625 + 2.0 ** -40, dtype=torch.float64))) == 1.0078125


ALL = dict(fc.CASES, one_layer=fc.ONE_LAYER)
# the chain form exists for 2..16 layers; FusedFit runs everything else in the layer form
RUNS = [pytest.param(n, c, id=f"{n}-{'chain' if c else 'layers'}") for n, (w, _) in ALL.items() for c in (True, False)
        if not c or 2 <= len(w) - 1 <= 16]


@pytest.mark.parametrize("name,chain", RUNS)
def test_emulation_passes_every_stage(name, chain):
    widths, B = ALL[name]
    out = fc.check_all(fc.emulate(fc.make_case(widths, B), chain))
    # the float32 emulation stays far below the 1 % caps (at most 0.017 % in any stage)
    for k, (value, tol) in out.items():
        if k.endswith("share"):
            assert value <= tol / 10, (k, value)
    if not chain:
        assert out["sigmoid share"][0] == 0


@pytest.mark.parametrize("chain", FORMS)
@pytest.mark.parametrize("mutation", list(fc.MUTATIONS))
def test_planted_error_is_rejected_by_its_stage(mutation, chain):
    widths, B = fc.CASES["B"]
    with pytest.raises(fc.StageFailure) as e:
        fc.check_all(fc.emulate(fc.make_case(widths, B), chain, mutate=mutation))
    assert e.value.stage == fc.MUTATIONS[mutation], str(e.value)


def test_padding_is_checked_where_the_batch_has_none():
    widths, B = fc.CASES["A"]                                    # batch 128 = its leading dimension: the error sits in p16
    with pytest.raises(fc.StageFailure) as e:
        fc.check_all(fc.emulate(fc.make_case(widths, B), False, mutate="padding_nonzero"))
    assert e.value.stage == "input"


@pytest.mark.parametrize("rounded", [True, False])
def test_dense_head_emulation_passes_stage_three(rounded):
    """The shapes of the aadff_psfnet_head_loss_grad test, shares pooled over them as there; the unrounded sigmoid (the fp32
    variant's) must not pass as the bf16 one."""
    pools = {"sigmoid": fc._Pool(), "dz": fc._Pool()}
    for B in (1, 3):
        for N in (1, 64, 65, 121, 128):
            g = torch.Generator().manual_seed(B * 1000 + N)
            z = ((torch.rand(B, N, generator=g) * 2 - 1) * 6).to(torch.bfloat16)
            t = torch.rand(B, N, generator=g)
            t = t / t.sum(-1, keepdim=True)
            pred, dz = fc.head32(z, t, B, rounded=rounded)
            args = (z.double(), z.double(), z.double(), pred.double(), t.double(), dz.to(torch.bfloat16).double(), B, True)
            if rounded:
                fc.check_head_values(*args, pools=pools)
            elif N > 1:                                          # N = 1: pred is s / s = 1 however s is rounded
                with pytest.raises(fc.StageFailure):
                    fc.check_head_values(*args, pools=pools)
    if rounded:
        out = fc.judge_head_pools(pools)
        assert out["sigmoid share"][0] == 0 and out["head dz share"][0] <= fc.SHARE_CAP


@pytest.mark.parametrize("t", [0, 1, T_MAX - 1, T_MAX, T_MAX + 5])
def test_schedule_scalars_emulation_is_within_one_ulp(t):
    """adamw_prepare rounds lr, the bias correction and their quotient to fp32 one after the other; at the steps the GPU test
    looks at, that stays within 1 ulp of the float64 closed form."""
    fc.check_scal(fc.scal_emulated(t, LR0, T_MAX, *BETAS, WD), t, LR0, T_MAX, *BETAS, WD)
    if t >= T_MAX:
        assert fc.scal_emulated(t, LR0, T_MAX, *BETAS, WD)[[0, 3]].tolist() == [0.0, 0.0]
    with pytest.raises(fc.StageFailure):
        fc.check_scal(fc.scal_emulated(t + 1, LR0, T_MAX, *BETAS, WD), t, LR0, T_MAX, *BETAS, WD)


def test_adamw_checker_accepts_float32_and_rejects_a_missing_decay():
    g = torch.Generator().manual_seed(5)
    p, gr, m = torch.randn(5000, generator=g), torch.randn(5000, generator=g) * 1e-3, torch.randn(5000, generator=g) * 1e-3
    v = (torch.randn(5000, generator=g) * 1e-3) ** 2
    scal = fc.scal_closed_form(3, LR0, T_MAX, *BETAS, WD).astype(np.float32)
    p2, m2, v2 = fc.adamw_formula(p, gr, m, v, scal, *BETAS, EPS, torch.float32)
    fc.check_adamw((p, gr, m, v), (p2, None, m2, v2), scal, *BETAS, EPS)
    nodecay = scal.copy()
    nodecay[2] = 1.0
    p3 = fc.adamw_formula(p, gr, m, v, nodecay, *BETAS, EPS, torch.float32)[0]
    with pytest.raises(fc.StageFailure):
        fc.check_adamw((p, gr, m, v), (p3, None, m2, v2), scal, *BETAS, EPS)
