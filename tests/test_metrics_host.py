"""CPU: the host side of the evaluation metrics (csrc/metrics.hip, aadff/ops.py, aadff/metrics.py) - the oracles of
tests/metrics_common.py against what the reference's own dff/metrics.py returned (tests/golden/g19_metrics.npz, written by
tests/golden/make_metrics_golden.py) and against each other, the quantisation rule of the library against torch's bytes, every argument
error of the C entries without a GPU, the fake-tensor shapes of the ops, the public functions' errors and empty results, and the opt-in
binding of `dff`.

Oracle against golden: the reference computes in float32 (a few roundings per term, then numpy's pairwise float32 sum), the oracle in
float64, so a score may differ by (8 + ceil(log2 n)) * 2^-24 relative, n the number of pixels that take part; the three accuracies are
quotients of two integers and are equal exactly."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_common as mc
from aadff import _abi, metrics
from metrics_common import DEPTH_FUNCS, f32_bound, golden_case, oracle_scores

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
ENTRIES = ("aadff_depth_metric_sums", "aadff_image_metric_sums", "aadff_quantise_u8_host")


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "g19_metrics.npz"))
    return {k: z[k] for k in z.files}


def test_golden_file_is_small_and_complete(gold, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g19_metrics.npz")) < 100 * 1000
    assert [tuple(s) for s in gold["shapes"]] == [(3, 5), (37, 70), (37, 76)]
    for i, shape in enumerate(gold["shapes"]):
        e, g, m = gold[f"s{i}_est"], gold[f"s{i}_gt"], gold[f"s{i}_mask"]
        assert e.shape == tuple(shape) and e.dtype == g.dtype == np.float32 and m.dtype == bool
        assert np.array_equal(m, g > 0) and (g == 0).any() and float(gold[f"s{i}_nearest"]) > 1e-5
        assert not np.isnan(e).any() and (e > 0).all()
        for name in DEPTH_FUNCS:
            assert f"s{i}_{name}" in gold, name
    zeros = float((gold["s1_gt"] == 0).mean())
    assert 0.15 < zeros < 0.25
    assert len(gold["signatures"]) == 26


@pytest.mark.parametrize("i", range(3))
def test_depth_oracle_reproduces_the_reference(gold, margin, i):
    """rmse_log squares a difference of logs, whose float32 rounding is relative to the logs and not to their difference; it is held to
    the same bound all the same: measured 5.5e-8, 2.5e-8 and 2.5e-8 relative at the three shapes against bounds of 7.2e-7 and 1.2e-6."""
    for name, (want, n) in oracle_scores(gold, i).items():
        ref = float(gold[f"s{i}_{name}"])
        assert np.isfinite(ref) and np.isfinite(want), name
        if "accuracy" in name:
            assert ref == want, f"{name}: reference {ref!r}, oracle {want!r}"
        else:
            margin(f"metrics oracle vs reference: {name} at shape {i}", abs(ref - want) / abs(want), f32_bound(n))


def test_finite_mode_meets_infinities_and_counts_them(gold):
    e, g, m, c = golden_case(gold, 1)
    s = mc.depth_sums(e, g, None, None, "finite")[0]
    assert s[0] == e.size and s[12] == s[13] == s[14] == s[15] == m.sum() < e.size
    assert np.isfinite(s).all()
    e2 = e.copy()
    e2[0, 0, 0, 0], g2 = 0.0, g.copy()
    g2[0, 0, 0, 0] = 0.0                                                            # 0 / 0: a nan, which every function keeps
    s2 = mc.depth_sums(e2, g2, None, None, "finite")[0]
    assert np.isnan(s2[3]) and np.isnan(s2[4]) and np.isnan(s2[5]) and s2[14] < s2[12]


@pytest.mark.parametrize("shape", [(7, 7), (7, 9), (13, 8), (37, 70)])
def test_integer_ssim_agrees_with_the_filter_form(margin, shape):
    """The float64 filter loses digits in uxx - ux^2: about 65025 * 2^-53 / C2 = 1e-13 relative to S <= 1; measured <= 2.7e-15."""
    H, W = shape
    pred, target = mc.image_inputs(2, 3, H, W, seed=H * 100 + W)
    x, y = mc.quantise(pred).numpy(), mc.quantise(target).numpy()
    sse, ssum, nwin = mc.ssim_integer(x, y)
    assert nwin == 3 * (H - 6) * (W - 6)
    want = mc.ssim_filter(x, y)
    assert 0.0 < float(want.min()) < float(want.max()) < 0.999 and want[0] != want[1]
    margin(f"integer SSIM vs filter SSIM at {H} x {W}", np.abs(ssum / nwin - want).max(), 1e-12)
    assert (sse > 0).all()


def test_ssim_of_an_image_with_itself_is_one_and_psnr_infinite():
    pred, _ = mc.image_inputs(2, 3, 13, 8, seed=5)
    x = mc.quantise(pred).numpy()
    sse, ssum, nwin = mc.ssim_integer(x, x)
    assert (sse == 0).all() and (ssum == nwin).all()                                # every S is exactly 1
    assert np.isposinf(mc.psnr_of(sse, x[0].size)).all()
    assert mc.psnr_of(np.array([65025 * 10]), 10)[0] == 0.0


def test_library_quantisation_gives_torch_bytes():
    lib = _abi.load_library()
    v = mc.adversarial_values()
    assert v.dtype == np.float32 and v.size > 5 * 255 and (v < 0).any() and (v > 1).any() and np.signbit(v[v == 0]).any()
    v = np.ascontiguousarray(v)
    got = np.zeros(v.size, np.uint8)
    assert lib.aadff_quantise_u8_host(v.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), v.size) == 0
    want = mc.quantise(torch.from_numpy(v)).numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert set(np.unique(want)) == set(range(256))                                  # every byte value occurs
    # the separately rounded steps matter: in float64, or with a fused multiply-add, some of these values land on the other byte
    exact = np.clip(np.floor(v.astype(np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)
    assert (exact != want).any()
    assert lib.aadff_quantise_u8_host(None, got.ctypes.data_as(C.c_void_p), 1) == -1 and b"values is NULL" in lib.aadff_last_error()
    assert lib.aadff_quantise_u8_host(v.ctypes.data_as(C.c_void_p), None, 1) == -1 and b"out is NULL" in lib.aadff_last_error()
    assert lib.aadff_quantise_u8_host(v.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), -1) == -1 and b"n = -1" in lib.aadff_last_error()


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9         # additions only
    assert _abi.VALID_MODES == {"mask": 0, "finite": 1} and (_abi.SSIM_TILE_H, _abi.SSIM_TILE_W, _abi.DEPTH_METRIC_COLS) == (32, 64, 16)


def test_depth_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def call(est=P8, gt=P8, mask=None, conf=None, sums=P8, ws=P8, nbytes=1 << 20, N=2, H=16, W=16, mode=0):
        return lib.aadff_depth_metric_sums(est, gt, mask, conf, sums, ws, nbytes, N, H, W, mode, None)

    for name in ("est", "gt", "sums"):
        assert call(**{name: None}) == -1 and b"%s is NULL" % name.encode() in err()
    for mode in (-1, 2):
        assert call(mode=mode) == -1 and b"valid_mode = %d" % mode in err()
    assert call(mode=1, mask=P8) == -1 and b"mask must be NULL" in err()
    assert call(N=0) == -1 and b"N = 0" in err()
    assert call(H=0) == -1 and b"H = 0" in err()
    assert call(W=-2) == -1 and b"W = -2" in err()
    assert call(N=70000, H=40000, W=40000) == -1 and b"too large" in err()
    assert call(ws=None) == -1 and b"workspace" in err()
    assert call(nbytes=2 * 128 - 1) == -1 and b"workspace of 255 bytes, 256 are needed" in err()      # one workgroup per 16 x 16 image
    assert call(nbytes=3 * 128 * 3 - 1, N=3, H=37, W=70) == -1 and b"1152 are needed" in err()          # 648 groups of four: 3 workgroups


def test_image_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def call(pred=P8, target=P8, sums=P8, ws=P8, nbytes=1 << 20, N=2, Cn=3, H=16, W=16, ssim=1):
        return lib.aadff_image_metric_sums(pred, target, sums, ws, nbytes, N, Cn, H, W, ssim, None)

    for name in ("pred", "target", "sums"):
        assert call(**{name: None}) == -1 and b"%s is NULL" % name.encode() in err()
    for Cn in (0, 5):
        assert call(Cn=Cn) == -1 and b"C = %d is outside 1..4" % Cn in err()
    assert call(N=0) == -1 and b"N = 0" in err()
    for ssim in (0, 1):
        assert call(H=0, ssim=ssim) == -1 and b"H = 0" in err()
        assert call(W=0, ssim=ssim) == -1 and b"W = 0" in err()
        assert call(ws=None, ssim=ssim) == -1 and b"workspace" in err()
    assert call(H=6) == -1 and b"H = 6, W = 16" in err() and b"SSIM" in err()
    assert call(W=6) == -1 and b"H = 16, W = 6" in err()
    assert call(nbytes=95) == -1 and b"workspace of 95 bytes, 96 are needed" in err()                   # 2 images x 3 channels x 1 tile
    assert call(nbytes=16 * 2 * 3 * 2 * 2 - 1, H=39, W=71) == -1 and b"384 are needed" in err()         # 33 x 65 windows: 2 x 2 tiles
    assert call(nbytes=31, ssim=0) == -1 and b"32 are needed" in err()                                  # 768 values: one workgroup per image
    assert call(ws=C.c_void_p(12)) == -1 and b"aligned" in err()
    assert call(N=60000, Cn=4, H=20000, W=20000, ssim=0) == -1 and b"too large" in err()


def test_ops_and_fake_shapes():
    from aadff import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.aadff, "depth_metric_sums") and hasattr(torch.ops.aadff, "image_metric_sums")
    with FakeTensorMode():
        new = lambda *s, **k: torch.empty(*s, device="cuda", **k)                  # noqa: E731
        e, g = new(3, 1, 37, 70, requires_grad=True), new(3, 1, 37, 70)
        s = torch.ops.aadff.depth_metric_sums(e, g, new(3, 1, 37, 70, dtype=torch.bool), new(0), "mask")
        assert s.shape == (3, 16) and s.dtype == torch.float64 and not s.requires_grad    # a differentiable input, no graph
        s = torch.ops.aadff.depth_metric_sums(g, g, new(0), new(3, 1, 37, 70), "finite")
        assert s.shape == (3, 16) and s.dtype == torch.float64
        x = new(2, 3, 40, 56, requires_grad=True)
        for flag in (True, False):
            s = torch.ops.aadff.image_metric_sums(x, new(2, 3, 40, 56), flag)
            assert s.shape == (2, 2) and s.dtype == torch.float64 and not s.requires_grad
    assert ops.depth_metric_workspace_bytes(2, 16, 16) == 256 and ops.depth_metric_workspace_bytes(3, 37, 70) == 1152
    assert ops.image_metric_workspace_bytes(2, 3, 16, 16, True) == 96 and ops.image_metric_workspace_bytes(2, 3, 39, 71, True) == 384
    assert ops.image_metric_workspace_bytes(2, 3, 16, 16, False) == 32


def test_public_errors():
    e, g = torch.ones(2, 1, 8, 8), torch.ones(2, 1, 8, 8)
    for bad in (dict(est=e[0]), dict(gt=g[:, :, :7]), dict(est=torch.ones(2, 2, 8, 8), gt=torch.ones(2, 2, 8, 8)), dict(est=torch.ones(8)),
                dict(mask=torch.ones(2, 1, 8, 7, dtype=torch.bool)), dict(conf=torch.ones(1, 1, 8, 8)), dict(valid="all"),
                dict(valid="finite", mask=torch.ones(2, 1, 8, 8, dtype=torch.bool)), dict(est=e[:, :, :0], gt=g[:, :, :0])):
        with pytest.raises(ValueError, match="depth_metrics"):
            metrics.depth_metrics(**{**dict(est=e, gt=g), **bad})
    for bad in (dict(est=[[1.0]]), dict(est=e.long()), dict(gt=None), dict(conf=torch.ones(2, 1, 8, 8, dtype=torch.int32))):
        with pytest.raises(TypeError, match="depth_metrics"):
            metrics.depth_metrics(**{**dict(est=e, gt=g), **bad})
    x = torch.zeros(2, 3, 8, 8)
    for bad in (dict(pred=x[:, :, :7]), dict(pred=torch.zeros(2, 5, 8, 8), target=torch.zeros(2, 5, 8, 8)), dict(pred=x[0, 0], target=x[0, 0]),
                dict(pred=x[:, :, :, :0], target=x[:, :, :, :0])):
        with pytest.raises(ValueError, match="image_metrics"):
            metrics.image_metrics(**{**dict(pred=x, target=x), **bad})
    with pytest.raises(TypeError, match="image_metrics"):
        metrics.image_metrics(x.to(torch.uint8), x)
    for H, W in ((6, 8), (8, 6), (1, 1)):                                           # as scikit-image refuses a window larger than the image
        with pytest.raises(ValueError, match=f"H = {H}, W = {W}"):
            metrics.image_metrics(torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W))
        with pytest.raises(ValueError, match=f"batch_SSIM.*H = {H}, W = {W}"):
            metrics.batch_SSIM(torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="mask_accuracy_k: k = 4"):
        metrics.mask_accuracy_k(e, g, 4, g > 0)
    with pytest.raises(ValueError, match="mask_mae"):
        metrics.mask_mae(np.ones((4, 4), np.float32), np.ones((4, 5), np.float32), np.ones((4, 4), bool))
    ev = metrics.Evaluator()
    assert set(ev.result()) == set(metrics.DEPTH_KEYS) | {"psnr", "ssim"} and all(np.isnan(v) for v in ev.result().values())


def test_empty_batches_need_no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    z = torch.zeros(0, 1, 8, 8)
    d = metrics.depth_metrics(z, z, z > 0, z)
    assert list(d) == list(metrics.DEPTH_KEYS) + ["count", "mae_w_conf", "mse_w_conf"]
    assert all(v.shape == (0,) and v.dtype == torch.float64 for v in d.values())
    assert list(metrics.depth_metrics(z[:, 0], z[:, 0], valid="finite")) == list(metrics.DEPTH_KEYS) + ["count"]
    a = metrics.image_metrics(torch.zeros(0, 3, 8, 8), torch.zeros(0, 3, 8, 8))
    assert list(a) == ["psnr", "ssim"] and all(v.shape == (0,) and v.dtype == torch.float64 for v in a.values())
    assert list(metrics.image_metrics(torch.zeros(0, 3, 2, 2), torch.zeros(0, 3, 2, 2), ssim=False)) == ["psnr"]
    with pytest.raises(RuntimeError, match="no HIP device"):                        # and no CPU fallback for the rest
        metrics.depth_metrics(torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no HIP device"):
        metrics.image_metrics(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no HIP device"):
        metrics.mask_mae(np.ones((4, 4), np.float32), np.ones((4, 4), np.float32), np.ones((4, 4), bool))


def test_wrappers_have_the_reference_signatures(gold):
    recorded = {str(s).split("(")[0]: str(s) for s in gold["signatures"]}
    assert len(recorded) == 26
    for name, sig in recorded.items():
        if name.startswith("get_bumpiness"):
            assert not hasattr(metrics, name)
            continue
        f = getattr(metrics, name)
        assert f"{name}{inspect.signature(f)}" == sig and name in metrics.__all__


def _dff_probe(env_extra, code, repo_root):
    pkg = os.path.join(repo_root, "aberration-aware-depth-from-focus_amd")
    env = {k: v for k, v in os.environ.items() if k not in ("AADFF_NATIVE_METRICS", "AADFF_REFERENCE_ROOT")}
    env.update(env_extra, PYTHONPATH=pkg + os.pathsep + env.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_dff_binds_the_native_metrics_on_request(repo_root):
    code = ("import dff, aadff.metrics as m\n"
            "assert dff.mask_mae is m.mask_mae and dff.batch_SSIM is m.batch_SSIM and dff.metrics is m\n"
            "import sys; assert sys.modules['dff.metrics'] is m\n"
            "for name in ('get_bumpiness', 'get_bumpiness_non_mask'):\n"
            "    try:\n"
            "        getattr(dff, name)(None, None, None)\n"
            "    except ImportError as e:\n"
            "        assert 'bumpiness' in str(e)\n"
            "    else:\n"
            "        raise SystemExit(name + ' is not a stub')\n"
            "try:\n"
            "    dff.AiFDepthNet()\n"
            "except ImportError:\n"
            "    print('native ok')\n")
    r = _dff_probe({"AADFF_NATIVE_METRICS": "1"}, code, repo_root)
    assert r.returncode == 0 and "native ok" in r.stdout, r.stderr[-2000:]


def test_dff_metrics_stay_stubs_without_the_variable(repo_root):
    code = ("import dff\n"
            "try:\n"
            "    dff.mask_mae(None, None, None)\n"
            "except ImportError as e:\n"
            "    assert 'dff/metrics.py' in str(e); print('stub ok')\n")
    for extra in ({}, {"AADFF_NATIVE_METRICS": "0"}):
        r = _dff_probe(extra, code, repo_root)
        assert r.returncode == 0 and "stub ok" in r.stdout, r.stderr[-2000:]
