"""Float64 reference, stage checkers and a float32 emulation for the bf16 fit step of the PSF network (csrc/mlp_train.hip,
aadff/mlp_fit.py, csrc/optim.hip).  A helper module, not a test; torch on the CPU only.  DESIGN.md §4.5.1 derives the bounds.

A `Snap` holds what ONE forward + backward stored: every activation, gradient and transpose with its padding, the bf16 operand
copies, the prediction and the fp32 gradient.  tests/test_gpu_fit_stages.py fills one from the buffers of `FusedFit`,
`emulate()` fills one from a float32 restatement with the kernels' rounding points.  Every checker takes as input what was
stored for the previous stage, so no error compounds, and judges
  * a bf16 output h of an fp32-accumulated sum by the INTERVAL RULE: with v the float64 value and d its bound,
    bf(f(v - d)) <= h <= bf(f(v + d)) for the monotone epilogue f, no element excluded; the share of h != bf(f(v)) pooled
    over the stage stays <= 1 %;
  * an fp32 output by max(error / bound) <= 1.
u = 2^-23 is twice the fp32 unit roundoff: a sum rounded in any order, or truncated, stays inside n u sum |terms|.
"""
import types

import numpy as np
import torch

U = 2.0 ** -23
SHARE_CAP = 0.01
STAGES = ("input", "forward", "head", "dx", "dw")

# name -> (activation widths w_0..w_L, batch): what each case meets is tabulated in DESIGN.md §4.5.1
CASES = {
    "A": ([4, 64, 256, 256, 121], 128),
    "B": ([4, 8, 36, 200, 68, 121], 50),
    "C": ([4, 8, 128], 129),
    "D": ([8, 256, 4, 9], 1),
    "E": ([4] + [16] * 15 + [25], 16),
    "F": ([4] + [8] * 16 + [9], 8),
    "G": ([4, 32, 121], 256),
}
ONE_LAYER = ([4, 25], 16)


def up(x, m):
    return (x + m - 1) // m * m


def bf(x):
    """float64 -> the nearest bf16 value, ties to even (subnormals included), as float64.  One rounding: not via float32."""
    x = torch.as_tensor(x, dtype=torch.float64)
    e = torch.frexp(x)[1].clamp_min(-125)
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), (8 - e).double())
    return torch.round(x * scale) / scale


def bits(t):
    return t.contiguous().view(torch.int16)


class StageFailure(AssertionError):
    def __init__(self, stage, msg):
        super().__init__(f"stage '{stage}': {msg}")
        self.stage = stage


def _need(cond, stage, msg):
    if not bool(cond):
        raise StageFailure(stage, msg() if callable(msg) else msg)


def _judge(record, stage, name, value, tol):
    if record is not None:
        record(name, value, tol)                         # the `margin` fixture: records, then asserts
    _need(value <= tol, stage, f"{name}: {value:.3e} exceeds {tol:.1e}")


class _Pool:
    """Elements of one stage that differ from bf(f(v)), pooled over its layers."""

    def __init__(self):
        self.diff = self.total = 0

    def share(self):
        return self.diff / max(1, self.total)


def interval(stage, name, h, v, d, pool, relu=False):
    """The interval rule on every element of h (float64 copies of stored bf16 values)."""
    f = (lambda t: t.clamp_min(0.0)) if relu else (lambda t: t)
    lo, hi = bf(f(v - d)), bf(f(v + d))
    bad = (h < lo) | (h > hi) | ~torch.isfinite(h)
    if bool(bad.any()):
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise StageFailure(stage, f"{name}: element {i} (feature tile {i[-1] // 16}, 32-wide tile {i[-1] // 32}) stores {float(h[i])!r}, "
                                  f"outside [{float(lo[i])!r}, {float(hi[i])!r}] around {float(v[i])!r}; {int(bad.sum())} of {h.numel()} outside")
    pool.diff += int((h != bf(f(v))).sum())
    pool.total += h.numel()


def ratio(err, bound):
    """max(error / bound), 0 where both are 0."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# what a step stored
# ---------------------------------------------------------------------------------------------------------------------
def new_snap(**kw):
    """chain, B, widths; inp, target, pred (fp32); flat, grad (fp32), w_off, b_off; p16 (bf16), dst, dst_t (int);
    XT[l] l = 0..L-1 [up4(w_l)][ldb] and dZT[l] l = 1..L [up4(w_l)][ldb] (bf16, index 0 of dZT is None);
    layer form also X[l] l = 0..L [B][up8(w_l)] and dZ[l] l = 1..L [B][up8(w_l)]; chain form X = dZ = None."""
    s = types.SimpleNamespace(**kw)
    s.L = len(s.widths) - 1
    return s


def weight(s, l):
    """W_l [w_{l+1}][w_l] and b_l as the kernels read them: the bf16 copies (stage 'input' ties them to the fp32 masters)."""
    n, k = s.widths[l + 1], s.widths[l]
    h = s.p16[s.dst.long()].double()
    return h[s.w_off[l]:s.w_off[l] + n * k].view(n, k), h[s.b_off[l]:s.b_off[l] + n]


def act(s, l, raw=False):
    """Stored X_l [B][w_l]: the row-major buffer in the layer form, the transpose (all the chain form stores) otherwise."""
    w = s.widths[l]
    t = s.X[l][:, :w] if s.X is not None else s.XT[l][:w, :s.B].T
    return t if raw else t.double()


def dz(s, l):
    w = s.widths[l]
    return (s.dZ[l][:, :w] if s.dZ is not None else s.dZT[l][:w, :s.B].T).double()


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: input cast, transposes, padding, operand copies
# ---------------------------------------------------------------------------------------------------------------------
def check_input(s):
    st, B, L = "input", s.B, s.L
    _need(torch.equal(bits(act(s, 0, raw=True)), bits(s.inp.to(torch.bfloat16))), st, "X_0 != bf(inp)")
    pads = []
    for l in range(L):
        pads.append((f"X_{l}^T", s.XT[l], s.widths[l], B))
    for l in range(1, L + 1):
        pads.append((f"dZ_{l}^T", s.dZT[l], s.widths[l], B))
    if s.X is not None:
        for l in range(L + 1):
            pads.append((f"X_{l}", s.X[l], B, s.widths[l]))
        for l in range(1, L + 1):
            pads.append((f"dZ_{l}", s.dZ[l], B, s.widths[l]))
        for l in range(L):
            _need(torch.equal(bits(s.X[l][:, :s.widths[l]]), bits(s.XT[l][:s.widths[l], :B].T)), st, f"X_{l}^T is not the transpose of X_{l}")
        for l in range(1, L + 1):
            _need(torch.equal(bits(s.dZ[l][:, :s.widths[l]]), bits(s.dZT[l][:s.widths[l], :B].T)), st, f"dZ_{l}^T is not the transpose of dZ_{l}")
    for name, t, r, c in pads:
        _need(t.shape[0] >= r and t.shape[1] >= c, st, f"{name}: buffer {tuple(t.shape)} smaller than {r} x {c}")
        _need(not bool(bits(t[r:, :]).any()) and not bool(bits(t[:, c:]).any()), st, f"{name}: non-zero padding outside {r} x {c}")
    h = s.flat.to(torch.bfloat16)
    _need(torch.equal(bits(s.p16[s.dst.long()]), bits(h)), st, "p16[dst] != bf(flat)")
    keep = s.dst_t >= 0
    _need(torch.equal(bits(s.p16[s.dst_t[keep].long()]), bits(h[keep])), st, "p16[dst_t] != bf(flat)")
    named = torch.zeros(s.p16.numel(), dtype=torch.bool)
    named[s.dst.long()] = True
    named[s.dst_t[keep].long()] = True
    _need(not bool(bits(s.p16[~named]).any()), st, "a p16 slot that neither dst nor dst_t names is non-zero")
    return {}


# ---------------------------------------------------------------------------------------------------------------------
# stage 2: forward of every layer from the stored X_l
# ---------------------------------------------------------------------------------------------------------------------
def check_forward(s):
    """Returns the pooled share and, for the head, the interval [z_lo, z_hi] and centre z of the logits where they are not stored."""
    pool, logits = _Pool(), None
    for l in range(s.L):
        W, b = weight(s, l)
        X = act(s, l)
        v = X @ W.T + b
        d = (s.widths[l] + 1) * U * (X.abs() @ W.abs().T + b.abs())
        last = l == s.L - 1
        if last and s.X is None:
            logits = (bf(v - d), bf(v + d), bf(v))
        else:
            interval("forward", f"forward of layer {l} ({s.widths[l]} -> {s.widths[l + 1]}, {'identity' if last else 'ReLU'} epilogue)",
                     act(s, l + 1), v, d, pool, relu=not last)
            if last:
                z = act(s, l + 1)
                logits = (z, z, z)
    _need(pool.share() <= SHARE_CAP, "forward", f"{pool.diff} of {pool.total} elements differ from bf(f(v))")
    return {"forward share": (pool.share(), SHARE_CAP)}, logits


# ---------------------------------------------------------------------------------------------------------------------
# stage 3: sigmoid, L1 normalisation, d MSE / dz
# ---------------------------------------------------------------------------------------------------------------------
def head_terms(pred, target, s_, B):
    """v and d of dz from a stored prediction and the (rounded) sigmoid, float64."""
    N = pred.shape[1]
    S = s_.sum(-1, keepdim=True)
    g = 2.0 * (pred - target) / (B * N)
    dot = (g * pred).sum(-1, keepdim=True)
    w = s_ * (1.0 - s_) / S
    return (g - dot) * w, (N + 8) * U * (g.abs() + (g * pred).abs().sum(-1, keepdim=True)) * w


def check_head_values(z_lo, z_hi, z, pred, target, dz_stored, B, exact_z, record=None, tag="", pools=None):
    """The head from logits known exactly (exact_z) or by interval; pred fp32, dz_stored bf16 values, all float64 [rows][N].
    `pools`: {"sigmoid": _Pool, "dz": _Pool} of a caller that pools the shares of several calls and judges them itself
    (`judge_head_pools`); N = 1 alone has pred = 1 and dz = g (1 - pred), a handful of elements that are all rounding."""
    st, N, out = "head", pred.shape[1], {}
    own = pools is None
    pools = {"sigmoid": _Pool(), "dz": _Pool()} if own else pools
    sref = bf(torch.sigmoid(z))
    srec = bf(pred * sref.sum(-1, keepdim=True))                       # the kernel's rounded sigmoid, from its own output
    lo, hi = bf(torch.sigmoid(z_lo) * (1 - 2.0 ** -12)), bf(torch.sigmoid(z_hi) * (1 + 2.0 ** -12))
    bad = (srec < lo) | (srec > hi) | ~torch.isfinite(pred)
    _need(not bool(bad.any()), st, lambda: f"sigmoid: element {tuple(int(k) for k in bad.nonzero()[0])} outside its interval ({int(bad.sum())} of {bad.numel()})")
    if exact_z:
        pools["sigmoid"].diff += int((srec != sref).sum())
        pools["sigmoid"].total += srec.numel()
    S = srec.sum(-1, keepdim=True)
    r = ratio((pred - srec / S).abs(), (N + 4) * U * pred)
    out["pred err/bound"] = (r, 1.0)
    _judge(record, st, tag + "pred err/bound", r, 1.0)
    v, d = head_terms(pred, target, srec, B)
    interval(st, "dz of the head", dz_stored, v, d, pools["dz"])
    if own:
        out.update(judge_head_pools(pools, record, tag))
    return out


def judge_head_pools(pools, record=None, tag=""):
    out = {}
    for k, name in (("sigmoid", "sigmoid share"), ("dz", "head dz share")):
        if pools[k].total:
            out[name] = (pools[k].share(), SHARE_CAP)
            _judge(record, "head", tag + name, pools[k].share(), SHARE_CAP)
    return out


def check_head(s, logits, record=None, tag=""):
    return check_head_values(*logits, s.pred.double(), s.target.double(), dz(s, s.L), s.B, s.X is not None, record, tag)


# ---------------------------------------------------------------------------------------------------------------------
# stage 4: dX chain;  stage 5: dW and db
# ---------------------------------------------------------------------------------------------------------------------
def check_dx(s):
    pool = _Pool()
    for l in range(s.L - 1, 0, -1):
        W, _ = weight(s, l)
        g = dz(s, l + 1)
        mask = act(s, l) > 0
        h = dz(s, l)
        _need(not bool(h[~mask].ne(0).any()), "dx", f"dZ_{l}: a masked element (X_{l} <= 0) is not exactly 0")
        v = torch.where(mask, g @ W, torch.zeros((), dtype=torch.float64))
        d = torch.where(mask, s.widths[l + 1] * U * (g.abs() @ W.abs()), torch.zeros((), dtype=torch.float64))
        interval("dx", f"dX of layer {l} (dZ_{l + 1} [{s.widths[l + 1]}] -> dZ_{l} [{s.widths[l]}])", h, v, d, pool)
    _need(pool.share() <= SHARE_CAP, "dx", f"{pool.diff} of {pool.total} elements differ from bf(v)")
    return {"dx share": (pool.share(), SHARE_CAP)}


def check_dw(s):
    rw = rb = 0.0
    for l in range(s.L):
        n, k = s.widths[l + 1], s.widths[l]
        g, x = s.dZT[l + 1][:n, :s.B].double(), s.XT[l][:k, :s.B].double()
        dW = s.grad[s.w_off[l]:s.w_off[l] + n * k].view(n, k).double()
        db = s.grad[s.b_off[l]:s.b_off[l] + n].double()
        _need(torch.isfinite(dW).all() and torch.isfinite(db).all(), "dw", f"layer {l}: non-finite gradient")
        rw = max(rw, ratio((dW - g @ x.T).abs(), s.B * U * (g.abs() @ x.abs().T)))
        rb = max(rb, ratio((db - g.sum(1)).abs(), s.B * U * g.abs().sum(1)))
    return {"dW err/bound": (rw, 1.0), "db err/bound": (rb, 1.0)}


def check_all(s, record=None, tag=""):
    """Every stage in order; the first that fails raises StageFailure.  `record` is the `margin` fixture or None."""
    out = dict(check_input(s))
    fwd, logits = check_forward(s)
    out.update(fwd)
    if record is not None:
        record(tag + "forward share", *fwd["forward share"])
    out.update(check_head(s, logits, record, tag))
    for stage, fn in (("dx", check_dx), ("dw", check_dw)):
        res = fn(s)
        out.update(res)
        for name, (value, tol) in res.items():
            _judge(record, stage, tag + name, value, tol)
    return out


def same_but_bias_gradients(a, b):
    """Two runs of one step: everything bit-identical except the bias gradients (fp32 atomics).  Names what differs."""
    diff = []
    for name in ("XT", "dZT", "X", "dZ"):
        la, lb = getattr(a, name), getattr(b, name)
        if la is not None:
            diff += [f"{name}[{i}]" for i, (x, y) in enumerate(zip(la, lb)) if x is not None and not torch.equal(bits(x), bits(y))]
    if not torch.equal(a.pred.view(torch.int32), b.pred.view(torch.int32)):
        diff.append("pred")
    for l in range(a.L):
        n = a.widths[l + 1] * a.widths[l]
        if not torch.equal(a.grad[a.w_off[l]:a.w_off[l] + n].view(torch.int32), b.grad[b.w_off[l]:b.w_off[l] + n].view(torch.int32)):
            diff.append(f"dW_{l}")
    return diff


# ---------------------------------------------------------------------------------------------------------------------
# stage 6: optimiser
# ---------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def scal_closed_form(t, lr0, T, b1, b2, wd):
    """(step size, sqrt of the second bias correction, decay, lr) of AdamW + CosineAnnealingLR after t completed steps, float64.
    The hyper-parameters are the float32 values the kernels are handed."""
    lr0, b1, b2, wd = f32(lr0), f32(b1), f32(b2), f32(wd)
    lr = 0.5 * lr0 * (1.0 + np.cos(np.pi * min(t, T) / T))
    return np.array([lr / (1.0 - b1 ** (t + 1)), np.sqrt(1.0 - b2 ** (t + 1)), 1.0 - lr * wd, lr], dtype=np.float64)


def scal_emulated(t, lr0, T, b1, b2, wd):
    """adamw_prepare's own roundings: float64 cos / pow, then fp32 lr, bias correction, quotient and decay."""
    F = np.float32
    lr = F(0.5 * float(F(lr0)) * (1.0 + np.cos(np.pi * min(t, T) / T)))
    bc1 = F(1.0 - float(F(b1)) ** (t + 1))
    return np.array([lr / bc1, F(np.sqrt(1.0 - float(F(b2)) ** (t + 1))), F(1) - lr * F(wd), lr], dtype=np.float32)


def check_scal(scal, t, lr0, T, b1, b2, wd):
    """Within 1 fp32 ulp of the closed form cast to fp32."""
    want = scal_closed_form(t, lr0, T, b1, b2, wd).astype(np.float32)
    got = np.asarray(scal, dtype=np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = err <= np.spacing(np.abs(want)).astype(np.float64)
    _need(ok.all(), "optimiser", f"scal at t = {t}: {got.tolist()} against {want.tolist()}")


def adamw_formula(p, g, m, v, scal, b1, b2, eps, dtype):
    """The update of fit_adamw_kernel / adamw_kernel, operation by operation, in `dtype`.  1 - beta is an fp32 value in the kernels."""
    c = lambda x: torch.tensor(float(x), dtype=dtype)
    omb1, omb2 = c(np.float32(1) - np.float32(b1)), c(np.float32(1) - np.float32(b2))
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    step, bc2s, decay = (c(np.float32(x)) for x in np.asarray(scal, dtype=np.float32)[:3])
    m2 = m + (g - m) * omb1
    v2 = v * c(f32(b2)) + g * g * omb2
    p2 = p * decay - step * (m2 / (v2.sqrt() / bc2s + c(f32(eps))))
    return p2, m2, v2


def rel_l2(a, b):
    den = float(torch.linalg.vector_norm(b.double()))
    num = float(torch.linalg.vector_norm(a.double() - b.double()))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def check_adamw(before, after, scal, b1, b2, eps, record=None, tag=""):
    """before / after: (p, g, m, v) as fp32 CPU tensors (g may be bf16 before).  p, m, v within 4 x d32 of float64 in relative L2,
    d32 being the float32 evaluation of the same formula on the same inputs; exact where d32 is 0."""
    ref = adamw_formula(*before, scal, b1, b2, eps, torch.float64)
    emu = adamw_formula(*before, scal, b1, b2, eps, torch.float32)
    for name, got, r64, r32 in zip("pmv", (after[0], after[2], after[3]), ref, emu):
        _need(torch.isfinite(got).all(), "optimiser", f"{name}: non-finite")
        d32, e = rel_l2(r32, r64), rel_l2(got, r64)
        if d32 == 0:
            _need(e == 0, "optimiser", f"{tag}{name}: {e:.3e} where the float32 formula is exact")
        else:
            _judge(record, "optimiser", f"{tag}adamw {name} rel_l2 / d32", e / d32, 4.0)


# ---------------------------------------------------------------------------------------------------------------------
# cases and the float32 emulation
# ---------------------------------------------------------------------------------------------------------------------
def make_case(widths, B, seed=0):
    """Weights uniform +- sqrt(6 / fan_in), biases uniform +- 0.5, inputs in [-1, 1], targets L1-normalised (fp32, CPU)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * len(widths) + B))
    uni = lambda *shape: torch.from_numpy((rng.random(shape, dtype=np.float32) * 2 - 1))
    W = [uni(n, k) * float(np.sqrt(6.0 / k)) for k, n in zip(widths[:-1], widths[1:])]
    b = [uni(n) * 0.5 for n in widths[1:]]
    target = torch.from_numpy(rng.random((B, widths[-1]), dtype=np.float32))
    return types.SimpleNamespace(widths=list(widths), B=B, W=W, b=b, inp=uni(B, widths[0]), target=target / target.sum(-1, keepdim=True))


def layer_layout(widths):
    """Row-major operand copies [W | W^T | bias] per layer with padded leading dimensions, and the maps flat index -> slot."""
    off, size, w_off, b_off, dst, dst_t = 0, 0, [], [], [], []
    for k, n in zip(widths[:-1], widths[1:]):
        n4, ldk, ldn = up(n, 4), up(k, 8), up(n, 8)
        r, c = np.divmod(np.arange(n * k), k)
        o_w, o_wt, o_b = size, size + n4 * ldk, size + n4 * ldk + k * ldn
        size = o_b + up(n4, 8)
        dst += [o_w + r * ldk + c, o_b + np.arange(n)]
        dst_t += [o_wt + c * ldn + r, np.full(n, -1)]
        w_off.append(off)
        b_off.append(off + n * k)
        off += n * k + n
    return torch.from_numpy(np.concatenate(dst)), torch.from_numpy(np.concatenate(dst_t)), size, w_off, b_off


MUTATIONS = {            # planted error -> the stage that must reject it
    "drop_last_contraction": "forward", "roll_bias": "forward", "mask_ge": "dx", "swap_transpose_rows": "input",
    "scale_without_batch": "head", "sigmoid_unrounded": "head", "dw_misses_last_row": "dw", "db_extra_row": "dw",
    "padding_nonzero": "input",
}


def head32(z, target, B, rounded=True, scale=None):
    """fit_head_kernel / head_kernel in float32: (pred, dz before its rounding).  `rounded`: the sigmoid is rounded to bf16."""
    sg = 1.0 / (1.0 + torch.exp(-z.float()))
    if rounded:
        sg = sg.to(torch.bfloat16).float()
    inv = 1.0 / sg.sum(-1, keepdim=True).clamp_min(1e-12)
    scale = torch.tensor(2.0 / (B * z.shape[1]) if scale is None else scale, dtype=torch.float32)
    pred = sg * inv
    g = scale * (pred - target)
    dot = (g * pred).sum(-1, keepdim=True)
    return pred, (g - dot) * inv * sg * (1.0 - sg)


def emulate(case, chain, mutate=None):
    """The step in float32 with the kernels' rounding points: bf16 operands, fp32 accumulation, bf16 activations / sigmoid / dz,
    fp32 dW.  `mutate` plants one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    widths, B, L = case.widths, case.B, len(case.widths) - 1
    h16 = lambda t: t.to(torch.bfloat16)
    dst, dst_t, size, w_off, b_off = layer_layout(widths)
    flat = torch.cat([t.reshape(-1) for W, b in zip(case.W, case.b) for t in (W, b)]).float()
    p16 = torch.zeros(size, dtype=torch.bfloat16)
    p16[dst] = h16(flat)
    p16[dst_t[dst_t >= 0]] = h16(flat)[dst_t >= 0]
    Wh, bh = [h16(W).float() for W in case.W], [h16(b).float() for b in case.b]
    X = [h16(case.inp)]
    for l in range(L):                                                       # ---- forward
        x, W, b = X[l].float(), Wh[l], bh[l]
        if mutate == "drop_last_contraction" and l == 0:
            x = x.clone()
            x[:, -1] = 0
        if mutate == "roll_bias" and l == L - 2:
            b = b.roll(1)
        y = x @ W.T + b
        X.append(h16(y if l == L - 1 else y.clamp_min(0)))
    N = widths[-1]                                                           # ---- head
    pred, dzl = head32(X[L].float(), case.target, B, rounded=mutate != "sigmoid_unrounded",
                       scale=2.0 / N if mutate == "scale_without_batch" else None)
    dZ = [None] * (L + 1)
    dZ[L] = h16(dzl)
    for l in range(L - 1, 0, -1):                                            # ---- dX chain
        keep = X[l].float() >= 0 if mutate == "mask_ge" else X[l].float() > 0
        dZ[l] = h16(torch.where(keep, dZ[l + 1].float() @ Wh[l], torch.zeros(())))
    grad = torch.zeros_like(flat)
    for l in range(L):                                                       # ---- dW, db
        gz, x = dZ[l + 1].float(), X[l].float()
        dW = (gz[:-1] if mutate == "dw_misses_last_row" else gz).T @ (x[:-1] if mutate == "dw_misses_last_row" else x)
        db = gz.sum(0)
        if mutate == "db_extra_row" and l == 0:
            db = db + gz[0]
        grad[w_off[l]:w_off[l] + dW.numel()] = dW.reshape(-1)
        grad[b_off[l]:b_off[l] + db.numel()] = db
    ldb = up(B, 8)

    def padded(t, rows, cols):
        out = torch.zeros(rows, cols, dtype=torch.bfloat16)
        out[:t.shape[0], :t.shape[1]] = t
        return out

    Xp = [padded(X[l], B, up(widths[l], 8)) for l in range(L + 1)]
    XT = [padded(X[l].T, up(widths[l], 4), ldb) for l in range(L)]
    dZp = [None] + [padded(dZ[l], B, up(widths[l], 8)) for l in range(1, L + 1)]
    dZT = [None] + [padded(dZ[l].T, up(widths[l], 4), ldb) for l in range(1, L + 1)]
    if mutate == "swap_transpose_rows":                                      # the chain form stores no original but the input's
        l = 0 if chain else min(1, L - 1)
        XT[l][[0, 1]] = XT[l][[1, 0]]
    if mutate == "padding_nonzero":
        if ldb > B:
            dZT[L][0, ldb - 1] = 1.0
        else:                                                                # no batch padding: a p16 slot that no map names
            named = torch.zeros(size, dtype=torch.bool)
            named[dst] = True
            named[dst_t[dst_t >= 0]] = True
            p16[int((~named).nonzero()[0])] = 1.0
    return new_snap(chain=chain, B=B, widths=list(widths), inp=case.inp, target=case.target, pred=pred, flat=flat, grad=grad,
                    w_off=w_off, b_off=b_off, p16=p16, dst=dst, dst_t=dst_t, XT=XT, dZT=dZT,
                    X=None if chain else Xp, dZ=None if chain else dZp)
