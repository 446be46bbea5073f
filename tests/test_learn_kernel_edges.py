"""Edge cases of the learner kernels (csrc/phc_learn.hip, phc_gae) through the C ABI, against the float64 references of oracle/learn_oracle.py.

Every output is a view inside a larger allocation: sentinel NaN patterns before it, after it and (for strided rows) between its rows.  After
each call the sentinels must be bit-unchanged, so a kernel that writes outside [0, n) fails here.  Sizes sit on the vector / scalar split
points, grid-stride boundaries and tail paths of each kernel; inputs are offset views where the C ABI allows unaligned buffers.

Tolerances are bounds derived from the fp32 / bf16 rounding of each operation (U = 2^-24, the unit round-off of fp32); counts, flags,
copies and results the kernels compute exactly are compared with exact equality.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import learn_oracle as lo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit round-off
UB = 2.0 ** -8          # bf16 unit round-off (8 significant bits)
PAD = 64                # sentinel elements on each side of a buffer
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.int64: torch.int64}
_SENT = {torch.float32: 0x7FC0BAD1, torch.bfloat16: 0x7FB1, torch.float64: 0x7FF8DEADBEEF0001, torch.int64: 0x7FF8DEADBEEF0001}


def _lib():
    from phc_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A [n] or [rows, cols] device tensor inside a sentinel-filled allocation: `offset` elements after PAD sentinels, rows `stride` elements
    apart, PAD sentinels after it.  `init` (None: the sentinel itself, so an element the kernel does not write shows up as NaN)."""

    def __init__(self, shape, dtype, offset=0, stride=None, init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        rows, cols = (1, shape[0]) if len(shape) == 1 else shape
        stride = stride or cols
        self.dtype, self.start, span = dtype, PAD + offset, rows * stride
        start = self.start
        self.base = torch.empty(start + span + PAD, dtype=dtype, device="cuda")
        self.base.view(_INT[dtype]).fill_(_SENT[dtype])
        region = self.base[start:start + span].view(rows, stride)[:, :cols]
        self.t = region.reshape(-1) if len(shape) == 1 else region       # (a view in both cases)
        self.outside = torch.ones(self.base.numel(), dtype=torch.bool, device="cuda")
        self.outside[start:start + span].view(rows, stride)[:, :cols] = False
        if init is not None:
            self.t.copy_(torch.as_tensor(init).reshape(self.t.shape))
        self.guard = self.base.view(_INT[dtype])[self.outside].clone()

    @property
    def ptr(self):      # (from the allocation: an empty view's data_ptr() is NULL)
        return self.base.data_ptr() + self.start * self.base.element_size()

    def np(self):
        return self.t.double().cpu().numpy() if self.dtype != torch.int64 else self.t.cpu().numpy()

    def check(self, what=""):
        assert torch.equal(self.base.view(_INT[self.dtype])[self.outside], self.guard), f"{what}: write outside the buffer"


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (NaN only where the reference is NaN)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
    err = np.abs(got - ref)[~nan]
    bad = err > tol[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} beyond tolerance, worst {float((err - tol[~nan]).max()):.3g} over"


# ------------------------------------------------------------------------------------------
# clip_grad_norm_ + Adam
# ------------------------------------------------------------------------------------------
ADAM_N = [1, 3, 4, 5, 1023, 1025, 4099, 524_287, 524_289, 1_000_003]   # 524 288 = 512 blocks x 256 lanes x 4: k_sumsq's grid-stride boundary

def f32(x):
    """x rounded to fp32: the value a float argument of the C ABI carries (1 - beta2 differs from 0.001 by 220 U otherwise)."""
    return float(np.float32(x))


LR, B1, B2, EPS, WD = f32(3e-3), f32(0.9), f32(0.999), f32(1e-8), f32(1e-3)


def _adam_data(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (1.0, 1e-3, 0.05)]
    return p, grads


def _adam_call(bufs, n, step, max_norm, wd, ws, norm_out=None, shadow=None, step_dev=None):
    p, g, m, v = bufs
    rc = _lib().phc_adam_clip_step(p.ptr, g.ptr, m.ptr, v.ptr, n, LR, B1, B2, EPS, wd, step, max_norm, ws.ptr,
                                   None if norm_out is None else norm_out.ptr, None if shadow is None else shadow.ptr,
                                   None if step_dev is None else step_dev.ptr, _stream())
    assert rc == 0


def _max_norm_for(grad, mode):
    """0: no clipping; 'on': max_norm at half the norm (clipping active); 'off': twice the norm (inactive)."""
    norm = float(grad.double().norm())
    return f32({"0": 0.0, "on": 0.5 * norm, "off": 2.0 * norm}[mode])


@pytest.mark.parametrize("max_norm_mode", ["0", "on"])
@pytest.mark.parametrize("n", ADAM_N, ids=lambda n: f"n{n}")
def test_adam_offset_views_equal_the_aligned_run(n, max_norm_mode):
    """Every fp32 array offset by 1, 2, 3 floats on its own, all four at once, the shadow offset by one bf16 or absent: the result is
    bit-identical to the aligned run of the same data (the per-element arithmetic of the vector and the scalar path is the same, and so is
    the order of the norm's partial sums), and nothing outside the buffers changes."""
    p0, grads = _adam_data(n, seed=n)
    g0 = grads[0]
    max_norm = _max_norm_for(g0, max_norm_mode)
    ws = Buf(_lib().phc_adam_workspace() // 8, torch.float64, init=torch.zeros(_lib().phc_adam_workspace() // 8, dtype=torch.float64))
    m0, v0 = torch.randn(n) * 0.01, torch.rand(n) * 1e-4

    def run(offsets, shadow_offset):
        bufs = [Buf(n, torch.float32, offset=o, init=x) for o, x in zip(offsets, (p0, g0, m0, v0))]
        sh = None if shadow_offset is None else Buf(n, torch.bfloat16, offset=shadow_offset)
        _adam_call(bufs, n, 2, max_norm, WD, ws, shadow=sh)
        torch.cuda.synchronize()
        for b, name in zip(bufs, "pgmv"):
            b.check(f"{name} offsets={offsets}")
        ws.check("workspace")
        if sh is not None:
            sh.check(f"shadow offset {shadow_offset}")
        return [b.t.clone() for b in bufs], None if sh is None else sh.t.clone()

    want, want_sh = run((0, 0, 0, 0), 0)
    assert torch.equal(want_sh, want[0].to(torch.bfloat16))
    # the aligned run against the fp64 reference (step 2 of an optimizer whose moments are m0, v0)
    rp, rg, rm, rv, _ = lo.adam_clip_step(p0.numpy(), g0.numpy(), m0.numpy(), v0.numpy(), 2, LR, B1, B2, EPS, WD, max_norm)
    AdamBound(p0.numpy(), m0.numpy(), v0.numpy()).check(want, (rp, rg, rm, rv), 2, WD, "aligned")
    configs = [((o if k == 0 else 0, o if k == 1 else 0, o if k == 2 else 0, o if k == 3 else 0), 0) for k in range(4) for o in (1, 2, 3)]
    configs += [((1, 2, 3, 1), 1), ((0, 0, 0, 0), 1), ((0, 0, 0, 0), None), ((3, 3, 3, 3), None)]
    for offsets, so in configs:
        got, got_sh = run(offsets, so)
        for a, b, name in zip(got, want, "pgmv"):
            assert torch.equal(a, b), f"{name}: offsets {offsets} / shadow {so} differ from the aligned run"
        if got_sh is not None:
            assert torch.equal(got_sh, want_sh)


class AdamBound:
    """Error bounds of the fp32 Adam step against the fp64 reference, carried from step to step.  Clip coefficient: fp32 lane sums of <= 8
    squares, fp64 beyond, an fp32 sqrt and division -> 8 U, so the clipped gradient is within 10 U.  Moments: m = b1 m + (1 - b1) d with
    d = g + wd p may cancel, so its error is 4 U of the magnitude M = b1 M + (1 - b1) |d| plus the carried error; v has no cancellation.
    Parameter: the step lr / bias1 * m / (sqrt(v) / sqrt(bias2) + eps) carries m's absolute error, half of v's relative one and 8 U (the
    rounded bias corrections, sqrt, two divisions); the subtraction adds 1 U of |p|."""

    def __init__(self, p, m, v):
        self.p, self.mag = np.asarray(p, np.float64), np.abs(np.asarray(m, np.float64))
        self.em, self.ev, self.ep = 0.0, 0.0, 0.0

    def check(self, got, ref, step, wd, what):
        p, g, m, v = (t.double().cpu().numpy() for t in got)
        rp, rg, rm, rv = ref[:4]
        eg = 10 * U * np.abs(rg)
        dmag = np.abs(rg) + wd * np.abs(self.p)
        ed = eg + 2 * U * dmag                       # d = g + wd p: the gradient's error, the product and the sum
        self.mag = B1 * self.mag + (1 - B1) * dmag
        self.em = B1 * self.em + 4 * U * self.mag + (1 - B1) * ed
        self.ev = B2 * self.ev + 4 * U * rv + (1 - B2) * 2 * np.abs(rg + wd * self.p) * ed
        den = np.sqrt(rv) / np.sqrt(1 - B2 ** step) + EPS
        ss = LR / (1 - B1 ** step)
        upd = ss * np.abs(rm) / den
        self.ep = self.ep + ss * self.em / den + upd * (self.ev / np.maximum(2 * rv, 1e-300) + 8 * U) + U * np.abs(rp)
        self.p = rp
        within(g, rg, eg, f"{what}: clipped gradient")
        within(m, rm, self.em + 1e-30, f"{what}: exp_avg")
        within(v, rv, self.ev + 1e-30, f"{what}: exp_avg_sq")
        within(p, rp, self.ep + 1e-30, f"{what}: param")


@pytest.mark.parametrize("weight_decay", [0.0, WD])
@pytest.mark.parametrize("max_norm_mode", ["0", "on", "off"])
@pytest.mark.parametrize("n", [1, 5, 1025, 524_289, 1_000_003], ids=lambda n: f"n{n}")
def test_adam_three_steps_against_fp64_and_device_step(n, max_norm_mode, weight_decay):
    """Three steps with the host `step` against the fp64 reference; `grad_norm_out` against the fp64 norm; the `step_device` path over three
    consecutive calls bit-identical to the host-step path (offset views: 1 float, shadow 1 bf16)."""
    p0, grads = _adam_data(n, seed=7 * n + 1)
    lib = _lib()
    nws = lib.phc_adam_workspace() // 8
    runs = {}
    for path in ("host", "device"):
        ws = Buf(nws, torch.float64, init=torch.zeros(nws, dtype=torch.float64))
        bufs = [Buf(n, torch.float32, offset=1, init=x) for x in (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n))]
        sh = Buf(n, torch.bfloat16, offset=1)
        norm = Buf(1, torch.float32)
        sdev = Buf(1, torch.int64, init=torch.zeros(1, dtype=torch.int64)) if path == "device" else None
        ref = (p0.numpy(), None, np.zeros(n), np.zeros(n))
        bound = AdamBound(p0.numpy(), ref[2], ref[3])
        outs = []
        for step, gr in enumerate(grads, start=1):
            max_norm = _max_norm_for(gr, max_norm_mode)
            bufs[1].t.copy_(gr)
            _adam_call(bufs, n, 0 if path == "device" else step, max_norm, weight_decay, ws, norm_out=norm, shadow=sh, step_dev=sdev)
            torch.cuda.synchronize()
            for b in bufs + [sh, norm, ws] + ([sdev] if sdev else []):
                b.check(f"{path} step {step}")
            ref = lo.adam_clip_step(ref[0], gr.numpy(), ref[2], ref[3], step, LR, B1, B2, EPS, weight_decay, max_norm)
            bound.check([b.t for b in bufs], ref, step, weight_decay, f"{path} step {step}")
            assert torch.equal(sh.t, bufs[0].t.to(torch.bfloat16))
            if max_norm > 0:
                # fp32 lane sums of <= 8 squares (8 U), fp64 beyond, fp32 sqrt (1 U)
                within(norm.np(), [ref[4]], 10 * U * ref[4], f"{path} grad_norm_out")
            if sdev is not None:
                assert int(sdev.t) == step
            outs.append([b.t.clone() for b in bufs] + [sh.t.clone()])
        runs[path] = outs
    for a, b in zip(runs["host"], runs["device"]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------
# weighted sums of squares
# ------------------------------------------------------------------------------------------
SSQ_SIZES = [0, 1, 7, 8, 9, 1024 * 256 * 4 - 1, 1024 * 256 * 4 + 1]     # 1024 blocks x 256 lanes x 4: the fp32 vector loop's grid-stride boundary


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_weighted_sumsq_sizes_types_offsets(count, dtype, offset):
    """out[0] = sum coef_t |x_t|^2, out[1 + t] = |x_t|^2 for every size of SSQ_SIZES (rotated over the tensors of a call); `offset`
    elements off a 16-byte boundary (offset 0: the vector loads).  Sums of positive terms: fp32 lane sums of <= 8 squares per grid-stride
    pass and 2 passes (16 U), fp64 beyond, one rounding to fp32 (1 U) -> 20 U relative; bf16 squares are exact in fp32."""
    lib = _lib()
    g = torch.Generator().manual_seed(count * 10 + offset)
    for rot in range(len(SSQ_SIZES)):
        sizes = [SSQ_SIZES[(rot + t) % len(SSQ_SIZES)] for t in range(count)]
        xs = [Buf(s, dtype, offset=offset, init=(torch.randn(s, generator=g) * (t + 1)).to(dtype)) for t, s in enumerate(sizes)]
        coefs = [0.5, 2.0, 1e-3, 7.0][:count]
        out = Buf(1 + count, torch.float32)
        nws = lib.phc_sumsq_workspace() // 8
        ws = Buf(nws, torch.float64, init=torch.zeros(nws, dtype=torch.float64))
        ptrs, szs, cfs = (C.c_void_p * count)(*[x.ptr for x in xs]), (C.c_int64 * count)(*sizes), (C.c_float * count)(*coefs)
        assert lib.phc_weighted_sumsq(count, ptrs, szs, cfs, int(dtype == torch.bfloat16), out.ptr, ws.ptr, _stream()) == 0
        torch.cuda.synchronize()
        for b in xs + [out, ws]:
            b.check(f"sizes {sizes}")
        ref = lo.weighted_sumsq([x.np() for x in xs], [float(np.float32(c)) for c in coefs])
        within(out.np(), ref, 20 * U * ref, f"sizes {sizes}")
        for t, s in enumerate(sizes):
            if s == 0:
                assert float(out.t[1 + t]) == 0.0


# ------------------------------------------------------------------------------------------
# discriminator BCE
# ------------------------------------------------------------------------------------------
def _bce_logits(na, nd, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(na + nd, generator=g) * 3
    special = torch.tensor([0.0, 80.0, -80.0, 1e4, -1e4, 0.0])
    for start, cnt in ((0, na), (na, nd)):
        k = min(cnt, len(special))
        x[start:start + k] = special[:k]
        x[start + cnt - 1] = 0.0      # exact zeros at both ends of each segment: the strict < 0 / > 0 accuracies
    return x


def _bce_run(na, nd, dtype, seed, scale=2.5):
    lib = _lib()
    x0 = _bce_logits(na, nd, seed).to(dtype)
    xb = Buf(na + nd, dtype, init=x0)
    grad, stats = Buf(na + nd, dtype), Buf(5, torch.float32)
    assert lib.phc_disc_bce(xb.ptr, int(dtype == torch.bfloat16), na, nd, scale, grad.ptr, stats.ptr, _stream()) == 0
    torch.cuda.synchronize()
    for b in (xb, grad, stats):
        b.check(f"disc_bce {na}+{nd}")
    x = x0.double().numpy()
    ref, rgrad = lo.disc_bce(x, na, scale)
    s = stats.np()
    a, d = x[:na], x[na:]
    # stats[0]: softplus to a few ulp per logit (4 U), a sum of positive terms in fp32: <= 2 per lane (grid-stride), a 6-level wavefront
    # tree, 16 wavefronts and <= 64 blocks added in sequence; the final scale and divisions (4 U)
    depth = 2 + 6 + 16 + min(64, (na + nd + 1023) // 1024)
    within(s[0], ref[0], (depth + 8) * U * ref[0], "loss")
    # accuracies: exact integer counts in fp32, one IEEE division
    assert s[1] == float(np.float32(np.float32((a < 0).sum()) / np.float32(na))) and s[2] == float(np.float32(np.float32((d > 0).sum()) / np.float32(nd)))
    # mean logits: signed sums -> bound relative to the sum of magnitudes
    for k, seg in ((3, a), (4, d)):
        within(s[k], ref[k], (depth + 2) * U * np.abs(seg).mean(), f"mean logit {k}")
    # gradient: sigmoid 1 / (1 + expf(-x)) to 6 U (expf 2 ulp), the scale and division 3 U; sg - 1 of the demo rows cancels, so their error
    # is 8 U of the scale absolute; bf16 output rounding on top
    base = np.concatenate([np.full(na, scale * 0.5 / na), np.full(nd, scale * 0.5 / nd)])
    tol = 12 * U * np.abs(rgrad) + 8 * U * base
    if dtype == torch.bfloat16:
        tol = tol + UB * (np.abs(rgrad) + tol)
    within(grad.np(), rgrad, tol + 1e-45, "grad")
    return s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("na,nd", [(1, 1), (1023, 1), (1024, 1024), (80_000, 40_000)])
def test_disc_bce_sizes_and_extreme_logits(na, nd, dtype):
    """(80 000, 40 000): 118 blocks' worth of logits under the 64-block cap (grid-stride loop); the agent / demo boundary inside a block;
    logits at +-80 and +-1e4 (softplus stability) and exact zeros."""
    _bce_run(na, nd, dtype, seed=na + nd)


def test_disc_bce_ticket_left_clean_across_launch_sizes():
    """A 64-block launch, a 1-block launch, a 3-block and a 64-block launch again: each result complete (the static partial sums and the
    ticket are left ready for the next launch whatever its grid)."""
    for na, nd in ((80_000, 40_000), (3, 2), (2000, 1000), (80_000, 40_000)):
        _bce_run(na, nd, torch.float32, seed=na)


# ------------------------------------------------------------------------------------------
# split-K slab sum
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2049, 4096], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("slabs", [1, 3, 8, 9, 17])
def test_sum_slabs_vector_and_scalar_paths(slabs, n, accumulate):
    """n % 8 == 0: 16-byte path (8, 4096); otherwise the scalar path.  The kernel adds the slabs in order in fp32 (then adds to `out`):
    bit-equal to that sum, and within (slabs + 1) U of the sum of magnitudes of the fp64 sum."""
    g = torch.Generator().manual_seed(slabs * 100000 + n)
    part = Buf((slabs, n), torch.bfloat16, init=(torch.randn(slabs, n, generator=g) * 3).to(torch.bfloat16))
    out0 = torch.randn(n, generator=g) * 10
    out = Buf(n, torch.float32, init=out0)
    assert _lib().phc_sum_slabs_bf16(part.ptr, slabs, n, out.ptr, accumulate, _stream()) == 0
    torch.cuda.synchronize()
    part.check("part"); out.check("out")
    p = part.t.float().cpu().numpy()
    seq = np.zeros(n, dtype=np.float32)
    for s in range(slabs):
        seq = seq + p[s]
    if accumulate:
        seq = out0.numpy() + seq
    assert np.array_equal(out.t.cpu().numpy(), seq)
    ref = lo.sum_slabs(p, out0.numpy(), bool(accumulate))
    within(out.np(), ref, (slabs + 1) * U * (np.abs(p).sum(0) + accumulate * np.abs(out0.numpy())), "slab sum")


# ------------------------------------------------------------------------------------------
# PPO loss
# ------------------------------------------------------------------------------------------
E_CLIP, CC, EC, BL = 0.25, 5.0, 0.01, 10.0      # (e_clip exact in binary: the clip range's ends are the same in fp32 and fp64)
PPO_VARIANTS = [(torch.float32, True, True), (torch.bfloat16, False, False), (torch.float32, False, False), (torch.bfloat16, True, True)]


def _ppo_case(B, D, dtype, use_index, clip_value, seed):
    g = torch.Generator().manual_seed(seed)
    N = 2 * B + 3 if use_index else B                 # rollout rows; the minibatch reads rows idx[r]
    idx = torch.randperm(N, generator=g)[:B] if use_index else None
    q = idx.numpy() if use_index else np.arange(B)
    logstd = torch.full((D,), -2.9) + torch.randn(D, generator=g) * 0.1
    mu = (torch.randn(B, D, generator=g) * 0.7).to(dtype)
    mu[0, 0] = 1.7                                     # outside the +-1 bound
    val = torch.randn(B, generator=g).to(dtype)
    old_mu = torch.randn(N, D, generator=g) * 0.7
    old_mu[q] = mu.float() + torch.randn(B, D, generator=g) * 0.004
    sg = torch.exp(logstd.double())
    actions = (old_mu.double() + sg * torch.randn(N, D, generator=g, dtype=torch.float64)).float()
    old_sigma = torch.exp(logstd).expand(N, D).contiguous()
    nlp = lo.neglogp(actions.numpy()[q], mu.double().numpy(), logstd.numpy())
    old_nlp = torch.randn(N, generator=g) * 0.3
    old_nlp[q] = torch.from_numpy(nlp).float() + torch.randn(B, generator=g) * 0.3
    old_nlp[q[:B // 4]] = torch.from_numpy(nlp[:B // 4]).float()     # ratio ~ 1: inside the clip range, where torch.max ties
    adv = torch.randn(N, generator=g)
    ret = torch.randn(N, generator=g)
    old_val = torch.randn(N, generator=g)
    old_val[q] = val.float() + torch.randn(B, generator=g) * 0.3
    return dict(mu=mu, val=val, logstd=logstd, actions=actions, old_nlp=old_nlp, adv=adv, ret=ret, old_val=old_val, old_mu=old_mu,
                old_sigma=old_sigma, idx=idx, q=q)


@pytest.mark.parametrize("variant", range(4), ids=["f32-idx-clipv", "bf16", "f32", "bf16-idx-clipv"])
@pytest.mark.parametrize("D", [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 8193, 16_387])
def test_ppo_loss_edges(B, D, variant):
    """B past 1024 blocks x 8 rows (grid-stride rows), D around the 32-lane half-wavefront, fp32 / bf16 heads, with and without the row index
    and the clipped value loss; a quarter of the rows at ratio ~ 1 (the tie of torch.max inside the clip range)."""
    dtype, use_index, clip_value = PPO_VARIANTS[variant]
    c = _ppo_case(B, D, dtype, use_index, clip_value, seed=B * 131 + D * 7 + variant)
    lib = _lib()
    from phc_amd import _lib as L
    ins = {k: Buf(tuple(v.shape), v.dtype, init=v) for k, v in c.items() if k not in ("idx", "q")}
    idx = None if c["idx"] is None else Buf(B, torch.int64, init=c["idx"])
    gmu, gval, stats = Buf((B, D), dtype, offset=1), Buf(B, dtype, offset=1), Buf(7, torch.float32)
    nws = lib.phc_ppo_loss_workspace() // 8
    ws = Buf(nws, torch.float64, init=torch.zeros(nws, dtype=torch.float64))
    prm = L.PpoParams(E_CLIP, CC, EC, BL, int(clip_value))
    rc = lib.phc_ppo_loss(ins["mu"].ptr, ins["val"].ptr, int(dtype == torch.bfloat16), ins["logstd"].ptr, ins["actions"].ptr, ins["old_nlp"].ptr,
                          ins["adv"].ptr, ins["ret"].ptr, ins["old_val"].ptr, ins["old_mu"].ptr, ins["old_sigma"].ptr, None if idx is None else idx.ptr,
                          B, D, C.byref(prm), gmu.ptr, gval.ptr, stats.ptr, ws.ptr, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, b in list(ins.items()) + [("idx", idx), ("grad_mu", gmu), ("grad_value", gval), ("stats", stats), ("workspace", ws)]:
        if b is not None:
            b.check(name)
    q = c["q"]
    f = lambda k: c[k].double().numpy()
    mu, val, logstd = f("mu"), f("val"), f("logstd")
    rs, rgmu, rgval, ratio = lo.ppo_loss(mu, val, logstd, f("actions"), f("old_nlp"), f("adv"), f("ret"), f("old_val"), f("old_mu"), f("old_sigma"),
                                         E_CLIP, CC, EC, BL, clip_value, row_index=None if c["idx"] is None else q)
    # fp32 neglogp: squares and sums over D (~(D / 32 + 16) U of 0.5 sum z^2), the constant 0.5 log(2 pi) D + sum logstd ((D / 32 + 8) U of
    # its terms' magnitudes), their sum (1 U of |neglogp|) and the rounded old_neglogp input (exact here: it is an input) -> exponent error `dl`;
    # the ratio then carries dl + 2 U relative
    a_q, ls = f("actions")[q], logstd
    z2 = (((a_q - mu) / np.exp(ls)) ** 2).sum(-1)
    const_mag = 0.5 * lo.LOG_2PI * D + np.abs(ls).sum()
    nlp = 0.5 * z2 + 0.5 * lo.LOG_2PI * D + ls.sum()
    dl = U * ((D / 32 + 16) * 0.5 * z2 + (D / 32 + 8) * const_mag + 2 * np.abs(nlp)) + 4 * U
    # rows whose ratio lies within that error of a clip-range end may take either branch of the clip (an O(1) jump of their gradient)
    lo_r, hi_r = 1.0 - E_CLIP, 1.0 + E_CLIP
    amb = (np.abs(ratio - lo_r) <= 2 * dl * ratio) | (np.abs(ratio - hi_r) <= 2 * dl * ratio)
    A, R = f("adv")[q], f("ret")[q]
    vp = f("old_val")[q]
    if clip_value:
        dv = val - vp
        l1, l2 = (val - R) ** 2, (vp + np.clip(dv, -E_CLIP, E_CLIP) - R) ** 2
        # |dv| at the clip's end, or -- outside it, where the clipped branch has no gradient -- the two losses equal to rounding
        amb |= (np.abs(np.abs(dv) - E_CLIP) <= 8 * U * (np.abs(val) + np.abs(vp))) \
            | ((np.abs(dv) > E_CLIP) & (np.abs(l1 - l2) <= 16 * U * (np.abs(val) + np.abs(vp) + np.abs(R) + 1) ** 2))
    ok = ~amb
    assert ok.sum() >= B - max(2, B // 200)
    # gradient w.r.t. mu: c_mu (ratio error dl + 6 U) times (a - m) / sigma^2 (6 U), the bounds term (6 U)
    sg2 = np.exp(2 * ls)
    bterm_g = BL / B * (2 * np.maximum(mu - 1, 0) + 2 * np.minimum(mu + 1, 0))
    tol_mu = (dl[:, None] + 16 * U) * np.abs(rgmu - bterm_g) + 8 * U * np.abs(bterm_g) + 8 * U * np.abs(A / B * ratio)[:, None] * (np.abs(a_q) + np.abs(mu)) / sg2
    if dtype == torch.bfloat16:
        tol_mu = tol_mu + UB * (np.abs(rgmu) + tol_mu)
    within(gmu.np()[ok], rgmu[ok], tol_mu[ok] + 1e-45, "grad_mu")
    # gradient w.r.t. the value: cc * 2 (v - R) / B (or the clipped branch): 4 U of the magnitudes involved
    tol_v = CC / B * 2 * 4 * U * (np.abs(val) + np.abs(R) + np.abs(vp) + E_CLIP)
    if dtype == torch.bfloat16:
        tol_v = tol_v + UB * (np.abs(rgval) + tol_v)
    within(gval.np()[ok], rgval[ok], tol_v[ok] + 1e-45, "grad_value")
    # statistics: per-row fp32 terms summed in fp64.  a_loss: ratio error; c_loss: 8 U of (|v| + |R| + |vp| + e)^2; b_loss, kl: fp32 sums
    # over D, (D / 32 + 16) U of the sum of the terms' magnitudes; ambiguous rows differ by the jump of the clip (continuous in the loss)
    s = stats.np()
    a_loss = np.maximum(-A * ratio, -A * np.clip(ratio, lo_r, hi_r))
    e_a = ((dl + 4 * U) * np.abs(A) * ratio).sum() / B
    e_c = (8 * U * (np.abs(val) + np.abs(R) + np.abs(vp) + E_CLIP) ** 2).sum() / B
    bterm = np.maximum(mu - 1, 0) ** 2 + np.minimum(mu + 1, 0) ** 2
    e_b = ((D / 32 + 16) * U * bterm.sum(-1)).sum() / B
    om, osg = f("old_mu")[q], f("old_sigma")[q]
    sg = np.exp(ls)
    kl_mag = (np.abs(np.log(osg / sg + 1e-5)) + (sg ** 2 + (om - mu) ** 2) / (2 * (osg ** 2 + 1e-5)) + 0.5).sum(-1)
    e_kl = ((D / 32 + 16) * U * kl_mag).sum() / B
    ent_mag = np.abs(0.5 + 0.5 * lo.LOG_2PI + ls).sum()
    e_ent = (D / 64 + 8) * U * ent_mag
    errs = np.array([0.0, e_a, e_c, e_b, e_ent, e_kl]) + U * np.abs(rs[:6])       # (+ the rounding of each mean to fp32)
    errs[0] = e_a + CC * e_c + EC * e_ent + BL * e_b + 8 * U * (np.abs(rs[1]) + CC * abs(rs[2]) + EC * abs(rs[4]) + BL * abs(rs[3]))
    within(s[:6], rs[:6], errs + 1e-30, "stats")
    assert abs(np.mean(a_loss) - rs[1]) < 1e-12
    # clip fraction: an exact count over the rows; only rows within `dl` of |ratio - 1| = e_clip may be counted either way
    clip_amb = np.abs(np.abs(ratio - 1) - E_CLIP) <= 2 * dl * ratio + 2 * U
    cnt = int(round(float(s[6]) * B))
    assert abs(float(s[6]) - float(np.float32(cnt / B))) == 0.0
    sure = int((np.abs(ratio - 1) > E_CLIP)[~clip_amb].sum())
    assert sure <= cnt <= sure + int(clip_amb.sum())


# ------------------------------------------------------------------------------------------
# policy sampling
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [1, 63, 64, 65])
@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_policy_sample_edges(N, D, dtype):
    """mu only, value only (un-normalised), masked value and the raw value (no statistics): each call writes exactly its own outputs."""
    lib = _lib()
    g = torch.Generator().manual_seed(N * 100 + D)
    mu0 = (torch.randn(N, D, generator=g) * 0.7).to(dtype)
    val0 = (torch.randn(N, generator=g) * 4).to(dtype)       # some beyond the +-5 clamp
    val0[0] = 9.0
    logstd0 = torch.full((D,), -2.9) + torch.randn(D, generator=g) * 0.1
    noise0 = torch.randn(N, D, generator=g)
    mask0 = (torch.arange(N) % 2).float()
    vmean, vvar = Buf(1, torch.float64, init=torch.tensor([0.7], dtype=torch.float64)), Buf(1, torch.float64, init=torch.tensor([2.5], dtype=torch.float64))
    mu, val, logstd, noise, mask = (Buf(tuple(t.shape), t.dtype, init=t) for t in (mu0, val0, logstd0, noise0, mask0))
    isb = int(dtype == torch.bfloat16)
    ref = lo.policy_sample(mu0.double().numpy(), val0.double().numpy(), logstd0.double().numpy(), noise0.double().numpy(), 0.7, 2.5, 1e-5)
    # mu only
    act, mus, sig = (Buf((N, D), torch.float32, offset=1) for _ in range(3))
    nlp = Buf(N, torch.float32, offset=1)
    assert lib.phc_policy_sample(mu.ptr, None, isb, logstd.ptr, noise.ptr, None, None, 1e-5, None, N, D, act.ptr, mus.ptr, sig.ptr, nlp.ptr, None, _stream()) == 0
    torch.cuda.synchronize()
    for b in (mu, val, logstd, noise, act, mus, sig, nlp):
        b.check("mu only")
    m, sgr, z = mu0.double().numpy(), np.exp(logstd0.double().numpy()), noise0.double().numpy()
    assert torch.equal(mus.t.cpu(), mu0.float())
    within(sig.np(), np.broadcast_to(sgr, (N, D)), 4 * U * sgr + 0 * m, "sigmas")                       # expf: <= 2 ulp = 4 U
    within(act.np(), ref["actions"], U * np.abs(ref["actions"]) + 6 * U * np.abs(sgr * z), "actions")  # m + sg z without contraction
    # neglogp recomputes z from the ROUNDED action: (a - m) / sg carries U |a| / sg absolute; squares, sums over D, the constant
    a = act.np()
    dz = (U * np.abs(a) + 6 * U * np.abs(sgr * z)) / sgr
    tol_n = ((2 * np.abs(z) + dz) * dz).sum(-1) * 0.5 + U * ((D / 64 + 16) * 0.5 * (z ** 2).sum(-1) + (D / 64 + 8) * abs(0.5 * lo.LOG_2PI * D + logstd0.double().numpy().sum()) + 2 * np.abs(ref["neglogp"]))
    within(nlp.np(), ref["neglogp"], tol_n, "neglogp")
    # value only (un-normalised), then masked, then raw
    for label, vm, vv, mk in (("unnorm", vmean, vvar, None), ("masked", vmean, vvar, mask), ("raw", None, None, None)):
        vals = Buf(N, torch.float32, offset=1)
        assert lib.phc_policy_sample(None, val.ptr, isb, None, None, None if vm is None else vm.ptr, None if vv is None else vv.ptr, 1e-5,
                                     None if mk is None else mk.ptr, N, D, None, None, None, None, vals.ptr, _stream()) == 0
        torch.cuda.synchronize()
        vals.check(label); val.check(label)
        r = lo.policy_sample(None, val0.double().numpy(), None, None, None if vm is None else 0.7, 2.5, 1e-5, None if mk is None else mask0.numpy())["values"]
        if vm is None:
            assert torch.equal(vals.t.cpu(), val0.float())
        else:   # float(var) + eps, sqrtf, the product and the sum: 4 U of each magnitude; the mask multiplies by exactly 0 or 1
            tol = 4 * U * (np.abs(r) + 0.7 + np.sqrt(2.5) * 5)
            within(vals.np(), r, tol, label)


# ------------------------------------------------------------------------------------------
# running normaliser
# ------------------------------------------------------------------------------------------
def _rn_call(x, rows, cols, nm, nv, out, out_bf16, stride, upd, ws):
    return _lib().phc_running_norm(x.ptr, None, rows, cols, nm.ptr, nv.ptr, 1e-5, 5.0, None if out is None else out.ptr, out_bf16, stride,
                                   *(None, None, None) if upd is None else (upd[0].ptr, upd[1].ptr, upd[2].ptr), None if ws is None else ws.ptr, _stream())


def _rn_exact(x, mean, var):
    """The kernel's fp32 expression: clamp((x - float(mean)) / sqrtf(float(var) + eps), -5, 5)."""
    m, v = mean.astype(np.float32), var.astype(np.float32)
    return np.clip((x - m) / np.sqrt(v + np.float32(1e-5)), np.float32(-5), np.float32(5))


@pytest.mark.parametrize("cols", [1, 255, 256, 257])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 8191, 8193, 40_000])
def test_running_norm_edges(rows, cols):
    """An update call writing fp32 rows `cols + 5` apart and a normalise-only call writing bf16 rows `cols + 1` apart: outputs bit-equal to
    the fp32 expression (and within 3 U of |y| + U (|x| + |mean|) / sigma of the fp64 one), padding columns untouched; 8193 and 40 000 rows
    run the finishing kernel's unrolled chunk loop and its tail; the ticket ends at zero."""
    lib = _lib()
    g = torch.Generator().manual_seed(rows + cols)
    x0 = torch.randn(rows, cols, generator=g) * 2 + 0.3
    x0[0, 0] = 40.0
    mean0 = torch.randn(cols, generator=g, dtype=torch.float64) * 0.5
    var0 = torch.rand(cols, generator=g, dtype=torch.float64) * 2 + 0.05
    x = Buf((rows, cols), torch.float32, init=x0)
    rm, rv, rc = (Buf(tuple(t.shape), torch.float64, init=t) for t in (mean0, var0, torch.tensor([1234.0], dtype=torch.float64)))
    nm, nv = Buf(cols, torch.float64, init=mean0), Buf(cols, torch.float64, init=var0)   # a frozen copy: the output uses the pre-update statistics
    nws = lib.phc_running_norm_workspace(rows, cols) // 8
    ws = Buf(nws, torch.float64, init=torch.zeros(nws, dtype=torch.float64))
    out = Buf((rows, cols), torch.float32, stride=cols + 5)
    assert _rn_call(x, rows, cols, nm, nv, out, 0, cols + 5, (rm, rv, rc), ws) == 0
    torch.cuda.synchronize()
    for name, b in (("x", x), ("out", out), ("run_mean", rm), ("run_var", rv), ("count", rc), ("workspace", ws)):
        b.check(name)
    assert int(ws.t[-1:].view(torch.int64)) == 0
    xn = x0.numpy()
    exact = _rn_exact(xn, mean0.numpy(), var0.numpy())
    assert np.array_equal(out.t.cpu().numpy(), exact)
    yref, (m1, v1, c1) = lo.running_norm(xn, mean0.numpy(), var0.numpy(), 1e-5, 5.0, mean0.numpy(), var0.numpy(), 1234.0)
    sd = np.sqrt(var0.numpy() + 1e-5)
    within(out.np(), yref, 3 * U * np.abs(yref) + U * (np.abs(xn) + np.abs(mean0.numpy()) + var0.numpy() / sd) / sd, "output vs fp64")
    assert float(rc.t) == c1
    # the batch mean and variance are rounded to fp32 before the fp64 update (as the reference's fp32 input.mean / input.var): 1 U of each,
    # plus the fp64 sums' own error (negligible) -- scaled by their weight in the update
    n, tot = float(rows), c1
    bm = xn.astype(np.float64).mean(0)
    within(rm.np(), m1, 2 * U * np.abs(bm) * n / tot + 1e-15, "run_mean")
    if rows > 1:
        bv = xn.astype(np.float64).var(0, ddof=1)
        delta = bm - mean0.numpy()
        within(rv.np(), v1, 2 * U * (bv * n + 2 * np.abs(delta) * np.abs(bm) * 1234.0 * n / tot) / tot + 1e-15, "run_var")
    else:
        assert np.isnan(rv.np()).all()       # the unbiased variance of one row is NaN, as torch's input.var(0)
    # normalise only, bf16 rows cols + 1 apart: the rounding of the same fp32 values
    outb = Buf((rows, cols), torch.bfloat16, stride=cols + 1)
    assert _rn_call(x, rows, cols, nm, nv, outb, 1, cols + 1, None, None) == 0
    torch.cuda.synchronize()
    outb.check("bf16 out"); nm.check("norm_mean")
    assert torch.equal(outb.t.cpu(), torch.from_numpy(exact).to(torch.bfloat16))


def test_running_norm_one_workspace_different_grids():
    """One workspace, calls whose finishing grids differ (256 columns: 16 blocks, 128 columns: 8 blocks; 64 x 256 and 128 x 128 put the ticket at
    the same place): every call updates the count and leaves the ticket at zero."""
    lib = _lib()
    assert lib.phc_running_norm_workspace(64, 256) == lib.phc_running_norm_workspace(128, 128)
    nws = lib.phc_running_norm_workspace(64, 256) // 8
    ws = Buf(nws, torch.float64, init=torch.zeros(nws, dtype=torch.float64))
    g = torch.Generator().manual_seed(3)
    count = 10.0
    stats = {c: [Buf(c, torch.float64, init=torch.zeros(c, dtype=torch.float64)), Buf(c, torch.float64, init=torch.ones(c, dtype=torch.float64))] for c in (256, 128)}
    cnt = {c: Buf(1, torch.float64, init=torch.tensor([count], dtype=torch.float64)) for c in (256, 128)}
    for it in range(6):
        rows, cols = ((64, 256), (128, 128))[it % 2]
        x0 = torch.randn(rows, cols, generator=g)
        x = Buf((rows, cols), torch.float32, init=x0)
        rm, rv = stats[cols]
        before = (rm.np(), rv.np(), float(cnt[cols].t))
        assert _rn_call(x, rows, cols, rm, rv, None, 0, 0, (rm, rv, cnt[cols]), ws) == 0
        torch.cuda.synchronize()
        ws.check("workspace")
        assert int(ws.t[-1:].view(torch.int64)) == 0
        _, (m1, v1, c1) = lo.running_norm(x0.numpy(), before[0], before[1], 1e-5, 5.0, before[0], before[1], before[2])
        assert float(cnt[cols].t) == c1
        bm = x0.double().numpy().mean(0)      # rounded to fp32 by the kernel before the fp64 update: 1 U of it, weighted by n / count
        within(rm.np(), m1, 2 * U * np.abs(bm) * rows / c1 + 1e-15, "run_mean")


# ------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------
def _colsum_tol(x, nchunks):
    """fp32: <= 64 sequential adds per lane in a chunk, a 4-way tree, <= nchunks / 16 sequential adds per slice, 16 slices: a bound of
    (70 + nchunks / 16) U of the column's sum of magnitudes."""
    return (70 + nchunks / 16) * U * np.abs(x).sum(0)


@pytest.mark.parametrize("cols", [1, 63, 65])
@pytest.mark.parametrize("rows", [255, 256, 257, 49 * 256 - 1, 49 * 256 + 1, 65 * 256 - 1, 65 * 256 + 1])
def test_colsum_and_relu_colsum_edges(rows, cols):
    lib = _lib()
    g = torch.Generator().manual_seed(rows * 3 + cols)
    x0 = torch.randn(rows, cols, generator=g).to(torch.bfloat16)
    y0 = torch.randn(rows, cols, generator=g).to(torch.bfloat16)
    y0[0] = -0.0
    x, y = Buf((rows, cols), torch.bfloat16, init=x0), Buf((rows, cols), torch.bfloat16, init=y0)
    nch = lib.phc_colsum_chunks(rows)
    assert nch == (rows + 255) // 256
    nws = lib.phc_colsum_workspace(rows, cols) // 4
    for relu in (False, True):
        ws, out = Buf(nws, torch.float32), Buf(cols, torch.float32)
        if relu:
            gm = Buf((rows, cols), torch.bfloat16)
            assert lib.phc_colsum_relu_bf16(x.ptr, y.ptr, rows, cols, gm.ptr, out.ptr, ws.ptr, _stream()) == 0
        else:
            assert lib.phc_colsum_bf16(x.ptr, rows, cols, out.ptr, ws.ptr, _stream()) == 0
        torch.cuda.synchronize()
        for b in (x, y, ws, out) + ((gm,) if relu else ()):
            b.check(f"relu={relu}")
        xs = x0.double().numpy()
        if relu:
            rgm, ref = lo.colsum_relu(xs, y0.double().numpy())
            assert torch.equal(gm.t.cpu(), torch.where(y0 > 0, x0, torch.zeros_like(x0)))
            xs = rgm
        else:
            ref = lo.colsum(xs)
        within(out.np(), ref, _colsum_tol(xs, nch), f"relu={relu}")


@pytest.mark.parametrize("njobs", [17, 33])
def test_colsum_finish_batch_many_jobs(njobs):
    """More than PHC_COLSUM_MAX_JOBS (16) deferred jobs: two and three batch launches; every other job accumulates into its output."""
    lib = _lib()
    from phc_amd import _lib as L
    g = torch.Generator().manual_seed(njobs)
    shapes = [((255, 257, 49 * 256 + 1, 65 * 256 - 1)[i % 4], (1, 63, 65)[i % 3]) for i in range(njobs)]
    jobs = (L.ColsumJob * njobs)()
    keep = []
    for i, (rows, cols) in enumerate(shapes):
        x0 = torch.randn(rows, cols, generator=g).to(torch.bfloat16)
        x = Buf((rows, cols), torch.bfloat16, init=x0)
        ws = Buf(lib.phc_colsum_workspace(rows, cols) // 4, torch.float32)
        assert lib.phc_colsum_bf16(x.ptr, rows, cols, None, ws.ptr, _stream()) == 0      # first stage only
        out0 = torch.randn(cols, generator=g)
        out = Buf(cols, torch.float32, init=out0)
        acc = i % 2
        jobs[i].partial, jobs[i].out, jobs[i].nchunks, jobs[i].cols, jobs[i].accumulate = ws.ptr, out.ptr, lib.phc_colsum_chunks(rows), cols, acc
        keep.append((x0, out0, acc, x, ws, out))
    assert lib.phc_colsum_finish_batch(njobs, jobs, _stream()) == 0
    torch.cuda.synchronize()
    for i, (x0, out0, acc, x, ws, out) in enumerate(keep):
        x.check(f"job {i}"); ws.check(f"job {i}"); out.check(f"job {i}")
        xs = x0.double().numpy()
        ref = lo.colsum(xs) + (out0.double().numpy() if acc else 0.0)
        within(out.np(), ref, _colsum_tol(xs, lib.phc_colsum_chunks(xs.shape[0])) + acc * U * np.abs(ref), f"job {i}")


# ------------------------------------------------------------------------------------------
# one-output linear layer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 63, 65, 513])
@pytest.mark.parametrize("rows", [1, 3, 15, 17])
def test_linear1_forward_backward_edges(rows, cols):
    lib = _lib()
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x0, w0 = torch.randn(rows, cols, generator=g).to(torch.bfloat16), torch.randn(cols, generator=g).to(torch.bfloat16)
    b0, gy0 = torch.randn(1, generator=g).to(torch.bfloat16), torch.randn(rows, generator=g).to(torch.bfloat16)
    x, w, b, gy = (Buf(tuple(t.shape), torch.bfloat16, init=t) for t in (x0, w0, b0, gy0))
    xs, ws_, bs, gs = (t.double().numpy() for t in (x0, w0, b0, gy0))
    y = Buf(rows, torch.bfloat16, offset=1)
    assert lib.phc_linear1_forward(x.ptr, w.ptr, b.ptr, rows, cols, y.ptr, _stream()) == 0
    torch.cuda.synchronize()
    y.check("y")
    ref = lo.linear1_forward(xs, ws_, bs)
    # products of bf16 are exact in fp32; <= cols / 64 sequential adds per lane, a 6-level tree, the bias: (cols / 64 + 8) U of the
    # magnitudes; then the bf16 rounding of the result
    e = (cols / 64 + 8) * U * (np.abs(xs * ws_).sum(-1) + abs(bs[0]))
    within(y.np(), ref, e + UB * (np.abs(ref) + e), "forward")
    for with_gx in (False, True):
        gx = Buf((rows, cols), torch.bfloat16) if with_gx else None
        gwb = Buf(cols + 1, torch.float32)
        wsb = Buf(lib.phc_linear1_workspace(rows, cols) // 4, torch.float32)
        assert lib.phc_linear1_backward(x.ptr, w.ptr, gy.ptr, rows, cols, None if gx is None else gx.ptr, gwb.ptr, wsb.ptr, _stream()) == 0
        torch.cuda.synchronize()
        for bb in (gwb, wsb, x, w, gy) + ((gx,) if gx else ()):
            bb.check(f"backward gx={with_gx}")
        rgx, rgwb = lo.linear1_backward(xs, ws_, gs)
        if gx is not None:      # g w is exact in fp32: one rounding to bf16
            assert torch.equal(gx.t.cpu(), (gy0.float()[:, None] * w0.float()[None, :]).to(torch.bfloat16))
        mags = np.concatenate([np.abs(gs[:, None] * xs).sum(0), [np.abs(gs).sum()]])
        within(gwb.np(), rgwb, (16 + 70 + lib.phc_linear1_chunks(rows) / 16) * U * mags, "gw_gb")


# ------------------------------------------------------------------------------------------
# GAE
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(1, 1), (1, 257), (16, 1), (16, 257), (33, 300)])
def test_gae_edges(T, n):
    """Dones on the first and the last step; per element the fp32 recurrence against fp64, bounded by 4 U of the discounted sum of the
    magnitudes that enter it (gamma * tau is rounded to fp32 once)."""
    g = torch.Generator().manual_seed(T * 1000 + n)
    fd0 = (torch.rand(T, n, generator=g) < 0.2).float()
    fd0[0, 0] = 1.0
    fd0[T - 1, n // 2] = 1.0
    v0, r0, nv0 = (torch.randn(T, n, generator=g) * 2 for _ in range(3))
    fd, v, r, nv = (Buf((T, n), torch.float32, init=t) for t in (fd0, v0, r0, nv0))
    adv = Buf((T, n), torch.float32)
    gamma, tau = f32(0.99), f32(0.95)
    assert _lib().phc_gae(T, n, fd.ptr, v.ptr, r.ptr, nv.ptr, gamma, tau, adv.ptr, _stream()) == 0
    torch.cuda.synchronize()
    for b in (fd, v, r, nv, adv):
        b.check("gae")
    ref = lo.gae(*(t.double().numpy() for t in (fd0, v0, r0, nv0)), gamma, tau)
    mag = np.zeros_like(ref)
    last = np.zeros(n)
    for t in reversed(range(T)):
        last = np.abs(r0[t].numpy()) + np.abs(nv0[t].numpy()) + np.abs(v0[t].numpy()) + gamma * tau * (1 - fd0[t].numpy()) * last
        mag[t] = last
    within(adv.np(), ref, 4 * U * mag * (T + 1), "gae")
