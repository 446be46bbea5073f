"""-m gpu: the distillation kernels (csrc/phc_distill.hip) through the C ABI against tests/distill_oracle.py, the trainer and the recording sweep on the device.

Every kernel output is a view inside a sentinel-filled allocation (tests/distill_util.py: Buf); after each call the sentinels must be bit-unchanged.  Bounds are
derived from the roundings involved and stated next to each assertion: U = 2^-24 (fp32 unit round-off), UB = 2^-8 (bf16: 8 significant bits, round to nearest)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import distill_oracle as do
from distill_util import U, UB, Buf, adam_steps, lib, stream, trainer_fixture, within

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -126      # smallest normal fp32 / bf16: below it a result may be flushed or rounded at subnormal spacing
BF16_MAX = 3.3895313892515355e38


# ------------------------------------------------------------------------------------------------------------------ 1. phc_dataset_record
@pytest.mark.parametrize("obs_dim,A,offset", [(7, 3, 0), (934, 69, 0), (934, 69, 1), (8, 4, 0), (8, 4, 1)], ids=lambda v: str(v))
def test_dataset_record_equals_the_torch_statement(obs_dim, A, offset):
    """N = 5 envs with rows 0, 1, 4, 2, 3 packed back to back (an overrun lands in a neighbour's rows or in the sentinels), steps 0 .. 4: `step == rows - 1` and
    `step == rows` both occur, the rows = 0 env never writes.  934 fp32 per row is no multiple of 16 bytes (8-byte vectors); 7 columns and the 4-byte offset take the
    element path; 8 columns the 16-byte one.  Exact equality with the torch statement after every call, obs_prev refreshed for all five envs, sentinels untouched."""
    from phc_amd import abi
    from phc_amd.learning.dataset_record import record_rows
    g = torch.Generator().manual_seed(obs_dim + offset)
    rows = torch.tensor([0, 1, 4, 2, 3], dtype=torch.int64)
    start = torch.cumsum(rows, 0) - rows
    N, R = 5, int(rows.sum())
    prev0 = torch.randn(N, obs_dim, generator=g)
    obs_prev = Buf((N, obs_dim), torch.float32, offset=offset, init=prev0)
    obs_buf = Buf((N, obs_dim), torch.float32, offset=offset, init=torch.zeros(N, obs_dim))
    blk = (Buf((R, obs_dim), torch.float32, offset=offset), Buf((R, A), torch.float32, offset=offset), Buf((R, A), torch.float32, offset=offset), Buf(R, torch.int64))
    ref_blk = tuple(b.t.clone() for b in blk)
    ref_prev = prev0.cuda()
    rows_d, start_d = rows.cuda(), start.cuda()
    for step in range(5):
        new_obs, clean, act = torch.randn(N, obs_dim, generator=g).cuda(), torch.randn(N, A, generator=g).cuda(), torch.randn(N, A, generator=g).cuda()
        reset = torch.randint(0, 2, (N,), generator=g).cuda()
        obs_buf.t.copy_(new_obs)
        a = abi.record_args_struct(N, obs_dim, A, step, R, rows=rows_d, row_start=start_d, clean_actions=clean, actions=act, reset_buf=reset)
        a.obs_buf, a.obs_prev, a.obs, a.clean, a.env, a.reset = obs_buf.ptr, obs_prev.ptr, blk[0].ptr, blk[1].ptr, blk[2].ptr, blk[3].ptr
        assert lib().phc_dataset_record(C.byref(a), stream()) == 0
        torch.cuda.synchronize()
        record_rows(step, rows_d, start_d, ref_prev, new_obs, clean, act, reset, ref_blk)
        for b, r, name in zip(blk + (obs_prev,), ref_blk + (ref_prev,), ("obs", "clean", "env", "reset", "obs_prev")):
            b.check(f"{name} step {step}")
            assert torch.equal(b.bits(), r.contiguous().view(b.bits().dtype)), f"{name} step {step}"
        obs_buf.check("obs_buf")
        assert torch.equal(obs_prev.t, new_obs)
    assert not any(torch.isnan(b.t).any() for b in blk[:3])      # every row of the block was written by the end
    a.num_envs = 0
    assert lib().phc_dataset_record(C.byref(a), stream()) == -1
    a.num_envs, a.obs = N, None
    assert lib().phc_dataset_record(C.byref(a), stream()) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. the SiLU pair
SPECIAL = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 20.0, -20.0, 88.5, -88.5, BF16_MAX, -BF16_MAX, -89.0, -100.0]


def _silu_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows * cols, generator=g) * 3.0
    k = min(len(SPECIAL), z.numel())
    z[:k] = torch.tensor(SPECIAL[:k])
    if rows * cols > 2 * len(SPECIAL):      # the specials a second time, at the far end (the ragged tail of the 16-byte path)
        z[-len(SPECIAL):] = torch.tensor(SPECIAL)
    gy = torch.randn(rows * cols, generator=g)
    return z.to(torch.bfloat16).view(rows, cols), gy.to(torch.bfloat16).view(rows, cols)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset2B"])
def test_silu_and_its_backward_against_the_fp64_oracle(offset):
    """rows in {1, 63, 64, 65, 257} x cols in {1, 7, 8, 69, 512} (one and two 256-row chunks; cols % 8 == 0 takes the 16-byte path when the views are aligned),
    values incl. 0, +-2^-20, +-1, +-20, +-88.5 and +- the largest finite bf16."""
    L_ = lib()
    from phc_amd import _lib as L
    shapes = [(r, c) for r in (1, 63, 64, 65, 257) for c in (1, 7, 8, 69, 512)] + [(16500, 8), (16500, 7)]     # (65 chunks: the finishing stage's second round)
    for rows, cols in shapes:
        if True:
            what = f"{rows}x{cols} offset {offset}"
            z, gy = _silu_inputs(rows, cols, rows * 1000 + cols)
            zb, gb = Buf((rows, cols), torch.bfloat16, offset=offset, init=z), Buf((rows, cols), torch.bfloat16, offset=offset, init=gy)
            z64, g64 = zb.np(), gb.np()
            # ---- forward.  y32 = z / (1 + expf(-z)): expf within 1 ulp (2 U), the addition and the division one rounding each: 4 U relative, taken as 8 U; one
            # bf16 rounding UB.  Where expf(-z) overflows (z < -88.72) the quotient is -0 and the true value at most 88.8 e^-88.7 = 2.6e-37: the absolute term.
            y = Buf((rows, cols), torch.bfloat16, offset=offset)
            assert L_.phc_silu_bf16(zb.ptr, rows, cols, y.ptr, stream()) == 0
            torch.cuda.synchronize()
            y.check("silu " + what); zb.check("z " + what)
            ref = do.silu(z64)
            within(y.np(), ref, (UB + 8 * U) * np.abs(ref) + 3e-37, "silu " + what)
            y2 = Buf((rows, cols), torch.bfloat16, offset=offset)
            assert L_.phc_silu_bf16(zb.ptr, rows, cols, y2.ptr, stream()) == 0
            assert torch.equal(y.bits(), y2.bits()), "silu twice " + what
            # ---- backward.  s and t = 1 - s come from e = expf(-|z|) (2 U), d = 1 + e, 1 / d, e / d (U each): 4 U each; (g s) U, z t U, 1 + z t U absolute to its
            # size: |error| <= |g| s (5 U |z| t + 7 U |1 + z t|), taken as 8 U |g| s (|z| t + |1 + z t|).  An s below the smallest normal may be flushed to zero:
            # |g| min(2^-126, s) |1 + z t|.  Then one bf16 rounding of gz (UB relative, flushed below 2^-126).
            s, t = do.sigmoid(z64), do.sigmoid(-z64)
            gref = do.silu_grad(g64, z64)
            e32 = 8 * U * np.abs(g64) * s * (np.abs(z64) * t + np.abs(1 + z64 * t)) + np.abs(g64) * np.minimum(FLOOR, s) * np.abs(1 + z64 * t)
            ws_n = L_.phc_colsum_workspace(rows, cols) // 4
            outs = []
            for mode in ("one call", "two stages", "one call again"):
                gz, out, ws = Buf((rows, cols), torch.bfloat16, offset=offset), Buf(cols, torch.float32), Buf(ws_n, torch.float32)
                if mode == "two stages":
                    assert L_.phc_colsum_silu_bf16(gb.ptr, zb.ptr, rows, cols, gz.ptr, None, ws.ptr, stream()) == 0
                    job = (L.ColsumJob * 1)()
                    job[0].partial, job[0].out, job[0].nchunks, job[0].cols, job[0].accumulate = ws.ptr, out.ptr, L_.phc_colsum_chunks(rows), cols, 0
                    assert L_.phc_colsum_finish_batch(1, job, stream()) == 0
                else:
                    assert L_.phc_colsum_silu_bf16(gb.ptr, zb.ptr, rows, cols, gz.ptr, out.ptr, ws.ptr, stream()) == 0
                torch.cuda.synchronize()
                for b, n in ((gz, "gz"), (out, "sums"), (ws, "workspace"), (gb, "gy"), (zb, "z")):
                    b.check(f"{n} {mode} {what}")
                outs.append((gz.bits(), out.bits()))
                within(gz.np(), gref, e32 + UB * np.abs(gref) + FLOOR, f"gz {mode} {what}")
                # the sums add the UNROUNDED fp32 products: their errors e32, plus fp32 summation in a fixed order: rows U sum|gz|
                within(out.np(), gref.sum(0), e32.sum(0) + rows * U * np.abs(gref).sum(0) + FLOOR, f"sums {mode} {what}")
            assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(outs[0], o)), "one call / two stages / second run differ in bits: " + what
    assert L_.phc_silu_bf16(zb.ptr, 0, 4, y.ptr, stream()) == -1


# ------------------------------------------------------------------------------------------------------------------ 3. phc_mse_loss
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("use_index", [False, True], ids=["rows", "row_index"])
def test_mse_loss_against_the_fp64_oracle(bf16, use_index):
    """batch in {1, 65, 1000} x dim in {1, 3, 69}; `row_index` repeats rows of a 37-row target.  e = pred - target, e^2 and at most three fp32 adds per lane (U each),
    the rest of the sum in fp64, the mean rounded to fp32 once: 8 U relative on the loss.  grad = (2 / n) e: the quotient, the difference and the product one rounding
    each, 4 U relative (5 U with the cross term of the bf16 rounding), plus one bf16 rounding for a bf16 `pred`."""
    L_ = lib()
    dt = torch.bfloat16 if bf16 else torch.float32
    ws_n = L_.phc_mse_loss_workspace() // 8
    for batch in (1, 65, 1000):
        for dim in (1, 3, 69):
            for offset in (0, 1):
                what = f"{batch}x{dim} offset {offset}"
                g = torch.Generator().manual_seed(batch * 100 + dim)
                T = 37 if use_index else batch
                target = torch.randn(T, dim, generator=g).cuda()
                idx = torch.randint(0, T, (batch,), generator=g).cuda() if use_index else None
                pred = Buf((batch, dim), dt, offset=offset, init=torch.randn(batch, dim, generator=g) * 1.5)
                ref_loss, ref_grad = do.mse_loss(pred.np(), target.double().cpu().numpy(), None if idx is None else idx.cpu().numpy())
                res = []
                for _ in range(2):
                    grad, loss, ws = Buf((batch, dim), dt, offset=offset), Buf(1, torch.float32), Buf(ws_n, torch.float64)
                    assert L_.phc_mse_loss(pred.ptr, int(bf16), target.data_ptr(), None if idx is None else idx.data_ptr(), batch, dim, grad.ptr, loss.ptr, ws.ptr, stream()) == 0
                    torch.cuda.synchronize()
                    for b, n in ((grad, "grad"), (loss, "loss"), (ws, "workspace"), (pred, "pred")):
                        b.check(f"{n} {what}")
                    within(loss.np(), [ref_loss], 8 * U * ref_loss + FLOOR, "loss " + what)
                    within(grad.np(), ref_grad, (5 * U + (UB if bf16 else 0)) * np.abs(ref_grad) + FLOOR, "grad " + what)
                    res.append((grad.bits(), loss.bits()))
                assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "two runs differ in bits: " + what
    assert L_.phc_mse_loss(None, int(bf16), target.data_ptr(), None, batch, dim, grad.ptr, loss.ptr, ws.ptr, stream()) == -1      # PHC_EINVAL, no launch
    assert L_.phc_mse_loss(pred.ptr, int(bf16), target.data_ptr(), None, 0, dim, grad.ptr, loss.ptr, ws.ptr, stream()) == -1


# ------------------------------------------------------------------------------------------------------------------ 4. the trainer on the device
T_ROWS, T_OBS, T_ACT, T_UNITS, T_BATCH, T_EPOCHS, T_LR = 300, 37, 5, [64, 32], 128, 2, 2e-3
_plain_cache = {}


def _plain(kind):
    """The plain torch loop on the shared fixture, computed once per kind: cpu32 / cpu64 (CPU), gpu32 / gpu_autocast (device)."""
    from phc_amd import distill
    if kind not in _plain_cache:
        fx = trainer_fixture(T_ROWS, T_OBS, T_ACT, seed=1)
        init = {k[len("model."):]: v.detach().clone() for k, v in distill.build_student(T_OBS, T_ACT, T_UNITS, "silu", 0).state_dict().items()}
        perms = [distill.epoch_permutation(0, e, T_ROWS) for e in range(T_EPOCHS)]
        dtype, device, autocast = {"cpu32": (torch.float32, "cpu", False), "cpu64": (torch.float64, "cpu", False), "gpu32": (torch.float32, "cuda", False),
                                   "gpu_autocast": (torch.float32, "cuda", True)}[kind]
        _plain_cache[kind] = do.plain_loop(fx["obs"], fx["clean_action"], fx["running_mean"], fx["running_var"], T_UNITS, T_BATCH, T_EPOCHS, T_LR, perms, init, dtype,
                                           autocast=autocast, device=device)[0]
    return _plain_cache[kind]


def _device_trainer(gemm):
    from phc_amd import distill
    fx = trainer_fixture(T_ROWS, T_OBS, T_ACT, seed=1)
    tr = distill.Trainer(fx["obs"], fx["clean_action"], fx["running_mean"], fx["running_var"], T_UNITS, "silu", T_BATCH, T_LR, 0, "cuda", gemm)
    for _ in range(T_EPOCHS):
        tr.run_epoch()
    torch.cuda.synchronize()
    assert torch.isfinite(tr.loss).all()
    return tr, {k[len("model."):]: v.detach().double().cpu() for k, v in tr.model.state_dict().items()}


def test_device_trainer_with_fp32_gemms_against_the_cpu_plain_loop():
    """300 rows, obs 37, actions 5, units [64, 32], batch 128 (a partial batch of 44), 2 epochs = 6 Adam steps.  fp32 GEMMs: phc_running_norm, torch's fp32 layers,
    phc_mse_loss, phc_adam_clip_step against the CPU plain loop in fp64; bound = 4 x the deviation of the CPU plain loop between fp32 and fp64 on this fixture
    (the rule of tests/test_distill_cpu.py), in Adam steps.  Measured on an MI355X: 1.54e-5 for the plain loop, 1.74e-5 for the trainer."""
    measured = adam_steps(_plain("cpu32"), _plain("cpu64"), T_LR)
    tr, got = _device_trainer("fp32")
    dev = adam_steps(got, _plain("cpu64"), T_LR)
    print(f"fp32 plain loop vs fp64: {measured:.3e} Adam steps; device trainer (fp32 GEMMs) vs fp64: {dev:.3e}")
    assert dev <= 4 * measured


def test_device_trainer_with_bf16_layers_against_torch_autocast():
    """The default path: phc_running_norm writes the bf16 input, the bf16 device layers with phc_silu_bf16 / phc_colsum_silu_bf16, phc_mse_loss on the bf16 head,
    phc_adam_clip_step.  Yardstick: torch's own bf16 autocast run of the plain model on the same fixture against its fp32 run, both on the device; the trainer may
    deviate from the fp32 run by 2 x that (bf16 rounding sits at the same places).  Measured on an MI355X (profiles/distill/README.md): yardstick 2.110 Adam steps,
    the trainer 2.115; the test re-measures the yardstick, it is not hard-coded."""
    yard = adam_steps(_plain("gpu_autocast"), _plain("gpu32"), T_LR)
    tr, got = _device_trainer("bf16")
    dev = adam_steps(got, _plain("gpu32"), T_LR)
    print(f"torch autocast vs fp32: {yard:.3e} Adam steps; device trainer (bf16 layers) vs fp32: {dev:.3e}")
    assert dev <= 2 * yard
    ck = tr.checkpoint()
    assert list(ck["model_state_dict"]) == [f"model.{k}.{p}" for k in (0, 2, 4) for p in ("weight", "bias")] and ck["model_state_dict"]["model.0.weight"].shape == (64, T_OBS)


# ------------------------------------------------------------------------------------------------------------------ 5. the sweep on the device
SMALL = {"learning.params.config.minibatch_size": 64, "learning.params.config.amp_obs_demo_buffer_size": 512, "learning.params.config.amp_replay_buffer_size": 512}
_sweeps = {}


def _sweep(mode, collect, noise=False, backend=None):
    """One evaluation sweep of an untrained agent: 8 envs, synthetic:10:3 (two batches, the second one wrapping); computed once per setting."""
    key = (mode, collect, noise, backend)
    if key in _sweeps:
        return _sweeps[key]
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.learning import dataset_record
    from phc_amd.learning.amp_agent import IMAmpAgent
    over = dict(SMALL, **{"+learning.params.config.eval_metrics": mode})
    if collect:
        over.update({"collect_dataset": True, "env.add_action_noise": noise, "+env.action_noise_std": 0.05})
    torch.manual_seed(0)
    task, env = parse_task(compose(["env.num_envs=8", "env.motion_file=synthetic:10:3"] + [f"{k}={v}" for k, v in over.items()]))
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    first_obs, num_steps, steps, real_reset, real_step = [], [], [], env.reset, env.step

    def reset(*a):      # (the sweep resets once per batch)
        out = real_reset(*a)
        first_obs.append(task.obs_buf.clone())
        num_steps.append(task._motion_lib.get_motion_num_steps().cpu().numpy().copy())
        steps.append(0)
        return out

    def step(actions):
        steps[-1] += 1
        return real_step(actions)
    env.reset, env.step = reset, step
    dataset_record.BACKEND = backend
    try:
        torch.manual_seed(2)
        info, failed = agent.eval(log=None)
    finally:
        dataset_record.BACKEND = None
        env.reset, env.step = real_reset, real_step
    torch.cuda.synchronize()
    _sweeps[key] = dict(info=info, failed=[str(k) for k in failed], rec=agent.last_dataset, first_obs=[o.cpu().numpy() for o in first_obs], num_steps=num_steps, steps=steps)
    return _sweeps[key]


@pytest.mark.parametrize("mode", ["host", "device"])
def test_sweep_records_on_the_device(mode):
    """The dataset from the launch is byte-equal to the one from the torch statement on a second, identically seeded run; every clip's first row is the row reset()
    returned for that env; lengths are min(T_batch, num_steps - 1); without noise clean == env action and eval_info equals a run without collect_dataset."""
    a, b = _sweep(mode, True, backend=None), _sweep(mode, True, backend="torch")
    ra, rb = a["rec"], b["rec"]
    assert ra is not None and len(ra.obs) == 16 and len(ra.keys) == 16 and len(set(ra.keys[:10])) == 10 and ra.keys[10:] == ra.keys[:6]      # the second batch wraps
    assert ra.keys == rb.keys and ra.lengths == rb.lengths and sum(ra.lengths) > 0
    assert len(a["steps"]) == 2 and a["steps"] == b["steps"]
    assert ra.lengths == [min(a["steps"][i // 8], max(int(a["num_steps"][i // 8][i % 8]) - 1, 0)) for i in range(16)]
    for k in ("obs", "clean", "env", "reset"):
        for i, (x, y) in enumerate(zip(getattr(ra, k), getattr(rb, k))):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (k, i)
    assert ra.obs[0].shape[1] == 934 and ra.clean[0].shape[1] == 69 and ra.reset[0].dtype == np.int64
    for i in range(16):
        if ra.lengths[i]:
            assert np.array_equal(ra.obs[i][0], a["first_obs"][i // 8][i % 8]), i       # (reset() is called once per batch)
        assert np.array_equal(ra.clean[i], ra.env[i])
        assert np.isfinite(ra.obs[i]).all() and np.isfinite(ra.clean[i]).all()
    plain = _sweep(mode, False)
    assert plain["rec"] is None and plain["failed"] == a["failed"]
    for k, v in plain["info"].items():
        assert (np.isnan(v) and np.isnan(a["info"][k])) or v == a["info"][k], k


def test_sweep_with_action_noise():
    """With noise on, clean and env actions differ by a draw of std 0.05."""
    n = _sweep("device", True, noise=True)
    rn = n["rec"]
    assert sum(rn.lengths) > 0
    diff = np.concatenate([e - c for e, c in zip(rn.env, rn.clean)])
    assert diff.size and 0.03 < diff.std() < 0.07 and np.abs(diff).max() > 0


def test_recorded_lengths_are_min_of_batch_steps_and_rows():
    """On a task driven by hand: rows = num_steps - 1 per env, a batch of T steps leaves min(T, rows) rows per clip (launch path)."""
    from phc_amd.learning.dataset_record import DatasetRecorder
    import types
    N, D, A = 6, 10, 4
    task = types.SimpleNamespace(obs_buf=torch.randn(N, D, device="cuda"), num_actions=A)
    rec = DatasetRecorder(task)
    num_steps = np.array([1, 2, 5, 9, 3, 0])
    rec.begin_batch(num_steps, [f"k{i}" for i in range(N)])
    first = task.obs_buf.clone()
    for s in range(4):
        task.clean_actions, task.actions = torch.randn(N, A, device="cuda"), torch.randn(N, A, device="cuda")
        task.reset_buf = torch.randint(0, 2, (N,), device="cuda")
        task.obs_buf = torch.randn(N, D, device="cuda")
        rec.record()
    rec.end_batch()
    assert rec.lengths == [0, 1, 4, 4, 2, 0] and [len(o) for o in rec.obs] == rec.lengths
    assert all(np.array_equal(rec.obs[i][0], first[i].cpu().numpy()) for i in range(N) if rec.lengths[i])


# ------------------------------------------------------------------------------------------------------------------ 6. end to end
@pytest.fixture
def restore_flags():
    """run.main sets the process-wide player flags (test / im_eval) as the reference's entry point does: put them back for the tests that follow."""
    from phc_amd.utils.flags import flags
    saved = (flags.test, flags.im_eval, flags.debug)
    yield
    flags.test, flags.im_eval, flags.debug = saved


def test_record_merge_train_play_through_run_main(tmp_path, restore_flags):
    """Record with run.main, `distill merge`, `distill train epochs=2`, then play the student in the sweep: a finite eval_info; a task with another obs_v is refused."""
    from phc_amd import distill, run
    out = str(tmp_path / "run")
    common = ["test=True", "im_eval=True", "env.num_envs=8", "env.motion_file=synthetic:10:3", f"output_path={out}"] + [f"{k}={v}" for k, v in SMALL.items()]
    torch.manual_seed(0)
    run.main(common + ["collect_dataset=True", "env.add_action_noise=True", "+env.action_noise_std=0.05", "+learning.params.config.eval_metrics=device"])
    d = os.path.join(out, "phc_act", "synthetic:10:3")
    files = os.listdir(d)
    assert len(files) == 1 and files[0].startswith("noise_True_0.05_")
    merged, meta = distill.main(["merge", f"dir={d}"])
    tr = distill.main(["train", f"dataset={merged}", f"metadata={meta}", f"output={out}/student", "units=[64,32]", "batch_size=256", "epochs=2", "save_frequency=100"])
    assert tr.epoch == 2 and os.path.exists(os.path.join(out, "student", "00002.pth")) and bool(torch.isfinite(tr.loss).all())
    info = run.main(common + [f"+student.checkpoint={out}/student/00002.pth"])
    assert all(np.isfinite(v) for k, v in info.items() if k in ("eval/success_rate", "eval/mpjpe_all")) and 0.0 <= info["eval/success_rate"] <= 1.0
    with pytest.raises(ValueError, match="934 observations"):
        run.main(common + ["env.obs_v=7", f"+student.checkpoint={out}/student/00002.pth"])
