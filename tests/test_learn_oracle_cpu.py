"""The float64 references of oracle/learn_oracle.py against the torch expressions that define the learner kernels, in float64 on the CPU.

tests/test_learn_kernel_edges.py compares the HIP kernels with these references; this file keeps the references honest without a GPU.
"""
import numpy as np
import pytest
import torch

import learn_oracle as lo
import phc_oracle as po
from phc_amd.learning.amp_agent import discount_values
from phc_amd.learning.network import ModelAMPContinuous, policy_kl
from phc_amd.learning.running_mean_std import RunningMeanStd

F64 = torch.float64


def _close(a, b, rtol=1e-12, atol=1e-14):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-3])
@pytest.mark.parametrize("max_norm", [0.0, 5.0])
def test_adam_reference_equals_clip_grad_norm_and_torch_adam(weight_decay, max_norm):
    g = torch.Generator().manual_seed(11)
    n = 1000
    p0 = torch.randn(n, generator=g, dtype=F64)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    clipped = 0
    for step, gscale in enumerate((1.0, 1e-3, 0.5), start=1):
        grad = torch.randn(n, generator=g, dtype=F64) * gscale
        pt.grad = grad.clone()
        norm_t = torch.nn.utils.clip_grad_norm_([pt], max_norm) if max_norm > 0 else grad.norm()
        opt.step()
        p, gc, m, v, norm = lo.adam_clip_step(p, grad.numpy(), m, v, step, 3e-3, 0.9, 0.999, 1e-8, weight_decay, max_norm)
        clipped += max_norm > 0 and norm > max_norm
        _close(norm, float(norm_t))
        _close(gc, pt.grad.numpy())
        _close(p, pt.detach().numpy())
        st = opt.state[pt]
        _close(m, st["exp_avg"].numpy())
        _close(v, st["exp_avg_sq"].numpy())
    assert clipped == (2 if max_norm > 0 else 0)      # clipping active on steps 1 and 3, inactive on step 2


def test_disc_bce_reference_equals_bce_with_logits_and_its_gradient():
    g = torch.Generator().manual_seed(12)
    na, nd, scale = 300, 200, 2.5
    x = torch.randn(na + nd, 1, generator=g, dtype=F64) * 4
    x[:4, 0] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=F64)
    x[na:na + 4, 0] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=F64)
    x[10, 0] = x[na + 10, 0] = 0.0
    xr = x.clone().requires_grad_(True)
    bce = torch.nn.BCEWithLogitsLoss()
    loss = scale * 0.5 * (bce(xr[:na], torch.zeros(na, 1, dtype=F64)) + bce(xr[na:], torch.ones(nd, 1, dtype=F64)))
    loss.backward()
    stats, grad = lo.disc_bce(x.numpy(), na, scale)
    _close(stats[0], float(loss.detach()))
    _close(grad, xr.grad.numpy().ravel(), atol=1e-18)
    a, d = x[:na, 0], x[na:, 0]
    _close(stats[1:], [float((a < 0).double().mean()), float((d > 0).double().mean()), float(a.mean()), float(d.mean())])


def _ppo_inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    logstd = torch.full((D,), -2.9, dtype=F64) + torch.randn(D, generator=g, dtype=F64) * 0.1
    mu0 = torch.randn(B, D, generator=g, dtype=F64) * 0.7
    val0 = torch.randn(B, 1, generator=g, dtype=F64)
    old_mu = mu0 + torch.randn(B, D, generator=g, dtype=F64) * 0.004
    old_sigma = torch.exp(logstd).expand(B, D).contiguous()
    actions = old_mu + old_sigma * torch.randn(B, D, generator=g, dtype=F64)
    old_nlp = ModelAMPContinuous.neglogp(actions, old_mu, old_sigma, logstd.expand(B, D))
    adv = torch.randn(B, generator=g, dtype=F64)
    ret = torch.randn(B, 1, generator=g, dtype=F64)
    old_val = val0 + torch.randn(B, 1, generator=g, dtype=F64) * 0.3
    return logstd, mu0, val0, old_mu, old_sigma, actions, old_nlp, adv, ret, old_val


@pytest.mark.parametrize("clip_value", [False, True])
def test_ppo_reference_equals_the_torch_losses_and_their_gradients(clip_value):
    """The torch expressions of test_fused_ppo_loss_equals_torch_losses (IMAmpAgent._ppo_loss_torch), in float64, with autograd."""
    B, D = 600, 37
    e_clip, cc, ec, bl = 0.2, 5.0, 0.01, 10.0
    logstd, mu0, val0, old_mu, old_sigma, actions, old_nlp, adv, ret, old_val = _ppo_inputs(B, D, 13)
    mu, value = mu0.clone().requires_grad_(True), val0.clone().requires_grad_(True)
    sigma = torch.exp(logstd).expand(B, D)
    nlp = ModelAMPContinuous.neglogp(actions, mu, sigma, logstd.expand(B, D))
    ratio = torch.exp(old_nlp - nlp)
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - e_clip, 1 + e_clip)).mean()
    if clip_value:
        vpc = old_val + (value - old_val).clamp(-e_clip, e_clip)
        c_loss = torch.max((value - ret) ** 2, (vpc - ret) ** 2).mean()
    else:
        c_loss = ((ret - value) ** 2).mean()
    b_loss = ((torch.clamp_min(mu - 1, 0) ** 2) + (torch.clamp_max(mu + 1, 0) ** 2)).sum(-1).mean()
    ent = (0.5 + 0.5 * np.log(2 * np.pi) + logstd).sum()
    loss = a_loss + cc * c_loss - ec * ent + bl * b_loss
    loss.backward()
    kl = policy_kl(mu.detach(), sigma, old_mu, old_sigma)
    clip_frac = ((ratio - 1.0).abs() > e_clip).double().mean()
    assert 0.05 < float(clip_frac) < 0.95 and (mu0.abs() > 1).any()
    stats, gmu, gval, r = lo.ppo_loss(mu0.numpy(), val0.numpy(), logstd.numpy(), actions.numpy(), old_nlp.numpy(), adv.numpy(), ret.numpy(),
                                      old_val.numpy(), old_mu.numpy(), old_sigma.numpy(), e_clip, cc, ec, bl, clip_value)
    _close(r, ratio.detach().numpy(), rtol=1e-11)
    _close(stats, [float(t.detach()) for t in (loss, a_loss, c_loss, b_loss, ent, kl, clip_frac)], rtol=1e-11)
    _close(gmu, mu.grad.numpy(), rtol=1e-9, atol=1e-16)
    _close(gval, value.grad.numpy().ravel(), rtol=1e-9, atol=1e-16)
    # with a row index: the rollout tensors read at row_index[r]
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(1))[:B // 3]
    s2, g2, v2, _ = lo.ppo_loss(mu0[idx].numpy(), val0[idx].numpy(), logstd.numpy(), actions.numpy(), old_nlp.numpy(), adv.numpy(), ret.numpy(),
                                old_val.numpy(), old_mu.numpy(), old_sigma.numpy(), e_clip, cc, ec, bl, clip_value, row_index=idx.numpy())
    s3, g3, v3, _ = lo.ppo_loss(*(t[idx].numpy() if t.dim() > 1 or t.shape[0] == B else t.numpy()
                                  for t in (mu0, val0, logstd, actions, old_nlp, adv, ret, old_val, old_mu, old_sigma)), e_clip, cc, ec, bl, clip_value)
    _close(s2, s3, rtol=0, atol=0); _close(g2, g3, rtol=0, atol=0); _close(v2, v3, rtol=0, atol=0)


def test_running_norm_reference_equals_running_mean_std():
    g = torch.Generator().manual_seed(14)
    cols = 9
    rms = RunningMeanStd(cols)
    rms.running_mean.copy_(torch.randn(cols, generator=g, dtype=F64))
    rms.running_var.copy_(torch.rand(cols, generator=g, dtype=F64) + 0.1)
    rms.count.fill_(321.0)
    rms.train()
    mean, var, count = rms.running_mean.numpy().copy(), rms.running_var.numpy().copy(), float(rms.count)
    for it in range(3):
        x = torch.randn(50 + it, cols, generator=g, dtype=F64) * (1 + it) + 0.5
        x[0, 0] = 60.0      # clamped
        y = rms(x)
        # the module rounds the statistics to fp32 before normalising (running_mean_std.py:95-96), as the kernel does
        out, (mean, var, count) = lo.running_norm(x.numpy(), mean.astype(np.float32), var.astype(np.float32), 1e-5, 5.0, mean, var, count)
        _close(out, y.numpy(), rtol=1e-7)      # (the module adds epsilon to the fp32 variance in fp32)
        _close(mean, rms.running_mean.numpy()); _close(var, rms.running_var.numpy()); _close(count, float(rms.count))
    assert out[0, 0] == 5.0


def test_gae_reference_equals_discount_values():
    """The recurrence of tests/test_learner_cpu.py::test_gae_matches_oracle, with dones on the first and last step and T = 1."""
    g = torch.Generator().manual_seed(15)
    for T, N in ((16, 33), (1, 5)):
        fd = (torch.rand(T, N, generator=g) < 0.3).to(F64)
        fd[0, 0] = fd[-1, 1] = 1.0
        v, r, nv = (torch.randn(T, N, 1, generator=g, dtype=F64) for _ in range(3))
        want = discount_values(fd, v, r, nv, 0.99, 0.95)[..., 0].numpy()
        got = lo.gae(fd.numpy(), v[..., 0].numpy(), r[..., 0].numpy(), nv[..., 0].numpy(), 0.99, 0.95)
        _close(got, want, rtol=1e-6, atol=1e-6)      # (discount_values forms gamma * tau * (1 - done) as an fp32 tensor: 0.9405 rounded to fp32)
        _close(got, po.discount_values(fd.numpy(), v.numpy(), r.numpy(), nv.numpy(), 0.99, 0.95)[..., 0])


def test_small_references_by_hand():
    """The one-line references: sums of squares, slab sums, column sums, the one-output layer, policy sampling."""
    rng = np.random.default_rng(16)
    a, b = rng.standard_normal(7), rng.standard_normal((3, 4))
    _close(lo.weighted_sumsq([a, b], [0.5, 2.0]), [0.5 * (a @ a) + 2.0 * (b * b).sum(), a @ a, (b * b).sum()])
    part, out = rng.standard_normal((3, 5)), rng.standard_normal(5)
    _close(lo.sum_slabs(part), part[0] + part[1] + part[2])
    _close(lo.sum_slabs(part, out, True), out + part[0] + part[1] + part[2])
    x, gy, y = rng.standard_normal((6, 4)), rng.standard_normal((6, 4)), rng.standard_normal((6, 4))
    _close(lo.colsum(x), x.sum(0))
    gm, s = lo.colsum_relu(gy, y)
    _close(gm, gy * (y > 0)); _close(s, (gy * (y > 0)).sum(0))
    w, bias, g1 = rng.standard_normal(4), rng.standard_normal(1), rng.standard_normal(6)
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w[None], requires_grad=True)
    bt = torch.tensor(bias, requires_grad=True)
    yt = torch.nn.functional.linear(xt, wt, bt)
    yt.backward(torch.tensor(g1[:, None]))
    _close(lo.linear1_forward(x, w, bias), yt.detach().numpy().ravel())
    gx, gwb = lo.linear1_backward(x, w, g1)
    _close(gx, xt.grad.numpy()); _close(gwb, np.concatenate([wt.grad.numpy().ravel(), bt.grad.numpy()]))
    mu, ls, z = rng.standard_normal((6, 4)), rng.standard_normal(4) * 0.1 - 2, rng.standard_normal((6, 4))
    o = lo.policy_sample(mu, np.array([9.0, -1.0, 0.5, 2.0, -7.0, 0.0]), ls, z, 0.7, 2.5, 1e-5, mask=np.array([0, 1, 0, 0, 1, 0.0]))
    act = torch.tensor(mu) + torch.exp(torch.tensor(ls)) * torch.tensor(z)
    _close(o["actions"], act.numpy())
    _close(o["neglogp"], ModelAMPContinuous.neglogp(act, torch.tensor(mu), torch.exp(torch.tensor(ls)).expand(6, 4), torch.tensor(ls).expand(6, 4)).numpy())
    _close(o["values"], np.sqrt(2.5 + 1e-5) * np.array([5.0, 0.0, 0.5, 2.0, 0.0, 0.0]) + 0.7 * np.array([1, 0, 1, 1, 0, 1.0]))
