"""Float64 references of the learner-side C ABI (include/phc_amd.h), written from the formulas documented there.

Plain numpy in double precision: nothing here calls the library or its host wrappers.  tests/test_learn_oracle_cpu.py pins each
function to the torch expression the project treats as the definition (clip_grad_norm_ + torch.optim.Adam, BCEWithLogitsLoss,
IMAmpAgent's PPO loss, RunningMeanStd, discount_values); tests/test_learn_kernel_edges.py compares the HIP kernels with them.
Inputs may be any float dtype; every computation is carried out in float64.
"""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def _f64(*xs):
    return [None if x is None else np.asarray(x, dtype=np.float64) for x in xs]


def adam_clip_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, max_norm):
    """phc_adam_clip_step: grad *= min(1, max_norm / (|grad| + 1e-6)) (max_norm <= 0: no clipping), then torch.optim.Adam with L2 weight
    decay and the bias corrections of the 1-based `step`.  Returns (param, clipped grad, exp_avg, exp_avg_sq, |grad| before clipping)."""
    p, g, m, v = _f64(param, grad, exp_avg, exp_avg_sq)
    norm = float(np.sqrt(np.sum(g * g)))
    if max_norm > 0:
        g = g * min(1.0, max_norm / (norm + 1e-6))
    d = g + weight_decay * p if weight_decay != 0 else g
    m = beta1 * m + (1.0 - beta1) * d
    v = beta2 * v + (1.0 - beta2) * d * d
    bias1 = 1.0 - beta1 ** step
    bias2 = 1.0 - beta2 ** step
    p = p - (lr / bias1) * m / (np.sqrt(v) / np.sqrt(bias2) + eps)
    return p, g, m, v, norm


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def disc_bce(logits, n_agent, scale):
    """phc_disc_bce: stats[5] = (scale * 0.5 (BCE(agent, 0) + BCE(demo, 1)), mean(agent < 0), mean(demo > 0), mean(agent), mean(demo)) and
    grad = d stats[0] / d logits."""
    (x,) = _f64(np.ravel(logits))
    a, d = x[:n_agent], x[n_agent:]
    loss = scale * 0.5 * (softplus(a).mean() + (softplus(d) - d).mean())
    stats = np.array([loss, (a < 0).mean(), (d > 0).mean(), a.mean(), d.mean()])
    grad = np.concatenate([scale * 0.5 * sigmoid(a) / len(a), scale * 0.5 * (sigmoid(d) - 1.0) / len(d)])
    return stats, grad


def weighted_sumsq(tensors, coefs):
    """phc_weighted_sumsq: out[0] = sum_i coefs[i] |t_i|^2, out[1 + i] = |t_i|^2."""
    sq = [float(np.sum(np.square(np.asarray(t, dtype=np.float64)))) for t in tensors]
    return np.array([sum(float(c) * s for c, s in zip(coefs, sq))] + sq)


def sum_slabs(part, out=None, accumulate=False):
    """phc_sum_slabs_bf16: part [slabs, n] -> sum over slabs, added to `out` when accumulating."""
    (p,) = _f64(part)
    s = p.sum(0)
    return s + np.asarray(out, dtype=np.float64) if accumulate else s


def neglogp(actions, mu, logstd):
    a, m, ls = _f64(actions, mu, logstd)
    sg = np.exp(ls)
    return 0.5 * (((a - m) / sg) ** 2).sum(-1) + 0.5 * LOG_2PI * a.shape[-1] + ls.sum(-1)


def ppo_loss(mu, value, logstd, actions, old_neglogp, adv, ret, old_value, old_mu, old_sigma, e_clip, critic_coef, entropy_coef,
             bounds_loss_coef, clip_value, row_index=None):
    """phc_ppo_loss: stats[7] = (loss, mean a_loss, mean c_loss, mean b_loss, entropy, mean kl, clip fraction), d loss / d mu [B, D] and
    d loss / d value [B].  Rollout tensors are read at row_index[r] for minibatch row r when a row index is given.  torch.max passes
    half the gradient to each operand of a tie; torch.clamp passes it on the closed interval."""
    mu, value, logstd = _f64(mu, value, logstd)
    value = value.reshape(-1)
    B, D = mu.shape
    q = np.arange(B) if row_index is None else np.asarray(row_index)
    a, onlp, A, R, om, osg = (x[q] for x in _f64(actions, np.ravel(old_neglogp), np.ravel(adv), np.ravel(ret), old_mu, old_sigma))
    sg = np.exp(logstd)
    nlp = 0.5 * (((a - mu) / sg) ** 2).sum(-1) + 0.5 * LOG_2PI * D + logstd.sum()
    ratio = np.exp(onlp - nlp)
    lo, hi = 1.0 - e_clip, 1.0 + e_clip
    t1, t2 = -A * ratio, -A * np.clip(ratio, lo, hi)
    a_loss = np.maximum(t1, t2)
    w1 = np.where(t1 > t2, 1.0, np.where(t1 == t2, 0.5, 0.0))
    inside = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)
    d_ratio = -A * (w1 + (1.0 - w1) * inside)                      # d a_loss / d ratio
    if clip_value:
        vp = np.ravel(_f64(old_value)[0])[q]
        dv = value - vp
        vpc = vp + np.clip(dv, -e_clip, e_clip)
        l1, l2 = (value - R) ** 2, (vpc - R) ** 2
        c_loss = np.maximum(l1, l2)
        u1 = np.where(l1 > l2, 1.0, np.where(l1 == l2, 0.5, 0.0))
        in2 = ((dv >= -e_clip) & (dv <= e_clip)).astype(np.float64)
        d_c = u1 * 2.0 * (value - R) + (1.0 - u1) * 2.0 * (vpc - R) * in2
    else:
        c_loss = (R - value) ** 2
        d_c = 2.0 * (value - R)
    b_loss = (np.maximum(mu - 1.0, 0.0) ** 2 + np.minimum(mu + 1.0, 0.0) ** 2).sum(-1)
    entropy = float((0.5 + 0.5 * LOG_2PI + logstd).sum())
    kl = (np.log(osg / sg + 1e-5) + (sg ** 2 + (om - mu) ** 2) / (2.0 * (osg ** 2 + 1e-5)) - 0.5).sum(-1)
    clipped = (np.abs(ratio - 1.0) > e_clip).astype(np.float64)
    loss = a_loss.mean() + critic_coef * c_loss.mean() - entropy_coef * entropy + bounds_loss_coef * b_loss.mean()
    stats = np.array([loss, a_loss.mean(), c_loss.mean(), b_loss.mean(), entropy, kl.mean(), clipped.mean()])
    # d nlp / d mu = -(a - mu) / sigma^2, d ratio / d nlp = -ratio
    grad_mu = (d_ratio * ratio / B)[:, None] * (a - mu) / sg ** 2 \
        + (bounds_loss_coef / B) * (2.0 * np.maximum(mu - 1.0, 0.0) + 2.0 * np.minimum(mu + 1.0, 0.0))
    grad_value = critic_coef * d_c / B
    return stats, grad_mu, grad_value, ratio


def policy_sample(mu, value, logstd, noise, value_mean, value_var, epsilon, mask=None):
    """phc_policy_sample: (actions, mus, sigmas, neglogp) from mu [N, D] (None: skipped) and the un-normalised, masked value [N]
    (None: skipped; value_mean None: no un-normalisation)."""
    out = {}
    if mu is not None:
        m, ls, z = _f64(mu, logstd, noise)
        sg = np.broadcast_to(np.exp(ls), m.shape)
        act = m + sg * z
        out.update(actions=act, mus=m, sigmas=sg, neglogp=neglogp(act, m, np.broadcast_to(ls, m.shape)))
    if value is not None:
        (v,) = _f64(np.ravel(value))
        if value_mean is not None:
            v = np.sqrt(float(value_var) + epsilon) * np.clip(v, -5.0, 5.0) + float(value_mean)
        if mask is not None:
            v = v * (1.0 - np.asarray(mask, dtype=np.float64))
        out["values"] = v
    return out


def running_norm(x, norm_mean, norm_var, epsilon, clamp, run_mean=None, run_var=None, run_count=None, row_index=None):
    """phc_running_norm: out = clamp((x - norm_mean) / sqrt(norm_var + eps), -clamp, clamp) and, when run_* are given, the parallel-variance
    update with the batch mean and unbiased variance.  Returns (out, (mean, var, count) or None)."""
    (xs,) = _f64(x)
    if row_index is not None:
        xs = xs[np.asarray(row_index)]
    nm, nv = _f64(norm_mean, norm_var)
    out = np.clip((xs - nm) / np.sqrt(nv + epsilon), -clamp, clamp)
    if run_mean is None:
        return out, None
    mean, var = _f64(run_mean, run_var)
    count, n = float(run_count), float(xs.shape[0])
    bm = xs.mean(0)
    bv = xs.var(0, ddof=1) if n > 1 else np.full(xs.shape[1], np.nan)
    tot = count + n
    delta = bm - mean
    new_mean = mean + delta * n / tot
    new_var = (var * count + bv * n + delta ** 2 * count * n / tot) / tot
    return out, (new_mean, new_var, tot)


def colsum(x):
    (x,) = _f64(x)
    return x.sum(0)


def colsum_relu(gy, y):
    """phc_colsum_relu_bf16: gm = gy where y > 0 else 0, and its column sums."""
    g, yy = _f64(gy, y)
    gm = np.where(yy > 0, g, 0.0)
    return gm, gm.sum(0)


def linear1_forward(x, w, b):
    x, w, b = _f64(x, w, b)
    return x @ w.reshape(-1) + float(np.ravel(b)[0])


def linear1_backward(x, w, gy):
    """phc_linear1_backward: gx = gy w^T [rows, cols], gw_gb = (gy^T x, sum gy) [cols + 1]."""
    x, w, g = _f64(x, w, np.ravel(gy))
    return np.outer(g, w.reshape(-1)), np.concatenate([g @ x, [g.sum()]])


def gae(fdones, values, rewards, next_values, gamma, tau):
    """phc_gae: tensors [T, N]; last = delta_t + gamma tau (1 - done_t) last, scanned backwards over t."""
    fd, v, r, nv = _f64(fdones, values, rewards, next_values)
    adv = np.zeros_like(r)
    last = np.zeros(r.shape[1:])
    for t in reversed(range(r.shape[0])):
        last = r[t] + gamma * nv[t] - v[t] + gamma * tau * (1.0 - fd[t]) * last
        adv[t] = last
    return adv
