"""float64 numpy statements of the four distillation kernels (csrc/phc_distill.hip) and the plain torch training loop the trainer is compared with.
Helper module of tests/test_distill_cpu.py and tests/test_distill_gpu.py (not a test)."""
import numpy as np


def sigmoid(z):
    """1 / (1 + exp(-z)) in float64 without overflow warnings: exp of -|z| only."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def silu(z):
    z = np.asarray(z, dtype=np.float64)
    return z * sigmoid(z)


def silu_grad(gy, z):
    """gy * d silu / dz = gy s (1 + z (1 - s)); (1 - s) = sigmoid(-z)."""
    gy, z = np.asarray(gy, dtype=np.float64), np.asarray(z, dtype=np.float64)
    return gy * sigmoid(z) * (1.0 + z * sigmoid(-z))


def colsum_silu(gy, z):
    """-> (gz [rows, cols], column sums of gz [cols])"""
    gz = silu_grad(gy, z)
    return gz, gz.sum(0)


def mse_loss(pred, target, row_index=None):
    """-> (loss, grad) of nn.MSELoss(): mean over all elements; grad = 2 (pred - target) / numel."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    t = target if row_index is None else target[np.asarray(row_index)]
    e = pred - t
    return float((e * e).mean()), 2.0 * e / e.size


def record(step, rows, row_start, obs_prev, obs_buf, clean, actions, reset_buf, block):
    """The recorder's rule on numpy arrays, in place: env i with step < rows[i] writes row row_start[i] + step of block = (obs, clean, env, reset);
    then obs_prev = obs_buf."""
    obs, cl, en, rs = block
    for i in range(len(rows)):
        if step < rows[i]:
            r = row_start[i] + step
            obs[r], cl[r], en[r], rs[r] = obs_prev[i], clean[i], actions[i], reset_buf[i]
    obs_prev[...] = obs_buf


def plain_loop(obs, act, mean, var, units, batch, epochs, lr, perms, init_state, dtype, autocast=False, device="cpu"):
    """The reference trainer's loop (train_phc_actor.py:73-80,165-188) as plain torch: standardise (eps 1e-5) + clamp +-5, nn.Sequential with nn.SiLU,
    nn.MSELoss, Adam(lr); minibatch k of epoch e is rows perms[e][k * batch:(k + 1) * batch].  `init_state`: state dict with the keys "<2k>.weight/bias".
    -> (final state dict in float64, last minibatch loss)."""
    import torch
    from torch import nn
    dims = [obs.shape[1]] + list(units)
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(a, b), nn.SiLU()]
    layers.append(nn.Linear(dims[-1], act.shape[1]))
    model = nn.Sequential(*layers).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in init_state.items()})
    model = model.to(device)
    x = torch.as_tensor(obs).to(dtype)
    x = ((x - torch.as_tensor(mean).float().to(dtype)) / torch.sqrt(torch.as_tensor(var).float().to(dtype) + 1e-05)).clamp(-5.0, 5.0).to(device)
    y = torch.as_tensor(act).to(dtype).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    crit = nn.MSELoss()
    loss = None
    for e in range(epochs):
        p = torch.as_tensor(perms[e]).to(device)
        for k in range(0, len(p), batch):
            idx = p[k:k + batch]
            if autocast:
                with torch.autocast(torch.device(device).type, dtype=torch.bfloat16):
                    out = model(x[idx])
                loss = crit(out.float(), y[idx])
            else:
                loss = crit(model(x[idx]), y[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
    return {k: v.detach().double().cpu() for k, v in model.state_dict().items()}, float(loss.detach())
