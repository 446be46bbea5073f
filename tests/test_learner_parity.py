"""Learner rows pinned to the REFERENCE'S OWN method bodies (A1, P2, P3, P5, P6, P8; 8b: B4).

The fixtures `tests/golden/learner_{fns,step,pnn}.npz` and `pd_offset_scale.npz` are outputs of the unmodified reference classes --
`CommonAgent.discount_values / _actor_loss / _critic_loss / bound_loss / _calc_advs`, one whole `AMPAgent.calc_gradients` (forward through
the reference's `AMPBuilder` network and `ModelAMPContinuous`, `_disc_loss` with the gradient penalty, backward, `clip_grad_norm_`, Adam),
`AMPAgent._calc_disc_rewards / _combine_rewards`, the PNN / MCP builders, `network_loader.load_pnn / load_mcp_mlp`,
`Humanoid._build_pd_action_offset_scale` -- produced by `oracle/gen_golden_learner.py` in the build container.

CPU tests: the agent's torch path (which is also the definition the HIP kernels are tested against elsewhere).
`-m gpu` tests: the SAME comparisons through the product path on the device -- `phc_gae`, `phc_running_norm`, `phc_ppo_loss`,
`phc_disc_bce`, `phc_weighted_sumsq`, FastLinear / FastLinearDD, `phc_adam_clip_step` -- in fp32 (tight tolerance) and with bf16 GEMMs.

Loading the reference's state dict with `strict=True` is the B4 check: the key sets are identical."""
import os

import numpy as np
import pytest
import torch

import phc_oracle as po
from phc_amd.config import compose
from phc_amd.learning.amp_agent import IMAmpAgent, discount_values

O, M, A, T, N, MB, AMB = 40, 36, 9, 8, 16, 64, 32


class _Task:
    temp_running_mean = True
    shape_resampling_interval = 500

    def __init__(self, device, actions=A, obs=O, amp=M):
        self.device, self.num_envs, self._a, self._m = device, N, actions, amp
        self.obs_buf = torch.zeros(N, obs, device=device)
        self.reset_buf = torch.zeros(N, dtype=torch.long, device=device)

    def get_num_amp_obs(self):
        return self._m

    def get_task_obs_size_detail(self):
        return {"num_prim": 3, "training_prim": 1, "has_lateral": False}


class _Env:
    clip_obs = np.inf

    def __init__(self, device="cpu", actions=A, obs=O, amp=M):
        self.task = _Task(device, actions, obs, amp)
        self.num_envs, self.num_obs, self.num_actions = N, obs, actions


def _cfg(learning="im", extra=(), mb=MB, amb=AMB, units=(64, 32), disc_units=(48, 24)):
    return compose([f"learning={learning}", f"learning.params.config.horizon_length={T}", f"learning.params.config.minibatch_size={mb}",
                    f"learning.params.config.amp_minibatch_size={amb}", "learning.params.config.amp_batch_size=16",
                    "learning.params.config.amp_obs_demo_buffer_size=256", "learning.params.config.amp_replay_buffer_size=256",
                    f"learning.params.network.mlp.units=[{','.join(str(int(u)) for u in units)}]",
                    f"learning.params.network.disc.units=[{','.join(str(int(u)) for u in disc_units)}]"] + list(extra))


def _dims(g):
    """(O, M, A, MB, AMB, units, disc_units) of a learner_step* fixture."""
    if "dims" in g:
        o, m, a, _, _, mb, amb = (int(v) for v in g["dims"])
        return o, m, a, mb, amb, tuple(g["units"]), tuple(g["disc_units"])
    return O, M, A, MB, AMB, (64, 32), (48, 24)


def _sub(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.asarray(g[k])) for k in g if k.startswith(prefix)}


def _agent_from_golden(g, device="cpu", bf16=False, extra=()):
    torch.manual_seed(0)
    o, m, a, mb, amb, units, disc_units = _dims(g)
    agent = IMAmpAgent(_Env(device, a, o, m), _cfg(mb=mb, amb=amb, units=units, disc_units=disc_units, extra=extra), bf16=bf16)
    agent.model.load_state_dict(_sub(g, "model/"), strict=True)          # B4: the reference's key set, nothing missing, nothing extra
    if agent.grads.shadow is not None:
        agent.grads.shadow.copy_(agent.grads.flat_param)
    agent.running_mean_std.load_state_dict(_sub(g, "running_mean_std/"))
    agent.value_mean_std.load_state_dict(_sub(g, "reward_mean_std/"))
    agent._amp_input_mean_std.load_state_dict(_sub(g, "amp_input_mean_std/"))
    agent._snapshot_running_mean_std()
    agent.running_mean_std_temp.load_state_dict(_sub(g, "running_mean_std_temp/"))
    return agent


# ------------------------------------------------------------------------------------------------------------------ A1
def test_pd_action_offset_scale_equals_the_reference_method(golden):
    from phc_amd.model import load_model
    g = golden("pd_offset_scale")
    tags = sorted({k.rsplit("/", 1)[0] for k in g if k.endswith("/offset")})
    assert len(tags) == 8
    for tag in tags:
        htype, flags_ = tag.split("/")
        m = load_model({"smpl": "smpl_humanoid", "h1": "h1_humanoid", "g1": "g1_humanoid"}[htype])
        lo, hi = m.dof_limits()
        np.testing.assert_array_equal(lo, g[f"{htype}/lim_low"])
        bias, pdoff, upright = (bool(int(f[-1])) for f in flags_.split("_"))
        off, scale = m.pd_action_offset_scale(bias, pdoff, upright)
        np.testing.assert_allclose(off, g[tag + "/offset"], rtol=0, atol=1e-7, err_msg=tag)
        np.testing.assert_allclose(scale, g[tag + "/scale"], rtol=1e-7, atol=0, err_msg=tag)
        if tag == "smpl/bias0_pdoff0_upright1":    # the numpy oracle's restatement (shipped SMPL configuration) against the same fixture
            o2, s2 = po.build_pd_action_offset_scale_smpl(lo, hi, m.body_names[1:])
            np.testing.assert_allclose(o2, g[tag + "/offset"], atol=1e-7)
            np.testing.assert_allclose(s2, g[tag + "/scale"], rtol=1e-7)


# ------------------------------------------------------------------------------------------------------------------ P5 + loss pieces
def test_gae_and_loss_terms_equal_the_reference_methods(golden):
    g = golden("learner_fns")
    t = lambda k: torch.from_numpy(g[k])
    advs = discount_values(t("gae_fdones"), t("gae_values"), t("gae_rewards"), t("gae_next_values"), float(g["gamma"]), float(g["tau"]))
    np.testing.assert_allclose(advs.numpy(), g["gae_advs"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(po.discount_values(g["gae_fdones"], g["gae_values"], g["gae_rewards"], g["gae_next_values"], float(g["gamma"]), float(g["tau"])),
                               g["gae_advs"], rtol=1e-6, atol=1e-6)
    agent = IMAmpAgent(_Env(), _cfg())
    for clip_value, key in ((True, "cl_loss_clip"), (False, "cl_loss_noclip")):
        agent.clip_value = clip_value
        B = g["al_adv"].shape[0]
        res = {"prev_neglogp": t("al_logp"), "values": t("cl_values"), "mus": t("bl_mu"), "sigmas": torch.ones(B, A), "entropy": torch.zeros(B)}
        d = {"old_logp_actions": t("al_old_logp"), "advantages": t("al_adv"), "returns": t("cl_returns"), "old_values": t("cl_value_preds"),
             "mu": t("bl_mu"), "sigma": torch.ones(B, A)}
        _, info = agent._ppo_loss_torch(res, d, {"disc_loss": torch.zeros(())})
        np.testing.assert_allclose(float(info["actor_loss"]), g["al_loss"].mean(), rtol=1e-6)
        np.testing.assert_allclose(float(info["critic_loss"]), g[key].mean(), rtol=1e-6)
        np.testing.assert_allclose(float(info["b_loss"]), g["bl_loss"].mean(), rtol=1e-6)
    np.testing.assert_allclose(agent.bound_loss(t("bl_mu")).numpy(), g["bl_loss"], rtol=1e-6)
    # _calc_advs (common_agent.py:589-599) is the first two lines of prepare_dataset
    ret, val = t("adv_returns"), t("adv_values")
    a = torch.sum(ret - val, axis=1)
    np.testing.assert_allclose(((a - a.mean()) / (a.std() + 1e-8)).numpy(), g["adv_out"], rtol=1e-6, atol=1e-7)


def _run_step(agent, g, device, dataset_form):
    d = {k: v.to(device) for k, v in _sub(g, "in/").items()}
    if dataset_form:   # the device form: persistent dataset + row index, the kernels gather in place
        _, _, _, mb, amb, _, _ = _dims(g)
        idx = torch.arange(mb, device=device)
        return agent.calc_gradients({"_dataset": d, "_idx": idx, "_amp_idx": idx[:amb]})
    return agent.calc_gradients(d)


def _check_step(agent, g, info, rtol_loss, grad_rtol, grad_atol, param_atol, skip=(), stats_rtol=1e-9):
    for k in ("actor_loss", "critic_loss", "b_loss", "entropy", "kl", "disc_loss", "disc_grad_penalty", "disc_logit_loss"):
        if k in skip:
            continue
        atol = rtol_loss * 1e-2
        if k == "actor_loss":   # a mean of signed terms of size |advantage| that nearly cancels: the error scales with the terms, not with the mean
            atol = max(atol, rtol_loss * 0.1 * float(np.abs(g["in/advantages"]).mean()))
        np.testing.assert_allclose(float(info[k]), float(g["res/" + k]), rtol=rtol_loss, atol=atol, err_msg=k)
    for k in ("disc_agent_acc", "disc_demo_acc"):
        assert abs(float(info[k]) - float(g["res/" + k])) <= (0.0 if rtol_loss < 1e-3 else 2.0 / _dims(g)[4]), k
    names = [str(n) for n in g["param_names"]]
    params = dict(agent.model.named_parameters())
    assert list(params) == names                                        # same parameters, same ORDER (optimizer state layout, B4)
    assert [bool(p.requires_grad) for p in params.values()] == [bool(x) for x in g["param_requires_grad"]]
    worst = 0.0
    for n in names:
        if "grad/" + n not in g:
            assert not params[n].requires_grad or params[n].grad is None or float(params[n].grad.abs().max()) == 0, n
            continue
        if any(t in n for t in skip):
            continue
        ref = g["grad/" + n]
        got = params[n].grad.detach().float().cpu().numpy()
        scale = max(np.abs(ref).max(), 1e-12)
        worst = max(worst, float(np.abs(got - ref).max() / scale))
        np.testing.assert_allclose(got, ref, rtol=grad_rtol, atol=grad_atol + grad_rtol * scale, err_msg="grad " + n)
    after = _sub(g, "model_after/")
    before = _sub(g, "model/")
    lr = float(agent.last_lr)
    for n, p in agent.model.state_dict().items():
        ref = after[n].numpy()
        atol = np.full(ref.shape, param_atol, np.float64)
        if "grad/" + n in g:
            # Adam's first step is -lr g / (|g| + eps) = -lr sign(g): an element whose reference gradient lies inside the gradient tolerance
            # may step the other way (seen: 1 of 18432 weights of the wide fixture)
            gr = g["grad/" + n]
            atol = np.where(np.abs(gr) <= grad_atol + grad_rtol * max(np.abs(gr).max(), 1e-12), param_atol + 2.0 * lr, param_atol)
        err = np.abs(p.detach().float().cpu().numpy().astype(np.float64) - ref)
        assert (err <= atol).all(), f"param {n}: {int((err > atol).sum())} of {err.size} elements off, worst {err.max():.3e}"
    moved = max(float((after[n] - before[n]).abs().max()) for n in names)
    assert moved > 1e-5            # lr 2e-5: Adam's first step moves every weight by ~lr
    for nm, mod in (("running_mean_std", agent.running_mean_std), ("amp_input_mean_std", agent._amp_input_mean_std)):
        for k, v in _sub(g, nm + "_after/").items():
            np.testing.assert_allclose(getattr(mod, k).detach().cpu().numpy(), v.numpy(), rtol=stats_rtol, atol=1e-12, err_msg=f"{nm}.{k}")
    return worst


# ------------------------------------------------------------------------------------------------------------------ P2 + P6 + P8 + B4 (CPU)
@pytest.mark.parametrize("fixture", ["learner_step", "learner_step_policy_actions", "learner_step_wide"])
def test_calc_gradients_equals_the_reference_agent_cpu(golden, fixture):
    g = golden(fixture)
    agent = _agent_from_golden(g)
    # P6 first (evaluation mode, statistics untouched)
    agent.set_eval()
    amp_r = agent._calc_amp_rewards(torch.from_numpy(g["p6_amp_obs"]))
    np.testing.assert_allclose(amp_r["disc_rewards"].numpy(), g["p6_disc_rewards"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(agent._combine_rewards(torch.from_numpy(g["p6_task_rewards"]), amp_r).numpy(), g["p6_combined"], rtol=1e-5, atol=1e-6)
    info = _run_step(agent, g, "cpu", dataset_form=False)
    _check_step(agent, g, info, rtol_loss=2e-5, grad_rtol=2e-4, grad_atol=1e-7, param_atol=2e-7)
    # the optimizer state this step produced, in the checkpoint's per-parameter layout == the reference optimizer's state
    sd = agent.get_full_state_weights()["optimizer"]
    assert sd["param_groups"][0]["params"] == list(g["opt/param_ids"]) and sorted(sd["state"]) == list(g["opt/state_ids"])
    for i in g["opt/state_ids"]:
        np.testing.assert_allclose(sd["state"][int(i)]["exp_avg"].numpy(), g[f"opt/{i}/exp_avg"], rtol=2e-4, atol=1e-9)
        np.testing.assert_allclose(sd["state"][int(i)]["exp_avg_sq"].numpy(), g[f"opt/{i}/exp_avg_sq"], rtol=4e-4, atol=1e-12)
        assert float(sd["state"][int(i)]["step"]) == float(g[f"opt/{i}/step"]) == 1.0


# ------------------------------------------------------------------------------------------------------------------ P3 + B4
def test_pnn_and_mcp_networks_and_checkpoint_loaders_equal_the_reference(golden):
    from phc_amd.env.tasks.humanoid_im_mcp import load_mcp_mlp, load_pnn
    from phc_amd.learning.network import A2CMCPNetwork, A2CNetwork, A2CPNNNetwork, ModelAMPContinuous, forward_pmcp
    g = golden("learner_pnn")
    x = torch.from_numpy(g["pnn_x"])
    detail = {"num_prim": 3, "training_prim": 1, "has_lateral": False}
    # PNN network: key set, trainable set, forward
    net = ModelAMPContinuous(A2CPNNNetwork(_cfg("im_pnn")["learning"]["params"]["network"], A, (O,), (M,), detail))
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g["pnn_param_names"]]
    assert [bool(p.requires_grad) for _, p in net.named_parameters() if "pnn" in _] == \
        [bool(r) for n, r in zip(g["pnn_param_names"], g["pnn_requires_grad"]) if "pnn" in str(n)]
    net.load_state_dict(_sub(g, "pnn_model/"), strict=True)
    net.eval()
    with torch.no_grad():
        mu, logstd = net.a2c_network.eval_actor(x)
        np.testing.assert_allclose(mu.numpy(), g["pnn_mu"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(logstd.numpy(), g["pnn_sigma"], rtol=0, atol=0)
        np.testing.assert_allclose(net.a2c_network.eval_critic(x).numpy(), g["pnn_value"], rtol=1e-5, atol=1e-6)
    # env-side loader on the reference-shaped checkpoint (network_loader.py:54-74)
    ck = {"model": _sub(g, "pnn_model/")}
    pnn = load_pnn(ck, num_prim=3, has_lateral=False, activation="relu", device="cpu")
    with torch.no_grad():
        _, acts = pnn(x)
    np.testing.assert_allclose(torch.stack(acts, dim=1).numpy(), g["load_pnn_actions"], rtol=1e-5, atol=1e-6)
    assert not any(p.requires_grad for p in pnn.parameters())
    # scripts/pmcp/forward_pmcp.py: column 1 -> column 2
    ck2 = forward_pmcp({"model": {k: v.clone() for k, v in ck["model"].items()}}, 1)
    want = _sub(g, "pmcp_model/")
    assert set(ck2["model"]) == set(want)
    for k, v in want.items():
        assert torch.equal(ck2["model"][k], v), k
    # MCP composer network
    pm = _cfg("im_mcp")["learning"]["params"]["network"]
    assert bool(pm.get("has_softmax", True)) == bool(g["mcp_has_softmax"]) and bool(pm.get("ending_act", True)) == bool(g["mcp_ending_act"])
    mcp = ModelAMPContinuous(A2CMCPNetwork(pm, 3, (O,), (M,), detail))
    assert [n for n, _ in mcp.named_parameters()] == [str(s) for s in g["mcp_param_names"]]
    mcp.load_state_dict(_sub(g, "mcp_model/"), strict=True)
    mcp.eval()
    with torch.no_grad():
        np.testing.assert_allclose(mcp.a2c_network.eval_actor(x)[0].numpy(), g["mcp_mu"], rtol=1e-5, atol=1e-6)
    # load_mcp_mlp on a plain `amp` checkpoint (network_loader.py:11-52) and the plain network itself
    plain = ModelAMPContinuous(A2CNetwork(_cfg()["learning"]["params"]["network"], A, (O,), (M,)))
    plain.load_state_dict(_sub(g, "amp_model/"), strict=True)
    plain.eval()
    mlp = load_mcp_mlp({"model": _sub(g, "amp_model/")}, activation="relu", device="cpu", mlp_name="actor_mlp")
    with torch.no_grad():
        np.testing.assert_allclose(mlp(x).numpy(), g["load_mcp_mlp_out"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(plain.a2c_network.eval_actor(x)[0].numpy(), g["amp_mu"], rtol=1e-5, atol=1e-6)


def test_pnn_lateral_connections_equal_the_reference(golden):
    """pnn.py:25-38,84-126 (has_lateral: off in the shipped yamls): same key set, same outputs for idx = -1 / 0 / 1."""
    from phc_amd.learning.network import PNN
    g = golden("learner_pnn")
    x = torch.from_numpy(g["pnn_x"])
    pnn = PNN(O, [64, 32], "relu", A, 3, has_lateral=True)
    sd = _sub(g, "lat_model/")
    assert set(pnn.state_dict()) == set(sd)
    pnn.load_state_dict(sd, strict=True)
    pnn.eval()
    with torch.no_grad():
        a_all, outs = pnn(x, idx=-1)
        np.testing.assert_allclose(torch.stack(outs, dim=1).numpy(), g["lat_out_all"], rtol=1e-5, atol=1e-6)
        a1, outs1 = pnn(x, idx=1)
        np.testing.assert_allclose(a1.numpy(), g["lat_out_idx1"], rtol=1e-5, atol=1e-6)
        assert len(outs1) == int(g["lat_n_idx1"])
        np.testing.assert_allclose(pnn(x, idx=0)[0].numpy(), g["lat_out_idx0"], rtol=1e-5, atol=1e-6)


def test_released_checkpoint_layout_round_trip(golden, tmp_path):
    """B4 / f-2: a file with the reference's full checkpoint layout (`get_full_state_weights`, common_agent.py:405-433: model, epoch,
    optimizer = Adam(model.parameters()).state_dict(), frame, running_mean_std, reward_mean_std, amp_input_mean_std) restores through
    `IMAmpAgent.restore`, acts identically to the reference network on fixed observations, and what we save loads back into a plain
    torch module + optimizer with the reference's layout."""
    g = golden("learner_step")
    agent = _agent_from_golden(g)
    ref_opt_state = {int(i): {"step": torch.tensor(float(g[f"opt/{i}/step"])), "exp_avg": torch.from_numpy(g[f"opt/{i}/exp_avg"]),
                              "exp_avg_sq": torch.from_numpy(g[f"opt/{i}/exp_avg_sq"])} for i in g["opt/state_ids"]}
    group = dict(torch.optim.Adam([torch.zeros(1, requires_grad=True)], 2e-5, eps=1e-8).state_dict()["param_groups"][0])
    group["params"] = [int(i) for i in g["opt/param_ids"]]
    ck = {"model": _sub(g, "model_after/"), "epoch": 12, "frame": 34, "optimizer": {"state": ref_opt_state, "param_groups": [group]},
          "running_mean_std": _sub(g, "running_mean_std_after/"), "reward_mean_std": _sub(g, "reward_mean_std/"),
          "amp_input_mean_std": _sub(g, "amp_input_mean_std_after/")}
    path = str(tmp_path / "Humanoid.pth")
    torch.save(ck, path)
    torch.manual_seed(5)
    fresh = IMAmpAgent(_Env(), _cfg(), bf16=False)
    fresh.restore(path)
    assert fresh.epoch_num == 12 and fresh.frame == 34
    st = fresh.optimizer.state[fresh.grads.flat_param]
    for k, i in enumerate(g["opt/state_ids"]):   # (per parameter: the flat state has 16-byte alignment gaps between segments)
        assert torch.equal(fresh.grads.param_view(st["exp_avg"], k), ref_opt_state[int(i)]["exp_avg"])
    assert float(st["step"]) == 1.0
    for n, p in fresh.model.state_dict().items():
        assert torch.equal(p, ck["model"][n]), n
    # second step from the restored state == continuing an agent that took the first step itself
    fresh._snapshot_running_mean_std()
    fresh.running_mean_std_temp.load_state_dict(_sub(g, "running_mean_std_temp/"))
    _run_step(agent, g, "cpu", False)                # step 1 (== the reference's, test above)
    info_a = _run_step(agent, g, "cpu", False)       # step 2
    info_b = _run_step(fresh, g, "cpu", False)       # step 2 from the reference's checkpoint after step 1
    for (n, p), (_, q) in zip(agent.model.state_dict().items(), fresh.model.state_dict().items()):
        np.testing.assert_allclose(p.numpy(), q.numpy(), rtol=0, atol=5e-7, err_msg=n)
    assert abs(float(info_a["disc_loss"]) - float(info_b["disc_loss"])) < 1e-5
    # and back: our file -> plain torch objects with the reference's layout
    out = str(tmp_path / "ours.pth")
    fresh.save(out)
    w = torch.load(out, weights_only=False)
    assert set(w) >= {"model", "epoch", "optimizer", "frame", "running_mean_std", "reward_mean_std", "amp_input_mean_std"}
    assert set(w["model"]) == set(ck["model"]) and w["optimizer"]["param_groups"][0]["params"] == group["params"]
    assert sorted(w["optimizer"]["state"]) == sorted(ref_opt_state)


# ------------------------------------------------------------------------------------------------------------------ the product path on the device
@pytest.mark.gpu
def test_gae_kernel_equals_the_reference_method(golden):
    g = golden("learner_fns")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    advs = discount_values(t("gae_fdones"), t("gae_values"), t("gae_rewards"), t("gae_next_values"), float(g["gamma"]), float(g["tau"]))
    np.testing.assert_allclose(advs.cpu().numpy(), g["gae_advs"], rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("fixture", ["learner_step", "learner_step_policy_actions", "learner_step_wide"])
def test_calc_gradients_equals_the_reference_agent_on_hip(golden, bf16, fixture):
    """P8 through the fused kernels: phc_running_norm (row-indexed, frozen source), FastLinear / FastLinearDD, phc_ppo_loss,
    phc_disc_bce, phc_weighted_sumsq (logit reg, weight decay, gradient penalty through the double backward), phc_adam_clip_step.
    fp32: every term at 2e-4 / 2e-3.  bf16 GEMMs (the benchmarked path): EVERY term as well on the two fixtures whose actions are draws of the
    fixture policy (`learner_step_policy_actions`, `learner_step_wide`): actor loss, KL and the actor's gradients included."""
    g = golden(fixture)
    agent = _agent_from_golden(g, device="cuda", bf16=bf16)
    agent.set_eval()
    amp_r = agent._calc_amp_rewards(torch.from_numpy(g["p6_amp_obs"]).cuda())
    tol = 5e-2 if bf16 else 1e-4
    np.testing.assert_allclose(amp_r["disc_rewards"].cpu().numpy(), g["p6_disc_rewards"], rtol=tol, atol=tol)
    info = _run_step(agent, g, "cuda", dataset_form=True)
    torch.cuda.synchronize()
    if bf16 and fixture == "learner_step":
        # GEMM inputs rounded to 8 mantissa bits.  THIS fixture's actions lie ~13 sigma from mu (sigma = exp(-2.9)), so neglogp ~ 760 and
        # a 1e-2 relative error of mu moves it by O(1): its actor terms are compared in fp32 only; the two other fixtures carry the bf16
        # statement for them
        worst = _check_step(agent, g, info, rtol_loss=8e-2, grad_rtol=0.6, grad_atol=1e-4, param_atol=4.1e-5, stats_rtol=1e-7,
                            skip=("actor_loss", "kl", "actor_mlp", "a2c_network.mu"))
        assert worst < 0.6
    elif bf16:
        # (the six-layer `im_big`-shaped actor on a 256-row batch: per-sample ratio errors of ~15 % -- 69 action dimensions x bf16 rounding of mu
        # against sigma = 0.055 -- do not average out over so few rows; measured worst element 0.29 of the parameter's gradient scale)
        tol = 0.5 if fixture == "learner_step_wide" else 8e-2
        worst = _check_step(agent, g, info, rtol_loss=8e-2, grad_rtol=tol, grad_atol=1e-4, param_atol=4.1e-5, stats_rtol=1e-7)
        print(f"{fixture}: worst relative gradient error with bf16 GEMMs {worst:.3e}")
        assert worst < tol
    else:   # (statistics: fp64 column sums in another order than torch's)
        worst = _check_step(agent, g, info, rtol_loss=2e-4, grad_rtol=2e-3, grad_atol=1e-6, param_atol=2e-6, stats_rtol=1e-7)
        assert worst < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["learner_step", "learner_step_policy_actions", "learner_step_wide"])
def test_split_bf16_actor_brings_the_actor_gradients_to_the_reference(golden, fixture):
    """Round 6, `+learning.params.config.actor_precision=split_bf16`: the actor's layers on fp32 activations with three bf16 MFMA GEMMs per product (operands cut into a bf16 head and tail).
    On the three whole-`calc_gradients` fixtures of the reference the ACTOR's terms -- actor loss, KL, bound loss and every gradient of `actor_mlp.*` / `mu.*` -- then agree with the reference's fp32 step to
    a few 1e-3 (bf16 GEMMs: 8e-2 .. 0.5, or not comparable at all on the first fixture), while critic and discriminator stay on the plain bf16 path and keep its tolerances."""
    g = golden(fixture)
    agent = _agent_from_golden(g, device="cuda", bf16=True, extra=["+learning.params.config.actor_precision=split_bf16"])
    assert agent._actor_split and agent.model.a2c_network.mu.split_precision and not agent.model.a2c_network.value.split_precision
    info = _run_step(agent, g, "cuda", dataset_form=True)
    torch.cuda.synchronize()
    for k in ("actor_loss", "kl", "b_loss"):
        atol = 2e-5 + (2e-3 * 0.1 * float(np.abs(g["in/advantages"]).mean()) if k == "actor_loss" else 0.0)
        np.testing.assert_allclose(float(info[k]), float(g["res/" + k]), rtol=2e-3, atol=atol, err_msg=k)
    params = dict(agent.model.named_parameters())
    worst = 0.0
    for n in (str(x) for x in g["param_names"]):
        if "grad/" + n not in g or not ("actor_mlp" in n or "a2c_network.mu" in n):
            continue
        ref = g["grad/" + n]
        scale = max(np.abs(ref).max(), 1e-12)
        err = float(np.abs(params[n].grad.detach().float().cpu().numpy() - ref).max() / scale)
        worst = max(worst, err)
    print(f"{fixture}: worst actor-gradient element error / parameter's gradient scale with the split-bf16 actor = {worst:.2e}")
    assert worst < 5e-3      # (VERDICT r5 item 7 asked for <= 5e-2; measured 1.5e-3 / 2.9e-5 / 1.0e-4)
    # the other networks: the bf16 tolerances of test_calc_gradients_equals_the_reference_agent_on_hip
    _check_step(agent, g, info, rtol_loss=8e-2, grad_rtol=0.6, grad_atol=1e-4, param_atol=4.1e-5, stats_rtol=1e-7, skip=("actor_loss", "kl", "actor_mlp", "a2c_network.mu"))


def test_bypass_mlp_loads_the_reference_class_state_dict(golden):
    """env.mlp_bypass (humanoid_im_mcp.py:31-38,83-84): a state dict laid out as the reference's own `phc.learning.mlp.MLP` writes it loads
    into BypassMLP (bare or under `model_state_dict`) and gives the reference class's actions (tests/golden/ref_bypass_mlp.npz: its keys,
    shapes, and its actions with seeded weights loaded, oracle/gen_golden_ref_fixtures.py)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    from gen_golden_ref_fixtures import seeded_state_dict
    from phc_amd.env.tasks.humanoid_im_mcp import load_bypass_mlp
    g = golden("ref_bypass_mlp")
    keys = [str(k) for k in g["keys"]]
    sd = seeded_state_dict(keys, g["shapes"], int(g["seed"]))
    x, want = torch.from_numpy(g["x"]), torch.from_numpy(g["actions"])
    for ck in (sd, {"model_state_dict": sd, "epoch": 3}):
        mine = load_bypass_mlp(ck, 934, 69)
        assert list(mine.state_dict()) == keys
        assert torch.equal(mine(x), want) and not any(p.requires_grad for p in mine.parameters())


# ------------------------------------------------------------------------------------------------------------------ P10 / f-2: the evaluation sweep
class _ScriptedLib:
    """Eval library stand-in of the fixture's script: U clips sorted by length, `num_envs` at a time from `start_idx` (wrapping)."""

    def __init__(self, g):
        self.g, self._num_unique_motions = g, int(g["U"])
        self._motion_data_keys = np.array([f"clip_{i:02d}" for i in range(self._num_unique_motions)])
        self.load(0)

    def load(self, start_idx):
        n = int(self.g["N"])
        self._curr_motion_ids = torch.remainder(torch.arange(n) + start_idx, self._num_unique_motions)
        self._steps = torch.from_numpy(self.g["script/num_steps"][self._curr_motion_ids.numpy()].astype(np.int32))

    def get_motion_num_steps(self, motion_ids=None):
        return self._steps


def _scripted_sweep(g, mode, tmp_path, dist=None):
    """im_eval.evaluate driven by the fixture's script through stand-ins for the task, the env and the agent."""
    import types
    from phc_amd.learning import im_eval
    from phc_amd.motion_lib import MotionLibBase
    U, n = int(g["U"]), int(g["N"])
    lib = _ScriptedLib(g)
    train = MotionLibBase.__new__(MotionLibBase)
    train._motion_data_keys, train._num_unique_motions, train._device = lib._motion_data_keys, U, torch.device("cpu")
    train._termination_history, train._sampling_prob = torch.zeros(U), torch.ones(U) / U
    state = dict(step=0, steps_per_batch={}, metric_args={})
    task = types.SimpleNamespace(_motion_lib=train, num_envs=n, start_idx=0, device=torch.device("cpu"), _termination_distances=torch.full((24,), 0.25),
                                 auto_pmcp=(mode == "hard"), auto_pmcp_soft=(mode == "soft"), get_eval_motion_lib=lambda: lib, reset=lambda: None)

    def begin():
        task.start_idx, state["step"] = 0, 0
        lib.load(0)

    def forward():
        task.start_idx += n
        state["step"] = 0
        lib.load(task.start_idx)
    task.begin_seq_motion_samples, task.forward_motion_samples = begin, forward

    def step(actions):
        b, s, ids = task.start_idx // n, state["step"], lib._curr_motion_ids.numpy()
        term = np.zeros(n, dtype=bool)
        for key_c, key_s in (("script/fail_clips", "script/fail_steps"), ("script/late_clips", "script/late_steps")):
            for c, st in zip(g[key_c], g[key_s]):
                term |= (ids == c) & (s == st)
        info = {"terminate": torch.from_numpy(term).long(), "mpjpe": torch.from_numpy(g["script/mpjpe"][b, s]),
                "body_pos": g["script/body_pos"][b, s], "body_pos_gt": g["script/body_gt"][b, s]}
        state["step"] += 1
        state["steps_per_batch"][b] = state["step"]
        return torch.zeros(n, 3), torch.zeros(n), torch.zeros(n, dtype=torch.long), info
    env = types.SimpleNamespace(reset=lambda: torch.zeros(n, 3), step=step)
    agent = types.SimpleNamespace(task=task, vec_env=env, set_eval=lambda: None, get_action_values=lambda obs: {"mus": torch.zeros(n, 2)},
                                  preprocess_actions=lambda a: a, epoch_num=7, rank=dist.get_rank() if dist is not None else 0, dist=dist)
    real = im_eval.compute_metrics_per_clip

    def recorder(pred_all, gt_all):   # (called once per batch with the batch's own clips)
        state["metric_args"][task.start_idx // n] = ([np.asarray(p) for p in pred_all], [np.asarray(x) for x in gt_all])
        return real(pred_all, gt_all)
    im_eval.compute_metrics_per_clip = recorder
    try:
        eval_info, failed = im_eval.evaluate(agent, output_dir=str(tmp_path), log=None)
    finally:
        im_eval.compute_metrics_per_clip = real
    return eval_info, failed, state, train


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_eval_sweep_bookkeeping_equals_the_reference_post_step_eval(golden, tmp_path, mode):
    """P10 / f-2: `im_eval.evaluate` against `IMAmpAgent._post_step_eval` + `update_training_data` of the reference (im_amp.py:126-132,244-363)
    run on a `__new__`-made agent (oracle/gen_golden_eval.py): same batch boundaries (env steps per batch, incl. the wrapping last batch), same
    failures (a terminate flag at / after a clip's last frame is not one), same success rate, same frames of the same clips handed to the metrics,
    same re-weighted sampler, same `failed_*.pkl` schema."""
    import joblib
    g = golden("eval_sweep")
    eval_info, failed, state, train = _scripted_sweep(g, mode, tmp_path)
    assert [state["steps_per_batch"][b] for b in sorted(state["steps_per_batch"])] == list(g["steps_per_batch"])
    assert list(failed) == list(g["failed_keys"])
    assert abs(eval_info["eval/success_rate"] - float(g["success_rate"])) < 1e-12
    pred_all = [p for b in sorted(state["metric_args"]) for p in state["metric_args"][b][0]]      # per-batch calls, in clip order
    gt_all = [x for b in sorted(state["metric_args"]) for x in state["metric_args"][b][1]]
    assert [len(p) for p in pred_all] == list(g["metric_frames_all"])
    np.testing.assert_allclose([float(np.sum(p, dtype=np.float64)) for p in pred_all], g["metric_sum_all"], rtol=1e-12)
    np.testing.assert_allclose([float(np.sum(p, dtype=np.float64)) for p in gt_all], g["metric_gt_sum_all"], rtol=1e-12)
    ok = [k not in set(g["failed_keys"]) for k in (f"clip_{i:02d}" for i in range(int(g["U"])))]
    assert [len(p) for p, s_ in zip(pred_all, ok) if s_] == list(g["metric_frames_succ"])
    # the recorder of the generator returned mean |pred - gt| per clip in metres; ours reports millimetres
    np.testing.assert_allclose(eval_info["eval/mpjpe_all"], float(g["eval_mpjpe_all"]) * 1000, rtol=1e-5)
    np.testing.assert_allclose(eval_info["eval/mpjpe_succ"], float(g["eval_mpjpe_succ"]) * 1000, rtol=1e-5)
    np.testing.assert_allclose(train._sampling_prob.numpy(), g[f"{mode}/sampling_prob"], rtol=1e-7)
    np.testing.assert_allclose(train._termination_history.numpy(), g[f"{mode}/termination_history"], rtol=0)
    dumped = joblib.load(str(tmp_path / "failed_0000000007.pkl"))
    assert sorted(dumped) == ["failed_keys", "termination_history"] and list(dumped["failed_keys"]) == list(g["failed_keys"])


def _sharded_eval_worker(rank, world, port, q, gpath, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = dict(np.load(gpath, allow_pickle=False))
    eval_info, failed, state, train = _scripted_sweep(g, "soft", tmp, dist=dist)
    q.put((rank, eval_info, [str(k) for k in failed], sorted(state["steps_per_batch"]), train._sampling_prob.numpy().tolist()))
    dist.destroy_process_group()


def test_eval_sweep_sharded_over_two_gloo_ranks_equals_the_single_rank_sweep(golden, tmp_path):
    """SURVEY.md 8e / VERDICT r2 weak #9: with two ranks the batches of the sweep are dealt round-robin (rank 0: batches 0, 2; rank 1: batch 1), ONE
    all-reduce(sum) merges the per-clip failed flags and metrics, and BOTH ranks end with the single-process result -- the reference's success rate,
    failed keys and re-weighted sampler (fixture of the test above) -- while each evaluated only its own batches."""
    import multiprocessing as mp
    g = golden("eval_sweep")
    single, _, _, _ = _scripted_sweep(g, "soft", tmp_path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 137) % 500)
    gpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_sweep.npz")
    procs = [ctx.Process(target=_sharded_eval_worker, args=(r, 2, port, q, gpath, str(tmp_path / f"r{r}"))) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=240)
        res[r[0]] = r
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][3] == [0, 2] and res[1][3] == [1]                       # who evaluated which batches
    for r in (0, 1):
        assert res[r][2] == [str(k) for k in g["failed_keys"]]
        for k, v in single.items():
            assert abs(res[r][1][k] - v) <= 1e-9 * max(1.0, abs(v)), (r, k)
        np.testing.assert_allclose(res[r][4], g["soft/sampling_prob"], rtol=1e-7)
    assert os.path.exists(str(tmp_path / "r0" / "failed_0000000007.pkl")) and not os.path.exists(str(tmp_path / "r1" / "failed_0000000007.pkl"))
