"""P4-P10: the PPO + AMP learner (`im_amp`), PyTorch-ROCm on the same device as the env.

Follows the reference's agent chain `IMAmpAgent -> AMPAgent -> CommonAgent` (phc/learning/im_amp.py,
amp_agent.py, common_agent.py; base classes from rl-games 1.1.4 are not vendored there -- their behaviour is
restated from PHC's call sites):

  train_epoch (amp_agent.py:413-504)
    play_steps (:309-397)           rollout of `horizon_length` steps, 3 MLP forwards per step
    _calc_amp_rewards (:859-878)    -log(max(1-sigmoid(D),1e-4)) * disc_reward_scale
    _combine_rewards (:848-853)     task_reward_w * r_task + disc_reward_w * r_disc
    discount_values (common_agent.py:493-505)   GAE -> `phc_gae` HIP kernel
    prepare_dataset (:399-411, common_agent.py:357-398)  advantage / value normalisation
    calc_gradients (:554-688)       PPO clip + critic + bound + discriminator (BCE, logit reg, grad penalty, weight decay)
    Adam (lr 2e-5), clip_grad_norm_(50)

MI355X-first differences (results-preserving):
  * GEMMs run in bf16 on MFMA under torch.autocast; parameters, Adam state and all losses stay fp32;
    running statistics stay fp64 (running_mean_std.py).
  * done envs are reset on the device from `reset_buf` (`task.reset_done()`), no `.nonzero()` host sync per step
    (set `faithful_reset=True` to get the reference's `env.reset(done_indices)` call sequence and RNG stream).
  * data parallelism: one process per GPU, envs sharded, ONE all-reduce (mean) of a single flat fp32 gradient
    bucket per optimizer step over RCCL (`FlatGradBucket`); it replaces horovod's `optimizer.synchronize()`
    (amp_agent.py:667-668).  Running-stat moments are averaged once per epoch (`hvd.sync_stats`).
  * on the device everything of the update that is not a GEMM runs as HIP kernels (csrc/phc_learn.hip via learning/fast_ops.py,
    DESIGN.md 4.3): observation normalisers incl. the minibatch gather, actor / critic and discriminator losses with their
    gradients, bias and split-K weight gradients of the layers, clip + Adam on the flat parameter, the rollout's sampling step;
    optionally (`hip_graph`) a step is replayed from captured hipGraphs (update_graph.py).  The torch expressions in
    this file (`_ppo_loss_torch`, `_disc_loss`, RunningMeanStd's CPU branch) remain the CPU path and the definition those kernels
    are tested against.

`IMAmpAgent` owns the reference's agent surface, the dataset and its minibatch draw, checkpoints, ONE definition of the rollout step -- `_rollout_step` on the device
(reset rule, `_rollout_policy`, env step, AMP row, `_rollout_after`), `_rollout_step_torch` on CPU tensors; `rollout_graph.CapturedRollout` captures those same methods,
per segment or as whole steps, and owns the graphs, their pool and the rule that drops them -- and ONE definition of the optimizer step: `_fwd_bwd` dispatches to
`_device_step` (`_policy_pass` + `_disc_pass`, on two streams or one) or to the torch path; `update_graph.CapturedUpdate` captures those same methods.  `__init__` assigns every attribute.
"""
import copy
import os
import sys
import time
import warnings

import numpy as np
import torch
from torch import nn

from .. import _lib as L
from .network import A2CMCPNetwork, A2CNetwork, A2CPNNNetwork, ModelAMPContinuous, policy_kl
from .replay_buffer import ReplayBuffer
from .fast_ops import (FastLinear, adam_clip_step, deferred_colsums, disc_bce, input_grad_only, param_grad_only, policy_sample, ppo_loss, register_lane, rows_with_grad,
                       set_wgrad, weighted_sumsq)
from .running_mean_std import RunningMeanStd
from .rollout_graph import CapturedRollout, call_segment
from .update_graph import CapturedUpdate


def swap_and_flatten01(arr):
    """rl_games a2c_common.swap_and_flatten01: [T, N, ...] -> [N*T, ...] (env-major)."""
    if arr is None:
        return arr
    s = arr.size()
    return arr.transpose(0, 1).reshape(s[0] * s[1], *s[2:])


def discount_values(mb_fdones, mb_values, mb_rewards, mb_next_values, gamma, tau):
    """P5 GAE (common_agent.py:493-505).  [T,N,1] tensors.  On the HIP device this is one `phc_gae` launch;
    for CPU tensors (unit tests of the learner logic under gloo) the same recurrence runs as torch ops."""
    T, N = mb_rewards.shape[0], mb_rewards.shape[1]
    advs = torch.empty_like(mb_rewards)
    if mb_rewards.is_cuda:
        fd = mb_fdones.reshape(T, N).float().contiguous()
        v, r, nv = (x.reshape(T, N).float().contiguous() for x in (mb_values, mb_rewards, mb_next_values))
        out = advs.view(T, N)
        L.check(L.load().phc_gae(T, N, fd.data_ptr(), v.data_ptr(), r.data_ptr(), nv.data_ptr(), float(gamma), float(tau), out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream), "phc_gae")
        return advs
    last = 0
    for t in reversed(range(T)):
        not_done = (1.0 - mb_fdones[t].float()).reshape(N, 1)
        delta = mb_rewards[t] + gamma * mb_next_values[t] - mb_values[t]
        last = delta + gamma * tau * not_done * last
        advs[t] = last
    return advs


class _marker:
    """roctx range (shows up in `rocprofv3 --marker-trace`) around the two phases of an epoch; a no-op off the device."""

    usable = True

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = False
        if _marker.usable and torch.cuda.is_available():
            try:
                torch.cuda.nvtx.range_push(self.name)
                self.on = True
            except Exception:   # no roctx in this build: markers off, training unaffected
                _marker.usable = False

    def __exit__(self, *a):
        if self.on:
            torch.cuda.nvtx.range_pop()


# K-padded weights are strided views with strided gradients of the SAME layout: autograd's "gradient layout contract" note does not apply
warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")


VERIFIED_GRAPH_STACKS = (("2.10", "7."),)   # (torch.__version__ prefix, torch.version.hip prefix)
_graph_default_warned = [False]


def graph_default_on():
    """Is the captured (hipGraph) update the default on this software stack?  See IMAmpAgent.__init__."""
    hip = getattr(torch.version, "hip", None) or ""
    ok = any(torch.__version__.startswith(a) and hip.startswith(b) for a, b in VERIFIED_GRAPH_STACKS)
    if not ok and torch.cuda.is_available() and not _graph_default_warned[0]:
        _graph_default_warned[0] = True
        print(f"[phc_amd] torch {torch.__version__} / HIP {hip or None} is not a stack the captured update has been verified on: hipGraphs are OFF by default "
              f"(eager launches); +learning.params.config.hip_graph=True turns them on", file=sys.stderr)
    return ok


class FlatGradBucket:
    """All trainable parameters AND their gradients as views of two flat fp32 buffers.

    * one all-reduce per optimizer step (22.1 MB for `im`, 78 MB for `im_big`): over the 7 point-to-point xGMI links of
      an MI355X node RCCL moves that in well under a millisecond, so there is nothing to overlap with and one bucket is
      the right size;
    * gradient clipping is one norm + one scale of the flat gradient (`clip_grad_norm_` semantics, max-norm 50);
    * Adam updates ONE tensor (the flat parameter) instead of 22 -- three launches instead of a foreach over all of them.
    Modules keep seeing their own `weight` / `bias` (views), so state_dicts are unchanged."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        # K-padded weights (round 2): a first-layer weight [N, K] whose K is no GEMM-friendly multiple (obs 934, AMP obs 1960) is STORED with
        # rows Kp = `_pad_cols` apart (network.build_mlp tags it); the module's parameter is the strided view [:, :K] -- shapes, state dicts
        # and checkpoints are unchanged -- while the GEMMs read the padded bf16 copy against K-padded inputs (pad = 0: same numbers; the
        # first-layer forward / weight-gradient GEMMs run 20-30 % faster, scripts/probes/gemm_pad_probe.py).  The pad elements start at zero and only
        # ever see zero gradients.
        def alloc(p):
            kp = int(getattr(p, "_pad_cols", 0))
            return p.shape[0] * kp if (dev.type == "cuda" and p.dim() == 2 and kp > p.shape[1]) else p.numel()
        self.segments = []
        n = 0
        for p in self.params:
            n = (n + 3) // 4 * 4          # segments start 16-byte aligned (vector loads / stores of the gradient kernels); the gaps stay zero
            self.segments.append((n, alloc(p)))
            n += alloc(p)
        self.flat_param = torch.zeros(n, device=dev, dtype=torch.float32)
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        for p, (o, k) in zip(self.params, self.segments):
            if k != p.numel():
                kp = k // p.shape[0]
                pv, gv = self.flat_param[o:o + k].view(p.shape[0], kp), self.flat[o:o + k].view(p.shape[0], kp)
                pv[:, :p.shape[1]].copy_(p.data)
                p._padded, p._grad_padded = pv, gv
                p.data, p.grad = pv[:, :p.shape[1]], gv[:, :p.shape[1]]
            else:
                self.flat_param[o:o + k].copy_(p.data.reshape(-1))
                p.data = self.flat_param[o:o + k].view_as(p)
                p.grad = self.flat[o:o + k].view_as(p)
        self.flat_param.grad = self.flat
        self.gen = 0   # bumped by zero(): lets a layer's backward store the first gradient of a step directly (fast_ops._first_write)
        for p in self.params:
            p._bucket = self
        # bf16 copy of the flat parameter for the GEMMs of the update phase: refreshed on entering shadow_scope(), then kept current
        # by the optimizer kernel; `_shadow_live` is the flag the layers look at (fast_ops.FastLinear)
        self.shadow, self._shadow_live = None, [False]
        if dev.type == "cuda":
            self.shadow = torch.zeros(n, device=dev, dtype=torch.bfloat16)
            for p, (o, k) in zip(self.params, self.segments):   # (a K-padded weight's bf16 copy is the PADDED matrix)
                sh = self.shadow[o:o + k]
                p._bf16_shadow, p._shadow_live = (sh.view(p.shape[0], k // p.shape[0]) if k != p.numel() else sh.view_as(p)), self._shadow_live

    def shadow_scope(self):
        """Context of the minibatch loop: inside it only the optimizer kernel changes the parameters, so their bf16 copies stay valid."""
        bucket = self

        class _Scope:
            def __enter__(self_):
                if bucket.shadow is not None:
                    bucket.shadow.copy_(bucket.flat_param)
                    bucket._shadow_live[0] = True

            def __exit__(self_, *a):
                bucket._shadow_live[0] = False
        return _Scope()

    def param_view(self, flat, i):
        """Parameter i's slice of a flat per-element tensor (optimizer moments) in the parameter's own shape."""
        p, (o, k) = self.params[i], self.segments[i]
        return flat[o:o + k].view(p.shape[0], k // p.shape[0])[:, :p.shape[1]] if k != p.numel() else flat[o:o + k].view_as(p)

    def spans_of(self, params):
        """([(lo, hi)] of the flat gradient that holds `params`, [(lo, hi)] of everything else): `params` must be consecutive in the bucket."""
        ids = {id(p) for p in params}
        idx = [i for i, p in enumerate(self.params) if id(p) in ids]
        if not idx or idx != list(range(idx[0], idx[-1] + 1)):
            raise ValueError("parameters are not one consecutive run of the gradient bucket")
        lo, hi, n = self.segments[idx[0]][0], self.segments[idx[-1]][0] + self.segments[idx[-1]][1], self.flat.numel()
        return [(lo, hi)], [(a, b) for a, b in ((0, lo), (hi, n)) if b > a]

    def zero(self, decay=None, spans=None):
        """`decay` [(parameter, c)]: start that parameter's gradient at c * parameter (an L2 term's gradient written in place instead of
        being handed to autograd as a tensor to add).  `spans`: only these ranges of the flat gradient (a pass that owns a part of the
        parameters: the other pass zeroes its own, possibly at the same time on another stream)."""
        if spans is None:
            self.flat.zero_()
        else:
            for lo, hi in spans:
                self.flat[lo:hi].zero_()
        self.gen += 1
        for p, c in decay or ():
            torch.mul(p.data, c, out=p.grad)
            p._grad_gen = self.gen

    def all_reduce_mean(self, dist, force=False, timing=None, spans=None):
        """The path's one collective.  `force`: issue it also in a one-rank group (exercises RCCL + the captured update on a 1-GPU box);
        `timing`: a list that receives (start, end) event pairs on the launch stream (bench.py: per-all-reduce time); `spans` [(lo, hi)]: only these ranges of
        the flat gradient, one all-reduce each (`split_allreduce`: the discriminator's part on its stream while the policy pass still runs).  -> number issued."""
        if dist is not None and dist.is_initialized() and (dist.get_world_size() > 1 or force):
            ev = None
            if timing is not None and self.flat.is_cuda and len(timing) < 4096:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            views = [self.flat] if spans is None else [self.flat[lo:hi] for lo, hi in spans]
            for v in views:
                dist.all_reduce(v, op=dist.ReduceOp.SUM)
                if dist.get_world_size() > 1:
                    v.div_(dist.get_world_size())
            if ev is not None:
                ev[1].record()
                timing.append(ev)
            return len(views)
        return 0

    def clip_grad_norm_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_ on the flat view: same total norm, same clip coefficient (clamped to 1)."""
        total = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        return total


class IMAmpAgent:
    def __init__(self, vec_env, cfg, dist=None, faithful_reset=False, bf16=True):
        self.vec_env = vec_env
        self.task = vec_env.task
        self.dist = dist
        self.rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
        self.multi_gpu = self.world > 1
        self.faithful_reset = faithful_reset
        params = cfg["learning"]["params"]
        c = params["config"]
        # `force_collectives`: run the gradient all-reduce also in a one-rank process group (tests: RCCL next to the captured update on one GPU)
        self._force_collectives = bool(c.get("force_collectives", False))
        self._reduces = self.multi_gpu or (self._force_collectives and dist is not None)   # is there a gradient all-reduce between backward and optimizer?
        self.allreduce_timing = None   # bench.py sets a list: (start, end) events of every gradient all-reduce
        self._trace = [] if c.get("trace_minibatches", False) else None
        for k in ("debug_actor_steps", "debug_critic_steps", "debug_disc_steps", "debug_reset_at_rollout_start"):
            if k in c:   # (the knobs of the round-6 seed study, DESIGN.md section 10: removed with their code, never ignored silently)
                raise ValueError(f"learning.params.config.{k} is set, but that diagnostic no longer exists (profiles/r06_multi_clip/README.md names the last commit that has it)")
        self.num_collectives = 0       # gradient all-reduces issued so far
        self.config = c
        self.device = self.task.device if hasattr(self.task, "device") else "cpu"
        self.bf16 = bf16 and str(self.device).startswith("cuda")
        self.num_actors = vec_env.num_envs
        self.horizon_length = c["horizon_length"]
        # rl_games' A2CBase.preprocess_actions (a dependency of the reference, not vendored; common_agent.py:47 reads the switch): the env gets
        # the sampled action clamped to the action space [-1, 1]; the experience buffer keeps the unclamped sample
        self.clip_actions = bool(c.get("clip_actions", True))
        self.batch_size = self.horizon_length * self.num_actors
        self.minibatch_size = min(c["minibatch_size"], self.batch_size)
        assert self.batch_size % self.minibatch_size == 0
        self.num_minibatches = self.batch_size // self.minibatch_size
        self.mini_epochs_num = c["mini_epochs"]
        # (Rounds 5 / 6, profiles/r06_multi_clip/README.md: on the 64-clip synthetic library every run first settles on a ~13-step plateau -- lean into the first reference
        # frames, fall -- and leaves it at a SEED-dependent epoch; more optimizer steps per rollout make the escape later / rarer, they do not forbid it.  The shipped
        # 3072 envs x 36 steps learn the library for most seeds; no notice is printed any more.)
        self.gamma, self.tau = c["gamma"], c["tau"]
        self.e_clip, self.critic_coef, self.entropy_coef = c["e_clip"], c["critic_coef"], c["entropy_coef"]
        self.bounds_loss_coef = c.get("bounds_loss_coef", None)
        self.clip_value = c["clip_value"]
        self.truncate_grads, self.grad_norm = c["truncate_grads"], c["grad_norm"]
        self.normalize_input, self.normalize_value = c["normalize_input"], c["normalize_value"]
        self.normalize_advantage = c["normalize_advantage"]
        self.last_lr = float(c["learning_rate"])
        self.reward_scale = c.get("reward_shaper", {}).get("scale_value", 1)
        # AMP (_load_config_params amp_agent.py:690-707)
        self._task_reward_w, self._disc_reward_w = c["task_reward_w"], c["disc_reward_w"]
        self._amp_batch_size = int(c["amp_batch_size"])
        self._amp_minibatch_size = min(int(c["amp_minibatch_size"]), self.minibatch_size)
        self._disc_coef, self._disc_logit_reg = c["disc_coef"], c["disc_logit_reg"]
        self._disc_grad_penalty, self._disc_weight_decay = c["disc_grad_penalty"], c["disc_weight_decay"]
        self._disc_reward_scale = c["disc_reward_scale"]
        self._normalize_amp_input = c.get("normalize_amp_input", True)
        self.temp_running_mean = getattr(self.task, "temp_running_mean", True)

        obs_dim = vec_env.num_obs
        amp_dim = self.task.get_num_amp_obs()
        self.obs_shape, self.actions_num = (obs_dim,), vec_env.num_actions
        net_name = params["network"].get("name", "amp")
        if net_name == "amp":
            net = A2CNetwork(params["network"], self.actions_num, (obs_dim,), (amp_dim,))
        elif net_name == "amp_pnn":  # run_hydra.py:259: model_builder.register_network('amp_pnn', ...)
            net = A2CPNNNetwork(params["network"], self.actions_num, (obs_dim,), (amp_dim,), self.task.get_task_obs_size_detail())
        elif net_name == "amp_mcp":  # run_hydra.py:258
            net = A2CMCPNetwork(params["network"], self.actions_num, (obs_dim,), (amp_dim,), self.task.get_task_obs_size_detail())
        else:
            raise NotImplementedError(f"network '{net_name}' is not built")
        self.model = ModelAMPContinuous(net).to(self.device)
        if self.multi_gpu:  # hvd.setup_algo: broadcast rank 0's initial parameters (common_agent.py:112-113)
            for p in self.model.parameters():
                dist.broadcast(p.data, src=0)
        self.running_mean_std = RunningMeanStd((obs_dim,)).to(self.device) if self.normalize_input else None
        self.value_mean_std = RunningMeanStd((1,)).to(self.device) if self.normalize_value else None
        self._amp_input_mean_std = RunningMeanStd((amp_dim,)).to(self.device) if self._normalize_amp_input else None
        self.running_mean_std_temp = None
        # `actor_precision=split_bf16` (round 6): the actor's layers work on fp32 activations with three bf16 GEMMs per product (fast_ops._SplitLinearFn)
        # -- an option between the bf16 path (actor-gradient parity 8e-2 on the small fixtures) and fp32 GEMMs for everything (4.8 x the update)
        self._actor_split = str(c.get("actor_precision", "bf16")) == "split_bf16" and self.bf16
        if str(c.get("actor_precision", "bf16")) not in ("bf16", "split_bf16"):
            raise ValueError(f"learning.params.config.actor_precision must be bf16 or split_bf16, not {c.get('actor_precision')!r}")
        if self._actor_split:
            if net_name != "amp" or not self.normalize_input or not self.temp_running_mean:
                raise NotImplementedError("actor_precision=split_bf16 is built for the plain `amp` network with normalize_input and temp_running_mean")
            for m in list(net.actor_mlp.modules()) + [net.mu]:
                if isinstance(m, FastLinear):
                    m.split_precision = True
                    m.weight._pad_cols = 0      # (the split layers read the fp32 master weights: no K-padded bf16 copy)
        # `wgrad=native`: the weight / bias gradients of the bf16 device layers by the project's own matrix-core kernel (fast_ops.set_wgrad, csrc/phc_gemm.hip)
        # instead of the library's batched GEMM between two reduction passes; opt-in, `library` is the default.  Inert off the device.
        self._wgrad = str(c.get("wgrad", "library"))
        set_wgrad(self.model, self._wgrad)
        self.grads = FlatGradBucket(self.model.parameters())
        # the fused discriminator path: its loss runs as kernels (`_disc_loss_fused`) and the whole optimizer step is `_device_step`
        self._fused_disc = self.grads.flat.is_cuda and self._disc_grad_penalty > 0 and bool(self._normalize_amp_input)
        # K-padded first layers: width of the padded input buffers the normalisers write (0: no padding; see FlatGradBucket)
        padded_k = {p.shape[1]: p._padded.shape[1] for p in self.grads.params if getattr(p, "_padded", None) is not None}
        self._obs_pad_cols = padded_k.get(obs_dim, 0)
        self._amp_pad_cols = padded_k.get(amp_dim, 0)
        # ON by default on the device since round 4 (`+learning.params.config.hip_graph=False` turns it off): a user of `python -m phc_amd.run` gets the
        # update the bench line quotes.  Known hazard (scripts/probes/graph_repro2.py): if the caller keeps an autograd-tracked copy of a
        # parameter alive (`w0 = p.clone()` instead of `p.detach().clone()`), that parameter's AccumulateGrad node lives on the stream it was
        # created on; the captured backward then has to hand the gradient to a stream that is not capturing and `hipStreamEndCapture` segfaults on
        # ROCm 7.2 instead of raising -- `update_graph.stale_grad_accumulators()` detects exactly that before capturing and the update falls back to eager
        # launches, as it does when a capture raises or the minibatch is small (< 2048 rows: not launch-bound).
        # the known failure mode of a bad capture on this stack is a crash, not an exception, so the DEFAULT is on only for the (torch, HIP)
        # pairs the -m gpu suite has run the captured update on (VERIFIED_GRAPH_STACKS: tests/test_env_gpu.py::test_update_graph_equals_eager_launches,
        # ::test_captured_update_trains_the_other_network_and_observation_variants incl. PNN / im_big / im_pnn_big); an explicit
        # `learning.params.config.hip_graph=True|False` always wins, `PHC_NO_GRAPH=1` / `PHC_NO_BRANCH_STREAMS=1` switch off at run time
        self._use_graph = bool(c["hip_graph"]) if "hip_graph" in c else graph_default_on()
        # The discriminator's share of an optimizer step (three input normalisers, forward, loss terms, the gradient penalty's double backward,
        # backward) shares nothing with actor + critic but the optimizer launches at the end: two chains of ~256-workgroup GEMMs and 5 us
        # finishing launches.  On the device the discriminator pass runs on its own HIP stream (_device_step); captured, it is its OWN linear
        # hipGraph replayed on that stream next to the policy graph (update_graph.CapturedUpdate).
        self._use_branches = bool(c.get("branch_streams", True)) and not os.environ.get("PHC_NO_BRANCH_STREAMS")
        # VERDICT r5 item 6b (UNMEASURED on multi-GPU hardware -- no node was ever available to this project; exercised by two-rank gloo and one-rank RCCL tests): the
        # gradient bucket cut at the policy / discriminator boundary, the discriminator's all-reduce issued on its stream as soon as its pass is done.  Off by default:
        # the shipped path is ONE all-reduce per optimizer step (north star); for `im` the discriminator holds 2.5 M of the 5.8 M gradient elements.
        self._split_allreduce = bool(c.get("split_allreduce", False))
        self._branches = None                              # the discriminator's stream, made by the first two-stream step (_branch_streams) ...
        self._disc_spans = self._policy_spans = None       # ... with the two passes' ranges of the flat gradient
        self._update = CapturedUpdate(self)                # the optimizer steps of an epoch as replayed hipGraphs (update_graph.py)
        self._graph_failed = False                         # the FIRST capture raised: eager launches from then on, rollout included
        # one flat fp32 parameter; on the device clip + step are two HIP launches over it (fast_ops.adam_clip_step) and this object
        # only holds the state (checkpoint format unchanged)
        self.optimizer = torch.optim.Adam([self.grads.flat_param], self.last_lr, eps=1e-08, weight_decay=c.get("weight_decay", 0.0))

        T, N, dev = self.horizon_length, self.num_actors, self.device
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.exp = {"obses": f(T, N, obs_dim), "next_obses": f(T, N, obs_dim), "rewards": f(T, N, 1), "values": f(T, N, 1),
                    "next_values": f(T, N, 1), "neglogpacs": f(T, N), "dones": torch.zeros(T, N, device=dev, dtype=torch.uint8),
                    "actions": f(T, N, self.actions_num), "mus": f(T, N, self.actions_num), "sigmas": f(T, N, self.actions_num),
                    "amp_obs": f(T, N, amp_dim)}
        self._amp_obs_demo_buffer = ReplayBuffer(int(c["amp_obs_demo_buffer_size"]), dev)
        self._amp_replay_buffer = ReplayBuffer(int(c["amp_replay_buffer_size"]), dev)
        self._amp_replay_keep_prob = c["amp_replay_keep_prob"]
        self._idx_buf = torch.randperm(self.batch_size, device=dev)
        self.current_rewards = f(N, 1)
        self.current_lengths = f(N)
        self.epoch_num = 0
        self.frame = 0
        self.obs = None
        self.dones = torch.zeros(N, device=dev, dtype=torch.long)
        self.dataset = None                # prepare_dataset()
        # created on first use; a captured graph keeps their addresses, so each is made once and kept
        self._pad_bufs = {}                # (use, rows, cols) -> zero-padded bf16 input buffer (_pad_buf)
        self._unit_cot = {}                # (dtype, device) -> the constant cotangent 1 of a loss root (_unit_cotangent)
        self._raw = None                   # the step's scalars as the fused kernels write them (_raw_buffer)
        self._ones_key = self._ones = None           # cotangent that selects the demo rows (_demo_row_mask)
        self._terminated_flags = self._terminated_mask = self._env_actions = None   # rollout scratch (play_steps)
        self._reward_raw_acc = None        # sum of the rollout's raw reward terms: made by the FIRST rollout, eagerly (whole-step graphs need it to exist)
        self._rollout = CapturedRollout(self)              # the rollout steps as replayed hipGraphs (rollout_graph.py)
        self._summary_file = self._summary_writer = None      # _log_train_info

    # ------------------------------------------------------------------ modes (rl_games set_eval / set_train + amp_agent.py:63-82)
    def _norms(self):
        return [m for m in (self.running_mean_std, self.value_mean_std, self._amp_input_mean_std) if m is not None]

    def set_eval(self):
        self.model.eval()
        for m in self._norms():
            m.eval()

    def set_train(self):
        self.model.train()
        for m in self._norms():
            m.train()

    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16)

    # ------------------------------------------------------------------ observation pre-processing (amp_agent.py:535-552)
    def _preproc_obs(self, obs_batch, use_temp=False, row_index=None):
        if not self.normalize_input:
            return obs_batch if row_index is None else obs_batch[row_index]
        # bf16 runs: the normaliser writes the bf16 tensor the GEMMs read (the same values autocast's cast would produce)
        dt = torch.bfloat16 if self.bf16 else None
        out = None
        if obs_batch.is_cuda and self.bf16 and self._obs_pad_cols > obs_batch.shape[1]:
            # K-padded first layers (FlatGradBucket): the normaliser writes the left columns of a persistent [rows, Kp] buffer (pad = 0)
            rows = obs_batch.shape[0] if row_index is None else row_index.numel()
            buf = self._pad_buf("obs", rows, self._obs_pad_cols)
            out = buf[:, :obs_batch.shape[1]]
        if use_temp:  # statistics keep updating, the frozen copy provides the values (amp_agent.py:527-532)
            y = self.running_mean_std(obs_batch, norm_from=self.running_mean_std_temp, out_dtype=dt, row_index=row_index, out=out)
        else:
            y = self.running_mean_std(obs_batch, out_dtype=dt, row_index=row_index, out=out)
        return y if out is None else buf

    def _actor_obs(self, obs_batch, use_temp=False, row_index=None):
        """The ACTOR's input in split-precision mode: the normalised observation in fp32, from the same statistics the bf16 tensor of `_preproc_obs` comes from, WITHOUT
        folding the batch into them again (the bf16 call of the same step does that once)."""
        src = self.running_mean_std_temp if use_temp else self.running_mean_std
        was_training = src.training
        src.eval()
        try:
            return src(obs_batch, out_dtype=torch.float32, row_index=row_index)
        finally:
            src.train(was_training)

    def _pad_buf(self, name, rows, cols):
        """Persistent zero-initialised bf16 [rows, cols] buffers (one per use and row count: a captured graph keeps their address)."""
        key = (name, rows, cols)
        if key not in self._pad_bufs:
            self._pad_bufs[key] = torch.zeros((rows, cols), dtype=torch.bfloat16, device=self.device)
        return self._pad_bufs[key]

    def _preproc_amp_obs(self, amp_obs, row_index=None):
        if not self._normalize_amp_input:
            return amp_obs if row_index is None else amp_obs[row_index]
        return self._amp_input_mean_std(amp_obs, out_dtype=torch.bfloat16 if self.bf16 else None, row_index=row_index)

    # ------------------------------------------------------------------ rollout (amp_agent.py:309-397)
    def preprocess_actions(self, actions, out=None):
        """What the env is stepped with (rl_games a2c_common.preprocess_actions; players: im_amp.py:68-74): clamp to [-1, 1] and rescale to the
        action space -- the identity here, VecTask's space is Box(-1, 1)."""
        if not self.clip_actions:
            return actions
        return torch.clamp(actions, -1.0, 1.0, out=out)

    def get_action_values(self, obs):
        processed = self._preproc_obs(obs)
        with torch.no_grad(), self._autocast():
            res = self.model({"is_train": False, "prev_actions": None, "obs": processed, "obs_actor": self._actor_obs(obs) if self._actor_split else None})
        if self.normalize_value:
            res["values"] = self.value_mean_std(res["values"], True)
        return res

    def _eval_critic(self, obs):
        processed = self._preproc_obs(obs)
        with torch.no_grad(), self._autocast():
            value = self.model.a2c_network.eval_critic(processed).float()
        if self.normalize_value:
            value = self.value_mean_std(value, True)
        return value

    def env_reset(self, env_ids=None):
        return self.vec_env.reset(env_ids)

    # ---- one rollout step: the reset rule, the two policy segments, the bookkeeping, and one body per family of regimes ------------------------------
    # (device: eager launches, segment graphs or whole-step graphs -- rollout_graph.py says which and owns the graphs; torch: CPU tensors)
    _roll_graphs = property(lambda self: self._rollout.graphs)            # read by tests and probes
    _roll_pool = property(lambda self: self._rollout.pool)
    _roll_generation = property(lambda self: self._rollout.generation)

    def _rollout_reset(self, n):
        """The reset in front of step n and the step's observation -> self.obs."""
        task = self.task
        # The reference starts every rollout with `done_indices = []` (amp_agent.py:313): the envs that finished on the LAST step of the previous
        # rollout are not reset at step 0 -- they run one more step, are flagged again by that step's `_compute_reset` (their clip is still over /
        # they are still down) and are reset at step 1.  Kept: one in `horizon_length` episode ends carries that extra transition in the reference's
        # data too (tests/test_learner_epoch.py pins it).
        if self.faithful_reset or not hasattr(task, "reset_done"):   # (a task without the device-side reset gets the reference's index list)
            self.obs = self.env_reset(self.dones.nonzero(as_tuple=False)[:, 0] if n > 0 else [])
            return
        if n > 0:
            task.reset_done()
        clip = self.vec_env.clip_obs   # finite: clamp straight into the experience buffer row
        self.obs = torch.clamp(task.obs_buf, -clip, clip, out=self.exp["obses"][n]) if np.isfinite(clip) else task.obs_buf

    def _rollout_policy(self, n):
        """(A) observation row, policy + value heads, sampling -> row n of the experience buffer."""
        e, net = self.exp, self.model.a2c_network
        if self.obs.data_ptr() != e["obses"][n].data_ptr():
            e["obses"][n].copy_(self.obs)
        processed = self._preproc_obs(self.obs)
        with self._autocast():
            mu, logstd = net.eval_actor(self._actor_obs(self.obs) if self._actor_split else processed)
            value = net.eval_critic(processed)
        if self._actor_split:
            value = value.float()       # (one dtype flag for both heads in phc_policy_sample)
        policy_sample(mu.contiguous(), value.contiguous(), (logstd[0] if logstd.dim() == 2 else logstd).float().contiguous(), self.value_mean_std,
                      e["actions"][n], e["mus"][n], e["sigmas"][n], e["neglogpacs"][n], e["values"][n])
        if self.clip_actions:
            self.preprocess_actions(e["actions"][n], out=self._env_actions)

    def _rollout_bookkeeping(self, n, rewards, terminate, reward_raw):
        """The step's outputs into row n of the experience buffer and the episode bookkeeping (amp_agent.py:321-341): rewards / dones rows, terminated flags,
        reward-term sums, episode statistics.  -> the step's `terminate` mask as floats."""
        e = self.exp
        e["next_obses"][n].copy_(self.obs)
        if self._reward_raw_acc is None:
            self._reward_raw_acc = torch.zeros(reward_raw.shape[1], dtype=reward_raw.dtype, device=self.device)
        if (rewards.is_cuda and rewards.dtype == torch.float32 and rewards.is_contiguous() and self.dones.dtype == torch.int64 and terminate.dtype == torch.int64
                and reward_raw.dtype == torch.float32 and reward_raw.is_contiguous() and reward_raw.shape[1] <= 8):   # on the device: one launch
            L.check(L.load().phc_rollout_bookkeeping(
                rewards.data_ptr(), float(self.reward_scale), self.dones.data_ptr(), terminate.data_ptr(), reward_raw.data_ptr(), reward_raw.shape[1],
                self.num_actors, e["rewards"][n].data_ptr(), e["dones"][n].data_ptr(), self._terminated_flags.data_ptr(), self._terminated_mask.data_ptr(),
                self._reward_raw_acc.data_ptr(), self.current_rewards.data_ptr(), self.current_lengths.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "phc_rollout_bookkeeping")
            return self._terminated_mask
        # the torch statement: the CPU path, the device's fallback for other dtypes / layouts, and what the launch is tested against
        e["rewards"][n].copy_(rewards if self.reward_scale == 1 else rewards * self.reward_scale)
        e["dones"][n].copy_(self.dones)
        terminated = terminate.float()
        self._terminated_flags.add_(terminated)
        self._reward_raw_acc.add_(reward_raw.mean(dim=0))
        not_dones = 1.0 - self.dones.float()
        self.current_rewards.add_(rewards).mul_(not_dones.unsqueeze(1))
        self.current_lengths.add_(1).mul_(not_dones)
        return terminated

    def _rollout_after(self, n, rewards, terminate, reward_raw):
        """(B) the step's outputs into row n and the bookkeeping, next-value critic (zeroed where the episode terminated)."""
        terminated = self._rollout_bookkeeping(n, rewards, terminate, reward_raw)
        with self._autocast():
            value = self.model.a2c_network.eval_critic(self._preproc_obs(self.obs))
        policy_sample(None, value.contiguous(), None, self.value_mean_std, None, None, None, None, self.exp["next_values"][n], mask=terminated)

    def _rollout_step(self, n, seg):
        """Rollout step n on the device.  `seg` runs a segment: `call_segment` (eager, and inside the capture of a whole step) or `CapturedRollout.segment` (a graph of its own)."""
        self._rollout_reset(n)
        seg("policy", (self.obs,), self._rollout_policy, n)
        self.obs, rewards, self.dones, infos = self.vec_env.step(self._env_actions if self.clip_actions else self.exp["actions"][n])
        rewards = rewards.unsqueeze(1) if rewards.dim() == 1 else rewards
        self.exp["amp_obs"][n].copy_(infos["amp_obs"])   # (eager: the window of the task's AMP strip moves every step)
        terminate, reward_raw = infos["terminate"], infos["reward_raw"]
        if self._reward_raw_acc is None:   # the first rollout (also that of a restored checkpoint, whatever its epoch_num) creates the accumulator: eagerly
            seg = call_segment
        seg("after", (self.obs, rewards, self.dones, terminate, reward_raw), self._rollout_after, n, rewards, terminate, reward_raw)

    def _rollout_step_torch(self, n):
        """Rollout step n as torch ops (CPU tensors): the reference's statements (amp_agent.py:315-345)."""
        e = self.exp
        self._rollout_reset(n)
        if self.obs.data_ptr() != e["obses"][n].data_ptr():
            e["obses"][n].copy_(self.obs)
        res = self.get_action_values(self.obs)
        for k in ("values", "neglogpacs", "actions", "mus", "sigmas"):
            e[k][n].copy_(res[k])
        self.obs, rewards, self.dones, infos = self.vec_env.step(self.preprocess_actions(res["actions"]))
        rewards = rewards.unsqueeze(1) if rewards.dim() == 1 else rewards
        e["amp_obs"][n].copy_(infos["amp_obs"])
        terminated = self._rollout_bookkeeping(n, rewards, infos["terminate"], infos["reward_raw"])
        e["next_values"][n].copy_(self._eval_critic(self.obs) * (1.0 - terminated.unsqueeze(-1)))

    def play_steps(self):
        self.set_eval()
        if self._terminated_flags is None:
            self._terminated_flags = torch.zeros(self.num_actors, device=self.device)
            self._terminated_mask = torch.zeros(self.num_actors, device=self.device)
            self._env_actions = torch.empty_like(self.exp["actions"][0])
        self._terminated_flags.zero_()
        if self._reward_raw_acc is not None:
            self._reward_raw_acc.zero_()
        roll = self._rollout
        roll.follow(self.task)
        if not self.exp["obses"].is_cuda:
            for n in range(self.horizon_length):
                self._rollout_step_torch(n)
        elif roll.whole_steps():
            roll.play_whole_steps()
        else:
            seg = roll.segment if roll.enabled() else call_segment
            for n in range(self.horizon_length):
                self._rollout_step(n, seg)
        return self._rollout_batch()

    def _rollout_batch(self):
        """The filled experience buffer as the epoch's batch: discriminator rewards, GAE, [T, N, ...] -> [N * T, ...]."""
        e = self.exp
        mb_fdones = e["dones"].float()
        amp_rewards = self._calc_amp_rewards(e["amp_obs"])
        mb_rewards = self._combine_rewards(e["rewards"], amp_rewards)
        mb_advs = discount_values(mb_fdones, e["values"], mb_rewards, e["next_values"], self.gamma, self.tau)
        batch = {k: swap_and_flatten01(e[k]) for k in ("obses", "rewards", "values", "neglogpacs", "dones", "actions", "mus", "sigmas", "amp_obs")}
        batch["returns"] = swap_and_flatten01(mb_advs + e["values"])
        batch["terminated_flags"] = self._terminated_flags
        batch["reward_raw"] = self._reward_raw_acc / self.horizon_length
        batch["played_frames"] = self.batch_size
        batch["disc_rewards"] = swap_and_flatten01(amp_rewards["disc_rewards"])
        batch["mb_rewards"] = swap_and_flatten01(mb_rewards)
        return batch

    def _eval_disc(self, amp_obs):
        with self._autocast():
            return self.model.a2c_network.eval_disc(self._preproc_amp_obs(amp_obs)).float()

    def _calc_amp_rewards(self, amp_obs):
        with torch.no_grad():
            T, N, A = amp_obs.shape
            logits = self._eval_disc(amp_obs.reshape(T * N, A)).reshape(T, N, 1)
            prob = 1 / (1 + torch.exp(-logits))
            disc_r = -torch.log(torch.maximum(1 - prob, torch.tensor(0.0001, device=amp_obs.device)))
            disc_r = disc_r * self._disc_reward_scale
        return {"disc_rewards": disc_r}

    def _combine_rewards(self, task_rewards, amp_rewards):
        return self._task_reward_w * task_rewards + self._disc_reward_w * amp_rewards["disc_rewards"]

    # ------------------------------------------------------------------ dataset (common_agent.py:357-398,589-599; amp_agent.py:399-411)
    def prepare_dataset(self, b):
        advantages = torch.sum(b["returns"] - b["values"], axis=1)
        if self.normalize_advantage:
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)  # per rank, as the reference (common_agent.py:596-597)
        values, returns = b["values"], b["returns"]
        if self.normalize_value:
            values = self.value_mean_std(values)
            returns = self.value_mean_std(returns)
        self.dataset = {"old_values": values, "old_logp_actions": b["neglogpacs"], "advantages": advantages, "returns": returns,
                        "actions": b["actions"], "obs": b["obses"], "mu": b["mus"], "sigma": b["sigmas"], "amp_obs": b["amp_obs"],
                        "amp_obs_demo": b["amp_obs_demo"], "amp_obs_replay": b["amp_obs_replay"]}

    def _draw_rows(self, i, out=None):
        """The dataset rows of minibatch `i` of the current pass over the batch (AMPDataset._get_item / _shuffle_idx_buf, amp_datasets.py:72-99), as a copy
        or written into `out`: `_idx_buf` is re-drawn behind the last minibatch of a pass, before that minibatch's kernels have run."""
        s, e = i * self.minibatch_size, (i + 1) * self.minibatch_size
        rows = self._idx_buf[s:e].clone() if out is None else out.copy_(self._idx_buf[s:e])
        if e >= self.batch_size:
            self._idx_buf[:] = torch.randperm(self.batch_size, device=self._idx_buf.device)
        return rows

    def _get_item(self, idx):
        sample_idx = self._draw_rows(idx)
        amp_idx = sample_idx[:self._amp_minibatch_size]  # calc_gradients only reads rows [0:amp_minibatch_size] (amp_agent.py:570-577)
        if sample_idx.is_cuda:
            # the device kernels read the dataset rows in place (phc_running_norm / phc_ppo_loss take the row index): nothing is gathered
            return {"_dataset": self.dataset, "_idx": sample_idx, "_amp_idx": amp_idx}
        return {k: v[amp_idx if k.startswith("amp_obs") else sample_idx] for k, v in self.dataset.items()}

    # ------------------------------------------------------------------ losses (common_agent.py:512-520,564-587; amp_agent.py:732-808)
    def bound_loss(self, mu):
        if self.bounds_loss_coef is None:
            return torch.zeros((), device=mu.device)
        soft_bound = 1.0
        hi = torch.clamp_min(mu - soft_bound, 0.0) ** 2
        lo = torch.clamp_max(mu + soft_bound, 0.0) ** 2
        return (lo + hi).sum(axis=-1)

    def _disc_loss(self, disc_agent_logit, disc_demo_logit, obs_demo):
        bce = torch.nn.BCEWithLogitsLoss()
        disc_loss = 0.5 * (bce(disc_agent_logit, torch.zeros_like(disc_agent_logit)) + bce(disc_demo_logit, torch.ones_like(disc_demo_logit)))
        net = self.model.a2c_network
        disc_logit_loss = torch.sum(torch.square(net.get_disc_logit_weights()))
        disc_loss = disc_loss + self._disc_logit_reg * disc_logit_loss
        with input_grad_only():
            grad = torch.autograd.grad(disc_demo_logit, obs_demo, grad_outputs=torch.ones_like(disc_demo_logit), create_graph=True,
                                       retain_graph=True, only_inputs=True)[0].float()   # bf16 leaf (device normaliser output): penalty in fp32
        disc_grad_penalty = torch.mean(torch.sum(torch.square(grad), dim=-1))
        disc_loss = disc_loss + self._disc_grad_penalty * disc_grad_penalty
        if self._disc_weight_decay != 0:
            w = torch.cat(net.get_disc_weights(), dim=-1)
            disc_loss = disc_loss + self._disc_weight_decay * torch.sum(torch.square(w))
        return {"disc_loss": disc_loss, "disc_grad_penalty": disc_grad_penalty.detach(), "disc_logit_loss": disc_logit_loss.detach(),
                "disc_agent_acc": (disc_agent_logit < 0).float().mean().detach(), "disc_demo_acc": (disc_demo_logit > 0).float().mean().detach(),
                # (the reference keeps the logit tensors and logs their mean over the epoch, amp_agent.py:786-787,911-912: equal-sized minibatches, same number)
                "disc_agent_logit": disc_agent_logit.detach().float().mean(), "disc_demo_logit": disc_demo_logit.detach().float().mean()}

    # Every scalar the fused loss kernels produce lands in ONE fp32 vector (`_raw`), which a graphed step adds to its accumulator
    # in one launch; the info dict is derived from it outside the step (all entries are linear in it).  Layout, nw = number of
    # discriminator weight matrices:  [0:7] phc_ppo_loss (loss, a_loss, c_loss, b_loss, entropy, kl, clip fraction) | [7:12] phc_disc_bce (k * bce,
    # agent acc, demo acc, mean agent logit, mean demo logit) | [12:13+nw] weight terms (k * (decay + logit reg), |W_i|^2 ...) |
    # [13+nw:15+nw] penalty (k * pen, |grad|^2).
    _RAW_FIXED = 15

    def _raw_buffer(self):
        nw = len(self.model.a2c_network.get_disc_weights_raw())
        if self._raw is None or self._raw.numel() != self._RAW_FIXED + nw:
            self._raw = torch.zeros(self._RAW_FIXED + nw, dtype=torch.float32, device=self.device)
        return self._raw, nw

    def _info_from_raw(self, raw):
        nw = raw.numel() - self._RAW_FIXED
        k = self._disc_coef
        return {"actor_loss": raw[1], "critic_loss": raw[2], "b_loss": raw[3], "entropy": raw[4], "kl": raw[5], "actor_clip_frac": raw[6],
                "disc_loss": (raw[7] + raw[12] + raw[13 + nw]) / k, "disc_grad_penalty": raw[13 + nw] / (self._disc_grad_penalty * k),
                "disc_logit_loss": raw[12 + nw], "disc_agent_acc": raw[8], "disc_demo_acc": raw[9], "disc_agent_logit": raw[10], "disc_demo_logit": raw[11]}

    def _disc_loss_fused(self, logits, m, obs_demo):
        """`_disc_loss` on the device with the pieces as kernels (fast_ops.disc_bce / weighted_sumsq): every term already carries
        `disc_coef` and enters the total loss with weight one.  `logits` [3m, 1]: agent, replay, demo rows.  -> the three loss terms; where
        `_disc_decay_terms` gives a preload, the gradient of the weight terms is not theirs to produce: FlatGradBucket.zero has written it."""
        k = self._disc_coef
        raw, nw = self._raw_buffer()
        bce, _ = disc_bce(logits, 2 * m, k, out=raw[7:12])
        ws, coefs, preload = self._disc_decay_terms()
        # (a K-padded weight enters with its padded storage -- the pad is zero --, when its gradient is preloaded anyway)
        l2 = weighted_sumsq([getattr(w, "_padded", w) if preload is not None else w.contiguous() for w in ws], coefs, out=raw[12:13 + nw], preloaded=preload is not None)
        # d(sum of the demo logits) / d(demo rows): cotangent = [0; 0; 1] over the [agent; replay; demo] logits, and the layers are told
        # that only the last row block carries anything (GEMMs over m instead of 3m rows, here and in the second-order pass)
        with input_grad_only(row_start=2 * m):
            grad = torch.autograd.grad(logits, obs_demo, grad_outputs=self._demo_row_mask(m, logits), create_graph=True, retain_graph=True,
                                       only_inputs=True)[0]
        pen = weighted_sumsq([grad], [self._disc_grad_penalty * k / m], out=raw[13 + nw:15 + nw])
        return [bce, l2, pen]

    def _disc_decay_terms(self):
        """(discriminator weights, coefficient of each one's sum of squares in the total loss, the preload: [(weight, 2 c)] for FlatGradBucket.zero
        to start each weight's gradient at these terms' gradient 2 c w -- None where a weight is outside the flat bucket and autograd has to add it)."""
        k = self._disc_coef
        ws = [p for p in self.model.a2c_network.get_disc_weights_raw()]
        coefs = [self._disc_weight_decay * k] * len(ws)
        coefs[-1] += self._disc_logit_reg * k   # the logit layer: regulariser + weight decay
        in_bucket = all(getattr(w, "_bucket", None) is self.grads for w in ws)
        return ws, coefs, ([(w, 2.0 * c) for w, c in zip(ws, coefs)] if in_bucket else None)

    def _demo_row_mask(self, m, like):
        key = (m, like.dtype, like.device)
        if self._ones_key != key:
            mask = torch.zeros((3 * m, 1), dtype=like.dtype, device=like.device)
            mask[2 * m:] = 1
            self._ones_key, self._ones = key, mask
        return self._ones

    def _fwd_bwd(self, d, want_info=True):
        """Forward + losses + backward into the flat gradient bucket (amp_agent.py:554-655); no host sync.  -> (info dict, whether the
        gradient was all-reduced on the way).  `want_info=False` (a pass of the captured update outside its graphs' replay): no collective,
        and when all scalars are in `self._raw` the info dict is not built (it would cost launches)."""
        idx = amp_idx = None
        if "_dataset" in d:   # device: minibatch = (dataset, row index); the kernels below read the rows in place
            d, idx, amp_idx = d["_dataset"], d["_idx"], d["_amp_idx"]
        if self._fused_disc:
            reduced = self._device_step(d, idx, amp_idx, collectives=want_info)
            return (self._info_from_raw(self._raw.clone()) if want_info else None), reduced   # (a copy: the next step overwrites `_raw`)
        # the torch path: the CPU, and the device when the fused discriminator loss does not apply (there with the fused actor / critic loss)
        obs = self._preproc_obs(d["obs"], use_temp=self.temp_running_mean, row_index=idx)
        fused = obs.is_cuda
        amp_obs, amp_obs_replay, amp_obs_demo = (self._preproc_amp_obs(d[k], amp_idx) for k in ("amp_obs", "amp_obs_replay", "amp_obs_demo"))
        amp_obs_demo.requires_grad_(True)
        inp = {"is_train": True, "prev_actions": d["actions"], "obs": obs, "amp_obs": amp_obs, "amp_obs_replay": amp_obs_replay,
               "amp_obs_demo": amp_obs_demo, "raw_disc_logits": False}
        if self._actor_split and fused:
            inp["obs_actor"] = self._actor_obs(d["obs"], use_temp=self.temp_running_mean, row_index=idx)
        with self._autocast():
            res = self.model.forward_heads(inp) if fused else self.model(inp)
        disc_info = self._disc_loss(torch.cat([res["disc_agent_logit"], res["disc_agent_replay_logit"]], dim=0), res["disc_demo_logit"], amp_obs_demo)
        if fused:
            disc = self._disc_coef * disc_info["disc_loss"]
            ppo, st = self._ppo_loss_fused(res["mu"], res["value"], res["logstd"], d, idx)
            info = {"actor_loss": st[0], "critic_loss": st[1], "b_loss": st[2], "entropy": st[3], "kl": st[4], "actor_clip_frac": st[5]}
            self.grads.zero()
            self._backward([ppo, disc])
        else:
            assert idx is None
            loss, info = self._ppo_loss_torch(res, d, disc_info)
            self.grads.zero()
            loss.backward()
        info.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in disc_info.items()})
        return info, False

    def _device_step(self, d, idx, amp_idx, collectives=True):
        """The device's forward + backward of one optimizer step: `_policy_pass` and `_disc_pass`, side by side on two streams or one after the
        other on the current one.  Every scalar lands in `self._raw`.  -> whether the gradient was all-reduced behind the passes."""
        br = self._branch_streams()
        if br is None:
            # ONE zero of the whole bucket, with the weight-decay preload, in front of both bodies: a second zero() between the preload and the
            # discriminator's backward would bump the bucket's generation and make that backward overwrite the preload (fast_ops._first_write)
            self.grads.zero(self._disc_decay_terms()[2])
            self._policy_pass(d, idx, zero=False)
            self._disc_pass(d, amp_idx, zero=False)
            return False
        # the discriminator pass on its stream next to the policy pass: see __init__
        main = torch.cuda.current_stream(self.device)
        br.wait_stream(main)
        split = collectives and self._split_active()
        with torch.cuda.stream(br):
            self._disc_pass(d, amp_idx)
            if split:
                self._grad_all_reduce("disc")
        self._policy_pass(d, idx)
        if split:
            self._grad_all_reduce("policy")
        main.wait_stream(br)
        return split

    def _branch_streams(self):
        """The discriminator's stream of the optimizer step, or None (switched off)."""
        if not self._use_branches:
            return None
        if self._branches is None:
            net = self.model.a2c_network
            disc_params = [p for mod in (net._disc_mlp, net._disc_logits) for p in mod.parameters()]
            try:
                self._disc_spans, self._policy_spans = self.grads.spans_of([p for p in disc_params if getattr(p, "_bucket", None) is self.grads])
            except ValueError:      # (a network whose discriminator parameters are not one run of the bucket: one stream, as before round 4)
                self._use_branches = False
                return None
            self._branches = torch.cuda.Stream(self.device)
            register_lane(self._branches, "disc")      # (its kernels get their own reduction scratch buffers)
        return self._branches

    def _amp_cat(self, d, amp_idx):
        """The three AMP batches normalised into the row blocks of ONE [agent; replay; demo] buffer (no torch.cat in front of the
        discriminator); the demo block is also the leaf the gradient penalty differentiates to.  -> (buffer, demo leaf, rows per block)"""
        m = amp_idx.numel() if amp_idx is not None else d["amp_obs"].shape[0]
        dt = torch.bfloat16 if self.bf16 else torch.float32
        A = d["amp_obs"].shape[1]
        if self.bf16 and self._amp_pad_cols > A:   # K-padded discriminator input (pad columns stay zero)
            cat = self._pad_buf("amp_cat", 3 * m, self._amp_pad_cols)
        else:
            cat = torch.empty((3 * m, A), dtype=dt, device=d["amp_obs"].device)
        for k, key in enumerate(("amp_obs", "amp_obs_replay", "amp_obs_demo")):
            self._amp_input_mean_std(d[key], out_dtype=dt, row_index=amp_idx, out=cat[k * m:(k + 1) * m, :A])
        return cat, cat[2 * m:].requires_grad_(True), m

    def _disc_pass(self, d, amp_idx, zero=True):
        """The discriminator's share of an optimizer step on the CURRENT stream: the three AMP batches normalised into one
        [agent; replay; demo] buffer, forward, loss terms, backward.  `zero`: its slice of the gradient bucket is zeroed first (weight-decay
        gradients preloaded); False when the caller has zeroed the whole bucket for both passes."""
        if zero:
            self.grads.zero(self._disc_decay_terms()[2], spans=self._disc_spans)
        cat, amp_obs_demo, m = self._amp_cat(d, amp_idx)
        with self._autocast():
            logits = self.model.a2c_network.eval_disc(rows_with_grad(cat, amp_obs_demo, 2 * m))
        self._backward(self._disc_loss_fused(logits, m, amp_obs_demo))

    def _policy_pass(self, d, idx, zero=True):
        """Actor + critic share of an optimizer step on the current stream: (`zero`) their slices of the gradient bucket zeroed, the observation
        normalised, both forward passes, the fused loss kernel, backward.  (The critic on a third stream was measured too: a graph with a
        fork inside leaves the runtime's packet-replay path -- profiles/r04_ppo/README.md.)"""
        net = self.model.a2c_network
        if zero:
            self.grads.zero(spans=self._policy_spans)
        obs = self._preproc_obs(d["obs"], use_temp=self.temp_running_mean, row_index=idx)
        with self._autocast():
            value = net.eval_critic(obs)
            mu, logstd = net.eval_actor(self._actor_obs(d["obs"], use_temp=self.temp_running_mean, row_index=idx) if self._actor_split else obs)
        self._backward([self._ppo_loss_fused(mu, value, logstd[0] if logstd.dim() == 2 else logstd, d, idx)[0]])

    def _ppo_loss_fused(self, mu, value, logstd, d, idx):
        """Actor / critic losses and their gradients w.r.t. the two heads: one HIP pass (phc_ppo_loss) instead of ~100 launches.
        -> (loss root, its six statistics); the scalars also land in `_raw[0:7]`."""
        if self._actor_split:
            value = value.float()           # (phc_ppo_loss takes both heads in one type)
        return ppo_loss(mu.contiguous(), value.contiguous(), logstd, d["actions"], d["old_logp_actions"], d["advantages"], d["returns"],
                        d["old_values"], d["mu"], d["sigma"], self.e_clip, self.critic_coef, self.entropy_coef, self.bounds_loss_coef,
                        self.clip_value, unit_grad=True, row_index=idx, out=self._raw_buffer()[0][0:7])

    def _backward(self, roots):
        """The fused loss terms enter the total with weight one (unit_grad): they are the roots of ONE backward pass with constant unit
        cotangents -- no sum node, no fill launches.  Bias gradients: first stages in the layers, ONE finishing launch at the end."""
        with param_grad_only(), deferred_colsums():
            torch.autograd.backward(roots, grad_tensors=[self._unit_cotangent(r) for r in roots])

    def _unit_cotangent(self, like):
        key = (like.dtype, like.device)
        if key not in self._unit_cot:
            self._unit_cot[key] = torch.ones((), dtype=like.dtype, device=like.device)
        return self._unit_cot[key]

    def _ppo_loss_torch(self, res, d, disc_info):
        """The actor / critic losses as torch expressions (amp_agent.py:598-640): the CPU path and the definition `phc_ppo_loss` is
        tested against."""
        ratio = torch.exp(d["old_logp_actions"] - res["prev_neglogp"])
        adv = d["advantages"]
        a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.e_clip, 1.0 + self.e_clip))
        values, ret, vp = res["values"], d["returns"], d["old_values"]
        if self.clip_value:
            vpc = vp + (values - vp).clamp(-self.e_clip, self.e_clip)
            c_loss = torch.max((values - ret) ** 2, (vpc - ret) ** 2)
        else:
            c_loss = (ret - values) ** 2
        b_loss = self.bound_loss(res["mus"])
        a_loss, c_loss, b_loss, entropy = a_loss.mean(), c_loss.mean(), b_loss.mean(), res["entropy"].mean()
        bl = self.bounds_loss_coef if self.bounds_loss_coef is not None else 0.0
        loss = a_loss + self.critic_coef * c_loss - self.entropy_coef * entropy + bl * b_loss + self._disc_coef * disc_info["disc_loss"]
        with torch.no_grad():
            kl = policy_kl(res["mus"].detach(), res["sigmas"].detach(), d["mu"], d["sigma"])
            clip_frac = (torch.abs(ratio - 1.0) > self.e_clip).float().mean()     # common_agent.py:570-571,327
        return loss, {"actor_loss": a_loss.detach(), "critic_loss": c_loss.detach(), "b_loss": b_loss.detach(), "entropy": entropy.detach(), "kl": kl,
                      "actor_clip_frac": clip_frac}

    def _clip_and_step(self, step_device=None):
        """`step_device`: inside a captured graph -- the kernels count the optimizer step on the device, the host-side `step` is advanced by
        the caller (one per replay)."""
        if self.grads.flat.is_cuda:
            adam_clip_step(self.optimizer, self.grads.flat_param, self.grads.flat, self.grad_norm if self.truncate_grads else None,
                           shadow=self.grads.shadow, step_device=step_device, count_host=step_device is None)
            return
        if self.truncate_grads:
            self.grads.clip_grad_norm_(self.grad_norm)
        self.optimizer.step()

    def calc_gradients(self, d):
        """One optimizer step (amp_agent.py:554-688): forward/backward, the path's one collective -- the flat gradient
        all-reduce, replacing `optimizer.synchronize()` (:667-668) -- then clip + Adam on the flat parameter."""
        self.set_train()
        if "_dataset" not in d:   # a gathered minibatch: only rows [0:amp_minibatch_size] of the AMP batches are read (amp_agent.py:570-577)
            d = {k: (v[0:self._amp_minibatch_size] if k.startswith("amp_obs") else v) for k, v in d.items()}
        info, reduced = self._fwd_bwd(d)
        if not reduced:
            self._grad_all_reduce()
        self._clip_and_step()
        return info

    def _grad_all_reduce(self, part=None):
        """`part` None: the whole flat gradient (one collective per optimizer step, the default).  "disc" / "policy" (`split_allreduce`): that pass's range of the
        bucket, issued on the CURRENT stream right behind the pass -- the discriminator's all-reduce then runs while the (longer) policy chain is still computing."""
        if self._reduces:
            spans = None if part is None else (self._disc_spans if part == "disc" else self._policy_spans)
            self.num_collectives += self.grads.all_reduce_mean(self.dist, force=self._force_collectives, timing=self.allreduce_timing, spans=spans)

    def _split_active(self):
        """Two all-reduces per optimizer step instead of one (`+learning.params.config.split_allreduce=True`; needs the two-stream step)."""
        return self._split_allreduce and self._reduces and self._branches is not None

    # ------------------------------------------------------------------ the optimizer step as a hipGraph (update_graph.CapturedUpdate)
    def _graph_enabled(self):
        return (self.grads.flat.is_cuda and self._use_graph and not self._graph_failed and self.minibatch_size >= int(self.config.get("hip_graph_min_rows", 2048))
                and not os.environ.get("PHC_NO_GRAPH"))

    @property
    def update_graphs(self):    # hipGraphs one captured optimizer step replays: 0 (eager launches), 1, or 3 (policy pass, discriminator pass, tail)
        return self._update.num_graphs

    @property
    def update_streams(self):   # 2 once an optimizer step has run its discriminator pass on a stream of its own, else 1
        return 2 if self._branches is not None else 1

    INFO_KEYS = ("actor_loss", "critic_loss", "b_loss", "entropy", "kl", "actor_clip_frac", "disc_loss", "disc_grad_penalty", "disc_logit_loss", "disc_agent_acc",
                 "disc_demo_acc", "disc_agent_logit", "disc_demo_logit")

    # ------------------------------------------------------------------ epoch (amp_agent.py:413-532)
    def _init_amp_demo_buf(self):
        n = int(np.ceil(self._amp_obs_demo_buffer.get_buffer_size() / self._amp_batch_size))
        for _ in range(n):
            self._amp_obs_demo_buffer.store({"amp_obs": self.vec_env.fetch_amp_obs_demo(self._amp_batch_size)})

    def _update_amp_demos(self):
        self._amp_obs_demo_buffer.store({"amp_obs": self.vec_env.fetch_amp_obs_demo(self._amp_batch_size)})

    def _store_replay_amp_obs(self, amp_obs):
        size = self._amp_replay_buffer.get_buffer_size()
        if self._amp_replay_buffer.get_total_count() > size:
            keep = torch.bernoulli(torch.full((amp_obs.shape[0],), self._amp_replay_keep_prob, device=amp_obs.device)) == 1.0
            amp_obs = amp_obs[keep]
        if amp_obs.shape[0] > size:
            amp_obs = amp_obs[torch.randperm(amp_obs.shape[0], device=amp_obs.device)[:size]]
        self._amp_replay_buffer.store({"amp_obs": amp_obs})

    def pre_epoch(self, epoch_num):
        t = self.task
        if (epoch_num > 1) and epoch_num % getattr(t, "shape_resampling_interval", 10 ** 9) == 1 and hasattr(t, "resample_motions"):
            t.resample_motions()
        if getattr(t, "getup_schedule", False) and hasattr(t, "update_getup_schedule"):  # amp_agent.py:518-525
            t.update_getup_schedule(epoch_num, getup_udpate_epoch=t.getup_udpate_epoch)
            warm = epoch_num > t.getup_udpate_epoch
            self._task_reward_w, self._disc_reward_w = (0.5, 0.5) if warm else (0, 1)
        self._snapshot_running_mean_std()

    def _snapshot_running_mean_std(self):
        """`self.running_mean_std_temp = copy.deepcopy(self.running_mean_std); .freeze()` (amp_agent.py:527-532), done as an
        in-place copy into ONE persistent module so that captured graphs keep valid buffer addresses."""
        if self.running_mean_std is None:
            return
        if self.running_mean_std_temp is None:
            self.running_mean_std_temp = copy.deepcopy(self.running_mean_std)
            self.running_mean_std_temp.freeze()
        else:
            for a, b in zip(self.running_mean_std_temp.buffers(), self.running_mean_std.buffers()):
                a.copy_(b)

    def post_epoch(self, epoch_num):
        self._snapshot_running_mean_std()
        for m in self._norms():
            m.sync(self.dist)

    def init_train(self):
        self.obs = self.env_reset()
        self._init_amp_demo_buf()

    _proj_seen = 0   # the projectiles' hit count at the last read (`projectile/hits` is the difference per epoch)
    _push_seen = 0   # the schedule's push count at the last read (`perturb/pushes` is the difference per epoch)

    def train_epoch(self):
        self.epoch_num += 1
        self.pre_epoch(self.epoch_num)
        sync = torch.cuda.synchronize if str(self.device).startswith("cuda") else (lambda: None)
        sync()
        t0 = time.time()
        with torch.no_grad(), self.grads.shadow_scope(), _marker("phc:rollout"):   # rollout inference reads the bf16 parameter copies
            batch = self.play_steps()
        sync()
        t1 = time.time()
        self._update_amp_demos()
        n = batch["amp_obs"].shape[0]
        batch["amp_obs_demo"] = self._amp_obs_demo_buffer.sample(n)["amp_obs"]
        batch["amp_obs_replay"] = batch["amp_obs"] if self._amp_replay_buffer.get_total_count() == 0 else self._amp_replay_buffer.sample(n)["amp_obs"]
        self.set_train()
        self.prepare_dataset(batch)
        infos, ginfo = [], None
        with self.grads.shadow_scope(), _marker("phc:update"):
            if self._graph_enabled():
                try:
                    ginfo = self._update.run_epoch()
                except Exception as exc:   # capture not possible on this stack: eager launches from here on
                    if self._update.num_graphs:
                        raise
                    self._graph_failed = True
                    torch.cuda.synchronize()
                    print(f"[phc_amd] update graph disabled ({type(exc).__name__}: {exc})", flush=True)
            if ginfo is None:
                for _ in range(self.mini_epochs_num):
                    for i in range(self.num_minibatches):
                        infos.append(self.calc_gradients(self._get_item(i)))
                        if self._trace is not None:
                            self._trace.append(torch.stack([infos[-1][k].float().reshape(()) for k in self.INFO_KEYS]))
        self._store_replay_amp_obs(batch["amp_obs"])
        self.post_epoch(self.epoch_num)
        sync()
        t2 = time.time()
        self.frame += self.batch_size * self.world
        info = {k: v.item() for k, v in ginfo.items()} if ginfo is not None else {k: torch.stack([i[k] for i in infos]).mean().item() for k in infos[0]}
        # (one host transfer for the rollout's reward statistics: amp_agent.py:900-925 logs mean / std of the discriminator reward, the mean combined reward and the mean return)
        dr_std, dr_mean = torch.std_mean(batch["disc_rewards"])
        rs = torch.stack([batch["rewards"].mean(), dr_mean, dr_std, batch["mb_rewards"].mean(), batch["returns"].mean()]).tolist()
        info.update(play_time=t1 - t0, update_time=t2 - t1, total_time=t2 - t0, mean_task_reward=rs[0], mean_disc_reward=rs[1], disc_reward_std=rs[2],
                    mean_mb_reward=rs[3], mean_return=rs[4], reward_raw=batch["reward_raw"].tolist(),
                    step_fps=self.batch_size / (t1 - t0), total_fps=self.batch_size / (t2 - t0))  # common_agent.py:134-138
        push = getattr(self.task, "_push", None)
        if push is not None:   # `+perturb.*` (train() admits the device schedule only): pushes started during this epoch's rollout in THIS rank's envs -- one scalar read, no reduction over ranks
            total = int(push.pushes)
            info["perturb/pushes"], self._push_seen = total - self._push_seen, total
        proj = getattr(self.task, "_proj", None)
        if proj is not None:   # `+projectile.*`: impacts on bodies during this epoch's rollout in THIS rank's envs -- one scalar read
            total = int(proj.hits)
            info["projectile/hits"], self._proj_seen = total - self._proj_seen, total
        if self._trace is not None:   # `+learning.params.config.trace_minibatches=True`: every optimizer step's scalars, in order (a diagnostic)
            tr = torch.stack(self._trace).cpu() if self._trace else torch.zeros(0)
            info["minibatch_trace"] = {k: tr[:, j].tolist() for j, k in enumerate(self.INFO_KEYS)} if tr.numel() else {}
            self._trace = []
        return info

    def assemble_train_info(self, info):
        """The scalars the reference hands its SummaryWriter / wandb every epoch, under the reference's tags (`CommonAgent._assemble_train_info`,
        common_agent.py:603-626; `AMPAgent._assemble_train_info`, amp_agent.py:900-933): performance, learning rate, losses, discriminator statistics, reward
        terms; plus the evaluation sweep's `eval/*` entries when the epoch ran one (im_amp.py:334-346).  Pinned to the reference's method by tests/test_learner_epoch.py."""
        raw = list(info.get("reward_raw", [])) + [0.0] * 5
        out = {"performance/update_time": info["update_time"], "performance/play_time": info["play_time"], "performance/total_fps": info["total_fps"],
               "learning_rate/last_lr": self.last_lr, "learning_rate/lr_mul": 1.0, "learning_rate/e_clip": self.e_clip,
               "loss/actor_loss": info["actor_loss"], "loss/critic_loss": info["critic_loss"], "loss/bounds_loss": info["b_loss"], "loss/entropy": info["entropy"],
               "loss/kl": info["kl"], "loss/clip_frac": info["actor_clip_frac"], "disc/loss": info["disc_loss"], "disc/agent_acc": info["disc_agent_acc"],
               "disc/demo_acc": info["disc_demo_acc"], "disc/agent_logit": info["disc_agent_logit"], "disc/demo_logit": info["disc_demo_logit"],
               "disc/grad_penalty": info["disc_grad_penalty"], "disc/logit_loss": info["disc_logit_loss"], "disc/reward_mean": info["mean_disc_reward"],
               "disc/reward_std": info["disc_reward_std"], "rewards/returns": info["mean_return"],
               "rewards/mb_rewards": info["mean_mb_reward"], "rewards/body_pos": raw[0], "rewards/body_rot": raw[1], "rewards/lin_vel": raw[2], "rewards/ang_vel": raw[3],
               "rewards/power": raw[4]}
        out.update({k: v for k, v in info.items() if k.startswith(("eval/", "perturb/", "projectile/"))})
        return {k: float(v) for k, v in out.items()}

    def _log_train_info(self, scalars, output_dir):
        """`CommonAgent._log_train_info` (common_agent.py:627-635): `writer.add_scalar(tag, value, epoch)` for every entry.  tensorboardX / wandb are not part of
        this image; the same (tag, value, step) stream goes to `<output_dir>/summaries/scalars.jsonl`, one line per epoch, and -- where a `torch.utils.tensorboard`
        SummaryWriter can be made -- into event files next to it."""
        import json
        d = os.path.join(output_dir, "summaries")
        if self._summary_file is None:
            os.makedirs(d, exist_ok=True)
            self._summary_file = open(os.path.join(d, "scalars.jsonl"), "a")
            try:
                from torch.utils.tensorboard import SummaryWriter
                self._summary_writer = SummaryWriter(d)
            except Exception:   # noqa: BLE001  (no tensorboard package: the jsonl stream is the record)
                self._summary_writer = None
        self._summary_file.write(json.dumps({"step": self.epoch_num, "frame": self.frame, **scalars}) + "\n")
        self._summary_file.flush()
        if self._summary_writer is not None:
            for k, v in scalars.items():
                self._summary_writer.add_scalar(k, v, self.epoch_num)

    def train(self, max_epochs, log=print, output_dir=None):
        """Training loop with the reference's checkpoint / evaluation cadence (common_agent.py:142-165): with `output_dir`,
        `Humanoid.pth` every min(50, save_best_after) epochs; every `save_frequency` epochs (save_intermediate) also
        `Humanoid_{epoch:08d}.pth` and the evaluation sweep `eval()`, which re-weights the clip sampling (auto-PMCP, im_amp.py:126-132)
        and writes `failed_{epoch:010d}.pkl`."""
        from ..motion_record import refuse_training
        refuse_training(getattr(self.task, "cfg", None))   # `+record.motion` belongs to the player and the sweep
        push = getattr(self.task, "_push", None)
        if push is not None and not getattr(push, "capturable", False):
            # the captured rollout graph freezes the launch sequence and the state of the schedule's generator
            raise NotImplementedError("training under a torch-generator push schedule (+perturb.rng=torch, the default) is not built: it pushes in play (test=True) "
                                      "and in the evaluation sweep; +perturb.rng=device is the schedule that trains")
        self.init_train()
        if push is not None:
            self._push_seen = int(push.pushes)
        proj = getattr(self.task, "_proj", None)
        if proj is not None:
            self._proj_seen = int(proj.hits)
        c = self.config
        save_freq, save_best_after = int(c.get("save_frequency", 0)), int(c.get("save_best_after", 100))
        save_intermediate = bool(c.get("save_intermediate", False))
        info = {}
        for _ in range(max_epochs):
            info = self.train_epoch()
            if self.rank == 0 and log is not None:
                log(f"epoch {self.epoch_num}: total_fps {info['total_fps']:.0f} step_fps {info['step_fps']:.0f} task_r {info['mean_task_reward']:.4f} "
                    f"disc_r {info['mean_disc_reward']:.4f} a_loss {info['actor_loss']:.4f} c_loss {info['critic_loss']:.4f} disc_loss {info['disc_loss']:.4f}"
                    + (f" perturb/pushes {info['perturb/pushes']}" if "perturb/pushes" in info else "")
                    + (f" projectile/hits {info['projectile/hits']}" if "projectile/hits" in info else ""))
            if output_dir is not None and save_freq > 0:
                if self.epoch_num % min(50, save_best_after) == 0 and self.rank == 0:
                    os.makedirs(output_dir, exist_ok=True)
                    self.save(os.path.join(output_dir, "Humanoid.pth"))
                if save_intermediate and self.epoch_num % save_freq == 0:
                    if self.rank == 0:
                        os.makedirs(output_dir, exist_ok=True)
                        self.save(os.path.join(output_dir, f"Humanoid_{self.epoch_num:08d}.pth"))
                    if hasattr(self.task, "_motion_lib") and hasattr(self.task, "_termination_distances"):
                        eval_info, _ = self.eval(output_dir=output_dir, log=log)
                        info.update(eval_info)
                        if push is not None:   # (the sweep ran on the same schedule: its pushes are in `perturb_pushes`, not in the next epoch's count)
                            self._push_seen = int(push.pushes)
                        if proj is not None:
                            self._proj_seen = int(proj.hits)
            if output_dir is not None and self.rank == 0:
                self._log_train_info(self.assemble_train_info(info), output_dir)
        return info

    def eval(self, output_dir=None, log=print):
        """IMAmpAgent.eval (im_amp.py:136-242): success rate / MPJPE over the whole motion set + auto-PMCP re-weighting."""
        from .im_eval import evaluate
        return evaluate(self, output_dir=output_dir, log=log if self.rank == 0 else None)

    # ------------------------------------------------------------------ checkpoint (amp_agent.py:69-108; SURVEY B4 key names)
    def _optimizer_state_dict(self):
        """The flat Adam state in the layout of the reference's `Adam(model.parameters())` (one entry per parameter, in
        `model.parameters()` order, common_agent.py:67): `exp_avg` / `exp_avg_sq` split at the bucket offsets.  Parameters that do
        not train (frozen PNN columns, the fixed sigma) appear in `params` without state, as torch writes them."""
        sd = self.optimizer.state_dict()
        flat_state = sd["state"].get(0, {})
        all_params = list(self.model.parameters())
        index = {id(p): i for i, p in enumerate(all_params)}
        state = {}
        for i, p in enumerate(self.grads.params):
            if flat_state:
                state[index[id(p)]] = {"step": flat_state["step"].clone() if torch.is_tensor(flat_state["step"]) else flat_state["step"],
                                       "exp_avg": self.grads.param_view(flat_state["exp_avg"], i).clone(),
                                       "exp_avg_sq": self.grads.param_view(flat_state["exp_avg_sq"], i).clone()}
        group = dict(sd["param_groups"][0])
        group["params"] = list(range(len(all_params)))
        return {"state": state, "param_groups": [group]}

    def _load_optimizer_state_dict(self, sd):
        """Inverse of `_optimizer_state_dict`; also accepts the one-entry flat layout of round-1 checkpoints.  A state that does not
        fit the current set of trainable parameters (another PNN stage, another network) is skipped with a warning, never mis-applied."""
        groups = sd.get("param_groups", [])
        n_entries = sum(len(g["params"]) for g in groups)
        if n_entries == 1 and len(list(self.model.parameters())) != 1:   # flat layout
            st = sd["state"].get(0)
            if st is not None and st["exp_avg"].numel() != self.grads.flat_param.numel():
                return self._skip_optimizer("flat optimizer state of another size")
            self.optimizer.load_state_dict(sd)
            return True
        all_params = list(self.model.parameters())
        if n_entries != len(all_params):
            return self._skip_optimizer(f"optimizer state for {n_entries} parameters, the model has {len(all_params)}")
        index = {id(p): i for i, p in enumerate(all_params)}
        state = sd["state"]
        mine = [index[id(p)] for p in self.grads.params]
        have = [i for i in mine if i in state]
        if not state:         # a checkpoint saved before the first optimizer step
            return True
        if len(have) != len(mine) or any(i not in mine for i in state):
            return self._skip_optimizer("optimizer state belongs to another set of trainable parameters (e.g. another PNN stage)")
        for p, i in zip(self.grads.params, mine):
            if tuple(state[i]["exp_avg"].shape) != tuple(p.shape):
                return self._skip_optimizer(f"optimizer state shape mismatch at parameter {i}")
        dev = self.grads.flat_param.device
        step = state[mine[0]]["step"]
        flat = {"step": (step.clone().float() if torch.is_tensor(step) else torch.tensor(float(step))),
                "exp_avg": torch.zeros_like(self.grads.flat_param), "exp_avg_sq": torch.zeros_like(self.grads.flat_param)}
        for k, i in enumerate(mine):   # (K-padded weights: the moments of the pad elements are zero)
            for key in ("exp_avg", "exp_avg_sq"):
                self.grads.param_view(flat[key], k).copy_(state[i][key].to(dev).float())
        group = {k: v for k, v in groups[0].items() if k != "params"}
        cur = self.optimizer.state_dict()["param_groups"][0]
        merged = dict(cur)
        merged.update({k: v for k, v in group.items() if k in cur})
        merged["params"] = [0]
        self.optimizer.load_state_dict({"state": {0: flat}, "param_groups": [merged]})
        return True

    def _skip_optimizer(self, why):
        if self.rank == 0:
            print(f"[phc_amd] optimizer state not restored: {why}", flush=True)
        return False

    def get_full_state_weights(self):
        s = {"model": self.model.state_dict(), "epoch": self.epoch_num, "optimizer": self._optimizer_state_dict(), "frame": self.frame}
        if self.running_mean_std is not None:
            s["running_mean_std"] = self.running_mean_std.state_dict()
        if self.value_mean_std is not None:
            s["reward_mean_std"] = self.value_mean_std.state_dict()
        if self._amp_input_mean_std is not None:
            s["amp_input_mean_std"] = self._amp_input_mean_std.state_dict()
        if hasattr(self.task, "get_env_rng_state"):   # (an extra key: the reference's loaders read the keys above by name)
            s["env_state"] = self.task.get_env_rng_state()
        return s

    def set_full_state_weights(self, w, load_optimizer=True):
        self.model.load_state_dict(w["model"])
        self.epoch_num = w.get("epoch", 0)
        self.frame = w.get("frame", 0)
        if "optimizer" in w and load_optimizer:
            self._load_optimizer_state_dict(w["optimizer"])
        for key, mod in (("running_mean_std", self.running_mean_std), ("reward_mean_std", self.value_mean_std), ("amp_input_mean_std", self._amp_input_mean_std)):
            if mod is not None and key in w:
                mod.load_state_dict(w[key])
        if self.grads.shadow is not None:
            self.grads.shadow.copy_(self.grads.flat_param)
        if "env_state" in w and hasattr(self.task, "set_env_rng_state"):
            self.task.set_env_rng_state(w["env_state"])

    def save(self, path):
        torch.save(self.get_full_state_weights(), path)

    def restore(self, path, load_optimizer=True):
        """`IMAmpAgent.restore` (im_amp.py:101-117): the checkpoint, then the newest `failed_*.pkl` next to it -- the termination
        history of the last evaluation sweep -- back into the motion library's sampling probabilities.  Players (`test=True`) pass
        `load_optimizer=False`, as the reference's `set_weights` path (amp_agent.py:84-90) does not touch the optimizer."""
        self.set_full_state_weights(torch.load(path, map_location=self.device, weights_only=False), load_optimizer=load_optimizer)
        import glob
        fails = glob.glob(os.path.join(os.path.dirname(os.path.abspath(path)), "failed_*"))
        lib = getattr(self.task, "_motion_lib", None)
        if fails and lib is not None and hasattr(lib, "update_sampling_prob"):
            import joblib
            newest = sorted(fails, key=lambda x: int(x.split("_")[-1].split(".")[0]))[-1]
            hist = joblib.load(newest)["termination_history"]
            ok = lib.update_sampling_prob(torch.as_tensor(hist, dtype=lib._termination_history.dtype, device=lib._termination_history.device))
            if self.rank == 0:
                print(f"[phc_amd] termination history {'restored from' if ok else 'does not match the motion set:'} {newest}", flush=True)
