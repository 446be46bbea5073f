"""The optimizer steps of an epoch as replayed hipGraphs (`hip_graph`; IMAmpAgent.train_epoch calls `CapturedUpdate.run_epoch`).

With the loss, normaliser and optimizer kernels fused, a step is ~140 launches of 2 ms total device time and the host needs
2.7-3.9 ms to issue them (it varies with the box): launch-bound.  Device runs therefore capture ONE step -- minibatch given by a
row-index buffer into persistent dataset tensors -- and replay it 48 times per epoch.  A graph holds no collective: with more than one
rank the gradient all-reduce and the two optimizer launches follow each replay eagerly.

What is captured is the agent's own step: `_policy_pass`, `_disc_pass`, `_fwd_bwd`, `_clip_and_step`, `_grad_all_reduce`.  This class owns
what a capture pins to fixed addresses and the graphs themselves."""
import os

import torch
from torch.autograd.graph import get_gradient_edge

from .. import _lib as L
from .fast_ops import _workspace, adam_state


def stale_grad_accumulators(params):
    """True if some parameter's AccumulateGrad node is kept alive by a graph outside the update (e.g. `w0 = p.clone()` held by
    the caller): such a node is bound to the stream it was created on and breaks stream capture.  A parameter caches its
    accumulator weakly, so a node nobody else holds is gone once we drop it -- a tag we leave on it tells the two cases apart."""
    for p in params:
        get_gradient_edge(p).node.metadata["phc_probe"] = True
    return any("phc_probe" in get_gradient_edge(p).node.metadata for p in params)


class CapturedUpdate:
    def __init__(self, agent):
        self.agent = agent
        self.data = None       # the epoch's dataset behind fixed addresses (_refresh_dataset)
        self.idx = None        # [minibatch] row index of the step that is replayed next
        self.acc = None        # sum of the steps' scalars over the epoch ...
        self.keys = None       # ... None: in the layout of the agent's `_raw` vector; a list: one entry per key of the step's info dict
        self.step = None       # optimizer step count on the device (graphs with clip + Adam inside)
        # one step is either ONE graph (one stream) or three linear ones: (policy pass, discriminator pass captured on its stream, tail)
        self.graph = self.passes = None
        self.key = None        # _opt_key() the graphs were captured under

    @property
    def num_graphs(self):
        """How many graphs one optimizer step replays: 0 (nothing captured yet), 1 or 3."""
        return 3 if self.passes is not None else int(self.graph is not None)

    def _opt_key(self):
        """What a graph with the optimizer step inside has baked in: a change (checkpoint with another lr, ...) forces a re-capture.
        First entry: are clip + Adam inside the graphs (one rank: no collective between backward and optimizer)?"""
        ag = self.agent
        g = ag.optimizer.param_groups[0]
        return (not (ag._reduces or bool(os.environ.get("PHC_NO_OPT_IN_GRAPH"))), float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"]),
                ag.grad_norm if ag.truncate_grads else None)

    def _refresh_dataset(self):
        """The dataset of this epoch behind fixed addresses (a captured graph keeps reading the same buffers)."""
        dataset = self.agent.dataset
        if self.data is None:
            # the tensors of the first graphed epoch BECOME the persistent buffers (the dict keeps them alive): rollout-buffer views
            # keep their address from epoch to epoch and are never copied, per-epoch temporaries are copied into these
            self.data, seen = {}, set()
            for k, v in dataset.items():   # (two keys may share one tensor: the replay batch IS the agent batch while the buffer is empty)
                self.data[k] = v.clone() if v.data_ptr() in seen else v
                seen.add(v.data_ptr())
        for k, v in dataset.items():
            g = self.data[k]
            if g.shape != v.shape:
                raise RuntimeError("dataset shape changed under a captured update graph")
            if g.data_ptr() != v.data_ptr():
                g.copy_(v)

    def _fold(self, info):
        """The step's scalars into the epoch's accumulator, one launch: the raw vector of the fused kernels (`info` None, see
        IMAmpAgent._raw_buffer), or the entries of the step's info dict."""
        if info is None:
            raw = self.agent._raw
            self.keys = None
            if self.acc.numel() != raw.numel():
                self.acc = torch.zeros_like(raw)
            self.acc += raw
            return
        self.keys = list(info)
        self.acc += torch.stack([info[k].float().reshape(()) for k in self.keys])

    def _step_body(self):
        """Forward + backward of one step and its scalars: a warm-up pass, and what the one-graph shape records."""
        minibatch = {"_dataset": self.data, "_idx": self.idx, "_amp_idx": self.idx[:self.agent._amp_minibatch_size]}
        self._fold(self.agent._fwd_bwd(minibatch, want_info=False)[0])

    def _capture(self, fuse_opt):
        ag = self.agent
        if stale_grad_accumulators(ag.grads.params):
            raise RuntimeError("an autograd graph outside the update holds a parameter's gradient accumulator (e.g. `p.clone()` kept "
                               "alive: use `p.detach().clone()`); stream capture would crash")
        self.idx.copy_(ag._idx_buf[:ag.minibatch_size])
        # the warm-up passes torch asks for before a capture must not train: they only touch the gradients (zeroed by every step)
        # and the normaliser statistics, which are restored afterwards; they issue no collective (want_info=False)
        norms = [(m, [b.clone() for b in m.buffers()]) for m in ag._norms()]
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._step_body()
            torch.cuda.current_stream().wait_stream(side)
            # with a process group alive its watchdog thread polls events while we capture: thread-local capture mode keeps
            # those calls from invalidating the capture (the graph itself holds no collective)
            in_group = ag.dist is not None and ag.dist.is_initialized()
            if in_group:   # nothing of the group may be in flight on this device while the capture starts
                torch.cuda.synchronize()
                ag.dist.barrier()
                torch.cuda.synchronize()
            if fuse_opt and self.step is None:
                self.step = torch.zeros((), dtype=torch.int64, device=ag.device)
            mode = "thread_local" if in_group else "global"
            g = torch.cuda.CUDAGraph()
            br = ag._branch_streams() if ag._fused_disc else None
            if br is not None:
                # three LINEAR graphs per step: the policy pass, the discriminator pass captured ON its stream, and the tail (scalars,
                # clip + Adam).  One graph with the passes as branches was measured first: a graph with a fork is enqueued node by node by
                # the host (286 vs 40 us per replay in scripts/probes/graph_branch_concurrency.py) in topological order, and the device
                # ran the chains mostly one after the other (profiles/r04_ppo/README.md)
                gd, gt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode=mode):
                    ag._policy_pass(self.data, self.idx)
                with torch.cuda.graph(gd, stream=br, capture_error_mode=mode):
                    ag._disc_pass(self.data, self.idx[:ag._amp_minibatch_size])
                with torch.cuda.graph(gt, capture_error_mode=mode):
                    self._fold(None)
                    if fuse_opt:
                        ag._clip_and_step(step_device=self.step)
                self.passes = (g, gd, gt)
            else:
                with torch.cuda.graph(g, capture_error_mode=mode):
                    self._step_body()
                    if fuse_opt:
                        ag._clip_and_step(step_device=self.step)
                self.graph = g
        finally:
            for m, bufs in norms:
                for b, k in zip(m.buffers(), bufs):
                    b.copy_(k)

    def run_epoch(self):
        """All mini-epochs of one epoch through the captured step; returns the mean info dict (device tensors).
        One rank (no collective between backward and optimizer): the clip + Adam launches are part of the captured step as well -- a step is
        then the row-index copy and ONE replay, which takes the host out of the loop (on a freshly started box the eager launches between
        the replays cost ~10 % of the update: 69 vs 62 ms)."""
        ag = self.agent
        ag.set_train()
        self._refresh_dataset()
        key = self._opt_key()
        if self.key != key:
            self.graph = self.passes = None
        fuse_opt = key[0]
        adam_state(ag.optimizer, ag.grads.flat_param)      # exists before any capture
        _workspace("adam", L.load().phc_adam_workspace(), ag.grads.flat_param.device, torch.float64)
        if self.idx is None:
            self.idx = torch.zeros(ag.minibatch_size, dtype=torch.int64, device=ag.device)
            self.acc = torch.zeros(len(ag.INFO_KEYS), dtype=torch.float32, device=ag.device)
        if not self.num_graphs:
            self._capture(fuse_opt)
            self.key = key
        self.acc.zero_()
        st = ag.optimizer.state[ag.grads.flat_param]
        if fuse_opt:   # the device step count follows the optimizer's (checkpoint restores, eager steps in between)
            self.step.fill_(int(st["step"].item()))
        n = 0
        for _ in range(ag.mini_epochs_num):
            for i in range(ag.num_minibatches):
                ag._draw_rows(i, out=self.idx)
                split = False
                if self.passes is not None:
                    gp, gd, gt = self.passes
                    main, sd = torch.cuda.current_stream(ag.device), ag._branches
                    split = (not fuse_opt) and ag._split_active()
                    sd.wait_stream(main)
                    with torch.cuda.stream(sd):
                        gd.replay()
                        if split:
                            ag._grad_all_reduce("disc")
                    gp.replay()
                    if split:
                        ag._grad_all_reduce("policy")
                    main.wait_stream(sd)
                    gt.replay()
                else:
                    self.graph.replay()
                if not fuse_opt:
                    if not split:
                        ag._grad_all_reduce()
                    ag._clip_and_step()
                if ag._trace is not None and self.keys is None:
                    inf = ag._info_from_raw(ag._raw.clone())
                    ag._trace.append(torch.stack([inf[k] for k in ag.INFO_KEYS]))
                n += 1
        if fuse_opt:
            st["step"] += n
        mean = self.acc / n
        if self.keys is None:
            return ag._info_from_raw(mean)
        return {k: mean[j] for j, k in enumerate(self.keys)}
