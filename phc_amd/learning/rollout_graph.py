"""The rollout steps of an epoch as replayed hipGraphs (`hip_graph`; IMAmpAgent.play_steps asks `CapturedRollout` which regime runs).

What is captured is the agent's own step: `_rollout_step` with its segments `_rollout_policy` and `_rollout_after`.  This class owns the graphs, their memory
pool, the task's launch generation they were captured under, and the rules that say which regime a rollout runs in."""
import gc
import os

import numpy as np
import torch

# scripts/profile_rollout.py: the rollout is HOST-bound (32 steps: 16.0 ms of launch / Python time for ~9.6 ms of device work).  Two shapes of graph:
# * segment graphs: the two policy segments of every rollout step -- (A) normalise + actor + critic + sampling into row n of the experience
#   buffer, (B) the copies of the step's outputs, the next-value critic and the episode bookkeeping -- are captured once per row n (their
#   inputs are the task's static buffers, their outputs rows of the persistent experience buffer) and replayed; the env itself (reset of
#   finished envs, stepper, post-physics) keeps its three eager launches, since its host side carries state (RNG counter, reset lists).
# * ONE hipGraph per rollout step (round 3): reset of the finished envs, observation row, actor / critic / sampling, stepper, post-physics, AMP
#   window copy, next-value critic and bookkeeping -- ~40 launches -- replayed with a single host call; the task's host-side state (AMP
#   window position, reset-list slot, info dict) is advanced by task.replay_step_host().  Keyed by the step index and that state; the
#   start-time draws of the captured reset launch stay fresh through the device-side call counter (phc_im_buffers_t.reset_rng_counter).


def call_segment(kind, pins, fn, *args):
    """Run a rollout segment with eager launches (or inside the capture of a whole step): the counterpart of `CapturedRollout.segment`."""
    fn(*args)


class CapturedRollout:
    def __init__(self, agent):
        self.agent = agent
        self.graphs = {}           # hipGraphs by key: ("policy", n, obs ptr), ("after", n, ...five ptrs), ("step", n) + task.rollout_step_key()
        self.pool = None           # their shared memory pool
        self.generation = None     # the task's launch_generation() they hold

    def follow(self, task):
        """Before every rollout: drop what was captured under another launch generation of the task."""
        # captured env launches hold the motion library, the parameter struct and the AMP reference table by value / raw pointer: when the task
        # says any of them moved (resample_motions(), evaluate() swapping libraries, flipped evaluation flags), every captured graph is dropped and
        # re-captured against the new objects (tests/test_env_gpu.py::test_rollout_graphs_follow_resample_motions_and_evaluate)
        gen = task.launch_generation() if hasattr(task, "launch_generation") else None
        if gen != self.generation:
            if self.graphs:
                torch.cuda.synchronize()
                self.graphs.clear()
                # ... and their memory pool with them (round 5): with every graph of the pool destroyed its use count is zero, and capturing into the
                # same pool id again trips `use_count > 0` in HIPCachingAllocator unless empty_cache() could free the whole pool -- it cannot while any
                # tensor allocated during a capture is still referenced (robots: a Unitree H1 run crashed at epoch 101, its first resample_motions())
                self.pool = None
            self.generation = gen

    def enabled(self):
        """May this rollout replay graphs at all (segments or whole steps)?"""
        ag = self.agent
        return (ag.exp["obses"].is_cuda and ag._use_graph and not ag._graph_failed and ag.epoch_num >= 2 and not ag.faithful_reset
                and hasattr(ag.task, "reset_done") and not np.isfinite(ag.vec_env.clip_obs) and not os.environ.get("PHC_NO_GRAPH")
                and not os.environ.get("PHC_NO_ROLLOUT_GRAPH"))

    def whole_steps(self):
        """... and whole steps?  Not in the first rollout: it creates the reward accumulator, which a captured step needs to exist."""
        ag = self.agent
        return (self.enabled() and ag._reward_raw_acc is not None and getattr(ag.task, "whole_step_capturable", lambda: False)()
                and not os.environ.get("PHC_NO_STEP_GRAPH"))

    def replay(self, key, fn, *args):
        """Replay the graph `key`; on first use `fn(*args)` is captured into it."""
        g = self.graphs.get(key)
        if g is None:
            in_group = self.agent.dist is not None and self.agent.dist.is_initialized()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            if self.pool is None:   # the rollout graphs replay one after the other and leave their results in the
                self.pool = torch.cuda.graph_pool_handle()   # persistent experience buffers: their temporaries can share one pool
            # no cyclic garbage collection inside the capture (torch no longer collects before one): an earlier agent of this process is a dead cycle
            # (agent <-> its captured update / rollout) that holds hipGraphs and their pools.  The -m gpu suite aborted once with the collector running
            # under the capture of an "after" segment, in a test that builds two agents in a row; that the collector was destroying the first agent's
            # graphs is the supposed cause, not a proven one
            collecting = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g, pool=self.pool, capture_error_mode="thread_local" if in_group else "global"):
                    fn(*args)
            finally:
                if collecting:
                    gc.enable()
            self.graphs[key] = g
        g.replay()

    def segment(self, kind, pins, fn, n, *args):
        """Segment `fn(n, *args)` of rollout step n as a graph of its own, keyed by the addresses of the tensors in `pins` (what the capture reads besides row n)."""
        self.replay((kind, n) + tuple(t.data_ptr() for t in pins), fn, n, *args)

    def play_whole_steps(self):
        """The rollout as one replay per step.  A key seen before: replay + the task's host bookkeeping; otherwise capture (which runs the task's own host
        bookkeeping), then the first replay: no bookkeeping."""
        ag, task = self.agent, self.agent.task
        task.align_amp_window()
        for n in range(ag.horizon_length):
            key = ("step", n) + task.rollout_step_key()
            g = self.graphs.get(key)
            if g is not None:
                g.replay()
                task.replay_step_host(reset=n > 0)
            else:
                self.replay(key, ag._rollout_step, n, call_segment)
        ag.obs, ag.dones = task.obs_buf, task.reset_buf
