"""HumanoidImDemo / HumanoidImMCPDemo: the humanoid tracks keypoints that are NOT in the motion library -- a pose estimator's output, a text-to-motion model,
a VR rig -- one frame [N, NB, 3] per env step (reference: phc/env/tasks/humanoid_im_demo.py, phc/env/tasks/humanoid_im_mcp_demo.py:252-321).

The reference polls an HTTP server for the frame and processes it on the host (numpy, scipy, torch).  Here the frame comes from `task.set_keypoints(j3d)` or
from a `stream.file` / `stream.motion` source (phc_amd/stream.py), and the per-step work -- joint order, root-relative limb normalisation, the causal gaussian
filters over the last `stream.window` frames, the frame rotation, the finite-difference velocity, the zero_out_far gating, the obs_v 7 task observation and
"never reset" (:319-321) -- is ONE launch per env step, phc_stream_track (include/phc_amd.h), issued right behind phc_im_post_physics through HumanoidIm's
`_post_physics_launch` hook.  It rewrites the task block of `obs_buf`, `ref_body_pos` / `ref_body_vel` (what the renderer's markers show) and the reset flags;
`post_physics_step`, `step` and `pre_physics_step` are not overridden.  After every reset launch the same entry point runs in its `observe` mode, so a reset
env's observation refers to the stream (the reference's `_compute_observations(env_ids)`).  The motion library stays what resets draw the initial pose from.

One deliberate difference: the first velocity of a stream is 0 (the reference's `prev_ref_body_pos` starts at zero: its first velocity is position / dt).

Not built (refused by name): env.obs_v other than 7 (the reference's v6 branch raises), env.fut_tracks, env.occl_training, env.cycle_motion; rotations in the
stream; the websocket / HTTP client."""
import torch

from ... import _lib as L
from ... import abi
from ... import stream as S
from ...utils.synthetic_motion import BASE_ROT, motion_from_spec
from .humanoid_im import HumanoidIm, _stream
from .humanoid_im_mcp import MCPMixin


class StreamMixin:
    """Shared by HumanoidImDemo and HumanoidImMCPDemo; in front of HumanoidIm in the class order."""
    _use_reset_list = False            # nothing finishes: reset_done() sweeps reset_buf, which the launch keeps at zero
    _default_close_distance = 0.25

    # ---- host phases: refusals and options ----
    def _load_humanoid_configs(self):
        env = self.cfg["env"]
        name = type(self).__name__
        if int(env.get("obs_v", 6)) != 7:
            raise NotImplementedError(f"env.obs_v={env.get('obs_v', 6)} with {name}: the keypoint stream is built for obs_v=7 (the reference's v6 branch raises, "
                                      "humanoid_im_mcp_demo.py:177-178)")
        for key, why in (("fut_tracks", "a stream has no future frames"), ("occl_training", "the occlusion mask is applied by the post-physics launch only"),
                         ("cycle_motion", "there is no clip to restart")):
            if env.get(key, False):
                raise NotImplementedError(f"env.{key}=True with {name}: {why}")
        super()._load_humanoid_configs()
        self.close_distance = env.get("close_distance", self._default_close_distance)

    def _setup_im_options(self):
        super()._setup_im_options()
        self._stream_opts = S.parse_options(self.cfg.get("stream", None), is_smpl=not self._is_robot, num_bodies=len(self._body_names),
                                            parents=self.model.parent, task_dt=self.dt)

    # ---- device phase ----
    def _allocate_im_state(self):
        super()._allocate_im_state()
        o, N, NB, dev = self._stream_opts, self.num_envs, self.num_bodies, self.device
        f32 = dict(device=dev, dtype=torch.float32)
        # phc_im_post_physics and the reset launches store the motion library's reference: they keep private tensors, the public ones are the stream's
        self._ref_body_pos_im, self._ref_body_vel_im = self.ref_body_pos, self.ref_body_vel
        self.ref_body_pos, self.ref_body_vel = torch.zeros((N, NB, 3), **f32), torch.zeros((N, NB, 3), **f32)
        W = o["window"]
        self._stream_ring_body = torch.zeros((N, W, NB, 3), **f32)
        self._stream_ring_root = torch.zeros((N, W, 3), **f32)
        self._stream_head = torch.zeros(N, device=dev, dtype=torch.int32)
        self._stream_count = torch.zeros(N, device=dev, dtype=torch.int32)
        self._stream_has_prev = torch.zeros(N, device=dev, dtype=torch.uint8)
        self._stream_err = torch.zeros(N, **f32)
        self._stream_stage = {N: torch.zeros((N, NB, 3), **f32), 1: torch.zeros((1, NB, 3), **f32)}   # set_keypoints copies into one of the two
        self._stream_cur = None          # the staged frame: one of the staging buffers, or the source's tensor of this step
        self._stream_fold = torch.from_numpy(S.fold_table(o["root_sigma"], o["body_sigma"], W)).to(dev)
        self._stream_perm = None if o["perm"] is None else torch.from_numpy(o["perm"]).to(dev)
        self._stream_source = None
        self._stream_args = None

    def _load_motion(self, motion_train_file, motion_test_file=[]):
        super()._load_motion(motion_train_file, motion_test_file)
        o = self._stream_opts
        if o["file"] is not None:
            self._stream_source = S.KeypointSource.from_file(o["file"], self.num_envs, self.num_bodies, self.device, loop=o["loop"])
        elif o["motion"] is not None:
            self._stream_source = S.KeypointSource.from_motion_lib(self._stream_motion_lib(o["motion"]), self.num_envs, self.dt, self.device, loop=o["loop"])

    def _stream_motion_lib(self, spec):
        """A motion library of the task's own kind over `spec` (any env.motion_file value), clip e for env e in the spec's order."""
        from ...config import EasyDict
        cfg = EasyDict(dict(self._motion_train_lib.m_cfg))
        cfg.motion_file = motion_from_spec(spec, self.model, self._is_robot, self._robot_consts["default_dof_pos"] if self._is_robot else None,
                                           num_extend=self.num_extend_bodies, min_frames=30, base_rot=None if self._has_upright_start else BASE_ROT)
        lib = self._motion_lib_cls(cfg)
        lib.load_motions(skeleton_trees=self.skeleton_trees, gender_betas=self.humanoid_shapes.cpu(), limb_weights=self.humanoid_limb_and_weights.cpu(),
                         random_sample=False, start_idx=0)
        return lib

    def _buffer_tensors(self):
        return super()._buffer_tensors() + (self.__dict__.get("_ref_body_pos_im"), self.__dict__.get("_ref_body_vel_im"))

    def _buffers_uncached(self, amp_in, amp_out):
        b = super()._buffers_uncached(amp_in, amp_out)
        b.ref_body_pos, b.ref_body_vel = self._ref_body_pos_im.data_ptr(), self._ref_body_vel_im.data_ptr()
        return b

    # ---- the stream ----
    def set_keypoints(self, j3d):
        """Stage one frame of keypoints: [N, NB, 3] or [1, NB, 3] (every env the same), a tensor on any device or numpy, in the order and frame the `stream`
        options name.  Every following step consumes it until it is replaced (the reference re-polls its server)."""
        if self._stream_source is not None:
            raise ValueError("set_keypoints on a task with a stream.file / stream.motion source: the source stages a frame in every step")
        x = torch.as_tensor(j3d)
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[0] not in (1, self.num_envs) or tuple(x.shape[1:]) != (self.num_bodies, 3):
            raise ValueError(f"set_keypoints takes [{self.num_envs}, {self.num_bodies}, 3] or [1, {self.num_bodies}, 3], not {tuple(x.shape)}")
        stage = self._stream_stage[int(x.shape[0])]
        stage.copy_(x.to(device=self.device, dtype=torch.float32))
        self._stream_cur = stage

    def restart_stream(self, env_ids=None):
        """Empty the rings of `env_ids` (default: all) and forget their previous frame: their next frame has velocity 0 and is its own filtered value."""
        if env_ids is None:
            self._stream_head.zero_(); self._stream_count.zero_(); self._stream_has_prev.zero_()
            return
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.long)
        self._stream_head[ids] = 0
        self._stream_count[ids] = 0
        self._stream_has_prev[ids] = 0

    def _stream_struct(self):
        """phc_stream_args_t of this task; rebuilt when a tensor it points at was rebound (the staged frame and the mode are set per launch)."""
        tensors = (self._stream_ring_body, self._stream_ring_root, self._stream_head, self._stream_count, self._stream_has_prev, self.ref_body_pos,
                   self.ref_body_vel, self._rigid_body_state, self.obs_buf, self.reset_buf, self._terminate_buf, self._stream_err, self._stream_fold,
                   self._stream_perm)
        hit = self._stream_args
        if hit is None or any(a is not b for a, b in zip(hit[1], tensors)):
            o = self._stream_opts
            args = abi.stream_args_struct(
                self.num_envs, o["window"], self._stream_fold, None, limb_pairs=o["limb_pairs"], limb_lengths=o["limb_lengths"], limb_scale=o["limb_scale"],
                frame_mat=o["frame_mat"], dt=o["dt"], close_distance=self.close_distance, far_distance=self.far_distance,
                track_root_body=self._body_names.index(self._track_bodies[0]), perm=self._stream_perm, ring_body=self._stream_ring_body,
                ring_root=self._stream_ring_root, head=self._stream_head, count=self._stream_count, has_prev=self._stream_has_prev, cur_ref=self.ref_body_pos,
                cur_vel=self.ref_body_vel, rigid_body_state=self._rigid_body_state, obs_buf=self.obs_buf, reset_buf=self.reset_buf,
                terminate_buf=self._terminate_buf, track_err=self._stream_err)
            hit = self._stream_args = (args, tensors)
        return hit[0]

    def _stream_launch(self, mode):
        a = self._stream_struct()
        a.mode = mode
        f = self._stream_cur
        if mode == L.STREAM_ADVANCE:
            if f is None:
                raise RuntimeError(f"{type(self).__name__}: no keypoints staged: call set_keypoints(j3d) before the first step, or configure +stream.file / +stream.motion")
            if f.dtype != torch.float32 or not f.is_contiguous() or f.shape[0] not in (1, self.num_envs) or tuple(f.shape[1:]) != (self.num_bodies, 3):
                raise ValueError(f"the stream's frame must be contiguous fp32 [{self.num_envs} or 1, {self.num_bodies}, 3], not {tuple(f.shape)}")
        a.frames, a.frame_rows = (None, 0) if f is None else (f.data_ptr(), int(f.shape[0]))
        L.check(self._lib.phc_stream_track(self._model_struct, self._im_params, a, _stream()), "phc_stream_track")

    def _post_physics_launch(self):
        """HumanoidIm.post_physics_step's hook, right behind phc_im_post_physics on its stream."""
        if self._stream_source is not None:
            self._stream_cur = self._stream_source.next()   # (kept until the next step: the launch reads it)
        self._stream_launch(L.STREAM_ADVANCE)
        self.extras["stream_err"] = self._stream_err

    def _reset_envs(self, env_ids):
        super()._reset_envs(env_ids)
        if len(env_ids):
            self._stream_launch(L.STREAM_OBSERVE)

    def reset_done(self):
        super().reset_done()
        self._stream_launch(L.STREAM_OBSERVE)


class HumanoidImDemo(StreamMixin, HumanoidIm):
    pass


class HumanoidImMCPDemo(StreamMixin, MCPMixin, HumanoidIm):
    _default_close_distance = 0.5      # humanoid_im_mcp_demo.py:65
