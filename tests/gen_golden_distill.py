"""TEST INFRASTRUCTURE -- golden for `collect_dataset=True`: what the reference's OWN player records and dumps.

Run where the reference checkout is available (oracle/ref_shim.py finds it):  python tests/gen_golden_distill.py   -> tests/golden/distill_sweep.npz

`IMAMPPlayerContinuous._post_step` (phc/learning/im_amp_players.py:67-242) runs on a `__new__`-made player whose `env.task` is a scripted stand-in (modelled on
oracle/gen_golden_eval.py): U = 10 clips, N = 4 envs -- three batches, the last one wrapping around --, a script of terminate flags in which EVERY env of the
second batch fails (that batch stops early), and per-step `info` dicts that also carry `obs_buf` / `clean_actions` / `actions` / `reset_buf` with recognisable
values (`scripted_rows`).  The module's `joblib.dump` and `exit` are replaced by a recorder, so the fixture holds what the player would have written: per-clip
lengths, the concatenated arrays, `key_names`, `motion_lengths` and the dtype of `reset`.  tests/test_distill_cpu.py drives `phc_amd.learning.im_eval.evaluate`
with the same script (it imports `make_script`, `terminate_flags` and `scripted_rows` from here) and compares exactly."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U, N, OBS, ACT = 10, 4, 3, 2


def make_script(seed=214):
    rng = np.random.default_rng(seed)
    num_steps = np.sort(rng.integers(6, 15, U))[::-1].copy()          # the eval library is sorted by length, longest first
    fail_at = {1: 3, 4: 2, 5: 3, 6: 1, 7: 4, 9: 1}                     # clip -> step at which it terminates early; clips 4..7 are the whole second batch
    late = {2: int(num_steps[2])}                                      # a terminate flag at the last frame: not a failure
    return dict(num_steps=num_steps.astype(np.int32), fail_clips=np.array(sorted(fail_at)), fail_steps=np.array([fail_at[k] for k in sorted(fail_at)]),
                late_clips=np.array(sorted(late)), late_steps=np.array([late[k] for k in sorted(late)]))


def terminate_flags(script, ids, step):
    t = np.zeros(len(ids), dtype=bool)
    for c, s in zip(script["fail_clips"], script["fail_steps"]):
        t |= (ids == c) & (step == s)
    for c, s in zip(script["late_clips"], script["late_steps"]):
        t |= (ids == c) & (step == s)
    return t


def scripted_rows(batch, step, term):
    """What the task holds around env step `step` of batch `batch`: (observation BEFORE the step [N, OBS], clean actions [N, ACT], noisy actions [N, ACT],
    reset_buf after the step [N] int64) -- 1000 batch + 10 step + env, told apart by sign, offset and column."""
    base = 1000.0 * batch + 10.0 * step + np.arange(N, dtype=np.float64)
    obs = (base[:, None] + 0.125 * np.arange(OBS)[None]).astype(np.float32)
    clean = (-base[:, None] - 0.25 * np.arange(ACT)[None]).astype(np.float32)
    act = (clean + 0.5).astype(np.float32)
    return obs, clean, act, np.asarray(term).astype(np.int64)


def main():
    import tempfile

    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import ref_shim
    ref_shim.install()
    # learning/common_player.py:210 also subclasses the discrete player, which the stub of rl_games does not carry: a base class of that name, nothing more
    import rl_games.algos_torch.players as stub_players
    if not hasattr(stub_players, "PpoPlayerDiscrete"):
        stub_players.PpoPlayerDiscrete = type("PpoPlayerDiscrete", (stub_players.PpoPlayerContinuous.__mro__[1],), {})
    pl = ref_shim.ref_module("phc.learning.im_amp_players")
    script = make_script()

    class Lib:
        def __init__(self):
            self._num_unique_motions = U
            self._motion_data_keys = np.array([f"clip_{i:02d}" for i in range(U)])
            self.load(0)

        def load(self, start_idx):
            self._curr_motion_ids = torch.remainder(torch.arange(N) + start_idx, U)      # motion_lib_base.py:210
            self._steps = torch.from_numpy(script["num_steps"][self._curr_motion_ids.numpy()].astype(np.int32))
            self.curr_motion_keys = self._motion_data_keys[self._curr_motion_ids.numpy()]

        def get_motion_num_steps(self, motion_ids=None):
            return self._steps

    lib = Lib()
    tmp = tempfile.mkdtemp()
    cfg = types.SimpleNamespace(env=types.SimpleNamespace(motion_file="data/amass/scripted_clips.pkl"))
    task = types.SimpleNamespace(_motion_lib=lib, num_envs=N, start_idx=0, collect_dataset=True, add_action_noise=True, action_noise_std=0.05, cfg=cfg, viewer=None)

    def forward_motion_samples():
        task.start_idx += N
        lib.load(task.start_idx)
    task.forward_motion_samples = forward_motion_samples

    dumped = {}

    class Done(Exception):
        pass

    def fake_dump(obj, path, **kw):
        if isinstance(obj, dict) and "clean_action" in obj:
            dumped.update(obj, path=path)

    def fake_exit(*a):
        raise Done
    pl.joblib = types.SimpleNamespace(dump=fake_dump)
    pl.exit = fake_exit
    pl.compute_metrics_lite = lambda pred, gt: {}
    pl.flags.im_eval, pl.flags.real_traj = True, False

    player = pl.IMAMPPlayerContinuous.__new__(pl.IMAMPPlayerContinuous)
    # the members IMAMPPlayerContinuous.__init__ makes (im_amp_players.py:29-50), restated: the constructor needs a built env and network
    player.env = types.SimpleNamespace(task=task)
    player.device = "cpu"
    player.config = {"network_path": tmp}
    player.terminate_state = torch.zeros(N)
    player.terminate_memory = []
    player.mpjpe, player.mpjpe_all = [], []
    player.gt_pos, player.gt_pos_all = [], []
    player.pred_pos, player.pred_pos_all = [], []
    player.curr_stpes = 0
    player.obs_buf, player.obs_buf_all = [], []
    player.env_actions, player.actions_all = [], []
    player.motion_length_all = []
    player.clean_actions, player.clean_actions_all = [], []
    player.keys_all = []
    player.reset_buf, player.reset_buf_all = [], []
    player.success_rate = 0
    player.pbar = types.SimpleNamespace(update=lambda *a: None, refresh=lambda: None, clear=lambda: None, set_description=lambda s: None)
    player.running_mean_std = types.SimpleNamespace(state_dict=lambda: {})
    steps_per_batch, batch, step = [], 0, 0
    try:
        while True:
            ids = lib._curr_motion_ids.numpy()
            term = terminate_flags(script, ids, step)
            obs, clean, act, reset = scripted_rows(batch, step, term)
            info = {"terminate": torch.from_numpy(term), "mpjpe": torch.zeros(N), "body_pos": np.zeros((N, 2, 3), np.float32), "body_pos_gt": np.zeros((N, 2, 3), np.float32),
                    "obs_buf": obs, "clean_actions": clean, "actions": act, "reset_buf": reset}
            done = player._post_step(info, torch.zeros(N, dtype=torch.long))
            step += 1
            if int(done.sum()) == N:
                steps_per_batch.append(step)
                batch, step = batch + 1, 0
    except Done:
        steps_per_batch.append(step + 1)
    assert dumped, "the player never dumped"
    lengths = np.array([len(o) for o in dumped["obs"]])
    assert list(lengths) == list(dumped["motion_lengths"])
    name = os.path.basename(dumped["path"]).split("_")
    out = {"script/" + k: v for k, v in script.items()}
    out.update(U=np.array(U), N=np.array(N), steps_per_batch=np.array(steps_per_batch), lengths=lengths, obs=np.concatenate(dumped["obs"]),
               clean_action=np.concatenate(dumped["clean_action"]), env_action=np.concatenate(dumped["env_action"]), reset=dumped["reset"],
               reset_dtype=np.array(str(dumped["reset"].dtype)), key_names=np.array([str(k) for k in dumped["key_names"]]), motion_lengths=dumped["motion_lengths"],
               dump_keys=np.array(sorted(k for k in dumped if k != "path")), file_name_fields=np.array(name[:3]),
               dump_dir=np.array(os.path.relpath(os.path.dirname(dumped["path"]), tmp)))
    np.savez_compressed(os.path.join(HERE, "golden", "distill_sweep.npz"), **out)
    print("steps per batch", steps_per_batch, "lengths", lengths.tolist(), "rows", len(out["obs"]), "reset dtype", out["reset_dtype"])


if __name__ == "__main__":
    main()
