"""Distilling a composed controller into one MLP (phc_amd/distill.py, learning/dataset_record.py, csrc/phc_distill.hip): everything that runs without a GPU.

  * the C ABI is extended, not changed (five symbols, phc_record_args_t, version 37);
  * `collect_dataset=True` in the evaluation sweep records exactly what the reference's own player records (tests/gen_golden_distill.py);
  * the trainer's bookkeeping against a plain torch loop written here; checkpoints, resume, standardise + clamp;
  * the float64 oracles of the kernels (tests/distill_oracle.py) on hand-computable cases;
  * merge and the `sample_pkl` file selection; the student wrapper and the refusals."""
import ctypes as C
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import distill_oracle as do
import distill_util as du
import gen_golden_distill as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("phc_dataset_record", "phc_silu_bf16", "phc_colsum_silu_bf16", "phc_mse_loss_workspace", "phc_mse_loss")


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def test_abi_is_extended_not_changed():
    from phc_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "phc_amd.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(phc_\w+)\s*\(", txt, flags=re.M))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.phc_abi_version() == 37
    body = re.search(r"typedef struct \{([^}]*)\} phc_record_args_t;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert fields == [n for n, _ in L.RecordArgs._fields_]
    # 4 x int32, int64, 11 pointers: no padding
    assert C.sizeof(L.RecordArgs) == 16 + 8 + 11 * C.sizeof(C.c_void_p)
    assert lib.phc_mse_loss_workspace() > 0
    assert lib.phc_dataset_record(None, None) == -1       # PHC_EINVAL before any device work
    assert lib.phc_mse_loss(None, 0, None, None, 1, 1, None, None, None, None) == -1
    assert lib.phc_silu_bf16(None, 1, 1, None, None) == -1
    assert lib.phc_colsum_silu_bf16(None, None, 1, 1, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. the reference's recording loop
class _ScriptedLib:
    def __init__(self, script):
        self.script, self._num_unique_motions = script, gg.U
        self._motion_data_keys = np.array([f"clip_{i:02d}" for i in range(gg.U)])
        self.load(0)

    def load(self, start_idx):
        self._curr_motion_ids = torch.remainder(torch.arange(gg.N) + start_idx, gg.U)
        self._steps = torch.from_numpy(self.script["num_steps"][self._curr_motion_ids.numpy()].astype(np.int32))
        self.curr_motion_keys = self._motion_data_keys[self._curr_motion_ids.numpy()]

    def get_motion_num_steps(self, motion_ids=None):
        return self._steps


def _scripted_agent(script, dist=None, collect=True):
    from phc_amd.motion_lib import MotionLibBase
    U, n = gg.U, gg.N
    lib = _ScriptedLib(script)
    train = MotionLibBase.__new__(MotionLibBase)
    train._motion_data_keys, train._num_unique_motions, train._device = lib._motion_data_keys, U, torch.device("cpu")
    train._termination_history, train._sampling_prob = torch.zeros(U), torch.ones(U) / U
    state = dict(step=0, steps_per_batch={})
    cfg = {"env": {"motion_file": "data/amass/scripted_clips.pkl"}}
    task = types.SimpleNamespace(_motion_lib=train, num_envs=n, start_idx=0, device=torch.device("cpu"), _termination_distances=torch.full((24,), 0.25),
                                 auto_pmcp=False, auto_pmcp_soft=False, get_eval_motion_lib=lambda: lib, reset=lambda: None, collect_dataset=collect, cfg=cfg,
                                 _add_action_noise=True, _action_noise_std=0.05, num_actions=gg.ACT)

    def hold(b, s):   # the observation the task holds BEFORE step s
        task.obs_buf = torch.from_numpy(gg.scripted_rows(b, s, np.zeros(n, bool))[0])

    def begin():
        task.start_idx, state["step"] = 0, 0
        lib.load(0)

    def forward():
        task.start_idx += n
        state["step"] = 0
        lib.load(task.start_idx)
    task.begin_seq_motion_samples, task.forward_motion_samples = begin, forward

    def reset():
        hold(task.start_idx // n, 0)
        return task.obs_buf

    def step(actions):
        b, s, ids = task.start_idx // n, state["step"], lib._curr_motion_ids.numpy()
        term = gg.terminate_flags(script, ids, s)
        _, clean, act, rs = gg.scripted_rows(b, s, term)
        task.clean_actions, task.actions, task.reset_buf = torch.from_numpy(clean), torch.from_numpy(act), torch.from_numpy(rs)
        hold(b, s + 1)
        info = {"terminate": torch.from_numpy(term).long(), "body_pos": np.zeros((n, 2, 3), np.float32), "body_pos_gt": np.zeros((n, 2, 3), np.float32)}
        state["step"] += 1
        state["steps_per_batch"][b] = state["step"]
        return task.obs_buf, torch.zeros(n), task.reset_buf, info
    env = types.SimpleNamespace(reset=reset, step=step)
    rms = types.SimpleNamespace(state_dict=lambda: {"running_mean": torch.zeros(gg.OBS, dtype=torch.float64), "running_var": torch.ones(gg.OBS, dtype=torch.float64)})
    agent = types.SimpleNamespace(task=task, vec_env=env, set_eval=lambda: None, get_action_values=lambda obs: {"mus": torch.zeros(n, 2)},
                                  preprocess_actions=lambda a: a, epoch_num=7, rank=0, dist=dist, running_mean_std=rms)
    return agent, state


def test_sweep_records_what_the_reference_player_records(golden, tmp_path):
    """`im_eval.evaluate` with `collect_dataset` (the recorder's torch statement, CPU) against `IMAMPPlayerContinuous._post_step` of the reference run on the same
    script: the same rows of the same clips in the same order -- wrapped-around duplicates of the last batch and the early-stopped second batch included --,
    the same key names, lengths, dtype of `reset`, dump keys and file-name pattern.  Exact."""
    import joblib
    from phc_amd.learning import im_eval
    g = golden("distill_sweep")
    script = gg.make_script()
    for k, v in script.items():
        assert np.array_equal(v, g["script/" + k])
    agent, state = _scripted_agent(script)
    im_eval.evaluate(agent, output_dir=str(tmp_path), log=None)
    assert [state["steps_per_batch"][b] for b in sorted(state["steps_per_batch"])] == list(g["steps_per_batch"])
    files = sorted((tmp_path / str(g["dump_dir"])).glob("*.pkl"))
    assert len(files) == 1
    assert files[0].name.split("_")[:3] == list(g["file_name_fields"]) and re.fullmatch(r"\d{4}-\d\d-\d\d-\d\d:\d\d:\d\d\.pkl", files[0].name.split("_")[3])
    d = joblib.load(files[0])
    assert sorted(d) == list(g["dump_keys"])
    assert isinstance(d["obs"], list) and [len(o) for o in d["obs"]] == list(g["lengths"]) == [len(a) for a in d["clean_action"]] == [len(a) for a in d["env_action"]]
    for k in ("obs", "clean_action", "env_action"):
        got = np.concatenate(d[k])
        assert got.dtype == g[k].dtype and np.array_equal(got, g[k]), k
    assert d["reset"].dtype == np.dtype(str(g["reset_dtype"])) and np.array_equal(d["reset"], g["reset"])
    assert list(d["key_names"]) == list(g["key_names"]) and np.array_equal(d["motion_lengths"], g["motion_lengths"])
    assert set(d["running_mean"]) == {"running_mean", "running_var"} and d["config"] == agent.task.cfg
    assert agent.last_dataset is not None


def test_sweep_without_collect_dataset_records_nothing(tmp_path):
    from phc_amd.learning import im_eval
    agent, _ = _scripted_agent(gg.make_script(), collect=False)
    im_eval.evaluate(agent, output_dir=str(tmp_path), log=None)
    assert agent.last_dataset is None and not (tmp_path / "phc_act").exists()


def test_collect_dataset_on_two_ranks_is_refused(tmp_path):
    from phc_amd.learning import im_eval
    dist = types.SimpleNamespace(is_initialized=lambda: True, get_world_size=lambda: 2, get_rank=lambda: 0)
    agent, state = _scripted_agent(gg.make_script(), dist=dist)
    td = agent.task._termination_distances.clone()
    with pytest.raises(ValueError, match="one process"):
        im_eval.evaluate(agent, output_dir=str(tmp_path), log=None)
    assert torch.equal(agent.task._termination_distances, td) and not state["steps_per_batch"]      # refused before anything changed


def test_record_rows_is_the_oracle_rule():
    """The torch statement against the loop of tests/distill_oracle.py on the GPU test's layout (rows 0, 1, 4, 2, 3 packed back to back, steps 0..4)."""
    from phc_amd.learning.dataset_record import record_rows
    g = np.random.default_rng(5)
    rows = np.array([0, 1, 4, 2, 3])
    start = np.concatenate([[0], np.cumsum(rows)[:-1]])
    R, D, A = int(rows.sum()), 7, 3
    blk_t = (torch.full((R, D), -1.0), torch.full((R, A), -1.0), torch.full((R, A), -1.0), torch.full((R,), -1, dtype=torch.int64))
    blk_n = tuple(b.numpy().copy() for b in blk_t)
    prev_t = torch.from_numpy(g.standard_normal((5, D)).astype(np.float32))
    prev_n = prev_t.numpy().copy()
    for step in range(5):
        obs, cl, ac = (g.standard_normal((5, k)).astype(np.float32) for k in (D, A, A))
        rs = g.integers(0, 2, 5)
        record_rows(step, torch.from_numpy(rows), torch.from_numpy(start), prev_t, torch.from_numpy(obs), torch.from_numpy(cl), torch.from_numpy(ac), torch.from_numpy(rs), blk_t)
        do.record(step, rows, start, prev_n, obs, cl, ac, rs, blk_n)
        assert np.array_equal(prev_t.numpy(), obs) and np.array_equal(prev_n, obs)
    for a, b in zip(blk_t, blk_n):
        assert np.array_equal(a.numpy(), b) and not (b == -1).any()


# ------------------------------------------------------------------------------------------------------------------ 3. trainer bookkeeping
ROWS, OBS, ACT, UNITS, BATCH, EPOCHS, LR = 50, 7, 3, [16, 8], 16, 3, 2e-3


def _fixture_files(tmp_path, fx):
    import joblib
    data = tmp_path / "merged.pkl"
    meta = tmp_path / "merged_metadata.pkl"
    joblib.dump({"obs": fx["obs"], "clean_action": fx["clean_action"], "env_action": fx["clean_action"], "reset": np.zeros(len(fx["obs"]), np.int64)}, data)
    joblib.dump({"running_mean": {"running_mean": fx["running_mean"], "running_var": fx["running_var"], "count": torch.ones((), dtype=torch.float64)}}, meta)
    return str(data), str(meta)


def _plain(fx, dtype, epochs=EPOCHS):
    from phc_amd import distill
    init = {k[len("model."):]: v.detach().clone() for k, v in distill.build_student(OBS, ACT, UNITS, "silu", 0).state_dict().items()}
    perms = [distill.epoch_permutation(0, e, ROWS) for e in range(epochs)]
    return do.plain_loop(fx["obs"], fx["clean_action"], fx["running_mean"], fx["running_var"], UNITS, BATCH, epochs, LR, perms, init, dtype)


def test_trainer_equals_a_plain_torch_loop(tmp_path):
    """50 rows, obs 7, actions 3, units [16, 8], batch 16 (three full batches and one of 2), 3 epochs = 12 Adam steps, on the CPU (plain torch fallback), against
    nn.Sequential / nn.SiLU / nn.MSELoss / Adam with the same permutations.  Bound in Adam steps (units of lr, as tests/test_learner_epoch.py): 4 x the deviation the
    plain loop shows between fp32 and fp64 on this fixture -- measured on the CPU here: 3.84e-5 steps (so the bound is 1.5e-4 of one step; it is re-measured by the
    test, not hard-coded).  The trainer itself differs from the fp32 plain loop by 0 steps here: same operations in the same order."""
    from phc_amd import distill
    fx = du.trainer_fixture(ROWS, OBS, ACT)
    data, meta = _fixture_files(tmp_path, fx)
    ref32, loss32 = _plain(fx, torch.float32)
    ref64, _ = _plain(fx, torch.float64)
    measured = du.adam_steps(ref32, ref64, LR)
    print(f"plain loop fp32 vs fp64: {measured:.3e} Adam steps")
    assert 0 < measured < 0.1
    tr = distill.train(data, meta, str(tmp_path / "out"), units=UNITS, batch_size=BATCH, lr=LR, epochs=EPOCHS, save_frequency=2, seed=0, device="cpu", log=None)
    got = {k[len("model."):]: v for k, v in tr.model.state_dict().items()}
    dev = du.adam_steps(got, ref64, LR)
    print(f"trainer vs fp64 plain loop: {dev:.3e} Adam steps; vs fp32 plain loop: {du.adam_steps(got, ref32, LR):.3e}")
    assert dev <= 4 * measured
    assert abs(float(tr.loss) - loss32) <= 1e-5 * abs(loss32)
    # something was learnt at all: 12 steps moved the parameters by steps of ~lr
    init = distill.build_student(OBS, ACT, UNITS, "silu", 0).state_dict()
    assert du.adam_steps({k[len("model."):]: v for k, v in init.items()}, ref64, LR) > 3
    # checkpoints: every 2 epochs and at the end, the reference's names and keys (+ `student`)
    assert sorted(os.listdir(tmp_path / "out")) == ["00002.pth", "00003.pth"]
    ck = torch.load(str(tmp_path / "out" / "00002.pth"), weights_only=False)
    assert sorted(ck) == ["epoch", "loss", "model_state_dict", "optimizer_state_dict", "student"] and ck["epoch"] == 1
    assert list(ck["model_state_dict"]) == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.4.weight", "model.4.bias"]
    plain_opt = torch.optim.Adam(torch.nn.Sequential(torch.nn.Linear(OBS, 16), torch.nn.SiLU(), torch.nn.Linear(16, 8), torch.nn.SiLU(), torch.nn.Linear(8, ACT)).parameters())
    osd = ck["optimizer_state_dict"]
    assert sorted(osd) == sorted(plain_opt.state_dict()) and osd["param_groups"][0]["params"] == [0, 1, 2, 3, 4, 5]
    assert sorted(osd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and osd["state"][0]["exp_avg"].shape == (16, OBS) and float(osd["state"][0]["step"]) == 8
    plain_opt.load_state_dict(osd)      # torch's own Adam takes it
    # resume from epoch 2's checkpoint: the same parameters as the uninterrupted run
    tr2 = distill.train(data, meta, str(tmp_path / "out"), units=UNITS, batch_size=BATCH, lr=LR, epochs=EPOCHS, save_frequency=2, seed=0, device="cpu", ckpt="00002.pth", log=None)
    assert tr2.epoch == EPOCHS
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, tr2.model.state_dict()[k]), k


def test_trainer_standardises_and_clamps():
    """The fixture's observation [3, 1] = 40 lies beyond 5 sigma of the metadata's statistics: the network input there is exactly 5 (and -5 at [7, 2])."""
    from phc_amd import distill
    fx = du.trainer_fixture(ROWS, OBS, ACT)
    tr = distill.Trainer(fx["obs"], fx["clean_action"], fx["running_mean"], fx["running_var"], UNITS, "silu", BATCH, LR, 0, "cpu")
    x = tr._input(torch.arange(ROWS))
    want = ((torch.from_numpy(fx["obs"]) - fx["running_mean"].float()) / torch.sqrt(fx["running_var"].float() + 1e-05))
    assert float(want[3, 1]) > 5 and float(want[7, 2]) < -5
    assert float(x[3, 1]) == 5.0 and float(x[7, 2]) == -5.0 and torch.equal(x, want.clamp(-5, 5))
    with pytest.raises(ValueError, match="Unsupported activation"):
        distill.StudentMLP(4, 2, [8], "softmax")


# ------------------------------------------------------------------------------------------------------------------ 4. oracles
def test_oracles_on_hand_computable_cases():
    assert do.silu(0.0) == 0.0 and do.silu_grad(1.0, 0.0) == 0.5
    np.testing.assert_allclose(do.silu(np.array([1.0, -1.0])), [1 / (1 + np.exp(-1.0)), -1 / (1 + np.e)], rtol=1e-15)
    assert do.silu(-1e30) == 0.0 and do.silu(1e30) == 1e30 and do.silu_grad(2.0, 1e30) == 2.0 and do.silu_grad(2.0, -1e30) == 0.0
    # silu'(z) by central differences
    z = np.linspace(-6, 6, 25)
    np.testing.assert_allclose(do.silu_grad(np.ones_like(z), z), (do.silu(z + 1e-6) - do.silu(z - 1e-6)) / 2e-6, rtol=1e-8, atol=1e-9)
    gz, sums = do.colsum_silu(np.full((4, 2), 3.0), np.zeros((4, 2)))
    assert np.array_equal(gz, np.full((4, 2), 1.5)) and np.array_equal(sums, [6.0, 6.0])
    # the loss of a constant offset c is c^2, its gradient 2 c / numel
    t = np.arange(12.0).reshape(4, 3)
    loss, grad = do.mse_loss(t + 0.5, t)
    assert loss == 0.25 and np.array_equal(grad, np.full((4, 3), 1.0 / 12))
    loss, grad = do.mse_loss(t[[2, 2, 0]] - 2.0, t, row_index=[2, 2, 0])
    assert loss == 4.0 and np.array_equal(grad, np.full((3, 3), -4.0 / 9))


# ------------------------------------------------------------------------------------------------------------------ 5. merge, sample_pkl
def test_merge_and_sample_pkl_file_selection(tmp_path):
    import joblib
    from phc_amd import distill
    d = tmp_path / "phc_act" / "clips"
    d.mkdir(parents=True)
    names = ["noise_False_0.05_2024-01-01-00:00:00.pkl", "noise_True_0.05_2024-01-01-00:00:01.pkl", "noise_True_0.075_2024-01-01-00:00:02.pkl"]
    for i, n in enumerate(names):
        obs = [np.full((2, 3), 10.0 * i, np.float32), np.full((1, 3), 10.0 * i + 1, np.float32)]
        joblib.dump({"obs": obs, "clean_action": [o[:, :2] for o in obs], "env_action": [o[:, :2] + 0.5 for o in obs], "key_names": np.array([f"a{i}", f"b{i}"]),
                     "motion_lengths": np.array([2, 1]), "reset": np.array([0, 1, 1]), "running_mean": {"running_mean": torch.full((3,), float(i)), "running_var": torch.ones(3)},
                     "config": {"i": i}}, d / n)
    out, meta = distill.merge(str(d), log=None)
    assert out == str(tmp_path / "phc_act" / "phc_act_clips.pkl") and meta == str(tmp_path / "phc_act" / "phc_act_clips_metadata.pkl")
    full, md = joblib.load(out), joblib.load(meta)
    assert full["obs"].shape == (9, 3) and list(full["obs"][:, 0]) == [0, 0, 1, 10, 10, 11, 20, 20, 21] and full["clean_action"].shape == (9, 2)
    assert list(full["reset"]) == [0, 1, 1] * 3 and list(full["key_names"]) == ["a0", "b0", "a1", "b1", "a2", "b2"] and list(full["motion_lengths"]) == [2, 1] * 3
    assert float(full["running_mean"]["running_mean"][0]) == 0.0 and full["config"] == [{"i": 0}, {"i": 1}, {"i": 2}]
    assert sorted(md) == ["config", "key_names", "motion_lengths", "running_mean"]
    # the sampler: low-noise files are `noise_False_*` or std 0.05, the high-noise one std 0.075
    for seed in range(4):
        got = distill.select_pkl_files(str(d), random.Random(seed), n_low=2, n_high=1)
        assert sorted(os.path.basename(f) for f in got[:2]) == names[:2] and os.path.basename(got[2]) == names[2]
    with pytest.raises(ValueError, match="sample_pkl needs 5"):
        distill.select_pkl_files(str(d), random.Random(0))
    obs, act = distill.load_rows([str(d / names[0]), str(d / names[2])])
    assert obs.shape == (6, 3) and act.shape == (6, 2) and obs.dtype == np.float32
    # a directory as the dataset: files re-drawn every save_frequency epochs
    tr = distill.train(str(d), meta, str(tmp_path / "o"), units=[4], batch_size=4, lr=1e-3, epochs=2, save_frequency=1, device="cpu", sample_low=2, sample_high=1, log=None)
    assert tr.obs.shape == (9, 3) and sorted(os.listdir(tmp_path / "o")) == ["00001.pth", "00002.pth"]


# ------------------------------------------------------------------------------------------------------------------ 6. the student wrapper
def test_student_policy_replaces_the_action_and_checks_widths():
    from phc_amd import distill
    fx = du.trainer_fixture(ROWS, OBS, ACT)
    tr = distill.Trainer(fx["obs"], fx["clean_action"], fx["running_mean"], fx["running_var"], UNITS, "silu", BATCH, LR, 0, "cpu")
    tr.run_epoch()
    ck = tr.checkpoint()
    task = types.SimpleNamespace(num_obs=OBS, num_actions=ACT, device="cpu")
    agent = types.SimpleNamespace(task=task, vec_env="env", set_eval=lambda: "delegated", preprocess_actions=lambda a: a * 0)
    sp = distill.StudentPolicy(agent, ck)
    obs = torch.from_numpy(fx["obs"][:9])
    plain = torch.nn.Sequential(torch.nn.Linear(OBS, 16), torch.nn.SiLU(), torch.nn.Linear(16, 8), torch.nn.SiLU(), torch.nn.Linear(8, ACT))
    plain.load_state_dict({k[len("model."):]: v for k, v in ck["model_state_dict"].items()})
    x = ((obs - fx["running_mean"].float()) / torch.sqrt(fx["running_var"].float() + 1e-05)).clamp(-5, 5)
    with torch.no_grad():
        want = plain(x)
    mus = sp.get_action_values(obs)["mus"]
    assert torch.equal(mus, want) and not mus.requires_grad
    assert sp.preprocess_actions(mus) is mus                      # the identity, not the agent's
    assert sp.vec_env == "env" and sp.set_eval() == "delegated" and sp.task is task      # the rest is the agent's
    for bad in (types.SimpleNamespace(num_obs=OBS + 1, num_actions=ACT, device="cpu"), types.SimpleNamespace(num_obs=OBS, num_actions=ACT + 2, device="cpu")):
        with pytest.raises(ValueError) as e:
            distill.StudentPolicy(types.SimpleNamespace(task=bad), ck)
        assert str(bad.num_obs) in str(e.value) and str(bad.num_actions) in str(e.value) and f"{OBS} observations" in str(e.value)
