"""Distil a composed controller into one MLP: the reference's last training stage (scripts/phc_act/create_phc_act_dataset.py:50-86, train_phc_actor.py).

    python -m phc_amd.distill merge dir=<output_path>/phc_act/<motion file stem>
    python -m phc_amd.distill train dataset=<merged.pkl | dir with noise_*.pkl> metadata=<..._metadata.pkl> output=<dir> \\
           [units=[2048,1024,512]] [activation=silu] [batch_size=16384] [lr=2e-5] [epochs=N] [save_frequency=100] [seed=0] [ckpt=<NNNNN.pth>]

The datasets are what `collect_dataset=True` sweeps write (learning/dataset_record.py).  `train` fits MLP(obs_dim, act_dim, units, activation) -- the reference's
layer order, `model.<k>.weight / bias` -- to (standardised, clamped observation -> clean action) pairs with MSE and Adam, a fresh shuffle every epoch, the last
partial batch kept, a checkpoint every `save_frequency` epochs.  On a HIP device the dataset lives on the device in fp32 and an optimizer step is: one
`phc_running_norm` pass (gather by row index, standardise, clamp, cast to bf16, K-padded), the bf16 device layers with their SiLU passes (fast_ops), `phc_mse_loss`
with the same row index, `phc_adam_clip_step` on the flat parameter.  Anywhere else the same loop runs as plain torch.  `StudentPolicy` plays a checkpoint in
`phc_amd.run test=True [im_eval=True] +student.checkpoint=<NNNNN.pth>`."""
import glob
import os
import random
import sys
from collections import defaultdict

import numpy as np
import torch
from torch import nn

ARRAY_KEYS = ("obs", "clean_action", "env_action", "reset")
EPSILON, CLAMP = 1e-05, 5.0     # train_phc_actor.py:79-80


# ------------------------------------------------------------------------------------------------------------------ datasets
def merge(directory, log=print):
    """create_phc_act_dataset.py:50-86 without the .h5: every *.pkl of `directory` concatenated -> (<parent>/phc_act_<name>.pkl, <parent>/phc_act_<name>_metadata.pkl);
    the metadata file holds the keys that are not row arrays (key_names, motion_lengths, running_mean of the first file, the configs)."""
    import joblib
    directory = os.path.abspath(str(directory))
    files = sorted(glob.glob(os.path.join(directory, "*.pkl")))
    if not files:
        raise FileNotFoundError(f"no .pkl files in {directory}")
    full = defaultdict(list)
    for f in files:
        for k, v in joblib.load(f).items():
            full[k].append(np.concatenate(v) if (k in ARRAY_KEYS and isinstance(v, list)) else v)
    for k, v in full.items():
        if k == "running_mean":
            full[k] = v[0]
        elif k != "config":
            full[k] = np.concatenate(v, axis=0)
    full = dict(full)
    name = os.path.basename(directory.rstrip("/"))
    out = os.path.join(os.path.dirname(directory), f"phc_act_{name}.pkl")
    meta = os.path.join(os.path.dirname(directory), f"phc_act_{name}_metadata.pkl")
    joblib.dump({k: v for k, v in full.items() if k not in ARRAY_KEYS}, meta, compress=True)
    joblib.dump(full, out, compress=True)
    if log is not None:
        log(f"merged {len(files)} files, {len(full['obs'])} rows -> {out}")
    return out, meta


def select_pkl_files(directory, rng, n_low=5, n_high=1):
    """train_phc_actor.py:39-51 (`sample_pkl`): the file name split at `_` is [noise, <add_action_noise>, <std>, <date>.pkl]; `n_low` files without noise or with
    std 0.05 plus `n_high` with std 0.075, drawn by `rng` (a random.Random)."""
    low, high = [], []
    for f in sorted(glob.glob(os.path.join(str(directory), "*.pkl"))):
        split = os.path.basename(f).split("_")
        if len(split) < 4:
            continue
        if split[1] == "False" or split[2] == "0.05":
            low.append(f)
        elif split[2] == "0.075":
            high.append(f)
    if len(low) < n_low or len(high) < n_high:
        raise ValueError(f"sample_pkl needs {n_low} low-noise and {n_high} 0.075-noise files in {directory}, found {len(low)} and {len(high)}")
    return rng.sample(low, n_low) + rng.sample(high, n_high)


def load_rows(files):
    """-> (obs fp32 [R, D], clean_action fp32 [R, A]) of one file or several (per-clip lists are concatenated)."""
    import joblib
    obs, act = [], []
    for f in [files] if isinstance(files, str) else files:
        d = joblib.load(f)
        for dst, k in ((obs, "obs"), (act, "clean_action")):
            dst.append(np.concatenate(d[k]) if isinstance(d[k], list) else np.asarray(d[k]))
    return np.concatenate(obs).astype(np.float32), np.concatenate(act).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the student
class StudentMLP(nn.Module):
    """phc/learning/mlp.py:4-58 `MLP(input_dim, output_dim, units, activation)`: Linear + activation per hidden width, a Linear head, under `model.*`; the layers are
    the device layers of learning/network.py (nn.Linear / nn.SiLU off the device)."""

    def __init__(self, input_dim, output_dim, units, activation):
        super().__init__()
        from .learning.fast_ops import FastLinear
        from .learning.network import _ACT, build_mlp
        if activation not in _ACT or activation == "None":
            raise ValueError(f"Unsupported activation function: {activation}")
        self.model = build_mlp(input_dim, list(units), activation, FastLinear)
        self.model.append(FastLinear(list(units)[-1], output_dim))

    def forward(self, x):
        return self.model(x)


def build_student(obs_dim, act_dim, units, activation, seed):
    torch.manual_seed(int(seed))
    return StudentMLP(obs_dim, act_dim, units, activation)


def epoch_permutation(seed, epoch, n):
    """The shuffle of epoch `epoch` (a function of the seed and the epoch alone, so a resumed run draws what the uninterrupted one would)."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(epoch))
    return torch.randperm(n, generator=g)


def standardise(obs, mean, var):
    """train_phc_actor.py:77-80: fp32 statistics, eps inside the root, clamp to +-5."""
    return torch.clamp((obs - mean.float()) / torch.sqrt(var.float() + EPSILON), min=-CLAMP, max=CLAMP)


class Trainer:
    def __init__(self, obs, act, running_mean, running_var, units=(2048, 1024, 512), activation="silu", batch_size=16384, lr=2e-5, seed=0, device=None, gemm="bf16"):
        from .learning.amp_agent import FlatGradBucket
        from .learning.running_mean_std import RunningMeanStd
        if gemm not in ("bf16", "fp32"):
            raise ValueError(f"gemm must be bf16 or fp32, not {gemm!r}")
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.on_device = self.device.type == "cuda"
        self.bf16 = self.on_device and gemm == "bf16"
        self.units, self.activation, self.batch_size, self.lr, self.seed = [int(u) for u in units], str(activation), int(batch_size), float(lr), int(seed)
        self.norm = RunningMeanStd((obs.shape[1],)).to(self.device).eval()      # frozen statistics: eval mode never folds a batch in
        self.norm.running_mean.copy_(torch.as_tensor(running_mean).double())
        self.norm.running_var.copy_(torch.as_tensor(running_var).double())
        self.model = build_student(obs.shape[1], act.shape[1], self.units, self.activation, seed).to(self.device)
        self.grads = FlatGradBucket(self.model.parameters())
        self.optimizer = torch.optim.Adam([self.grads.flat_param], lr=self.lr)
        self._pad = {p.shape[1]: p._padded.shape[1] for p in self.grads.params if getattr(p, "_padded", None) is not None}.get(obs.shape[1], 0)
        self._bufs, self._one = {}, torch.ones((), dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.set_data(obs, act)
        self.epoch = 0

    def set_data(self, obs, act):
        self.obs = torch.as_tensor(obs, dtype=torch.float32).to(self.device).contiguous()
        self.act = torch.as_tensor(act, dtype=torch.float32).to(self.device).contiguous()

    # ---- one optimizer step
    def _input(self, idx):
        """The minibatch's network input: gathered, standardised, clamped (and on the bf16 path cast and K-padded) in one phc_running_norm pass."""
        if not self.on_device:
            return standardise(self.obs[idx], self.norm.running_mean, self.norm.running_var)
        if not self.bf16:
            return self.norm(self.obs, row_index=idx)
        rows, D = idx.numel(), self.obs.shape[1]
        key = (rows, max(self._pad, D))
        if key not in self._bufs:
            self._bufs[key] = torch.zeros(key, dtype=torch.bfloat16, device=self.device)
        buf = self._bufs[key]
        self.norm(self.obs, out_dtype=torch.bfloat16, row_index=idx, out=buf[:, :D])
        return buf

    def step(self, idx):
        from .learning.fast_ops import adam_clip_step, deferred_colsums, mse_loss
        x = self._input(idx)
        self.grads.zero()
        if self.on_device:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
                pred = self.model(x)
            loss = mse_loss(pred.contiguous(), self.act, idx, unit_grad=True, out=self.loss)
            with deferred_colsums():
                torch.autograd.backward([loss], grad_tensors=[self._one])
            adam_clip_step(self.optimizer, self.grads.flat_param, self.grads.flat, None, shadow=self.grads.shadow if self.bf16 else None)
        else:
            loss = nn.functional.mse_loss(self.model(x), self.act[idx])
            loss.backward()
            self.optimizer.step()
            self.loss.copy_(loss.detach().reshape(1))

    def run_epoch(self):
        perm = epoch_permutation(self.seed, self.epoch, self.obs.shape[0]).to(self.device)
        with self.grads.shadow_scope():
            for k in range(0, perm.numel(), self.batch_size):
                self.step(perm[k:k + self.batch_size].contiguous())
        self.epoch += 1
        return self.loss

    # ---- checkpoints: the reference's keys (train_phc_actor.py:91-98) + `student`
    def _optimizer_state_dict(self):
        sd = self.optimizer.state_dict()
        flat = sd["state"].get(0, {})
        state = {}
        if flat:
            for i in range(len(self.grads.params)):
                state[i] = {"step": flat["step"].detach().clone().cpu(), "exp_avg": self.grads.param_view(flat["exp_avg"], i).detach().clone().contiguous().cpu(),
                            "exp_avg_sq": self.grads.param_view(flat["exp_avg_sq"], i).detach().clone().contiguous().cpu()}
        group = dict(sd["param_groups"][0])
        group["params"] = list(range(len(self.grads.params)))
        return {"state": state, "param_groups": [group]}

    def checkpoint(self):
        return {"epoch": self.epoch - 1, "model_state_dict": {k: v.detach().clone().contiguous().cpu() for k, v in self.model.state_dict().items()},
                "optimizer_state_dict": self._optimizer_state_dict(), "loss": self.loss.detach().cpu().reshape(()).clone(),
                "student": {"units": self.units, "activation": self.activation, "obs_dim": int(self.obs.shape[1]), "act_dim": int(self.act.shape[1]),
                            "running_mean": self.norm.running_mean.detach().cpu().clone(), "running_var": self.norm.running_var.detach().cpu().clone(),
                            "epsilon": EPSILON, "clamp": CLAMP}}

    def save(self, folder):
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, f"{self.epoch:05d}.pth")
        torch.save(self.checkpoint(), path)
        return path

    def load(self, ck):
        """train_phc_actor.py:100-116: parameters, optimizer state, and the epoch to continue with."""
        from .learning.fast_ops import adam_state
        if isinstance(ck, str):
            ck = torch.load(ck, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ck["model_state_dict"])
        osd = ck["optimizer_state_dict"]
        if osd["state"]:
            st = adam_state(self.optimizer, self.grads.flat_param)
            for i in range(len(self.grads.params)):
                for k in ("exp_avg", "exp_avg_sq"):
                    self.grads.param_view(st[k], i).copy_(osd["state"][i][k])
            st["step"] = torch.as_tensor(float(osd["state"][0]["step"]), dtype=torch.float32)
        self.epoch = int(ck["epoch"]) + 1
        self.loss.copy_(torch.as_tensor(ck["loss"], dtype=torch.float32).reshape(1))


def train(dataset, metadata, output, units=(2048, 1024, 512), activation="silu", batch_size=16384, lr=2e-5, epochs=100, save_frequency=100, seed=0, ckpt=None,
          device=None, gemm="bf16", sample_low=5, sample_high=1, log=print):
    """-> the Trainer after `epochs` epochs (a resumed run continues at the checkpoint's epoch + 1)."""
    import joblib
    meta = joblib.load(metadata)["running_mean"]
    sample_pkl = os.path.isdir(str(dataset))
    pick = lambda epoch: select_pkl_files(dataset, random.Random(int(seed) * 1000003 + epoch), sample_low, sample_high)
    save_frequency = max(int(save_frequency), 1)
    start = 0
    state = None
    if ckpt:
        path = ckpt if os.path.exists(str(ckpt)) else os.path.join(str(output), str(ckpt))
        if os.path.exists(path):
            state = torch.load(path, map_location="cpu", weights_only=False)
            start = int(state["epoch"]) + 1
        elif log is not None:
            log("No checkpoint found. Starting training from scratch.")
    obs, act = load_rows(pick(start - start % save_frequency) if sample_pkl else str(dataset))
    tr = Trainer(obs, act, meta["running_mean"], meta["running_var"], units, activation, batch_size, lr, seed, device, gemm)
    if state is not None:
        tr.load(state)
    for epoch in range(start, int(epochs)):
        if sample_pkl and epoch % save_frequency == 0 and epoch != start - start % save_frequency:
            tr.set_data(*load_rows(pick(epoch)))
        tr.run_epoch()
        if (epoch + 1) % save_frequency == 0 or epoch + 1 == int(epochs):
            path = tr.save(str(output))
            if log is not None:
                log(f"Epoch [{epoch + 1}/{epochs}], Loss: {float(tr.loss):.6f} -> {path}")
    return tr


# ------------------------------------------------------------------------------------------------------------------ playing the student
class StudentPolicy:
    """`+student.checkpoint=<NNNNN.pth>`: the agent with the student's output where the policy's action stands.  The student was fitted to what the task RECEIVED
    (clean_action), so its output goes to env.step as it is: `preprocess_actions` is the identity.  Everything else is the wrapped agent's."""

    def __init__(self, agent, checkpoint):
        ck = torch.load(checkpoint, map_location="cpu", weights_only=False) if isinstance(checkpoint, str) else checkpoint
        s = ck["student"]
        task = agent.task
        if int(s["obs_dim"]) != int(task.num_obs) or int(s["act_dim"]) != int(task.num_actions):
            raise ValueError(f"student checkpoint maps {int(s['obs_dim'])} observations to {int(s['act_dim'])} actions, the task has num_obs {int(task.num_obs)} and "
                             f"num_actions {int(task.num_actions)}")
        self._agent = agent
        dev = getattr(task, "device", "cpu")
        self.student = StudentMLP(int(s["obs_dim"]), int(s["act_dim"]), s["units"], s["activation"])
        self.student.load_state_dict(ck["model_state_dict"])
        self.student = self.student.to(dev).eval()
        for p in self.student.parameters():
            p.requires_grad = False
        self._mean, self._var = s["running_mean"].to(dev), s["running_var"].to(dev)

    def __getattr__(self, name):
        return getattr(self.__dict__["_agent"], name)

    def get_action_values(self, obs):
        with torch.no_grad():
            return {"mus": self.student(standardise(obs.float(), self._mean, self._var))}

    def preprocess_actions(self, actions, out=None):
        return actions

    def eval(self, output_dir=None, log=print):
        from .learning.im_eval import evaluate
        return evaluate(self, output_dir=output_dir, log=log if getattr(self._agent, "rank", 0) == 0 else None)


def main(argv=None):
    from .config import _parse_value
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("merge", "train"):
        raise SystemExit(__doc__)
    kw = {}
    for a in argv[1:]:
        k, _, v = a.partition("=")
        kw[k] = _parse_value(v)
    if argv[0] == "merge":
        return merge(kw["dir"])
    for k in ("dataset", "metadata", "output"):
        if k not in kw:
            raise SystemExit(f"distill train needs {k}=...")
    return train(**kw)


if __name__ == "__main__":
    main()
