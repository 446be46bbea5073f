"""Entry point with the reference's command line (`python phc/run_hydra.py learning=im env=env_im ... key=val`,
phc/run_hydra.py:264-339):

    python -m phc_amd.run learning=im env=env_im env.num_envs=4096 env.motion_file=<amass.pkl | synthetic:N:seed> [max_epochs=100]
    torchrun --nproc-per-node 8 -m phc_amd.run ...          # one process per GPU, RCCL gradient all-reduce

Registers the env under the names the reference uses ('rlgpu') and runs the `im_amp` agent."""
import os
import sys

import torch


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    from .config import compose
    from .env.tasks.vec_task import RLGPUEnv, parse_task
    from .learning.amp_agent import IMAmpAgent
    from .utils.flags import flags
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
    max_epochs = 10
    for a in list(argv):
        if a.startswith("max_epochs="):
            max_epochs = int(a.split("=", 1)[1])
            argv.remove(a)
    cfg = compose(argv + [f"device_id={local_rank}", f"rl_device=cuda:{local_rank}"])
    flags.test, flags.im_eval, flags.debug = bool(cfg.test), bool(cfg.im_eval), bool(cfg.debug)  # run_hydra.py:278-295
    seed = int(cfg.seed) + rank  # per-rank seed offset (run_hydra.py:121)
    torch.manual_seed(seed)
    task, env = parse_task(cfg, device_id=local_rank)
    vec_env = RLGPUEnv(env)
    agent = IMAmpAgent(env, cfg, dist=dist)
    ckpt = cfg.get("checkpoint", None)
    if not ckpt and (cfg.test or cfg.get("epoch", 0) != 0):
        # run_hydra.py:312-318: epoch=-1 -> output_path/Humanoid.pth, epoch=N -> Humanoid_{N:08d}.pth
        ep = int(cfg.get("epoch", 0))
        cand = os.path.join(cfg.output_path, "Humanoid.pth" if ep <= 0 else f"Humanoid_{ep:08d}.pth")
        ckpt = cand if os.path.exists(cand) else None
    if ckpt:
        agent.restore(ckpt, load_optimizer=not cfg.test)
    student = (cfg.get("student", None) or {}).get("checkpoint", None)
    if student:
        # `+student.checkpoint=<NNNNN.pth>` (phc_amd/distill.py): a distilled MLP acts in place of the policy, in `play` and in the sweep alike
        if not cfg.test:
            raise ValueError("+student.checkpoint plays a distilled student: it needs test=True")
        from .distill import StudentPolicy
        agent = StudentPolicy(agent, str(student))
    if cfg.test:
        # player mode (phc/learning/im_amp_players.py:25-384): no learning; im_eval=True sweeps the whole motion set and reports the
        # success rate / MPJPE table, otherwise a deterministic-policy rollout of `games` env steps reports episode statistics
        if cfg.im_eval:
            info, failed = agent.eval(output_dir=cfg.output_path)
            if rank == 0:
                print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()}, "failed clips:", len(failed))
        else:
            info = play(agent, task, env, steps=int(cfg.get("games", 300)))
            task.close()   # (finishes a `+render.video` recording)
            video = getattr(getattr(getattr(task, "_recorder", None), "recorder", None), "avi_path", None)   # `+render.format=avi|both` (phc_amd/video.py)
            if video:
                print("video:", video)
            if rank == 0:
                print(info)
        if dist is not None:
            dist.destroy_process_group()
        return info
    info = agent.train(max_epochs, output_dir=cfg.output_path)
    if rank == 0:
        out = os.path.join(cfg.output_path, "Humanoid.pth")
        os.makedirs(cfg.output_path, exist_ok=True)
        agent.save(out)
        print("saved", out)
    if dist is not None:
        dist.destroy_process_group()
    return info


def play(agent, task, env, steps=300):
    """Deterministic-policy rollout (players.PpoPlayerContinuous with is_determenistic=True): mean reward and episode length."""
    agent.set_eval()
    # `+record.motion=<out.pkl>` (phc_amd/motion_record.py): the rollout's motion as clips `<env>_<segment>`, split where reset_buf fired
    from . import motion_record
    ropt = motion_record.options(getattr(task, "cfg", None))
    if ropt is not None:
        motion_record.refuse_ranks(os.environ.get("WORLD_SIZE", "1"))
    mrec = motion_record.MotionRecorder(task, ropt["max_frames"], ropt["ref"]) if ropt is not None else None
    pushes0 = int(task._push.pushes) if getattr(task, "_push", None) is not None else 0
    proj = getattr(task, "_proj", None)
    proj0 = (int(proj.thrown), int(proj.hits)) if proj is not None else (0, 0)
    obs = env.reset()
    if mrec is not None:
        mrec.begin_play()
    rew_sum = torch.zeros(task.num_envs, device=task.device)
    ep_len = torch.zeros(task.num_envs, device=task.device)
    lens, rews = [], []
    streams = hasattr(task, "set_keypoints")   # HumanoidImDemo / HumanoidImMCPDemo: the tracking error of the streamed keypoints, summed on the device
    stream_err = torch.zeros((), device=task.device) if streams else None
    with torch.no_grad():
        for _ in range(steps):
            obs, r, done, info = env.step(agent.preprocess_actions(agent.get_action_values(obs)["mus"]))
            task.render()   # one frame per env step with `+render.video=DIR` (base_task.py:405-437); a no-op otherwise
            if mrec is not None:   # (one launch behind the post-physics launch, before the finished envs are reset)
                mrec.record()
            if streams:
                stream_err += task.extras["stream_err"].mean()
            rew_sum += r
            ep_len += 1
            ids = done.nonzero(as_tuple=False).flatten()
            if len(ids):
                lens.append(ep_len[ids].clone())
                rews.append(rew_sum[ids].clone())
                rew_sum[ids] = 0
                ep_len[ids] = 0
                obs = env.reset(ids)
    lens = torch.cat(lens) if lens else ep_len
    rews = torch.cat(rews) if rews else rew_sum
    out = {"episodes": int(lens.numel()), "mean_episode_length": float(lens.mean()), "mean_episode_reward": float(rews.mean()), "steps": steps}
    if getattr(task, "_push", None) is not None:   # `+perturb.*` (phc_amd/perturb.py): pushes started during the rollout, all envs
        out["perturb_pushes"] = int(task._push.pushes) - pushes0
    if proj is not None:   # `+projectile.*` (phc_amd/projectile.py): projectiles thrown and impacts on bodies during the rollout, all envs
        out["projectile_thrown"], out["projectile_hits"] = int(proj.thrown) - proj0[0], int(proj.hits) - proj0[1]
    if mrec is not None:
        out.update(mrec.close())
        mrec.export(ropt["path"], log=None)
        agent.last_motion_record = mrec
    if streams:
        out["stream_err_mm"] = float(stream_err) / max(steps, 1) * 1000.0
    return out


if __name__ == "__main__":
    main()
