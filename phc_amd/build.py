"""Build libphc_amd.so (HIP, gfx950) in-tree with hipcc.  `python -m phc_amd.build`."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libphc_amd.so")
# source -> extra flags.
#   task kernels: parity with the reference's torch ops is pinned at 1e-5 and torch does not fuse multiply-add, so
#     -ffp-contract=off (e.g. sqrt(1 - w*w) in quat_to_angle_axis is cancellation-prone: a contracted fma moves exp-map
#     outputs by 1e-3); -fno-slp-vectorize avoids v_pk_* register marshalling (reset 68 -> 49 us, post-physics 35 -> 27 us).
#     phc_kernels_plain.hip holds the plain instantiations of the two env-step task kernels (phc_task_kernel.h) and is compiled with the same flags.
#   stepper: see the header of phc_sim.hip (-ffast-math -fno-slp-vectorize: 158 -> 109 us).  phc_sim_wrench.hip holds the external-wrench instantiations of the
#     same kernel (phc_sim_kernel.h) and is compiled with the same flags; so is phc_sim_plain.hip, the plain instantiation of the default SMPL task's launch (phc_sim_plain.h).
#   learner kernels: bandwidth-bound passes; IEEE division / no contraction so the normalised values equal torch's.
#   matrix-core kernels (phc_gemm.hip): no contraction either (the fp32 slab and bias sums are plain adds in a fixed order).
#   renderer (phc_render.hip, phc_render_mesh.hip; off the training path): IEEE fp32 (no fast-math): its error bound assumes correctly rounded sqrt / division.
#   evaluation metrics (phc_eval.hip): no contraction -- its reference positions are bit-equal to phc_motion_state's.
#   push schedule (phc_push.hip): no contraction, no fast-math -- its integer state is bit-equal to the host build of phc_push.h.
#   domain randomisation: phc_sim_dr.hip holds the DR instantiations of the stepper's kernel and is compiled with phc_sim.hip's flags; phc_dr.hip (control delay,
#     velocity push) like the push schedule -- its state and draws are bit-equal to the host build of phc_dr.h.
#   clip processing (phc_clip.hip): fp64, no contraction, no fast-math -- it restates process_clip (motion_lib.py) operation by operation and is compared with it
#     at one fp32 rounding.  phc_clip_real.hip (the robots' clips: matrix FK, height fix) the same, against process_clip_real.
#   teleop rewards (phc_teleop.hip): like phc_dr.hip -- no contraction, no fast-math: its sums and its integer state follow the host build of phc_teleop.h.
#   distillation (phc_distill.hip): like the learner kernels -- bandwidth-bound passes; IEEE division / exp and no contraction, so the SiLU follows its fp32 statement
#     (phc_distill.h) operation by operation.
#   keypoint-stream tracking (phc_stream.hip): like phc_teleop.hip -- its fp64 filter sums and its ring counters follow the host build of phc_stream.h.
#   retargeting fit (phc_fit.hip): fp32, no contraction, no fast-math -- its sums, Adam step and step counters follow the host build of phc_fit.h; the device's sin / cos / sqrt are its only difference.
#     phc_fit_sph.hip (the spherical-joint keypoint fit over the same per-lane pieces) is compiled with the same flags, against the host build of phc_fit_sph.h.
#   getup draws (phc_getup.hip): like the push schedule -- its draws, kinds and slots are bit-equal to the host build of phc_getup.h.
#   observation noise / dropout / occlusion draws (phc_obs_aug.hip): like phc_fit.hip -- no contraction, no fast-math: its draws, counters and dropout decisions are
#     bit-equal to the host build of phc_obs_aug.h; the device's logf / sinf / cosf / sqrtf are the only difference of a noised element.
#   motion recording (phc_record.hip): like phc_obs_aug.hip -- no contraction, no fast-math: its headers, counters and copied floats are bit-equal to the host
#     build of phc_record.h; the root's exp map and the robots' axis x angle rows differ by the device's elementary functions alone.
#   thrown projectiles (phc_proj.hip): like the push schedule -- no contraction, no fast-math: its decisions and floats follow the host build of phc_proj.h; the
#     sinf / cosf of a throw are the only difference.
#   video output (phc_jpeg.hip; off the training path): no contraction, no fast-math -- the transform is stated as fp32 sums in a fixed order, and the host
#     build of phc_jpeg.h follows them operation by operation.
SOURCES = {"phc_kernels.hip": ["-fno-slp-vectorize", "-ffp-contract=off"], "phc_kernels_plain.hip": ["-fno-slp-vectorize", "-ffp-contract=off"], "phc_sim.hip": ["-ffast-math", "-fno-slp-vectorize"],
           "phc_sim_wrench.hip": ["-ffast-math", "-fno-slp-vectorize"], "phc_sim_plain.hip": ["-ffast-math", "-fno-slp-vectorize"],
           "phc_learn.hip": ["-ffp-contract=off"], "phc_gemm.hip": ["-ffp-contract=off"], "phc_render.hip": [], "phc_render_mesh.hip": [], "phc_eval.hip": ["-ffp-contract=off"],
           "phc_push.hip": ["-ffp-contract=off"], "phc_sim_dr.hip": ["-ffast-math", "-fno-slp-vectorize"], "phc_dr.hip": ["-ffp-contract=off"],
           "phc_clip.hip": ["-ffp-contract=off"], "phc_clip_real.hip": ["-ffp-contract=off"], "phc_teleop.hip": ["-ffp-contract=off"],
           "phc_stream.hip": ["-ffp-contract=off"], "phc_distill.hip": ["-ffp-contract=off"],
           "phc_fit.hip": ["-ffp-contract=off"], "phc_fit_sph.hip": ["-ffp-contract=off"], "phc_getup.hip": ["-ffp-contract=off"],
           "phc_obs_aug.hip": ["-ffp-contract=off"], "phc_record.hip": ["-ffp-contract=off"], "phc_proj.hip": ["-ffp-contract=off"],
           "phc_jpeg.hip": ["-ffp-contract=off"]}


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP extension cannot be built")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    headers = [f for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join("..", "..", "include", "phc_amd.h")]   # every header, so none can be forgotten
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in list(SOURCES) + headers)


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into phc_amd/libphc_amd.so."""
    if not force and not needs_build():
        return LIB
    hipcc = _hipcc()
    common = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment"]
    objs = []
    os.makedirs(os.path.join(HERE, "_obj"), exist_ok=True)
    for src, extra in SOURCES.items():
        obj = os.path.join(HERE, "_obj", src.replace(".hip", ".o"))
        cmd = [hipcc, *common, *extra, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n" + r.stdout + r.stderr)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + r.stdout + r.stderr)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
