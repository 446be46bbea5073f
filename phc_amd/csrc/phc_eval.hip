// phc_eval.hip -- phc_eval_accumulate: the evaluation sweep's tracking metrics, accumulated on the device (contract: include/phc_amd.h).
//
// Thread mapping of the task kernels (phc_kernels.hip): one lane per body, G = 32 lanes per env up to 32 bodies (two envs per wavefront), G = 64
// above; 256-thread blocks.  Each launch looks up the reference position of every body (the position quarter of phc_motion_state's lookup), forms
// the five per-frame error sums of learning/im_eval.py compute_metrics_per_clip by lane-group reductions and adds them to the env's fp64 totals
// (lane 0).  The two previous frames the velocity / acceleration terms need live in a caller-owned ring; nothing is static.
// Built with -ffp-contract=off: the lookup's arithmetic is the bit-exact part of the contract.
#include <hip/hip_runtime.h>
#include "phc_eval.h"
#include "phc_group.h"

using namespace phc;

template <int G>
__global__ __launch_bounds__(256) void k_eval_accumulate(phc_motion_lib_t lib, phc_eval_args_t a) {
    __shared__ int s_alive[256 / G], s_max[256 / G];
    const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const int64_t env = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int nb = a.num_bodies;
    int alive = 0, amax = 0;
    if (env < a.num_envs) {   // (a whole lane group takes or skips this together)
        const bool on = lane < nb;
        const int j = on ? lane : 0;
        const float w = on ? 1.f : 0.f;
        const int64_t mid = a.motion_ids ? a.motion_ids[env] : env;
        const int cs = a.clip_steps[env];
        const float t = motion_time(a.progress_buf[env], a.dt, a.motion_start_times[env], a.motion_start_times_offset[env]);
        const FrameRef fr = frame_ref(lib, mid, t);
        const V3 goff = ld3(a.global_offset + env * 3);
        V3 gt = ref_body_pos(lib, fr, j);
        gt += goff;
        const V3 pr = ld3(a.rigid_body_state + (env * nb + j) * 13);
        if (on && a.gt_out) st3(a.gt_out + (env * nb + j) * 3, gt);
        const float s_g = group_sum<G>(w * norm(pr - gt));
        if (lane == 0) a.mpjpe_step[env] = s_g / (float)nb;
        if (a.step < cs - 1) {   // a counted frame: the frames before it were counted too, so this is the env's frame number `step`
            // root-relative: lane root_idx (< nb, so it is `on`) already holds the root body's two positions
            const V3 rg = v3(group_bcast<G>(gt.x, a.root_idx), group_bcast<G>(gt.y, a.root_idx), group_bcast<G>(gt.z, a.root_idx));
            const V3 rp = v3(group_bcast<G>(pr.x, a.root_idx), group_bcast<G>(pr.y, a.root_idx), group_bcast<G>(pr.z, a.root_idx));
            const V3 pl = pr - rp, gl = gt - rg;
            const float s_l = group_sum<G>(w * norm(pl - gl));
            // similarity alignment of the root-relative pred onto the root-relative gt (im_eval._procrustes)
            const float inv_nb = 1.0f / (float)nb;
            const V3 mu_p = v3(group_sum<G>(w * pl.x) * inv_nb, group_sum<G>(w * pl.y) * inv_nb, group_sum<G>(w * pl.z) * inv_nb);
            const V3 mu_g = v3(group_sum<G>(w * gl.x) * inv_nb, group_sum<G>(w * gl.y) * inv_nb, group_sum<G>(w * gl.z) * inv_nb);
            const V3 pc = w * (pl - mu_p), gc = gl - mu_g;
            float H[9], R[9], scale;
            H[0] = group_sum<G>(pc.x * gc.x); H[1] = group_sum<G>(pc.x * gc.y); H[2] = group_sum<G>(pc.x * gc.z);
            H[3] = group_sum<G>(pc.y * gc.x); H[4] = group_sum<G>(pc.y * gc.y); H[5] = group_sum<G>(pc.y * gc.z);
            H[6] = group_sum<G>(pc.z * gc.x); H[7] = group_sum<G>(pc.z * gc.y); H[8] = group_sum<G>(pc.z * gc.z);
            const float ssq = group_sum<G>(norm2(pc));
            eval_similarity(H, ssq, R, &scale);   // uniform over the group
            const V3 al = v3(scale * (R[0] * pc.x + R[1] * pc.y + R[2] * pc.z), scale * (R[3] * pc.x + R[4] * pc.y + R[5] * pc.z),
                             scale * (R[6] * pc.x + R[7] * pc.y + R[8] * pc.z));
            const float s_pa = group_sum<G>(w * norm(al - gc));
            // differences in time: ring slot step & 1 holds frame step - 2 until this launch overwrites it, the other one frame step - 1
            float* h2 = a.history + ((env * 2 + (a.step & 1)) * 2) * (int64_t)(nb * 3) + j * 3;
            const float* h1 = a.history + ((env * 2 + ((a.step + 1) & 1)) * 2) * (int64_t)(nb * 3) + j * 3;
            float e_v = 0.f, e_a = 0.f;
            if (a.step >= 1) {
                const V3 p1 = ld3(h1), g1 = ld3(h1 + nb * 3);
                const V3 vp = pr - p1, vg = gt - g1;
                e_v = norm(vp - vg);
                if (a.step >= 2) {
                    const V3 p2 = ld3(h2), g2 = ld3(h2 + nb * 3);
                    e_a = norm((vp - (p1 - p2)) - (vg - (g1 - g2)));
                }
            }
            if (on) { st3(h2, pr); st3(h2 + nb * 3, gt); }
            const float s_v = group_sum<G>(w * e_v), s_a = group_sum<G>(w * e_a);
            if (lane == 0) {
                double* s = a.sums + env * 5;
                s[0] += (double)s_g; s[1] += (double)s_l; s[2] += (double)s_pa; s[3] += (double)s_a; s[4] += (double)s_v;
                a.count[env] += 1;
            }
        }
        if (lane == 0) {
            const int f = a.failed[env] | ((a.terminate_buf[env] != 0 && a.step <= cs - 1) ? 1 : 0);
            a.failed[env] = f;
            alive = f ? 0 : 1;
            amax = (alive && env < a.bound) ? cs : 0;
        }
    }
    if (lane == 0) { s_alive[grp] = alive; s_max[grp] = amax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0, m = 0;
        for (int g = 0; g < 256 / G; ++g) { n += s_alive[g]; m = s_max[g] > m ? s_max[g] : m; }
        if (n) atomicAdd(a.status, n);
        if (m > 0) atomicMax(a.status + 1, m);
    }
}

extern "C" int32_t phc_eval_accumulate(const phc_motion_lib_t* lib, const phc_eval_args_t* a, void* stream) {
    if (!lib || !a || !lib->frames || !lib->motion_lengths || !lib->motion_dt || !lib->motion_num_frames || !lib->length_starts) return PHC_EINVAL;
    if (!a->rigid_body_state || !a->progress_buf || !a->terminate_buf || !a->motion_start_times || !a->motion_start_times_offset ||
        !a->global_offset || !a->clip_steps || !a->history || !a->sums || !a->count || !a->failed || !a->status || !a->mpjpe_step) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_bodies < 1 || a->num_bodies > PHC_MAX_BODIES || a->num_bodies != lib->num_bodies) return PHC_EINVAL;
    if (a->root_idx < 0 || a->root_idx >= a->num_bodies || a->step < 0 || a->bound < 0 || a->bound > a->num_envs) return PHC_EINVAL;
    hipError_t e = hipMemsetAsync(a->status, 0, 2 * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int32_t)e;
    if (a->num_envs == 0) return 0;
    const int lanes = a->num_bodies > 32 ? 64 : 32;
    const int blocks = (int)(((int64_t)a->num_envs * lanes + 255) / 256);
    if (lanes == 64) hipLaunchKernelGGL(k_eval_accumulate<64>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *lib, *a);
    else hipLaunchKernelGGL(k_eval_accumulate<32>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *lib, *a);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
