// phc_kernels.hip -- gfx950 kernels + the extern "C" entry points declared in include/phc_amd.h.
//
// Thread mapping used by every env kernel: ONE LANE PER RIGID BODY, G = 32 lanes per environment (two environments per
// 64-wide wavefront) for articulations of up to 32 bodies incl. the extended reference bodies, G = 64 (one environment per
// wavefront) above.  Task kernels: 256-thread workgroups (8 or 4 envs), per-env sums by G-lane butterfly shuffles.
// Stepper: one wavefront per workgroup (phc_sim.hip).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "phc_aba.h"  // model table accessors (k_fk)
#include <type_traits>
#include "phc_im.h"
#include "phc_im_check.h"  // what the entry points refuse
#include "phc_task_kernel.h"  // k_im_post_physics, k_im_reset; im_is_plain

using namespace phc;

// The two task kernels of the env step, k_im_post_physics and k_im_reset, are templates in phc_task_kernel.h; this file instantiates the generic ones (through
// task_launch below), phc_kernels_plain.hip the plain ones.
#ifdef PHC_SIM_PROFILE
extern "C" int32_t phc_debug_post_timeline(unsigned long long* out32, long long env) {
    if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(phc::g_phc_ptl), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(phc::g_phc_ptl), z, sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(phc::g_phc_ptl_env), &env, sizeof(env)) == hipSuccess ? 0 : -1;
}
#endif

// phc_amp_ref_table: one lane group per frame of the library.
template <int DPJ, int G>
__global__ __launch_bounds__(256) void k_amp_ref_table(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm, int64_t num_frames,
                                                       const int64_t* __restrict__ next_frame, float* __restrict__ table) {
    pin_family<DPJ>(lib, prm);
    const int lane = threadIdx.x & (G - 1);
    const int64_t f = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (f >= num_frames) return;
    FrameRef fr;
    fr.f0 = f; fr.f1 = next_frame[f]; fr.idx0 = fr.idx1 = 0; fr.blend = 0.f;
    amp_obs_from_frames_lane(lib, prm, model.num_bodies, lane, fr, table + f * (int64_t)(prm.num_amp_obs_per_step - prm.num_amp_obs_extra));
}

// HumanoidImGetup fall / recovery resets: one lane group per listed env (state kept, see im_reset_from_state_lane).
template <int G>
__global__ __launch_bounds__(256) void k_im_reset_from_state(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm, phc_sim_state_t sim,
                                                            phc_im_buffers_t buf, int num_reset, const int64_t* __restrict__ env_ids,
                                                            int fill_history) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (r >= num_reset) return;
    im_reset_from_state_lane(model, lib, prm, sim, buf, env_ids[r], lane, fill_history);
}

// ... and the same for the envs phc_getup_assign marked (kind 3 = FALL: history filled, kind 2 = RECOVERY: history kept): one lane group per env, masked.
template <int G>
__global__ __launch_bounds__(256) void k_im_reset_from_state_masked(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm, phc_sim_state_t sim,
                                                                   phc_im_buffers_t buf, const int32_t* __restrict__ kind) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t env = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (env >= sim.num_envs) return;
    const int kd = kind[env];
    if (kd != 2 && kd != 3) return;
    im_reset_from_state_lane(model, lib, prm, sim, buf, env, lane, kd == 3);
}

#ifdef PHC_SIM_PROFILE   // one lane group's timeline through the reset kernel (scripts/probes/reset_timeline.py; the product library has none of this)
extern "C" int32_t phc_debug_reset_timeline(unsigned long long* out64, int32_t group) {
    if (out64 && hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_phc_rtl), sizeof(g_phc_rtl)) != hipSuccess) return -1;
    unsigned long long z[64] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phc_rtl), z, sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phc_rtl_group), &group, sizeof(group)) == hipSuccess ? 0 : -1;
}
#endif

// build_amp_obs_demo: n samples x S history steps.  One lane group per (sample, step).
template <int G>
__global__ __launch_bounds__(256) void k_amp_obs_demo(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm, int n,
                                                     const int64_t* __restrict__ motion_ids, const float* __restrict__ times0,
                                                     float* __restrict__ out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;   // sample (grid.x), history step k (grid.y)
    const int k = (int)blockIdx.y;
    const int S = prm.num_amp_obs_steps, A = prm.num_amp_obs_per_step;
    if (i >= n) return;
    // (demo start times are multiples of 1/30 s too -- sample_time_interval, humanoid_amp.py:262 -- : the per-frame table serves them as it serves resets)
    if (prm.amp_ref_table != nullptr) amp_obs_from_table_lane(lib, prm, model.num_bodies, lane, G, motion_ids[i], history_time(times0[i], prm.dt, k), out + (i * S + k) * A);
    else amp_obs_from_ref_lane(lib, prm, model.num_bodies, lane, motion_ids[i], history_time(times0[i], prm.dt, k), out + (i * S + k) * A);
}

// M9 standalone: get_motion_state for n (id, time) pairs.  One lane group per lookup.
template <int G>
__global__ __launch_bounds__(256) void k_motion_state(phc_motion_lib_t lib, int n, const int64_t* __restrict__ ids,
                                                     const float* __restrict__ times, const float* __restrict__ offset,
                                                     float* rg_pos, float* rb_rot, float* body_vel, float* body_ang_vel,
                                                     float* dof_pos, float* dof_vel, int64_t* idx0, int64_t* idx1, float* blend,
                                                     float* rg_pos_ext, float* rb_rot_ext) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (i >= n) return;
    motion_state_lane(lib, i, lane, ids, times, offset, rg_pos, rb_rot, body_vel, body_ang_vel, dof_pos, dof_vel, idx0, idx1, blend, rg_pos_ext, rb_rot_ext);
}

__global__ void k_sample_time_interval(phc_motion_lib_t lib, int n, const int64_t* __restrict__ ids,
                                       const float* __restrict__ phase, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sample_time_interval(lib, ids[i], phase[i]);
}

// P5 GAE: one thread per env, reversed scan over the horizon (common_agent.py:493-505)
__global__ void k_gae(int T, int n, const float* __restrict__ fdones, const float* __restrict__ values,
                      const float* __restrict__ rewards, const float* __restrict__ next_values, float gamma, float tau,
                      float* __restrict__ advs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float last = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const int64_t k = (int64_t)t * n + i;
        const float not_done = 1.0f - fdones[k];
        const float delta = rewards[k] + gamma * next_values[k] - values[k];
        last = delta + gamma * tau * not_done * last;
        advs[k] = last;
    }
}

// M5 poselib FK (skeleton3d.py:390-426): one thread per frame, bodies in tree order; quat_mul_norm semantics
// (positive real part, unit norm; rotation3d.py:31-98,195-201).
__device__ __forceinline__ Q4 pl_quat_mul_norm(Q4 a, Q4 b) {
    Q4 q = quat_mul16(a, b);
    if (q.w < 0.f) q = q4(-q.x, -q.y, -q.z, -q.w);
    float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-9f);
    return q4(q.x / n, q.y / n, q.z / n, q.w / n);
}
__global__ void k_fk(phc_model_t model, int64_t T, const float* __restrict__ local_rot, const float* __restrict__ root_trans,
                     float* __restrict__ grot, float* __restrict__ gpos) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= T) return;
    const int nb = model.num_bodies;
    for (int j = 0; j < nb; ++j) {
        const int p = model_tab(model, 0, j);
        Q4 lq = ld4(local_rot + (f * nb + j) * 4);
        if (p < 0) {
            st4(grot + (f * nb + j) * 4, lq);
            st3(gpos + (f * nb + j) * 3, ld3(root_trans + f * 3));
        } else {
            Q4 pq = ld4(grot + (f * nb + p) * 4);
            const float* mb = model_body(model, j);
            // poselib quat_rotate = Im(q * (v,0) * conj(q))
            V3 off = quat_rotate(pq, v3(mb[0], mb[1], mb[2]));
            st4(grot + (f * nb + j) * 4, pl_quat_mul_norm(pq, lq));
            st3(gpos + (f * nb + j) * 3, off + ld3(gpos + (f * nb + p) * 3));
        }
    }
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
static inline int32_t launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
static inline int env_blocks(int64_t groups, int lanes) { return (int)((groups * lanes + 255) / 256); }
// (lanes per env: group_lanes, phc_im_plain.h)

// The launch chooser of the task kernels: the run-time triple (joint family, lanes per env, plain feature set) as compile-time constants.  `launch(dpj, g, plain)`
// is a generic lambda that names its kernel with them -- k<dpj, g, plain>, k<dpj, g> or k<g> for the kernels that do not specialise further -- and launches it.
// `plain` (im_is_plain, phc_im_plain.h) implies the spherical family at 32 lanes: the one shape the plain kernels are instantiated for.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F>
static inline int32_t task_launch(bool revolute, int lanes, bool plain, F launch) {
    constexpr std::false_type no;
    if (plain) launch(int_c<3>(), int_c<32>(), std::true_type());
    else if (revolute) { if (lanes == 64) launch(int_c<1>(), int_c<64>(), no); else launch(int_c<1>(), int_c<32>(), no); }
    else { if (lanes == 64) launch(int_c<3>(), int_c<64>(), no); else launch(int_c<3>(), int_c<32>(), no); }
    return launch_status();
}

// the plain instantiations live in phc_kernels_plain.hip
extern template __global__ void k_im_post_physics<3, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int);
extern template __global__ void k_im_reset<3, false, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int, const int64_t* __restrict__,
                                                               const float* __restrict__, int, uint64_t);
extern template __global__ void k_im_reset<3, true, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int, const int64_t* __restrict__,
                                                              const float* __restrict__, int, uint64_t);

// phc_task_force_generic: a process-wide host switch that sends plain tasks through the generic kernels too (the A/B of tests/test_task_plain_gpu.py and of
// profiles/task_plain_instantiation).  The instrumented library stamps the generic kernels only.
#ifdef PHC_SIM_PROFILE
static int32_t g_force_generic = 1;
#else
static int32_t g_force_generic = 0;
#endif
static inline bool launch_plain(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_im_buffers_t* buf) {
    return !g_force_generic && im_is_plain(model, lib, prm, buf);
}

// both reset launches: `n` lane groups per row of the grid
template <bool RNG>
static int32_t reset_launch(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                            const phc_im_buffers_t* buf, int n, const int64_t* env_ids, const float* phase, int start_at_zero, uint64_t key, void* stream) {
    return task_launch(prm->dofs_per_joint == 1, group_lanes(model->num_bodies, prm->num_ext_bodies), launch_plain(model, lib, prm, buf), [&](auto dpj, auto g, auto plain) {
        hipLaunchKernelGGL((k_im_reset<dpj(), RNG, g(), plain()>), dim3(env_blocks(n, g()), prm->num_amp_obs_steps + 2), dim3(256), 0, (hipStream_t)stream, *model, *lib,
                           *prm, *sim, *buf, n, env_ids, phase, start_at_zero, key);
    });
}

extern "C" {

int32_t phc_abi_version(void) { return PHC_ABI_VERSION; }

int32_t phc_task_force_generic(int32_t on) {
    const int32_t old = g_force_generic;
    g_force_generic = on ? 1 : 0;
    return old;
}

int32_t phc_im_is_plain(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_im_buffers_t* buf) {
    return im_is_plain(model, lib, prm, buf) ? 1 : 0;
}

int32_t phc_motion_state(const phc_motion_lib_t* lib, int32_t n, const int64_t* motion_ids, const float* motion_times,
                         const float* offset, float* rg_pos, float* rb_rot, float* body_vel, float* body_ang_vel,
                         float* dof_pos, float* dof_vel, int64_t* frame_idx0, int64_t* frame_idx1, float* blend, float* rg_pos_ext,
                         float* rb_rot_ext, void* stream) {
    if (int32_t rc = check_motion_state(lib, n); rc || n == 0) return rc;
    return task_launch(lib->dofs_per_joint == 1, group_lanes(lib->num_bodies, lib->num_ext_bodies), false, [&](auto, auto g, auto) {
        hipLaunchKernelGGL(k_motion_state<g()>, dim3(env_blocks(n, g())), dim3(256), 0, (hipStream_t)stream, *lib, n, motion_ids, motion_times, offset,
                           rg_pos, rb_rot, body_vel, body_ang_vel, dof_pos, dof_vel, frame_idx0, frame_idx1, blend, rg_pos_ext, rb_rot_ext);
    });
}

int32_t phc_sample_time_interval(const phc_motion_lib_t* lib, int32_t n, const int64_t* motion_ids, const float* phase,
                                 float* motion_times, void* stream) {
    if (!lib || n < 0) return PHC_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sample_time_interval, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *lib, n, motion_ids, phase, motion_times);
    return launch_status();
}

int32_t phc_im_post_physics(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                            const phc_sim_state_t* sim, const phc_im_buffers_t* buf, void* stream) {
    if (int32_t rc = check_im_post_physics(model, lib, prm, sim, buf); rc || sim->num_envs == 0) return rc;
    const int n_reset_bodies = prm->num_reset_bodies > 0 ? prm->num_reset_bodies : 1;
    return task_launch(prm->dofs_per_joint == 1, group_lanes(model->num_bodies, prm->num_ext_bodies), launch_plain(model, lib, prm, buf), [&](auto dpj, auto g, auto plain) {
        hipLaunchKernelGGL((k_im_post_physics<dpj(), g(), plain()>), dim3(env_blocks(sim->num_envs, g())), dim3(256), 0, (hipStream_t)stream, *model, *lib, *prm, *sim,
                           *buf, n_reset_bodies);
    });
}

int32_t phc_amp_ref_table(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int64_t num_frames,
                          const int64_t* next_frame, float* table, void* stream) {
    if (int32_t rc = check_amp_ref_table(model, lib, prm, num_frames, next_frame, table); rc || num_frames == 0) return rc;
    const int lanes = group_lanes(model->num_bodies, prm->num_ext_bodies);
    const int64_t blocks = (num_frames * lanes + 255) / 256;
    if (blocks > 0x7fffffffLL) return PHC_EUNSUPPORTED;   // (launch geometry, not an argument check: grid.x is 31 bits)
    return task_launch(prm->dofs_per_joint == 1, lanes, false, [&](auto dpj, auto g, auto) {
        hipLaunchKernelGGL((k_amp_ref_table<dpj(), g()>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *model, *lib, *prm, num_frames, next_frame,
                           table);
    });
}

int32_t phc_im_reset(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                     const phc_im_buffers_t* buf, int32_t num_reset, const int64_t* env_ids, const float* phase,
                     int32_t start_at_zero, void* stream) {
    if (int32_t rc = check_im_reset(model, lib, prm, sim, buf, num_reset, phase, start_at_zero); rc || num_reset == 0) return rc;
    return reset_launch<false>(model, lib, prm, sim, buf, num_reset, env_ids, phase, start_at_zero, 0ull, stream);
}

int32_t phc_im_reset_done(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                          const phc_im_buffers_t* buf, uint64_t seed, uint64_t counter, int32_t start_at_zero, void* stream) {
    if (int32_t rc = check_im_reset_done(model, lib, prm, sim, buf); rc || sim->num_envs == 0) return rc;
    const int n = buf->reset_list ? buf->reset_sublist_cap * PHC_RESET_SUBLISTS : sim->num_envs;   // groups to launch
    return reset_launch<true>(model, lib, prm, sim, buf, n, nullptr, nullptr, start_at_zero, im_reset_done_key(*buf, seed, counter), stream);
}

int32_t phc_im_reset_from_state(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                                const phc_sim_state_t* sim, const phc_im_buffers_t* buf, int32_t num_reset, const int64_t* env_ids,
                                int32_t fill_history, void* stream) {
    if (int32_t rc = check_im_reset_from_state(model, lib, prm, sim, buf, num_reset, env_ids); rc || num_reset == 0) return rc;
    return task_launch(prm->dofs_per_joint == 1, group_lanes(model->num_bodies, prm->num_ext_bodies), false, [&](auto, auto g, auto) {
        hipLaunchKernelGGL(k_im_reset_from_state<g()>, dim3(env_blocks(num_reset, g())), dim3(256), 0, (hipStream_t)stream, *model, *lib, *prm, *sim, *buf,
                           num_reset, env_ids, fill_history);
    });
}

int32_t phc_im_reset_from_state_masked(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                                       const phc_im_buffers_t* buf, const int32_t* kind, void* stream) {
    if (int32_t rc = check_im_reset_from_state(model, lib, prm, sim, buf, 0, nullptr); rc) return rc;
    if (!kind || sim->num_envs < 0) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    return task_launch(prm->dofs_per_joint == 1, group_lanes(model->num_bodies, prm->num_ext_bodies), false, [&](auto, auto g, auto) {
        hipLaunchKernelGGL(k_im_reset_from_state_masked<g()>, dim3(env_blocks(sim->num_envs, g())), dim3(256), 0, (hipStream_t)stream, *model, *lib, *prm, *sim,
                           *buf, kind);
    });
}

int32_t phc_amp_obs_demo(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int32_t n,
                         const int64_t* motion_ids, const float* motion_times0, float* amp_obs_demo, void* stream) {
    if (int32_t rc = check_amp_obs_demo(model, lib, prm, n); rc || n == 0) return rc;
    return task_launch(prm->dofs_per_joint == 1, group_lanes(model->num_bodies, prm->num_ext_bodies), false, [&](auto, auto g, auto) {
        hipLaunchKernelGGL(k_amp_obs_demo<g()>, dim3(env_blocks(n, g()), prm->num_amp_obs_steps), dim3(256), 0, (hipStream_t)stream, *model, *lib, *prm, n,
                           motion_ids, motion_times0, amp_obs_demo);
    });
}

int32_t phc_gae(int32_t horizon, int32_t n, const float* fdones, const float* values, const float* rewards,
                const float* next_values, float gamma, float tau, float* advs, void* stream) {
    if (horizon < 0 || n < 0) return PHC_EINVAL;
    if (horizon == 0 || n == 0) return 0;
    hipLaunchKernelGGL(k_gae, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, horizon, n, fdones, values, rewards,
                       next_values, gamma, tau, advs);
    return launch_status();
}

int32_t phc_fk(const phc_model_t* model, int64_t num_frames, const float* local_rot, const float* root_trans, float* global_rot,
               float* global_pos, void* stream) {
    if (!model || model->num_bodies < 1 || model->num_bodies > PHC_MAX_BODIES || num_frames < 0) return PHC_EINVAL;
    if (num_frames == 0) return 0;
    hipLaunchKernelGGL(k_fk, dim3((unsigned)((num_frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *model, num_frames,
                       local_rot, root_trans, global_rot, global_pos);
    return launch_status();
}

}  // extern "C"
