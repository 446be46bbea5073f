// phc_sim_kernel.h -- k_sim_step, the articulated-body stepper kernel (S10), and what it is made of outside phc_aba.h: the action -> PD-target map and the staged
// epilogue; behind the kernel, the chooser of the instantiation to launch.  A header because the kernel is instantiated in four translation units that are compiled with the same flags (phc_amd/build.py): phc_sim.hip holds every
// instantiation phc_sim_step and the refresh entry points launch, phc_sim_wrench.hip the WRENCH twins of phc_sim_step_wrench, phc_sim_plain.hip the PLAIN instantiation of the default SMPL launch, phc_sim_dr.hip the DR twins of phc_sim_step_dr.  Separate units, so that adding the twins
// leaves the instruction streams of the plain instantiations exactly what they were (the compiler's output for one kernel depends on what else its module holds;
// profiles/ext_wrench/README.md).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "phc_aba.h"
#include "phc_group.h"   // wave_sync
#include "phc_sim_plain.h"
#include "phc_dr.h"

using namespace phc;

// instrumentation hooks of the profiling build (phc_sim.hip defines them under PHC_SIM_PROFILE before it includes this header); empty in the product
#ifndef PHC_PROF_DECL
#define PHC_PROF_DECL
#define PHC_PROF(i)
#define PHC_PROF_FLUSH
#define PHC_SKIP_DECL
#define PHC_SKIP(b) false
#define PHC_TL_DECL
#define PHC_TL(id)
#endif

// A2: pd_tar = offset + scale * action (humanoid.py:1711-1713); env.res_action (sim.pd_ref set): reference joint position + scale * action,
// kept within pi / 2 of the current joint position (humanoid_im.py:1094-1099); frozen DoFs -> 0 (humanoid.py:1549-1554)
// The K DoFs of one joint at once: every input of the K targets -- scale, action, offset or reference position, joint position, freeze flag -- is
// requested before the first target is formed, through pointers that are valid in every mode (no branch between the loads; what a mode does not use
// is dropped by a select), so the prologue waits for them once instead of 2-4 times per DoF.
template <int K>
__device__ __forceinline__ void pd_targets_of(const phc_sim_state_t& sim, const float* __restrict__ actions, const float* __restrict__ pd_off,
                                              const float* __restrict__ pd_scale, const int32_t* __restrict__ freeze, const int32_t* valid_ints,
                                              int64_t env, int nd, int d0, float* tg) {
    const bool ref = sim.pd_ref != nullptr, frz = freeze != nullptr;
    const int64_t i0 = env * nd + d0;
    const float* basep = ref ? sim.pd_ref + i0 : pd_off + d0;
    const int32_t* frzp = frz ? freeze + d0 : valid_ints;
    float sc[K], ac[K], base[K], q[K];
    int32_t fz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        sc[k] = pd_scale[d0 + k]; ac[k] = actions[i0 + k]; base[k] = basep[k];
        q[k] = sim.dof_state[(i0 + k) * 2];   // (the state load requested it already)
        fz[k] = frzp[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float sa = __fmul_rn(sc[k], ac[k]);
        asm("" : "+v"(sa));   // the product is rounded on its own: this file's -ffast-math would otherwise contract it with the add below into one fma
        const float half_pi = 1.57079637f;   // float32(np.pi / 2)
        const float t0 = __fadd_rn(base[k], sa);
        const float t = ref ? fmaxf(fminf(t0, __fadd_rn(q[k], half_pi)), __fsub_rn(q[k], half_pi)) : t0;
        tg[k] = (frz && fz[k]) ? 0.f : t;
    }
}


// ------------------------------------------------------------------------------------------
// Staged epilogue.  A lane would otherwise issue ~50 scattered 4-byte global stores, all wavefronts at the same instant.  The output slices of the E consecutive envs of ONE wavefront are contiguous and 16-byte aligned in every
// simulator tensor (E * 13, E * NB * 13, E * ND * 2, ... floats), so the lanes first write their values into the (now idle) LDS
// exchange area in exactly that layout and the wavefront then streams each slice out with coalesced dwordx4 / dwordx2 stores, four LDS reads
// in flight per wait (stage_copy_out).
// ------------------------------------------------------------------------------------------
struct StageLayout { int root, dof, force, contact, rbs, total; };
__device__ __forceinline__ StageLayout stage_layout(int E, int nb, int nd, bool with_force, bool with_contact) {
    StageLayout o;
    o.root = 0;
    o.dof = o.root + ((E * 13 + 3) & ~3);
    o.force = o.dof + ((E * nd * 2 + 3) & ~3);
    o.contact = o.force + (with_force ? ((E * nd + 3) & ~3) : 0);
    o.rbs = o.contact + (with_contact ? ((E * nb * 3 + 3) & ~3) : 0);
    o.total = o.rbs + ((E * nb * 13 + 3) & ~3);
    return o;
}
// a phc_sim_state_t whose tensors are the staging slices, indexed by the env's position in the wavefront
__device__ __forceinline__ phc_sim_state_t stage_state(const phc_sim_state_t& sim, float* stage, const StageLayout& o) {
    phc_sim_state_t st = sim;
    st.root_states = stage + o.root;
    st.dof_state = stage + o.dof;
    st.dof_force = sim.dof_force ? stage + o.force : nullptr;
    st.contact_force = sim.contact_force ? stage + o.contact : nullptr;
    st.rigid_body_state = stage + o.rbs;
    return st;
}
template <int W>
__device__ __forceinline__ void stage_copy_out(float* __restrict__ dst, const float* __restrict__ src, int n, int tid, int nthreads) {
    // four independent LDS reads per wait, then their four stores (one read per iteration cost the wavefront one LDS latency per 512 bytes streamed out)
    typedef typename std::conditional<W == 4, float4, float2>::type T;
    const int m = n / W;
    const T* s = reinterpret_cast<const T*>(src);
    T* d = reinterpret_cast<T*>(dst);
    int i = tid;
    for (; i + 3 * nthreads < m; i += 4 * nthreads) {
        const T a = s[i], b = s[i + nthreads], c = s[i + 2 * nthreads], e = s[i + 3 * nthreads];
        d[i] = a; d[i + nthreads] = b; d[i + 2 * nthreads] = c; d[i + 3 * nthreads] = e;
    }
    for (; i < m; i += nthreads) d[i] = s[i];
}
// all lanes of the wavefront: stream the staged slices of envs [env0, env0 + E) to the simulator tensors
template <int E>
__device__ __forceinline__ void stage_flush(const phc_sim_state_t& sim, const float* stage, const StageLayout& o, int64_t env0, int nb, int nd) {
    constexpr int W = (E % 4 == 0) ? 4 : 2;
    const int tid = threadIdx.x;
    stage_copy_out<W>(sim.root_states + env0 * 13, stage + o.root, E * 13, tid, 64);
    stage_copy_out<W>(sim.dof_state + env0 * nd * 2, stage + o.dof, E * nd * 2, tid, 64);
    if (sim.dof_force) stage_copy_out<W>(sim.dof_force + env0 * nd, stage + o.force, E * nd, tid, 64);
    if (sim.contact_force) stage_copy_out<W>(sim.contact_force + env0 * nb * 3, stage + o.contact, E * nb * 3, tid, 64);
    stage_copy_out<W>(sim.rigid_body_state + env0 * nb * 13, stage + o.rbs, E * nb * 13, tid, 64);
}
__device__ __forceinline__ bool stage_aligned(const phc_sim_state_t& sim) {
    const uintptr_t a = (uintptr_t)sim.root_states | (uintptr_t)sim.dof_state | (uintptr_t)sim.rigid_body_state |
                        (uintptr_t)sim.dof_force | (uintptr_t)sim.contact_force;
    return (a & 15) == 0;
}

// ------------------------------------------------------------------------------------------
// S10: the stepper.  One lane per body, GRP = 32 lanes per env (articulations of up to 32 bodies: two envs per wavefront) or
// GRP = 64 (up to 64 bodies -- Unitree G1 has 38: one env per wavefront), blockDim = 64: ONE wavefront per workgroup, so
// the level-synchronous tree sweeps need no barrier instruction at all -- their hand-over points are wave_sync() (phc_group.h; a __syncthreads() there is not
// "a 9-cycle s_barrier": the compiler drops the barrier of a one-wavefront workgroup and keeps the fence, an LDS-queue drain) -- and every SIMD of the chip carries
// two independent dependency chains (2048 wavefronts at N = 4096).
// Measured alternative (round 1, profiles/r01_notes.md): a level-major mapping (workgroup = 16 envs, wavefront = same
// body of many envs, multi-wave barriers) runs ~100 % of its lanes but leaves 3 of 4 SIMDs idle at N = 4096 and needs
// >256 VGPRs: 214-252 us vs 158 us for this mapping.  __launch_bounds__(64, 2): two wavefronts per SIMD (<= 256 VGPRs,
// 68 B/lane of scratch) beats one (272 registers, no scratch: 195 us) and three (168 VGPRs, 412 B scratch: 280 us).
// ------------------------------------------------------------------------------------------
// OCC: wavefronts per SIMD the register allocation aims at.  2 (<= 256 VGPRs, no scratch) is what every launch uses.  OCC = 3 (168 VGPRs, 116 B / lane
// of scratch) keeps 3072 wavefronts resident instead of 2048 -- and was measured SLOWER at every size (round 4, profiles/r04_stepper/occupancy_2_vs_3_waves_per_simd.txt:
// 96.6 vs 78.0 us at 4096 envs, 168.9 vs 145.3 at 8192, 241.0 vs 211.9 at 12288): the spilled wavefront's longer stream costs more than the
// third resident wavefront hides.  Kept behind lane_mapping = 3 so that the measurement can be repeated; never chosen automatically.
// (Round 5: the per-lane force accumulators of `force_average` took the workgroup's LDS from 16.9 to 18.4 KB; eight workgroups per CU = two per SIMD still fit
// the 160 KB, a third per SIMD would not -- the compiler says so when it builds this instantiation; the knob now measures the 168-VGPR code at occupancy 2.)
// LAG: the instantiation whose sub-steps behind the first one of a simulate() call keep its articulated inertias (phc_sim_params_t.inertia_lag); a
// template parameter, not a run-time branch: with the switch compiled into the one kernel it took 256 VGPRs + 12 spilled SGPRs instead of 224 and the
// every-sub-step-fresh launch went from 77 to 82 us (round 5, same box).
// WRENCH: the instantiations of phc_sim_step_wrench (external force / torque per body, include/phc_amd.h; launched from phc_sim_wrench.hip) -- a template parameter
// for the reason LAG is one.  The wrench's kernel arguments exist in these instantiations only (WrenchArgs<false> is empty) and every line the wrench adds stands
// behind `if constexpr (WRENCH)`: the plain instantiations are, instruction for instruction, the code they were before the wrench existed
// (profiles/ext_wrench/README.md).  The six floats of a lane are RE-READ from the tensors in every sub-step that applies them: requested at the top of the sub-step,
// before the body-body contact and the velocity products, and used in aba_body_init where the bias force is formed -- in flight while those phases run, so the read
// adds no round trip to the dependent chain, and in registers from there to aba_add_wrench only.  Every twin keeps its plain twin's occupancy and has no scratch.
// Alternatives, by the compiler's resource report (same README): the wrench applied behind aba_body_init spills in the lagged revolute twins and, read there as
// well, in the rigid spherical ones; a per-lane LDS slot (1.5 KB) takes the penalty / spherical workgroup from 19200 to 20736 bytes, and eight of those per CU no
// longer fit the 160 KB.  The two lagged revolute twins needed one register more than they had: WRENCH_TIGHT below.
// PLAIN: the instantiation of the default SMPL task's launch (phc_sim_plain.h; instantiated once, in phc_sim_plain.hip, for <true, SPHERICAL, 32, false, false, 2,
// LAG = true, WRENCH = false>).  pin_sim_plain turns every launch option and nullable pointer of that list into a constant, SimPlainModel the body / DoF counts and the
// solver-tree constants the generic kernel reads from the model table; what is fixed for the whole launch --
// the implicit drive diagonals dt kd + dt^2 kp (+ armature) and kd + dt kp -- is formed once in front of the sub-step loop instead of in each of its four passes
// (aba_plain_drive; a reversed body takes its solver parent's diagonal there, so that the drive exchange of a sub-step moves the torque alone); and the two sub-steps
// of a simulate() call are one loop body, so that `lag` and the sub-step's parity are constants in each half (SIM_PL_LAG_PAIR).
// Every line this adds stands behind `PLAIN`: the other instantiations are, instruction for instruction, what they were (profiles/stepper_plain_instantiation/README.md).
// PHC_SIM_PLAIN_ITEMS: which items the plain kernel is built with -- all of them in the product; the "new minus one item" libraries of that README are built with
// one bit cleared (0: the pins alone).
#define SIM_PL_LAG_PAIR 8   // (behind the ABA_PL_* bits of phc_aba.h)
#ifndef PHC_SIM_PLAIN_ITEMS
#define PHC_SIM_PLAIN_ITEMS (ABA_PL_NO_CP_TAIL | ABA_PL_DRIVE_CONST | SIM_PL_LAG_PAIR)
#endif
// PHC_SIM_WAVE_ITEMS: the hand-over points of the kernel, in EVERY instantiation (profiles/stepper_wave_order/README.md); -DPHC_SIM_WAVE_ITEMS=0 builds the
// library without the item (the A/B baseline of that README).
//   SIM_WV_ORDER    every hand-over point of the kernel is wave_sync() (phc_group.h) instead of __syncthreads().  The workgroup is ONE wavefront (SIM_BLOCK), so
//                   the compiler dropped the barrier instruction already; what __syncthreads() left was its workgroup-scope fence, an `s_waitcnt lgkmcnt(0)` that
//                   drains the LDS queue at each of the ~119 points a wavefront passes per launch before the next level's read may be issued.  Everything that
//                   crosses such a point goes from LDS to LDS within the wavefront (the list is in the README), and one wavefront's LDS operations are performed
//                   in program order.
// (Bits 2 and 8 were two more items of that README -- the lagged backward level-step's own products formed in front of the sweep, and the root's two level-steps
//  as one; both were built, measured no faster, and are not in the source.)
#define SIM_WV_ORDER 1
#ifndef PHC_SIM_WAVE_ITEMS
#define PHC_SIM_WAVE_ITEMS SIM_WV_ORDER
#endif
// threads per workgroup of every k_sim_step launch: one wavefront -- what wave_sync() (and the lane == body mapping) presupposes.  sim_launch_cm is the only
// place that launches the kernel and launches it with this.
constexpr int SIM_BLOCK = 64;
static_assert(SIM_BLOCK == 64, "k_sim_step's hand-over points are wave_sync(): the workgroup must be one wavefront");
template <int WV>
__device__ __forceinline__ void sim_sync() {
    if constexpr ((WV & SIM_WV_ORDER) != 0) wave_sync(); else __syncthreads();
}
template <bool PLAIN>
__device__ __forceinline__ void pin_sim_plain(phc_sim_params_t& prm, phc_sim_state_t& sim, const float* __restrict__& actions, const int32_t* __restrict__& freeze,
                                              int& num_sim_calls) {
    if constexpr (PLAIN) {
#define PHC_PIN_prm(f) prm.f
#define PHC_PIN_sim(f) sim.f
#define PHC_PIN_arg(f) f
#define PHC_PIN_VAL(s, f, v) PHC_PIN_##s(f) = (v);
#define PHC_PIN_NUL(s, f) PHC_PIN_##s(f) = nullptr;
#define PHC_PIN_SET(s, f) __builtin_assume(PHC_PIN_##s(f) != nullptr);
        PHC_SIM_PLAIN_FIELDS(PHC_PIN_VAL, PHC_PIN_NUL, PHC_PIN_SET)
#undef PHC_PIN_VAL
#undef PHC_PIN_NUL
#undef PHC_PIN_SET
#undef PHC_PIN_prm
#undef PHC_PIN_sim
#undef PHC_PIN_arg
    }
}

template <bool WRENCH> struct WrenchArgs {};
template <> struct WrenchArgs<true> { const float* force; const float* torque; int nsub; };   // [N, NB, 3] each (nullable); sub-steps the wrench acts in

// DR: the instantiations of phc_sim_step_dr (per-env friction, per-env model blocks for both joint families, torque noise; include/phc_amd.h; launched from
// phc_sim_dr.hip) -- a template parameter for the reason LAG and WRENCH are.  Its kernel arguments exist in these instantiations only (DrArgs<false> is empty)
// and every line it adds stands behind `if constexpr (DR)`.  Friction: each call into phc_aba.h that reads prm.friction gets a copy of the parameter struct
// that carries the env's coefficient (dr_params below), so no signature of phc_aba.h changes.  Torque noise (revolute, control_mode 1 / 2): at the first
// sub-step of a simulate call the lane's PD target is the un-noised one + u amp / kp (phc_dr.h) -- aba_body_init samples the spring there and nowhere else.
// DR twins are SHAPES twins: the env's block of the model tables is a per-lane pointer pair whether the launch has one block or many.  All twelve keep two
// wavefronts per SIMD; their scratch (the publishers' indexed parameter copies; 8 - 10 spilled VGPRs in the lagged revolute twins) is in
// profiles/domain_rand/README.md.
template <bool DR> struct DrArgs {};
template <> struct DrArgs<true> { const float* env_friction; const float* torque_noise; const int32_t* k; uint64_t key; int64_t env_offset; };   // (phc_sim_dr_t)

template <bool STEP, int JT, int GRP, bool SHAPES = false, bool RIGID = false, int OCC = 2, bool LAG = false, bool WRENCH = false, bool PLAIN = false, bool DR = false>
__global__ __launch_bounds__(SIM_BLOCK, OCC) void k_sim_step(phc_model_t model_all, phc_sim_params_t prm, phc_sim_state_t sim,
                                                const float* __restrict__ actions, const float* __restrict__ pd_off,
                                                const float* __restrict__ pd_scale, const int32_t* __restrict__ freeze,
                                                int num_sim_calls, const int64_t* __restrict__ env_ids, int num_listed, WrenchArgs<WRENCH> wr, DrArgs<DR> dr) {
    __shared__ __attribute__((aligned(16))) float xch_all[64 * PHC_XCH_STRIDE];   // one exchange slot per lane == body (16-byte aligned: the lagged hand-over moves as b128 + b64)
    __shared__ float cap_all[64 * PHC_CAP_STRIDE];
    __shared__ int pair_all[PHC_SC_MAX_PER_LANE * 64];   // candidate pairs of body-body contact: [pair slot][thread]
    __shared__ float favg_all[STEP ? 64 * 6 : 1];        // force_average: per-lane sums of S4 / S5 over the sub-steps
    // every body's solver-reference offset f[44..47): read in every sub-step by the body and its solver children.  (The rigid-contact and the revolute
    // instantiations sit at the register limit -- the table's address is one more live value -- and keep reading the model.)
    constexpr bool BATCH = STEP && aba_batched_constants<JT, RIGID>();   // (phc_aba.h)
    __shared__ float off_all[BATCH ? 64 * 3 : 1];
    // the lagged revolute twins (see WRENCH above): aba_body_init gets a time step the compiler cannot see through, so that what it derives from dt alone is formed
    // where it is used instead of being held in a register across the sub-step loop
    constexpr bool WRENCH_TIGHT = WRENCH && LAG && JT == PHC_JT_REVOLUTE;
    static_assert(!DR || (STEP && SHAPES && OCC == 2 && !WRENCH && !PLAIN), "the DR twins");
    static_assert(!PLAIN || (STEP && JT == PHC_JT_SPHERICAL && GRP == 32 && !SHAPES && !RIGID && OCC == 2 && LAG && !WRENCH), "the one plain instantiation");
    constexpr int PL = PLAIN ? (PHC_SIM_PLAIN_ITEMS) : 0;   // (phc_aba.h ABA_PL_*)
    constexpr int WV = PHC_SIM_WAVE_ITEMS;
    pin_sim_plain<PLAIN>(prm, sim, actions, freeze, num_sim_calls);
    const int lane = threadIdx.x & (GRP - 1);
    const int grp = threadIdx.x / GRP;
    const int64_t slot = (int64_t)blockIdx.x * (64 / GRP) + grp;
    // env_ids (refresh of a teleported subset only): slot -> listed env
    const int64_t env = (!STEP && env_ids != nullptr) ? (slot < num_listed ? env_ids[slot] : sim.num_envs) : slot;
    // SHAPES (per-env body shapes): the env's block of the model tables -- a per-lane pointer pair; the single-shape instantiation keeps the
    // tables behind scalar registers (with the select compiled in unconditionally the kernel spilled 188 B / lane: 35 MB of scratch traffic)
    const phc_model_t model = SHAPES ? model_for_env(model_all, sim, env) : model_all;
    // the env's own friction coefficient.  It reaches phc_aba.h in a copy of the parameters made at each call that reads prm.friction (dr_params): a copy the
    // sub-step loop uses is never indexed, so it lives in registers; the ones the publishers index (force_sensor_body[k]) are stack objects touched once per launch
    float dr_friction = 0.f;
    if constexpr (DR) dr_friction = (dr.env_friction != nullptr && env < sim.num_envs) ? fmaxf(dr.env_friction[env], 0.f) : prm.friction;
    auto dr_params = [&]() { phc_sim_params_t p = prm; p.friction = dr_friction; return p; };
    const int nb = PLAIN ? SimPlainModel::num_bodies : model.num_bodies, nd = PLAIN ? SimPlainModel::num_dof : model.num_dof;
    const bool active = env < sim.num_envs && lane < nb;
    const int body = lane;   // one lane per body, in the model's body order
    Xch x;
    x.base = xch_all + grp * GRP * PHC_XCH_STRIDE;

    AbaLane L;
    L.level = L.slevel = -1;
    PHC_SKIP_DECL
    PHC_PROF_DECL
    PHC_TL_DECL
    if (active) {
        aba_load_model(L, model, body);
        if (JT == PHC_JT_REVOLUTE) aba_load_model_rev(L, model, body);
        if (BATCH) { const float* f = model_body(model, body); float* o = off_all + grp * GRP * 3 + body * 3; o[0] = f[44]; o[1] = f[45]; o[2] = f[46]; }   // (read behind the barriers of the kinematics below)
        // (the state is requested BEFORE the new PD targets are stored: no load of this prologue has to wait behind a store, and the targets go
        //  into the lane's registers directly instead of through memory)
        const bool new_targets = STEP && actions != nullptr && body >= 1;
        aba_load_state<JT>(L, sim, nd, env, body, !new_targets);
        if (new_targets) {
            constexpr int K = JT == PHC_JT_REVOLUTE ? 1 : 3;
            float tg[3] = {0.f, 0.f, 0.f};
            pd_targets_of<K>(sim, actions, pd_off, pd_scale, freeze, model.ints, env, nd, L.dof_start, tg);
#pragma unroll
            for (int k = 0; k < K; ++k) sim.pd_target[env * nd + L.dof_start + k] = tg[k];   // (stored after all K are formed: no load waits behind a store)
            L.target = v3(tg[0], tg[1], tg[2]);
        }
    }
    // torque noise: the lane's un-noised target and amp / kp (kp: the env's block), once
    float dr_target = 0.f, dr_gain = 0.f;
    if constexpr (DR && JT == PHC_JT_REVOLUTE) {
        if (dr.torque_noise != nullptr && active && L.level > 0) {
            dr_target = L.target.x;
            dr_gain = dr_noise_gain(dr.torque_noise[env * nd + L.dof_start], model_body(model, body)[13]);
        }
    }
    // the idle lanes behind the bodies publish the extra collision shapes (phc_aba.h): their capsule records are loaded once, here
    const bool shape_lane = active || (STEP && prm.self_collision && env < sim.num_envs && lane < nb + (PLAIN ? SimPlainModel::extra_shapes : model_num_extra_shapes(model)));
    if (shape_lane && !active) aba_load_extra_shape(L, model, lane - nb);
    // initial kinematics by pointer jumping too (round 4: 4 composition steps instead of max_level + 1 = 9 level-steps for the SMPL tree)
    if (!PHC_SKIP(8)) {
        const int jsteps = PLAIN ? SimPlainModel::jump_steps : model_jump_steps(model);
        aba_fk_jump_begin(L, body, x);
        sim_sync<WV>();
        for (int k = 0; k < jsteps; ++k) {
            aba_fk_jump_step(L, k, x);
            sim_sync<WV>();
            if (active) aba_write_kin(L, xslot(x, body), Xch::es, 6);
            sim_sync<WV>();
        }
    }
    PHC_PROF(0)
    if (STEP) {
        const float dt = prm.sim_dt / (float)prm.substeps;
        const int nsub = num_sim_calls * prm.substeps;
        float* caps = cap_all + grp * GRP * PHC_CAP_STRIDE;
        const float* offs = BATCH ? off_all + grp * GRP * 3 : nullptr;
        uint32_t near_pairs = 0;
        if (prm.self_collision) aba_load_pairs<PHC_SC_MAX_PER_LANE>(pair_all + threadIdx.x, 64, model, lane, GRP);
        // the backward / acceleration sweeps walk the solver tree (model.py solver_tree(): re-rooted where that makes it shallower)
        const int solver_depth = PLAIN ? SimPlainModel::solver_depth : model_solver_depth(model, true);
        const int jump_steps = PLAIN ? SimPlainModel::jump_steps : model_jump_steps(model);
        const bool rerooted = PLAIN ? SimPlainModel::rerooted != 0 : model_tab(model, 11, 3) != 0;
        // the plain launch: what the drive needs and no sub-step changes, once (aba_plain_drive); a reversed body takes its solver parent's diagonal
        constexpr int SUBSTEP_UNROLL = (PL & SIM_PL_LAG_PAIR) ? 2 : 1;
        AbaPlainDrive pdrive;
        if constexpr ((PL & ABA_PL_DRIVE_CONST) != 0) {
            if (active && L.level > 0) aba_plain_drive(L, pdrive, model_body(model, body), dt);
            if (active) { if (L.level == 0) L.diso = 0.f; aba_publish_diso(L, body, x); }
            sim_sync<WV>();
            if (active) aba_fetch_diso(L, body, x);
            sim_sync<WV>();
        }
        // (SIM_PL_LAG_PAIR: the two sub-steps of a simulate() call as one loop body, so that `lag` and the sub-step's parity are constants in each half)
#pragma unroll SUBSTEP_UNROLL
        for (int s = 0; s < nsub; ++s) {
            const int tl_sub = s; (void)tl_sub;
            PHC_TL(1)
            // external wrench of this sub-step: requested here, used in aba_body_init (see WRENCH above).  Only a body's own lane reads: the tensors end with the last
            // env's last body
            V3 ext_f = v3(0.f, 0.f, 0.f), ext_t = v3(0.f, 0.f, 0.f);
            bool ext_on = false;
            if constexpr (WRENCH) {
                ext_on = s < wr.nsub;   // (uniform)
                if (ext_on && active) {
                    const int64_t wi = (env * nb + body) * 3;
                    if (wr.force != nullptr) ext_f = v3(wr.force[wi], wr.force[wi + 1], wr.force[wi + 2]);
                    if (wr.torque != nullptr) ext_t = v3(wr.torque[wi], wr.torque[wi + 1], wr.torque[wi + 2]);
                }
            }
            if (prm.self_collision && !PHC_SKIP(0)) {   // body-body contact from the kinematics the last sweep left in the exchange slots
                if (shape_lane) aba_publish_shape(L, lane, x, caps);   // body lanes: the primary capsules; the idle lanes behind them: the extra shapes
                sim_sync<WV>();
                if (env < sim.num_envs) aba_collide_pairs<PHC_SC_MAX_PER_LANE>(pair_all + threadIdx.x, 64, prm, dt, x, caps, near_pairs, s == 0);
                sim_sync<WV>();
                if (active) aba_collect_self(L, body, caps);
            }
            PHC_PROF(1)
            PHC_TL(2)
            if (active && !PHC_SKIP(1)) aba_velocity_products(L, model, body, x, true, offs);
            // contact_model 1 (rigid): the sub-step's solve is repeated contact_iterations times, each pass with the active set and friction cone the
            // previous one implies (phc_aba.h aba_ground_contact_rigid); the penalty model is the single pass it always was
            const int passes = RIGID ? (prm.contact_iterations < 1 ? 1 : prm.contact_iterations) : 1;
            // inertia_lag (round 5; penalty contact): the sub-steps behind the first one of a simulate() call keep its articulated inertias and joint-space
            // inverses and only redo the bias-force recursion (aba_body_init / aba_backward_level, `lag`)
            const bool lag = LAG && !RIGID && (s % prm.substeps) != 0;
            if constexpr (DR && JT == PHC_JT_REVOLUTE) {   // a new simulate call: a new draw (only a joint's own lane reads; the tensors end with the last env's last DoF)
                if (dr.torque_noise != nullptr && active && L.level > 0 && s % prm.substeps == 0)
                    L.target.x = dr_target_shift(dr_target, dr_noise_u(dr.key, (uint32_t)dr.k[env], (uint32_t)(s / prm.substeps),
                                                                       (uint32_t)((dr.env_offset + env) * nd + L.dof_start)), dr_gain);
            }
            for (int pass = 0; pass < passes; ++pass) {
            PHC_TL(3)
            // (penalty contact: the body's slice of the contact-point table from the lane's registers, not from two table loads the point loads would wait for)
            if (active && !PHC_SKIP(1)) {
                if constexpr (WRENCH) {
                    float dt_b = dt;
                    if constexpr (WRENCH_TIGHT) asm volatile("" : "+v"(dt_b));
                    if (!BATCH) aba_body_init<JT, RIGID>(L, model, prm, dt_b, body, s % prm.substeps == 0, true, pass, lag, ext_on, ext_f, ext_t);
                    else aba_body_init<JT, RIGID>(L, model, prm, dt_b, body, s % prm.substeps == 0, model_body(model, body), L.cp_range & 0xffff, L.cp_range >> 16, true, pass, lag,
                                                  ext_on, ext_f, ext_t);
                } else if constexpr (DR) {
                    const phc_sim_params_t pf = dr_params();
                    if (!BATCH) aba_body_init<JT, RIGID>(L, model, pf, dt, body, s % prm.substeps == 0, true, pass, lag);
                    else aba_body_init<JT, RIGID>(L, model, pf, dt, body, s % prm.substeps == 0, model_body(model, body), L.cp_range & 0xffff, L.cp_range >> 16, true, pass, lag);
                } else if constexpr (PLAIN) {
                    aba_body_init<JT, RIGID, PL>(L, model, prm, dt, body, s % prm.substeps == 0, model_body(model, body), L.cp_range & 0xffff, L.cp_range >> 16, true, pass, lag,
                                                 false, V3(), V3(), &pdrive);
                } else {
                if (!BATCH) aba_body_init<JT, RIGID>(L, model, prm, dt, body, s % prm.substeps == 0, true, pass, lag);
                else aba_body_init<JT, RIGID>(L, model, prm, dt, body, s % prm.substeps == 0, model_body(model, body), L.cp_range & 0xffff, L.cp_range >> 16, true, pass, lag);
                }
            }
            if (active && PHC_SKIP(9)) aba_body_init<JT, RIGID>(L, model, prm, dt, body, s % prm.substeps == 0, true, pass, lag);   // (profiling builds: the phase a second time, loads warm -- its pure instruction cost)
            PHC_PROF(2)
            PHC_TL(4)
            if (JT == PHC_JT_SPHERICAL && rerooted && pass == 0 && !PHC_SKIP(2)) {   // reversed bodies take the drive terms of their solver parent's joint
                if (active) aba_publish_drive(L, body, x, (PL & ABA_PL_DRIVE_CONST) != 0);
                sim_sync<WV>();
                if (active) aba_fetch_drive(L, body, x, (PL & ABA_PL_DRIVE_CONST) != 0);
                sim_sync<WV>();
            }
            PHC_PROF(3)
            PHC_TL(5)
            if (!PHC_SKIP(3)) for (int l = solver_depth; l >= 0; --l) { aba_backward_level<JT, (PL & ABA_PL_DRIVE_CONST) != 0>(L, l, body, x, lag); sim_sync<WV>(); PHC_TL(120 + l) }
            PHC_PROF(4)
            if (!PHC_SKIP(4)) {
                for (int l = 0; l <= solver_depth; ++l) { aba_accel_level<JT>(L, l, body, x); sim_sync<WV>(); PHC_TL(140 + l) }
            }
            }
            if constexpr (DR) { if (RIGID && active && (s == nsub - 1 || prm.force_average)) { const phc_sim_params_t pf = dr_params(); aba_publish_contact_rigid(L, model, pf, sim, dt, env, body, true); } }
            else
            if (RIGID && active && (s == nsub - 1 || prm.force_average)) aba_publish_contact_rigid(L, model, prm, sim, dt, env, body, true);   // S4 / S6 from the final solve
            if (JT == PHC_JT_SPHERICAL && rerooted && !PHC_SKIP(4)) aba_accel_finish(L, model, body, x, offs);
            PHC_PROF(5)
            PHC_TL(6)
            if (!PHC_SKIP(5)) aba_integrate_joint<JT>(L, prm, dt);
            if (prm.force_average) aba_force_accumulate(L, s, nsub, favg_all + threadIdx.x * 6);   // S4 / S5 as means over the sub-steps of the env step instead of the last one's values
            PHC_PROF(6)
            PHC_TL(7)
            if (!PHC_SKIP(6)) aba_fk_jump_begin(L, body, x);   // kinematics by pointer jumping: jump_steps composition steps instead of max_level + 1 level-steps
            sim_sync<WV>();
            for (int k = 0; k < (PHC_SKIP(6) ? 0 : jump_steps); ++k) {
                aba_fk_jump_step(L, k, x);
                sim_sync<WV>();
                if (active) aba_write_kin(L, xslot(x, body), Xch::es, 6);
                sim_sync<WV>();
                PHC_TL(160 + k)
            }
            PHC_PROF(7)
            PHC_TL(8)
        }
    }
    // S7: the last forward sweep already produced the end-of-step kinematics
    constexpr int E = 64 / GRP;
    const int64_t env0 = (int64_t)blockIdx.x * E;
    const StageLayout so = stage_layout(E, nb, nd, sim.dof_force != nullptr, sim.contact_force != nullptr);
    if (PHC_SKIP(7)) {
    } else if (STEP && E >= 2 && env0 + E <= sim.num_envs && (PLAIN || stage_aligned(sim)) && so.total <= 64 * PHC_XCH_STRIDE) {   // staged epilogue, see above
        const phc_sim_state_t st = stage_state(sim, xch_all, so);
        if (active) {
            aba_store_state<JT>(L, st, nd, grp, body);
            aba_publish_body(L, st, nb, grp, body, true);
        }
        sim_sync<WV>();
        stage_flush<E>(sim, xch_all, so, env0, nb, nd);
    } else if (active) {
        if (STEP) aba_store_state<JT>(L, sim, nd, env, body);
        aba_publish_body(L, sim, nb, env, body, STEP);
    }
    if constexpr (DR) { if (!RIGID && active && sim.force_sensor != nullptr) { const phc_sim_params_t pf = dr_params(); aba_publish_sensors(L, model, pf, sim, prm.sim_dt / (float)prm.substeps, env, body); } }
    else
    if (STEP && !RIGID && active && sim.force_sensor != nullptr) aba_publish_sensors(L, model, prm, sim, prm.sim_dt / (float)prm.substeps, env, body);   // S6
    PHC_PROF(8)
    if (STEP) { PHC_PROF_FLUSH }
}

// ------------------------------------------------------------------------------------------
// The launch chooser: which instantiation a model and its options run.  One chooser for both translation units; WRENCH = true names only the instantiations
// phc_sim_step_wrench launches (one env-shape block, two wavefronts per SIMD: it refuses the rest), DR = true only the twins of phc_sim_step_dr, so each unit
// holds exactly its own kernels.
// ------------------------------------------------------------------------------------------
// phc_sim_force_generic (include/phc_amd.h): the process-wide host switch that sends plain launches through the generic kernel too; defined in phc_sim.hip
extern int32_t g_phc_sim_force_generic;
// the plain instantiation lives in phc_sim_plain.hip
extern template __global__ void k_sim_step<true, PHC_JT_SPHERICAL, 32, false, false, 2, true, false, true, false>(phc_model_t, phc_sim_params_t, phc_sim_state_t, const float* __restrict__,
                                                                                                           const float* __restrict__, const float* __restrict__,
                                                                                                           const int32_t* __restrict__, int, const int64_t* __restrict__, int,
                                                                                                           WrenchArgs<false>, DrArgs<false>);

template <bool STEP, int JT, bool SHAPES, bool RIGID, bool WRENCH, bool DR>
static void sim_launch_cm(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions, const float* off,
                          const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream, const int64_t* env_ids, int num_listed,
                          const WrenchArgs<WRENCH>& wr, const DrArgs<DR>& dr) {
    const int64_t groups = env_ids ? num_listed : sim->num_envs;
    const bool wide = model->num_bodies > 32;   // more bodies than a 32-lane group holds: one env per wavefront
    constexpr bool LAG = STEP && !RIGID;
    const bool lag = LAG && prm.inertia_lag != 0;
    auto launch = [&](auto kernel, int64_t blocks) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SIM_BLOCK), 0, stream, *model, prm, *sim, actions, off, scale, freeze, num_sim_calls, env_ids, num_listed, wr, dr);
    };
    if constexpr (!WRENCH && !DR && LAG && !SHAPES && JT == PHC_JT_SPHERICAL)   // (experiment knob, see OCC above)
        if (!wide && prm.lane_mapping == 3) return launch(k_sim_step<STEP, JT, 32, SHAPES, RIGID, 3>, (groups + 1) / 2);
    if constexpr (STEP && !WRENCH && !DR && LAG && !SHAPES && JT == PHC_JT_SPHERICAL)   // the plain launch: every entry of phc_sim_plain.h holds (and the switch is off)
        if (lag && !wide && !g_phc_sim_force_generic && sim_is_plain(model, &prm, sim, actions, freeze, num_sim_calls))
            return launch(k_sim_step<true, PHC_JT_SPHERICAL, 32, false, false, 2, true, false, true, false>, (groups + 1) / 2);
    if (lag && wide) launch(k_sim_step<STEP, JT, 64, SHAPES, RIGID, 2, LAG, WRENCH, false, DR>, groups);
    else if (lag) launch(k_sim_step<STEP, JT, 32, SHAPES, RIGID, 2, LAG, WRENCH, false, DR>, (groups + 1) / 2);
    else if (wide) launch(k_sim_step<STEP, JT, 64, SHAPES, RIGID, 2, false, WRENCH, false, DR>, groups);
    else launch(k_sim_step<STEP, JT, 32, SHAPES, RIGID, 2, false, WRENCH, false, DR>, (groups + 1) / 2);
}

template <bool STEP, int JT, bool SHAPES, bool WRENCH, bool DR>
static void sim_launch_jt(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions, const float* off,
                          const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream, const int64_t* env_ids, int num_listed,
                          const WrenchArgs<WRENCH>& wr, const DrArgs<DR>& dr) {
    if (STEP && prm.contact_model == 1)   // rigid ground contact: its own instantiation, the penalty kernel is untouched by it
        sim_launch_cm<STEP, JT, SHAPES, STEP, WRENCH, DR>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
    else
        sim_launch_cm<STEP, JT, SHAPES, false, WRENCH, DR>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
}
template <bool STEP, bool WRENCH, bool DR = false>
static void sim_launch(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions, const float* off,
                       const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream, const int64_t* env_ids, int num_listed,
                       const WrenchArgs<WRENCH>& wr, const DrArgs<DR>& dr = DrArgs<DR>()) {
    const bool revolute = model->num_dof == model->num_bodies - 1 && model->num_bodies > 2;   // one revolute joint per body (robots)
    if constexpr (DR) {   // the DR twins: the env's block of the model tables for both joint families (one block: block 0)
        if (revolute) return sim_launch_jt<STEP, PHC_JT_REVOLUTE, true, false, true>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
        return sim_launch_jt<STEP, PHC_JT_SPHERICAL, true, false, true>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
    } else {
    if (revolute)  // (one shape)
        return sim_launch_jt<STEP, PHC_JT_REVOLUTE, false, WRENCH, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
    if constexpr (!WRENCH)
        if (model->num_shapes > 1 && sim->env_shape != nullptr)   // per-env body shapes (SMPL family)
            return sim_launch_jt<STEP, PHC_JT_SPHERICAL, true, false, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
    sim_launch_jt<STEP, PHC_JT_SPHERICAL, false, WRENCH, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed, wr, dr);
    }
}

static inline int32_t launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
