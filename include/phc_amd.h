/* phc_amd.h -- C ABI of libphc_amd.so: the MI355X-native humanoid env-step hot path.
 *
 * The reference (ZhengyiLuo/PHC) is pure Python; its boundary for this path is the
 * Isaac Gym tensor API seen by the task plus the task's own
 * @torch.jit.script functions.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  All pointers are DEVICE pointers
 * (HBM) unless a field says "host"; `stream` is a hipStream_t passed as void*.  No torch
 * types cross this boundary: the host side (phc_amd/*.py, ctypes) hands over
 * tensor.data_ptr() values and the current stream.
 *
 * Return value: 0 on success, a negative PHC_E* code on argument errors, or the positive
 * hipError_t of a failed launch.
 *
 * Layouts are the reference's (Isaac Gym) layouts so that torch views with the same
 * shapes as `humanoid.py:201-235` alias these buffers:
 *   root_states      f32 [N,13]      pos3 quat4(xyzw) linvel3 angvel3        (S1)
 *   dof_state        f32 [N,D,2]     (pos, vel) pairs; spherical joints = exp-map (S2)
 *   rigid_body_state f32 [N,NB,13]   pos3 quat4 linvel3 angvel3 per body      (S3)
 *   contact_force    f32 [N,NB,3]                                             (S4)
 *   dof_force        f32 [N,D]                                                (S5)
 */
#ifndef PHC_AMD_H
#define PHC_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHC_ABI_VERSION 37
#define PHC_MAX_BODIES 64   /* bodies (incl. extended reference bodies) per articulation; also the slot count of the model tables */
#define PHC_EINVAL (-1)
#define PHC_EUNSUPPORTED (-2)
#define PHC_RESET_SUBLISTS 16
#define PHC_RESET_COUNT_STRIDE 32   /* ints between two sub-list counters: one 128-byte line each */

/* Compiled articulation (phc_amd/model.py: ArticulationModel.pack()).  Replaces
 * gym.load_asset / get_actor_dof_properties / get_actor_rigid_body_properties
 * (phc/env/tasks/humanoid.py:768-990,1093-1106). */
typedef struct {
    int32_t num_bodies;       /* NB <= PHC_MAX_BODIES; up to 32 bodies an env takes 32 lanes (two envs per wavefront), above one wavefront */
    int32_t num_dof;          /* D */
    int32_t max_level;        /* tree depth */
    int32_t num_contact_pts;
    const int32_t* ints;      /* packed tables, see model.py pack() */
    const float* floats;
    int32_t num_collision_pairs; /* body pairs that may collide (listed after the int tables); capacity 576 (NB <= 32) / 1152, see phc_sim_step */
    /* Per-env body shapes (robot.has_shape_variation, humanoid.py:726-766,824-866): K compiled articulations with ONE topology (names,
     * parents, joint types) but their own link offsets, masses, inertias, gains, collision geometry.  ints / floats then hold K blocks
     * int_stride / float_stride elements apart, phc_sim_state_t.env_shape picks an env's block, and the scalar fields above are the
     * maxima over the shapes.  num_shapes <= 1: one model for all envs. */
    int32_t num_shapes;
    int32_t int_stride;
    int32_t float_stride;
    int32_t max_body_contact_pts; /* ABI 36: the largest number of ground-contact points any one body carries (int table 9; the maximum over the shapes).  The per-point
                                   * masks of the solver are finite: phc_sim_step returns PHC_EUNSUPPORTED for contact_model 1 above 32 (c_active / c_removed) and for
                                   * inertia_lag above 64 (c_touch: the tail points of a lagged sub-step would lose their force while their impedance stays in I^A) */
    int32_t sim_plain_facts;      /* what phc_sim_model_facts returned for the HOST copy of these tables (PHC_SIM_FACTS_PLAIN), or 0 = not examined: the stepper's launch
                                   * chooser cannot read the device tables, so the model facts of csrc/phc_sim_plain.h travel with the struct.  The field takes what was
                                   * the struct's tail padding: size and layout of ABI 37 are unchanged, and a caller that zero-fills the struct gets the generic kernels */
} phc_model_t;
#define PHC_SIM_FACTS_PLAIN 0x504c4e01

/* Flat reference-motion buffer.  Replaces MotionLibBase's gts/grs/lrs/gvs/gavs/dvs tensors
 * (phc/utils/motion_lib_base.py:300-318; H1/G1: motion_lib_real.py:196-215).  One record per frame, fields contiguous:
 *   [pos (NB+E)*3 | rot (NB+E)*4 | vel NB*3 | angvel NB*3 | joints | dof_vel | pad]
 *   joints / dof_vel = local_rot NB*4 / (NB-1)*3 for spherical models (dofs_per_joint 3: dof_pos is the exp-map of the
 *   slerped local rotation), dof_pos ND / ND for revolute models (dofs_per_joint 1: linear blend, motion_lib_real.py:285-291);
 *   E = num_ext_bodies reference-only bodies (H1 hands / head) appended to the position and rotation blocks.
 * One lookup touches one contiguous run instead of six (ten) separate tensors. */
typedef struct {
    const float* frames;              /* [F, frame_stride] */
    int64_t num_frames_total;         /* F */
    int32_t frame_stride;             /* floats per frame record */
    int32_t num_bodies;
    int32_t num_motions;              /* one clip per env (motion_lib_base.py:205-216) */
    const float* motion_lengths;      /* [M] seconds */
    const float* motion_dt;           /* [M] */
    const int64_t* motion_num_frames; /* [M] */
    const int64_t* length_starts;     /* [M] first frame of each clip */
    int32_t num_ext_bodies;           /* E (0 for SMPL) */
    int32_t dofs_per_joint;           /* 3 spherical (0 is read as 3), 1 revolute */
} phc_motion_lib_t;

/* Simulator-owned state tensors (S1-S5, S8).  Float tensors need 4-byte alignment only; with root_states, dof_state, rigid_body_state, contact_force and
 * dof_force all 16-byte aligned phc_sim_step takes its staged epilogue (same values, wider stores). */
typedef struct {
    int32_t num_envs;
    float* root_states;
    float* dof_state;
    float* rigid_body_state;
    float* contact_force;
    float* dof_force;
    float* pd_target;                 /* [N,D] set_dof_position_target_tensor (humanoid.py:1559-1560) */
    float* force_sensor;              /* [N,S,6] S6: gym.acquire_force_sensor_tensor (humanoid.py:183-190), force then torque of each sensor in
                                         the sensor body's LOCAL frame (create_humanoid_force_sensors :1031-1040: identity pose on the
                                         body, use_world_frame False); nullable.  Written by phc_sim_step at the end of the step: the net
                                         ground-contact wrench on the body about its origin (PhysX's reading is closed: parity unpinned) */
    const int32_t* env_shape;         /* [N] shape block of each env (phc_model_t.num_shapes > 1); nullable = block 0 */
    const float* pd_ref;              /* [N,D] env.res_action (humanoid_im.py:1094-1099): non-null = residual actions, pd_tar = pd_ref +
                                         scale * action limited to the current joint position +- pi / 2; the caller passes the task's
                                         ref_dof_pos (phc_im_buffers_t.ref_dof_pos, the reference pose of the next frame); nullable */
} phc_sim_state_t;

/* Solver parameters.  Replaces gymapi.SimParams as filled by parse_sim_params
 * (phc/run_hydra.py:76-111, phc/data/cfg/sim/default_sim.yaml). */
typedef struct {
    float sim_dt;                     /* physx.step_dt, 1/60 */
    int32_t substeps;                 /* 2 */
    int32_t control_freq_inv;         /* simulate() calls per env step, 2 */
    float gravity_z;                  /* -9.81 */
    float contact_stiffness;          /* penalty ground contact, N/m */
    float contact_damping;            /* N s/m */
    float friction;                   /* mu (plane static=dynamic=1, env_im.yaml) */
    float friction_viscous;           /* regularised Coulomb: tangential damping N s/m before the cone clamp */
    float angular_damping;            /* asset_options.angular_damping 0.01 (humanoid.py:819-822) */
    float max_angular_velocity;       /* 100 */
    float contact_offset;             /* 0.02: contact activates this far above the plane with zero force */
    int32_t control_mode;             /* 0: implicit position drive (`isaac_pd`, S8); 1: `pd` -- explicit torque
                                         clip(kp (target - q) - kd qd, +-limit) recomputed every simulate call (S9,
                                         humanoid.py:1575-1599,1608-1616; robot_control.yaml); 2: as 1 but only the spring
                                         term is held, the damper follows the joint rate implicitly (stable on light
                                         links).  1 and 2: revolute models only. */
    float limit_stiffness;            /* joint-limit penalty spring N m/rad outside [lower, upper] (revolute models; 0 = off) */
    float limit_damping;              /* N m s/rad */
    int32_t self_collision;           /* 1: penalty contact between the collision capsules of non-adjacent bodies (robot.has_self_collision,
                                         humanoid.py:1205-1226), explicit in time with k = self_stiffness_scale * mu / dt^2 per pair
                                         (mu = reduced mass) and damping ratio self_damping_ratio */
    float self_stiffness_scale;       /* <= 1 (explicit stability bound is 4); default 0.25 */
    float self_damping_ratio;         /* default 0.5 */
    int32_t lane_mapping;             /* stepper thread mapping: one body per lane (32 lanes per env, 2 envs per wavefront; NB > 32: 64 lanes, 1 env).
                                         0 / 1 = the product kernel (two wavefronts per SIMD); 3 = the same kernel compiled for three wavefronts per
                                         SIMD (SMPL-family penalty kernel only; measured slower at every env count, profiles/r04_stepper/occupancy_2_vs_3_waves_per_simd.txt --
                                         an experiment knob); other values PHC_EUNSUPPORTED (2 was the two-bodies-per-lane kernel, removed in ABI 31) */
    int32_t num_force_sensors;        /* S <= 4: force sensors (env.force_sensor_joints, default L_Ankle / R_Ankle, humanoid.py:268) */
    int32_t force_sensor_body[4];     /* body id of each sensor */
    /* ---- ABI 34: ground-contact model (solver.contact) ----
     * 0 = penalty spring-damper with regularised Coulomb friction (contact_stiffness / contact_damping / friction_viscous above).
     * 1 = rigid ("tgs"): what parse_sim_params asks PhysX for (phc/run_hydra.py:88-91 solver_type 1 = TGS, num_position_iterations 4,
     *     phc/data/cfg/sim/default_sim.yaml contact_offset / bounce_threshold_velocity / max_depenetration_velocity) restated for the
     *     articulated-body recursion: a velocity-level unilateral constraint per contact point, u_n(t + dt) >= v_target, enforced through
     *     the impedance contact_impedance (N s/m; its compliance 1 / c is the constraint's CFM), v_target = min(depth / dt,
     *     max_depenetration_velocity) for a penetrating point, -gap / dt for a speculative one inside contact_offset, and
     *     -restitution * u_n(t) when the approach speed exceeds bounce_threshold_velocity; Coulomb cone |F_t| <= mu F_n evaluated on the
     *     END-of-step normal force and slip velocity; active set and cone are found by contact_iterations fixed-point passes, each an exact
     *     O(n) articulated-body solve of the whole tree with the contact impedances of the previous pass. */
    int32_t contact_model;
    int32_t contact_iterations;       /* passes per sub-step in model 1 (PhysX num_position_iterations: 4); >= 2 (a single pass never re-evaluates the active set
                                         or the friction cone on predicted velocities: PHC_EINVAL) */
    float contact_impedance;          /* model 1: N s/m per contact point (default 1e5: dt * c = 833 kg of apparent mass per point) */
    float max_depenetration_velocity; /* m/s (default_sim.yaml: 10) */
    float bounce_threshold_velocity;  /* m/s (default_sim.yaml: 0.2) */
    float restitution;                /* plane / shape restitution (env_im.yaml plane.restitution: 0) */
    /* ---- ABI 35 ---- */
    int32_t inertia_lag;              /* 1 (solver.inertia_lag; contact_model 0 only): the articulated inertias I^A and the joint-space inverses are formed in the FIRST
                                         sub-step of every simulate() call and kept over its other sub-steps, which only redo the bias-force recursion
                                         (forces, drives and velocity products at the current state; a third of the backward sweep's arithmetic).  The kept
                                         I^A is O(dt) old, the velocities it produces differ by O(dt^2) per sub-step: the scheme stays first-order consistent
                                         (tests/test_dynamics.py: dt-convergence with the switch on).  A ground-contact point that starts to touch in a
                                         lagged sub-step joins at the next fresh one (its impedance is not in the kept I^A).  0 = every sub-step fresh.
                                         The host side (HumanoidIm) sets 1 by default for contact_model 0 since round 6: pinned against the double-precision build
                                         of this recursion (oracle/hostemu/hostemu64.cpp; tests/test_stepper_options.py), and that build -- like the HIP kernel
                                         directly -- against an independent fp64 statement of the lagged scheme, oracle/aba_oracle.py
                                         (tests/test_aba_oracle.py, tests/test_lag_regimes.py). */
    int32_t force_average;            /* 1 (solver.force_average): contact_force (S4) and dof_force (S5) are the MEANS over all sub-steps of the env step
                                         (what a power / contact reward integrates over the control interval); 0 = the last sub-step's values -- what Isaac
                                         Gym's tensors hold after simulate() with substeps > 1, as far as its documentation says (humanoid.py:185,193-194) */
} phc_sim_params_t;

/* Imitation-task parameters (phc/env/tasks/humanoid_im.py:37-123, env_im.yaml). */
typedef struct {
    float dt;                         /* control dt = control_freq_inv * sim_dt, as fp32 */
    int32_t max_episode_length;       /* episode_length 300 */
    float k_pos, k_rot, k_vel, k_ang_vel, w_pos, w_rot, w_vel, w_ang_vel; /* reward_specs :57 */
    int32_t power_reward;             /* env.power_reward */
    float power_coefficient;          /* :107 */
    int32_t enable_early_termination;
    int32_t use_mean_termination;     /* flags.im_eval and not strict_eval (:1174) */
    int32_t disable_collision_check;  /* flags.no_collision_check */
    int32_t local_root_obs, root_height_obs;
    int32_t num_track_bodies;         /* len(trackBodies) */
    const int32_t* track_slot;        /* [NB] slot of body in trackBodies or -1 */
    const int32_t* reset_mask;        /* [NB] 1 if body in reset_bodies */
    int32_t num_reset_bodies;         /* len(reset_bodies) */
    int32_t first_reset_body;         /* body id of reset_bodies[0]: `termination_distance[0]` of the mean variant (:1586) */
    const float* termination_distances; /* [NB] per body (humanoid_im.py:539-543), live-editable by the learner (im_amp.py:174) */
    int32_t num_key_bodies;
    const int32_t* key_body_ids;      /* [K] */
    int32_t num_amp_joints;           /* joints in dof_subset (19 for SMPL) */
    const int32_t* amp_joint_slot;    /* [NB] slot of joint (body j) in dof_subset order or -1 */
    int32_t num_amp_obs_steps;        /* numAMPObsSteps 10 */
    int32_t num_amp_obs_per_step;     /* 196 */
    int32_t num_self_obs, num_task_obs; /* 358, 576 */
    /* config 3 (getup / MCP composer envs, env_im_getup_mcp.yaml) */
    int32_t cycle_motion;             /* env.cycle_motion: restart the clip in place instead of ending the episode (:1120-1150) */
    int32_t zero_out_far;             /* env.zero_out_far: point-goal reward + task-obs gating when far from the reference (:783-797,890-905) */
    float close_distance;             /* humanoid.py:328 (0.25) */
    float far_distance;               /* humanoid.py:329 (3) */
    /* config 5 (H1 / G1 robots) */
    int32_t dofs_per_joint;           /* 3 spherical (0 is read as 3), 1 revolute: DoF layout of dof_state / AMP obs (humanoid_amp.py:1063-1104) */
    int32_t num_ext_bodies;           /* robot.extend_config entries used by the full-body reward (humanoid_im.py:74-82,916-923) */
    const int32_t* ext_parent;        /* [E] body id of each extended body's parent */
    const float* ext_offset;          /* [E,3] position in the parent frame */
    int32_t obs_v;                    /* task-observation version: 6 (0 is read as 6; `compute_imitation_observations_v6`, humanoid_im.py:1300-1360: 24 floats per
                                         tracked body), 7 (`_v7`, :1362-1393, the keypoint models: position / velocity differences + reference positions, 9),
                                         or 1 / 2 / 3 / 8 / 9 (`compute_imitation_observations`, `_v2`, `_v3`, `_v8`, `_v9`, :1203-1306,1395-1515: 15 J,
                                         15 J + 3 (J - 1), 9 J, 30 J, 18 J + 6 floats; 2 and 9 need the root as the first tracked body) */
    int32_t self_obs_v;               /* 1 (0 is read as 1): compute_humanoid_observations_smpl_max; 3: `_v3` (humanoid.py:2113-2169) = the same
                                         followed by the force-sensor readings [S*6] (num_self_obs grows by 6 S, humanoid.py:683); 2: `_v2`
                                         (:2054-2108): the v1 block for each of the past_track_steps previous body states and the current one,
                                         all relative to the CURRENT root position / heading (num_self_obs = (P + 1) x the v1 size, :513-514) */
    int32_t num_force_sensors;        /* S of phc_sim_state_t.force_sensor (self_obs_v 3) */
    int32_t amp_obs_v;                /* 1 (0 is read as 1): build_amp_observations_smpl; 2: `_v2` (humanoid_amp.py:1015-1059) = the same followed by the
                                         key bodies' heading-local velocities [3 K] (num_amp_obs_per_step grows by 3 K, :303) */
    int32_t remove_base_rot;          /* robot.has_upright_start False: the observation functions strip the asset's base rotation (0.5,0.5,0.5,0.5)
                                         from the root rotation before taking the heading (`remove_base_rot`, humanoid.py:1936-1939 and every
                                         `if not upright:` of humanoid.py / humanoid_amp.py / humanoid_im.py) */
    int32_t num_self_obs_extra;       /* per-env constant columns at the end of the self observation: body-shape parameters
                                         (robot.has_shape_obs, humanoid.py:669-673,2043-2044) then limb weights (has_weight_obs, :676,2046-2047);
                                         counted in num_self_obs */
    int32_t num_amp_obs_extra;        /* the same at the end of every AMP step (has_shape_obs_disc / has_weight_obs_disc, humanoid_amp.py:1005-1008);
                                         counted in num_amp_obs_per_step */
    int32_t num_traj_samples;         /* env.fut_tracks: T = numTrajSamples reference frames in the task observation -- the next one and T - 1 more,
                                         traj_sample_timestep apart (humanoid_im.py:39-47,741-747); obs_v 6 / 7 / 9 (time-major blocks); 0 / 1 = off;
                                         num_task_obs counts all T blocks */
    float traj_sample_timestep;       /* 1 / env.trajSampleTimestepInv (30) */
    int32_t track_body_reward;        /* env.full_body_reward False: the imitation reward runs over the tracked bodies only (humanoid_im.py:925-936:
                                         the `_track_bodies_id` subsets; means over len(trackBodies), no extended bodies) */
    int32_t num_self_obs_hist;        /* P = env.past_track_steps (5) of self_obs_v 2; 0 otherwise */
    int32_t zero_out_far_train;       /* env.zero_out_far_train (with zero_out_far): a reset / a clip restart moves the reference to a random spot of a
                                         5 m disk around the humanoid and arms the cycle counter with zero_out_far_steps (humanoid_im.py:966-980,1133-1140) */
    int32_t zero_out_far_steps;       /* env.zero_out_far_steps (90) */
    int32_t cycle_motion_xp;          /* env.cycle_motion_xp: a clip restart shifts the reference by up to one metre in x and y (:1131-1132) */
    const float* self_obs_extra;      /* [N, num_self_obs_extra] row of the env */
    const float* amp_obs_extra;       /* [N, num_amp_obs_extra] row of the env (observations from simulator state) or of the MOTION (observations
                                         built from the reference clip: the clip carries its humanoid's shape, motion_lib_base.py:244,
                                         humanoid_amp.py:253-284,575-603) -- the same row, clip i belongs to env i */
    const float* amp_ref_table;       /* [F, num_amp_obs_per_step - num_amp_obs_extra] (nullable; ABI 33): the AMP observation of every frame of the motion
                                         library (build_amp_observations of the frame itself), written by phc_amp_ref_table.  With it a reset fills an
                                         env's AMP history from S consecutive ROWS instead of S lookups + observation builds: start times are multiples
                                         of 1/30 s (sample_time_interval) and the history steps back by dt, so on 30 fps clips stepped at dt = k/30 every
                                         history time falls on a frame up to fp32 rounding of the blend factor: exactly 0 for ~5 lookups in 6 (the row IS
                                         the full build then, bit for bit), below 1e-4 for most others (first-order blend with the next row, error
                                         ~1e-6); lookups with any other blend factor (a few % land just below the next frame) are built in full.
                                         NULL: every history frame is looked up and built (robots at 50 Hz). */
} phc_im_params_t;

/* Task-owned per-env buffers (phc/env/tasks/base_task.py:99-105, humanoid_amp.py:109-116,
 * humanoid_im.py:71-121).  int64 where the reference uses torch.long. */
typedef struct {
    int64_t* progress_buf;            /* [N] */
    int64_t* reset_buf;               /* [N] */
    int64_t* terminate_buf;           /* [N] */
    float* rew_buf;                   /* [N] */
    float* reward_raw;                /* [N,4 or 5] */
    float* obs_buf;                   /* [N, num_self_obs+num_task_obs] */
    float* amp_obs_in;                /* [N,S,A] history before this step */
    float* amp_obs_out;               /* [N,S,A] history after this step (ping-pong; may equal amp_obs_in only for reset) */
    const int64_t* sampled_motion_ids;/* [N]; NULL = the identity (env i follows clip i: humanoid_im.py:121) -- saves a dependent load per lookup chain */
    float* motion_start_times;        /* [N] */
    float* motion_start_times_offset; /* [N] */
    float* global_offset;             /* [N,3] */
    float* ref_body_pos;              /* [N,NB,3] side-effect buffers of _compute_task_obs (:855-868), nullable */
    float* ref_body_rot;              /* [N,NB,4] nullable */
    float* ref_body_vel;              /* [N,NB,3] nullable */
    float* ref_dof_pos;               /* [N,D] nullable */
    int32_t* cycle_counter;           /* [N] humanoid_im.py:72,1077-1078,1128,1186; nullable unless cycle_motion */
    int32_t* recovery_counter;        /* [N] humanoid_im_getup.py:62,203-216; nullable (plain HumanoidIm) */
    float* point_goal;                /* [N] humanoid_im.py:95,792,898; nullable unless zero_out_far */
    const float* cycle_phase;         /* [N] the caller's torch.rand draw for _sample_time of cycled envs (:1127); nullable unless cycle_motion */
    /* device-side lists of the envs that finished in the last post-physics launch (nullable): phc_im_post_physics appends every
     * env whose reset flag it sets to one of PHC_RESET_SUBLISTS sub-lists (sub-list = (env / 8) % 16, capacity reset_sublist_cap
     * each) and counts them in reset_count[reset_slot][sub]; phc_im_reset_done then works on exactly those envs (dense wavefronts
     * instead of a masked sweep over all envs) and zeroes reset_count[(reset_slot + 1) % 3][*] for the next step -- the caller
     * rotates reset_slot 0,1,2 per step. */
    int32_t* reset_list;              /* [PHC_RESET_SUBLISTS * reset_sublist_cap] */
    int32_t* reset_count;             /* [3, PHC_RESET_SUBLISTS, PHC_RESET_COUNT_STRIDE], counter in element 0 */
    int32_t reset_slot;
    int32_t reset_sublist_cap;        /* >= 8 * ceil(ceil(N / 8) / PHC_RESET_SUBLISTS) */
    float* body_state_hist;           /* [N, P, NB, 13] self_obs_v 2: the P previous rigid-body states, oldest first (`_rigid_body_*_hist`,
                                         humanoid.py:229-232,1621-1631); shifted by the post-physics launch, filled by the resets; nullable otherwise */
    const float* offset_rand;         /* [N,2] the caller's torch.rand draw for the random reference offsets of zero_out_far_train / cycle_motion_xp
                                         (row of the env; refreshed by the caller before every launch that may use it); nullable unless one is set */
    const uint8_t* occl_mask;         /* [N, J] env.occl_training (humanoid_im.py:96-97,796-804,845-851,1081-1092,1180-1181): non-zero = the tracked body
                                         (slot order) is occluded: its reference state in the task observation and its reference position in
                                         the early-termination distance are the simulated ones; the caller keeps the mask; nullable */
    int64_t amp_env_stride;           /* floats between two envs' AMP history windows; 0 = S * P (plain [N,S,P] buffers).  Larger: every env owns a strip of
                                         more than S frames and amp_obs_in / amp_obs_out point at window positions inside env 0's strip.  When
                                         amp_obs_out + P == amp_obs_in (the new window starts one frame before the old one) phc_im_post_physics
                                         writes the new frame only -- the history shift of humanoid_amp.py:662-670 (14 KB of traffic per env and
                                         step) is then implicit; the caller moves the window back to the end of the strip every (strip - S) steps
                                         with one ordinary shifting call (HumanoidIm: strips of 2 S frames) */
    uint64_t* reset_rng_counter;      /* [1] device-side call counter of phc_im_reset_done (nullable).  Non-null: the start-time draws of a call are keyed by
                                         (seed, *reset_rng_counter) -- the counter argument is ignored -- and phc_im_post_physics advances it by one -- a launch captured in
                                         a hipGraph then draws fresh phases on every replay (the host-side counter argument is frozen at capture) */
} phc_im_buffers_t;

int32_t phc_abi_version(void);

/* M9: MotionLibBase.get_motion_state (phc/utils/motion_lib_base.py:437-520; robots: MotionLibReal.get_motion_state,
 * motion_lib_real.py:236-361) incl. M8 _calc_frame_blend (:549-559).  Outputs nullable.  n lookups; offset nullable [n,3].
 * dof_pos / dof_vel are [n,ND]; rg_pos_ext / rb_rot_ext [n,E,3/4] are the extended bodies' part of rg_pos_t / rg_rot_t. */
int32_t phc_motion_state(const phc_motion_lib_t* lib, int32_t n, const int64_t* motion_ids, const float* motion_times,
                         const float* offset, float* rg_pos /*[n,NB,3]*/, float* rb_rot /*[n,NB,4]*/,
                         float* body_vel /*[n,NB,3]*/, float* body_ang_vel /*[n,NB,3]*/, float* dof_pos /*[n,ND]*/,
                         float* dof_vel /*[n,ND]*/, int64_t* frame_idx0 /*[n]*/, int64_t* frame_idx1 /*[n]*/,
                         float* blend /*[n]*/, float* rg_pos_ext /*[n,E,3]*/, float* rb_rot_ext /*[n,E,4]*/, void* stream);

/* M7: MotionLibBase.sample_time_interval (motion_lib_base.py:414-423); `phase` is the
 * caller's torch.rand draw so the reference RNG stream is preserved. */
int32_t phc_sample_time_interval(const phc_motion_lib_t* lib, int32_t n, const int64_t* motion_ids, const float* phase,
                                 float* motion_times, void* stream);

/* A2 + S8 + S10 + S7: pre_physics_step's action->PD target (humanoid.py:1522-1572,1711-1713),
 * then control_freq_inv x gym.simulate (humanoid.py:1602-1619) with `substeps` sub-steps each,
 * then publication of body state / dof force / contact force (humanoid_amp.py:639-660).
 * actions nullable (then pd_target is used as is).  freeze_mask [D] nullable: 1 -> target forced to 0
 * (humanoid.py:1549-1554). */
int32_t phc_sim_step(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim,
                     const float* actions /*[N,D]*/, const float* pd_action_offset /*[D]*/, const float* pd_action_scale /*[D]*/,
                     const int32_t* freeze_mask /*[D]*/, int32_t num_sim_calls, void* stream);

/* phc_sim_step with an EXTERNAL WRENCH per rigid body (gym.apply_rigid_body_force_tensors in ENV_SPACE, phc/env/tasks/base_task.py:372-381; an addition to
 * ABI 37).  ext_force [N,NB,3] in newtons acts at each body's CENTRE OF MASS, ext_torque [N,NB,3] in newton metres; both in env (= world) axes, each nullable.
 * The wrench is constant over every sub-step of the first wrench_sim_calls simulate calls of the launch (clamped to 0..num_sim_calls; the gym clears applied
 * forces after one simulate(), so a binding passes 1).  With both pointers NULL or wrench_sim_calls == 0 the call IS phc_sim_step: same checks, same launch,
 * same bits.  The tensors are only read, and only at the [env, body] entries that exist.
 * The wrench enters the bias force of the articulated-body recursion and nothing else: it depends on no state and adds no impedance, so the lagged sub-steps
 * (inertia_lag) and every pass of the rigid contact model take it unchanged.  It is NOT part of contact_force (S4), force_sensor (S6) or dof_force (S5): those
 * publish ground and body-body contact and the joint drives, as without a wrench.
 * Both joint families, both group widths, both contact models, lag on and off.  PHC_EUNSUPPORTED (with a wrench): per-env body shapes
 * (phc_model_t.num_shapes > 1) and lane_mapping 3. */
int32_t phc_sim_step_wrench(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim,
                            const float* actions /*[N,D]*/, const float* pd_action_offset /*[D]*/, const float* pd_action_scale /*[D]*/,
                            const int32_t* freeze_mask /*[D]*/, int32_t num_sim_calls,
                            const float* ext_force /*[N,NB,3]*/, const float* ext_torque /*[N,NB,3]*/, int32_t wrench_sim_calls, void* stream);

/* The PLAIN launch of the stepper (csrc/phc_sim_plain.h; additions to ABI 37, which stays 37): phc_sim_step launches an instantiation of its kernel with the launch
 * options, the nullable pointers and the tree constants of the default SMPL task as compile-time constants when every entry of that list holds for the caller's
 * structs and arguments.  That kernel also forms what is fixed for a launch -- the implicit drive diagonals -- once instead of in every sub-step.  The translation unit is compiled with fast-math like the generic one: results agree within the stepper's tolerance against its double-precision
 * recursion, not bit for bit.  Every other launch (and phc_sim_step_wrench with a wrench) runs the generic kernels as before.
 * phc_sim_model_facts: `model` with ints / floats at HOST addresses -> PHC_SIM_FACTS_PLAIN if the tables satisfy the model facts of the list (counts, solver tree,
 *   one shape block, <= 32 contact points per body, every joint with equal per-axis kp, kd and armature), else 0.  The caller stores it in phc_model_t.sim_plain_facts
 *   of the struct it launches with (phc_amd/abi.py model_struct does).
 * phc_sim_is_plain: 1 if structs and arguments satisfy the predicate, else 0 (a null struct: 0).  It does not look at the switch below.
 * phc_sim_force_generic: a process-wide HOST switch; on != 0 sends plain launches through the generic kernel too (A/B comparisons); returns the previous value.
 *   The instrumented build (-DPHC_SIM_PROFILE) starts with it on.  A launch captured in a hipGraph holds the kernel chosen at capture. */
int32_t phc_sim_model_facts(const phc_model_t* model_on_host);
int32_t phc_sim_is_plain(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                         const int32_t* freeze_mask, int32_t num_sim_calls);
int32_t phc_sim_force_generic(int32_t on);

/* S7 alone: forward kinematics from (root_states, dof_state) to rigid_body_state. */
int32_t phc_refresh_body_state(const phc_model_t* model, const phc_sim_state_t* sim, void* stream);

/* S7 for a list of envs (after a teleport of root_states / dof_state: gym.set_*_indexed + refresh): rigid_body_state of the `num` listed envs (any order, each
 * < num_envs), every other row untouched.  num == 0 returns 0 and num < 0 or a null list with num > 0 PHC_EINVAL, all without a launch. */
int32_t phc_refresh_body_state_indexed(const phc_model_t* model, const phc_sim_state_t* sim, int32_t num, const int64_t* env_ids,
                                       void* stream);

/* post_physics_step of HumanoidIm in one launch (humanoid.py:1634-1650, humanoid_amp.py:194-210,
 * humanoid_im.py:694-948,1117-1190): progress_buf += 1, reference lookup at t and t+dt,
 * imitation + power reward, reset / terminate, self obs, task obs v6, AMP obs + history shift. */
int32_t phc_im_post_physics(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                            const phc_sim_state_t* sim, const phc_im_buffers_t* buf, void* stream);

/* phc_im_params_t.amp_ref_table: row f = AMP observation (without the per-env extra columns) of the lookup (f0 = f, f1 = next_frame[f], blend 0), i.e.
 * of a time that falls on frame f of its clip; next_frame[f] = f + 1, or f at the last frame of a clip (the pair matters even at blend 0: the
 * reference's slerp returns the MEAN of two nearly equal rotations whatever the blend factor, isaacgym torch_utils slerp).
 * Rebuild after every (re)load of the motion library and whenever prm's AMP options change. */
int32_t phc_amp_ref_table(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int64_t num_frames,
                          const int64_t* next_frame /*[num_frames]*/, float* table /*[num_frames, A - extra]*/, void* stream);

/* Humanoid.reset(env_ids) -> _reset_envs (humanoid.py:585-621, humanoid_amp.py:378-398,508-528,559-637,
 * humanoid_im.py:955-1023): per listed env sample a start time from `phase`, impose the reference
 * state on root/dof/body tensors and PD targets, zero progress/reset/terminate/contact, recompute
 * obs for those envs, and rebuild their AMP history from the reference motion.
 * env_ids == NULL selects the MASKED mode: num_reset must be num_envs, phase is [num_envs], and exactly the envs
 * with reset_buf != 0 are reset (lets a rollout loop reset done envs without a device->host sync); in this mode
 * reset_buf itself is left untouched (the caller zeroes it after the launch). */
int32_t phc_im_reset(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                     const phc_sim_state_t* sim, const phc_im_buffers_t* buf, int32_t num_reset,
                     const int64_t* env_ids, const float* phase /*[num_reset]*/, int32_t start_at_zero, void* stream);

/* The PLAIN feature set (csrc/phc_im_plain.h; additions to ABI 37, which stays 37): the values the feature selectors of phc_im_params_t / phc_im_buffers_t have in the
 * default SMPL imitation task.  phc_im_post_physics, phc_im_reset and phc_im_reset_done launch an instantiation of their kernel with those selectors as
 * compile-time constants when every listed field of the caller's structs has its listed value, the joints are spherical and an env takes 32 lanes -- the same
 * results bit for bit (no fast-math, no contraction in that translation unit), fewer registers and branches.  Any other task runs the generic kernels as before.
 * phc_im_is_plain: 1 if the structs satisfy the predicate, else 0 (a null struct: 0).  It looks at the structs only, not at the switch below.
 * phc_task_force_generic: a process-wide HOST switch; on != 0 sends plain tasks through the generic kernels too (A/B comparisons); returns the previous
 * value.  A launch captured in a hipGraph holds the kernel chosen at capture. */
int32_t phc_im_is_plain(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_im_buffers_t* buf);
int32_t phc_task_force_generic(int32_t on);

/* `reset_done()`: phc_im_reset's masked mode with the start-time phase drawn INSIDE the kernel, so that the rollout idiom
 * "reset the envs that are done" is one launch with no host round trip and no auxiliary torch kernels:
 * phase(env) = 24-bit uniform from a 32-bit avalanche hash of env under the stream key splitmix64(seed, counter) (like
 * torch.rand: 24 mantissa bits).  The caller advances `counter` per call. */
int32_t phc_im_reset_done(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                          const phc_sim_state_t* sim, const phc_im_buffers_t* buf, uint64_t seed, uint64_t counter,
                          int32_t start_at_zero, void* stream);

/* HumanoidImGetup._reset_fall_episode + the shared tail of _reset_envs (humanoid_im_getup.py:166-196, humanoid.py:585-621,
 * humanoid_amp.py:559-573): the caller has written root_states / dof_state of the listed envs (a stored fall state);
 * after phc_refresh_body_state_indexed made their rigid_body_state current, this call zeroes
 * progress/reset/terminate/contact, sets the PD target to the joint positions, recomputes their observations against
 * the reference at the env's (unchanged) motion clock and recomputes the current AMP observation; fill_history != 0
 * copies it into every history slot (_init_amp_obs_default) -- 0 is the "recovery episode" case (:160-164) where the
 * env keeps its state and its AMP history. */
int32_t phc_im_reset_from_state(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm,
                                const phc_sim_state_t* sim, const phc_im_buffers_t* buf, int32_t num_reset,
                                const int64_t* env_ids, int32_t fill_history, void* stream);

/* HumanoidAMP.build_amp_obs_demo (humanoid_amp.py:253-284): n samples x S steps back in time. */
int32_t phc_amp_obs_demo(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int32_t n,
                         const int64_t* motion_ids, const float* motion_times0, float* amp_obs_demo /*[n,S,A]*/, void* stream);

/* P5: CommonAgent.discount_values (phc/learning/common_agent.py:493-505), tensors [T,N]. */
int32_t phc_gae(int32_t horizon, int32_t n, const float* fdones, const float* values, const float* rewards,
                const float* next_values, float gamma, float tau, float* advs, void* stream);

/* poselib FK for motion loading (M5): SkeletonState.global_transformation
 * (poselib/poselib/skeleton/skeleton3d.py:390-426) in fp32 on device.  local_rot [T,NB,4],
 * root_trans [T,3] -> global_rot [T,NB,4], global_pos [T,NB,3]. */
int32_t phc_fk(const phc_model_t* model, int64_t num_frames, const float* local_rot, const float* root_trans,
               float* global_rot, float* global_pos, void* stream);

/* P1: RunningMeanStd.forward in train mode (phc/utils/running_mean_std.py:69-111) on a device batch x [rows, cols] fp32 -- or, with
 * row_index [rows] (int64), on the minibatch x[row_index] of a larger tensor without materialising it (the dataset gather of
 * common_agent.py:357-398 folded into the pass):
 *   out = clamp((x - float(norm_mean)) / sqrt(float(norm_var) + epsilon), -clamp, clamp)      (:95-96; fp32 or bf16 [rows, cols], may be NULL)
 *   run_mean / run_var / run_count (fp64, in place; NULL = no update, eval mode or frozen) <- parallel-variance update with the batch
 *   mean and unbiased variance (:56-67,100-104).  norm_* may alias run_* (output from the statistics BEFORE the update, as the
 *   reference computes it) or be a frozen copy (amp_agent.py:527-532 `running_mean_std_temp`).
 * out_stride (ABI 23): elements between two output rows (0 = cols): the output may be the left columns of a wider buffer whose K is
 *   padded to a GEMM-friendly multiple (934 -> 1024: the first-layer GEMMs of the update run 20-30 % faster, profiles/r02_notes.md).
 * workspace: phc_running_norm_workspace(rows, cols) bytes of device memory (only used when updating); its LAST 8 bytes (a ticket
 * counter of the finishing kernel) must be zero before the first call and are left at zero. */
int64_t phc_running_norm_workspace(int64_t rows, int32_t cols);
int32_t phc_running_norm(const float* x, const int64_t* row_index, int64_t rows, int32_t cols, const double* norm_mean, const double* norm_var, float epsilon,
                         float clamp, void* out, int32_t out_bf16, int32_t out_stride, double* run_mean, double* run_var, double* run_count,
                         double* workspace, void* stream);

/* Column sums of a bf16 matrix x [rows, cols] -> out fp32 [cols]: the bias gradient of a linear layer (autograd's `sum(0)` of
 * the output gradient, AddmmBackward).  workspace: phc_colsum_workspace(rows, cols) bytes. */
int64_t phc_colsum_workspace(int64_t rows, int32_t cols);
int32_t phc_colsum_bf16(const void* x, int64_t rows, int32_t cols, float* out, float* workspace, void* stream);
/* The same behind a ReLU whose output `y` was saved (round 2: layers whose ReLU rides in the GEMM epilogue): gm = gy where y > 0 else 0
 * (torch's ThresholdBackward, phc/learning/network_builder.py:126-137 `activation: relu`) written as bf16 [rows, cols], and its column sums
 * (the bias gradient) -- one pass instead of two.  Same workspace size. */
int32_t phc_colsum_relu_bf16(const void* gy, const void* y, int64_t rows, int32_t cols, void* gm, float* out, float* workspace, void* stream);
/* ABI 35: `out` == NULL in phc_colsum_bf16 / phc_colsum_relu_bf16 / `gw_gb` == NULL in phc_linear1_backward runs the FIRST stage only -- the per-chunk partial
 * sums stay in `workspace`, [phc_colsum_chunks(rows)] (resp. [phc_linear1_chunks(rows)], `cols + 1` wide) rows -- and phc_colsum_finish_batch later finishes
 * up to any number of such sums in one launch per PHC_COLSUM_MAX_JOBS of them: the bias gradients of a backward pass (autograd's AccumulateGrad of
 * `AddmmBackward`'s `sum(0)`, read by nobody before clip_grad_norm_ + Adam, phc/learning/amp_agent.py:669-676) cost one dependent ~5 us launch at the end
 * of the pass instead of one per layer.  `accumulate` != 0 adds to `out` instead of storing. */
#define PHC_COLSUM_MAX_JOBS 16
typedef struct {
    const float* partial;             /* [nchunks, cols] fp32: a first stage's workspace (must stay untouched until the batch has run) */
    float* out;                       /* [cols] fp32 */
    int32_t nchunks, cols, accumulate;
} phc_colsum_job_t;
int32_t phc_colsum_chunks(int64_t rows);
int32_t phc_linear1_chunks(int64_t rows);
int32_t phc_colsum_finish_batch(int32_t count, const phc_colsum_job_t* jobs /* host array */, void* stream);
/* Weight gradient of a linear layer as a split-K batched GEMM (autograd's `grad_output.t() @ input`, AddmmBackward): `part` [slabs, n] bf16 are the
 * slab products; out [n] fp32 receives their sum (accumulate 0) or has it added (accumulate != 0: a parameter's second and later gradient
 * contributions of a step, torch's AccumulateGrad).  part and out 16-byte aligned. */
int32_t phc_sum_slabs_bf16(const void* part, int32_t slabs, int64_t n, float* out, int32_t accumulate, void* stream);
/* ABI 37.  Operand of a split-precision linear layer (`+learning.params.config.actor_precision=split_bf16`; no reference counterpart: the reference's layers are fp32
 * `torch.nn.Linear`s, phc/learning/network_builder.py, and this is the precision option between bf16 and fp32 GEMMs).  x fp32 [rows, cols], rows `ld_in` floats apart,
 * optionally gated (gate fp32, rows `ld_gate` apart: x where gate > 0, else 0 -- the ReLU mask of a backward pass; NULL = no gate), is cut into bf16 head h = bf16(x) and
 * tail l = bf16(x - h) and written as the three chunks ONE bf16 GEMM with a three times longer reduction reads:
 *   out[row * row_stride + c * chunk_stride + col] (bf16), c = 0, 1, 2 = (h, h, l) for order 0, (h, l, h) for order 1,
 * with zeros in columns cols .. cols_pad - 1 and rows rows .. rows_pad - 1.  (x h)(w h) + (x l)(w h) + (x h)(w l) = an order-1 operand against an order-0 one.
 * extra_mode 1 writes the constant 1 into column `cols` of the valid rows, extra_mode 2 writes extra[row] (fp32 [rows]) there (cols_pad > cols then): an activation
 * operand with the ones column against a weight operand carrying the bias in that column makes the bias part of the product, and row `cols` of the weight-gradient
 * product (gradient operand^T x activation operand) is the bias gradient.  extra_mode 0: `extra` unused.
 * cols_pad, row_stride, chunk_stride multiples of 4; out 8-byte aligned. */
int32_t phc_split3_bf16(const float* x, int64_t ld_in, const float* gate, int64_t ld_gate, int64_t rows, int32_t cols, int64_t rows_pad, int32_t cols_pad,
                        const float* extra, int32_t extra_mode, void* out, int64_t row_stride, int64_t chunk_stride, int32_t order, void* stream);

/* Native weight gradient of a bf16 linear layer (csrc/phc_gemm.hip; opt-in, `+learning.params.config.wgrad=native`; additions to ABI 37, which stays 37).
 * For gy, y bf16 [rows, n] (contiguous) and x bf16 [rows, k] whose rows are `ld_x` elements apart (ld_x >= k: K-padded inputs):
 *   gz[r, j]  = y == NULL ? gy[r, j] : (y[r, j] > 0 ? gy[r, j] : 0)        bf16 [rows, n], a select (autograd's ThresholdBackward)
 *   gw[j, c] (=|+=) sum_r gz[r, j] * x[r, c]                                fp32, rows `ld_gw` floats apart (ld_gw >= k)   (AddmmBackward: gz^T x)
 *   gb[j]    (=|+=) sum_r gz[r, j]                                          fp32 [n]
 * on the matrix cores with fp32 accumulation; the rows are cut into phc_wgrad_bf16_slices(rows, n, k) slices (a function of the shape alone) whose fp32
 * partial tiles are added in slice order inside the same launch, so the result is bit-identical from call to call.  `accumulate` / `gb_accumulate`
 * != 0 add to gw / gb instead of storing.
 * May be NULL: y (no mask), gz (not written), gb (not computed).  gz may not alias gy or y.
 * Alignment: bf16 pointers 2 bytes, gw / gb 4 bytes, workspace 16 bytes.  16-byte accesses are used for gy / y / gz when all three are 16-byte aligned and n
 * is a multiple of 8, and for x when it is 16-byte aligned and ld_x and k are multiples of 8; element accesses otherwise (every rows, n, k >= 1 is served).
 * workspace: phc_wgrad_bf16_workspace(rows, n, k) bytes of device memory holding one arrival counter per 128 x 128 output tile (zeroed on `stream` by every
 * call, by a kernel node -- a captured memset node does not replay reliably on this stack --: nothing to initialise), the slices' fp32 tile slabs and their bias partial sums.  It must not be shared by launches that may run concurrently
 * (one per stream).  Null / non-positive arguments return PHC_EINVAL before the device is touched. */
int32_t phc_wgrad_bf16_slices(int64_t rows, int32_t n, int32_t k);
int64_t phc_wgrad_bf16_workspace(int64_t rows, int32_t n, int32_t k);
int32_t phc_wgrad_bf16(const void* gy, const void* y, const void* x, int64_t ld_x, int64_t rows, int32_t n, int32_t k, float* gw, int64_t ld_gw,
                       int32_t accumulate, void* gz, float* gb, int32_t gb_accumulate, void* workspace, void* stream);

/* Discriminator loss pieces (phc/learning/amp_agent.py:732-808 `_disc_loss`).
 * phc_disc_bce: logits [n_agent + n_demo] (agent and replay rows first, demo rows last; bf16 or fp32):
 *   stats[0] = scale * 0.5 (BCEWithLogits(agent, 0) + BCEWithLogits(demo, 1)), stats[1] = mean(agent < 0), stats[2] = mean(demo > 0),
 *   stats[3] = mean(agent logits), stats[4] = mean(demo logits) (ABI 36: `stats` holds 5 floats; the reference's `disc/agent_logit`, `disc/demo_logit`
 *   scalars, amp_agent.py:911-912);
 *   grad [same shape / type] = d stats[0] / d logits.
 * phc_weighted_sumsq: out[0] = sum_i coefs[i] * |tensors[i]|^2 over count <= 4 device tensors of sizes[i] elements (all fp32 or all
 *   bf16): the logit regulariser + weight decay in one pass, or -- one bf16 tensor, coef = c / rows -- the gradient penalty
 *   c * mean_rows(sum_cols g^2).  out[1 + i] = |tensors[i]|^2 (ABI 20: `out` holds 1 + count floats; the last one of the weight call
 *   is the reference's `disc_logit_loss`, amp_agent.py:757-758).  workspace: phc_sumsq_workspace() bytes. 
 * (Round 6: one block per 1024 logits, the last block to finish adds the per-block sums; they live in a static device buffer, so launches of phc_disc_bce on DIFFERENT streams
 * of one process must not overlap.) */
int32_t phc_disc_bce(const void* logits, int32_t is_bf16, int32_t n_agent, int32_t n_demo, float scale, void* grad, float* stats,
                     void* stream);
int64_t phc_sumsq_workspace(void);
int32_t phc_weighted_sumsq(int32_t count, const void* const* tensors, const int64_t* sizes, const float* coefs, int32_t is_bf16, float* out,
                           double* workspace, void* stream);

/* Rollout bookkeeping of one env step (phc/learning/amp_agent.py:321-341 inside play_steps; rl_games' current_rewards / current_lengths):
 *   exp_rewards[i] = reward_scale * rewards[i];  exp_dones[i] = dones[i] != 0;  terminated_mask[i] = terminate[i] != 0 (the mask of the
 *   next-value write, :327-329);  terminated_flags[i] += terminated_mask[i];  reward_raw_acc[k] += mean_i reward_raw[i, k];
 *   current_rewards[i] = (current_rewards[i] + rewards[i]) * (1 - done);  current_lengths[i] = (current_lengths[i] + 1) * (1 - done). */
int32_t phc_rollout_bookkeeping(const float* rewards, float reward_scale, const int64_t* dones, const int64_t* terminate, const float* reward_raw,
                                int32_t num_reward_terms, int64_t num_envs, float* exp_rewards, uint8_t* exp_dones, float* terminated_flags,
                                float* terminated_mask, float* reward_raw_acc, float* current_rewards, float* current_lengths, void* stream);

/* Rollout policy step (phc/learning/amp_agent.py:309-341 with rl_games' ModelA2CContinuousLogStd in eval mode), per env r:
 *   actions = mu + exp(logstd) * noise, mus = mu, sigmas = exp(logstd), neglogp = neglogp(actions | mu, sigma)            (mu != NULL)
 *   values[r] = unnorm(value[r]) = sqrt(float(value_var) + epsilon) * clamp(value[r], -5, 5) + float(value_mean)             (value != NULL;
 *               value_mean == NULL: no un-normalisation), times (1 - mask[r]) when mask is given (next_values of terminated envs).
 * mu [N, D] / value [N] are the network heads (bf16 when is_bf16, else fp32); outputs fp32 (rows of the experience buffer). */
int32_t phc_policy_sample(const void* mu, const void* value, int32_t is_bf16, const float* logstd, const float* noise, const double* value_mean,
                          const double* value_var, float epsilon, const float* mask, int64_t num_envs, int32_t num_actions, float* actions, float* mus,
                          float* sigmas, float* neglogp, float* values, void* stream);

/* Linear layer with one output (the value head `a2c_network.value`, 512 -> 1), bf16: y [rows] = x [rows, cols] w [cols] + b[0];
 * backward: gx [rows, cols] = gy w^T (optional), gw_gb fp32 [cols + 1] = (gy^T x, sum gy).  workspace: phc_linear1_workspace(). */
int64_t phc_linear1_workspace(int64_t rows, int32_t cols);
int32_t phc_linear1_forward(const void* x, const void* w, const void* b, int64_t rows, int32_t cols, void* y, void* stream);
int32_t phc_linear1_backward(const void* x, const void* w, const void* gy, int64_t rows, int32_t cols, void* gx, float* gw_gb,
                             float* workspace, void* stream);

/* P9: gradient clipping + optimizer step on the flat fp32 parameter (phc/learning/amp_agent.py:669-676: `clip_grad_norm_(grad_norm)`
 * then `optimizer.step()` with torch.optim.Adam): grad *= min(1, max_norm / (|grad| + 1e-6)) in place (max_norm <= 0: no clipping),
 * then Adam with L2 weight decay; `step` is the 1-based step count (bias corrections computed on the host in fp64).
 * grad_norm_out (optional, device) receives |grad| before clipping (written when max_norm > 0); param_bf16 (optional, [n] bf16) receives the
 * updated parameter rounded to bf16 -- the copy the next step's GEMMs read.  step_device (optional, device int64): incremented by one and used
 * for the bias corrections instead of `step` -- for launches replayed from a captured hipGraph, whose by-value arguments are frozen.
 * Alignment: param, grad, exp_avg and exp_avg_sq need only be 4-byte aligned and param_bf16 2-byte aligned (offset views are fine); 16-byte
 * aligned fp32 arrays with an 8-byte aligned param_bf16 take the vectorised path, with the same per-element arithmetic.
 * workspace: phc_adam_workspace() bytes. */
int64_t phc_adam_workspace(void);
int32_t phc_adam_clip_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int64_t step, float max_norm, double* workspace, float* grad_norm_out,
                           void* param_bf16, int64_t* step_device, void* stream);

/* P8: actor + critic part of the PPO loss and its gradient (phc/learning/amp_agent.py:598-640 with rl_games' neglogp, bound_loss
 * common_agent.py:512-520 and torch_ext.policy_kl), tensors on the device, value_size 1:
 *   loss = mean(max(-adv r, -adv clamp(r, 1 -+ e_clip))) + critic_coef mean(c_loss) - entropy_coef entropy + bounds_loss_coef mean(b_loss),
 *   r = exp(old_neglogp - neglogp(actions | mu, exp(logstd)))
 * mu [B, D] and value [B] are the network heads (bf16 when is_bf16, else fp32); grad_mu / grad_value receive d loss / d mu, d loss / d value
 * in the same type; stats[7] = loss, mean a_loss, mean c_loss, mean b_loss, entropy, mean kl(policy || old policy), mean(|r - 1| > e_clip)
 * (ABI 36: the clip fraction, `actor_clipped` of common_agent.py:570-571 -> `loss/clip_frac`).
 * old_values is only read when clip_value.  row_index (optional, [B] int64): minibatch row r takes actions / old_* / advantages /
 * returns from row row_index[r] of the rollout tensors (mu, value and the gradients stay minibatch-ordered).
 * workspace: phc_ppo_loss_workspace() bytes. */
typedef struct {
    float e_clip, critic_coef, entropy_coef, bounds_loss_coef;
    int32_t clip_value;
} phc_ppo_params_t;
int64_t phc_ppo_loss_workspace(void);
int32_t phc_ppo_loss(const void* mu, const void* value, int32_t is_bf16, const float* logstd, const float* actions, const float* old_neglogp,
                     const float* advantages, const float* returns, const float* old_values, const float* old_mu, const float* old_sigma,
                     const int64_t* row_index, int64_t batch, int32_t num_actions, const phc_ppo_params_t* prm, void* grad_mu, void* grad_value, float* stats,
                     double* workspace, void* stream);

/* Offscreen renderer (csrc/phc_render.hip; additions to ABI 37, which stays 37).  Replaces the reference's camera sensor + video writer of the
 * player (phc/env/tasks/base_task.py:176-195,405-437; humanoid.py:1715-1743 `_init_camera` / `_update_camera`; humanoid_im.py:597-619 markers):
 * a ray caster over the articulation's collision capsules, off the training path.  Each view is a pinhole camera on ONE env; the scene of a view:
 *   * every collision capsule s < num_capsules of the env's shape block (a box is drawn as its capsule stand-in), posed by the owner body's
 *     rigid_body_state row (pos3, xyzw quaternion);
 *   * the ground plane z = 0 with a 1 m two-tone checker: ground_color[(floor(x) + floor(y)) & 1];
 *   * optional marker spheres at markers[env, m]: radius marker_radii[m] and colour marker_colors[m] where those arrays are given, else marker_radius
 *     and marker_color for all (both NULL: the frames of a scene without the two fields, byte for byte); a marker of radius <= 0 is not drawn;
 *   * sky_color where a ray hits nothing.
 * Shading of a hit with unit normal n, base colour C (palette[owner % PHC_RENDER_PALETTE] for a capsule, marker_color, the checker tone):
 *   lit = max(n . light_dir, 0), set to 0 when the shadow ray from (hit + 1e-3 n) toward light_dir enters any capsule or marker at t > 0
 *   (the ground is not an occluder: a light above the horizon is assumed);
 *   rgb = C * (ambient + diffuse * lit), each channel stored as u8 floor(min(max(v, 0), 1) * 255 + 0.5); alpha 255.
 * Ray of pixel (x, y) (row y = 0 at the top): f = |target - eye|^-1 (target - eye), r = |f x up|^-1 (f x up), u = r x f,
 *   d = unit(f + ((2 (x + 0.5) / W - 1) tan(fov_y / 2) W / H) r + ((1 - 2 (y + 0.5) / H) tan(fov_y / 2)) u).
 * Outputs: rgba u8 [V, H, W, 4]; depth f32 [V, H, W] (nullable): t of the first hit along the unit ray, +inf on a miss; hit_id i32 [V, H, W]
 * (nullable): -1 sky, -2 ground, s for capsule s of the env's block, PHC_RENDER_MARKER_ID + m for marker m.  Deterministic (no atomics).
 * PHC_EINVAL before any device work for: a null required pointer (scene, cameras, rgba, body_state, capsules; markers when num_markers > 0),
 * views <= 0, width or height <= 0, width * height > PHC_RENDER_MAX_PIXELS, a camera env outside [0, num_envs), num_capsules outside
 * [1, PHC_RENDER_MAX_SHAPES], num_markers outside [0, PHC_RENDER_MAX_MARKERS], num_bodies outside [1, PHC_MAX_BODIES], num_shape_blocks < 1,
 * a capsule_stride below 8 num_capsules.  An env_shape entry outside [0, num_shape_blocks) selects block 0; a capsule whose owner is outside
 * [0, num_bodies) or whose radius is <= 0 is not drawn. */
#define PHC_RENDER_MAX_PIXELS (1 << 24)   /* width * height of one view */
#define PHC_RENDER_MAX_SHAPES 128
#define PHC_RENDER_MAX_MARKERS 128
#define PHC_RENDER_PALETTE 16
#define PHC_RENDER_MARKER_ID 1000
typedef struct {
    int32_t env;                      /* env whose bodies the view shows */
    float eye[3], target[3], up[3];   /* world frame, metres */
    float fov_y;                      /* vertical field of view, radians */
} phc_camera_t;
typedef struct {
    int32_t num_envs, num_bodies;     /* N, NB */
    const float* body_state;          /* [N, NB, 13] rigid_body_state */
    const float* capsules;            /* [K, capsule_stride]: capsule s of block k at capsules[k * capsule_stride + 8 s]: a[3], b[3] (owner frame), radius, owner (as a float) */
    int32_t num_capsules;             /* S (ArticulationModel.shape_capsules(): primary then extra capsules) */
    int32_t num_shape_blocks;         /* K */
    int64_t capsule_stride;           /* floats between two blocks, >= 8 S */
    const int32_t* env_shape;         /* [N] block of each env (phc_sim_state_t.env_shape); nullable = block 0 */
    const float* markers;             /* [N, M, 3] world positions; nullable when M = 0 */
    int32_t num_markers;              /* M */
    float marker_radius;
    float palette[PHC_RENDER_PALETTE][3];   /* body colours, linear 0..1 */
    float marker_color[3];
    float ground_color[2][3];
    float sky_color[3];
    float light_dir[3];               /* unit vector toward the light */
    float ambient, diffuse;
    const float* marker_radii;        /* [M] radius of each marker; nullable = marker_radius for all */
    const float* marker_colors;       /* [M, 3] colour of each marker, linear 0..1; nullable = marker_color for all */
} phc_render_scene_t;
int32_t phc_render(const phc_render_scene_t* scene /* host */, const phc_camera_t* cameras /* host, [views] */, int32_t views, int32_t width,
                   int32_t height, uint8_t* rgba, float* depth, int32_t* hit_id, void* stream);

/* Renderer with triangle meshes (csrc/phc_render_mesh.hip; an addition to ABI 37, which stays 37): the scene of phc_render plus posed instances
 * of triangle meshes (the robots' visual meshes), each traversed through a bounding-volume hierarchy.  The scene of a view is phc_render's, except:
 *   * every instance i < num_instances is drawn.  Its mesh frame M_i in the world: rotation q = unit(q_body (x) quat_i) (xyzw, Hamilton product;
 *     q_body = body_state[env, owner_i, 3:7] as stored), origin p_body + rotate(q_body, pos_i).  Vertices are never moved: a ray is taken into
 *     the mesh frame.
 *   * a capsule whose owner body owns at least one instance is neither drawn nor casts a shadow; bodies without an instance keep theirs.
 *   * ground, markers, sky, light, shading formula, camera rays and the u8 rounding are phc_render's.
 * Triangle hit: triangle (v0, v1, v2), e1 = v1 - v0, e2 = v2 - v0, g = e1 x e2.  It is two-sided; the point o + t d (t > 0) hits it when its
 * barycentric coordinates u, v satisfy u >= 0, v >= 0, u + v <= 1.  A triangle with |g|^2 <= PHC_RENDER_MESH_MIN_CROSS^2 (m^4) or with d . g = 0
 * is never hit.  Shading is flat: n = the unit of g, taken to the world, flipped so that n . d < 0; the base colour is the instance's rgb.  The
 * shadow ray from (hit + 1e-3 n) is occluded by every drawn capsule, every marker and every instance (the hit triangle's own mesh included).
 * Outputs: hit_id = PHC_RENDER_MESH_ID + i where instance i is hit first; tri_id i32 [V, H, W] (nullable) = tri_perm[k] of the hit triangle k,
 * i.e. its index in the caller's original order, and -1 where no mesh is hit.
 * Ties (deterministic, no atomics; "<" below is on the fp32 t the kernel computes): the first hit is the candidate of smallest t; among equal
 * t a capsule or marker (lowest index) wins over an instance, the lowest instance index wins over a higher one, inside one instance the lowest
 * position k in `triangles` wins, and any shape wins over the ground at equal t.
 * Tree: nodes of one mesh are contiguous and in depth-first order: the first child of an interior node n is n + 1, and skip is the node that
 * follows n's subtree (-1 after the last node of the mesh): traversal is node = (box hit and interior) ? node + 1 : skip, after testing a leaf's
 * triangles.  skip must be > n or -1 (the kernel stops a traversal that would step backwards or leave [0, num_nodes)).  leaf < 0: interior; else
 * leaf = 16 first + count: triangles first .. first + count - 1 (count <= 15) of `triangles`, leaves in increasing `first` along the depth-first
 * order (the tie rule above relies on it).  A box may have zero thickness; a ray direction component may be 0 (then the slab holds the whole ray
 * or none of it, by lo <= o <= hi).  Triangle and vertex indices outside their arrays are never dereferenced (such a triangle is skipped).
 * meshes == NULL or num_instances == 0: rgba / depth / hit_id are phc_render's, byte for byte (the same kernel runs), tri_id is all -1.
 * PHC_EINVAL before any device work for everything phc_render refuses, and for: num_instances outside [0, PHC_RENDER_MAX_INSTANCES];
 * with num_instances > 0: a null instances / instances_dev / vertices / triangles / tri_perm / nodes, num_vertices < 1, num_triangles outside
 * [1, PHC_RENDER_MAX_TRIANGLES], num_nodes outside [1, 2 PHC_RENDER_MAX_TRIANGLES], an instance owner outside [0, num_bodies), an instance root
 * outside [0, num_nodes), nodes not 16-byte aligned; tri_id not 4-byte aligned. */
#define PHC_RENDER_MESH_ID 2000
#define PHC_RENDER_MAX_INSTANCES 128
#define PHC_RENDER_MAX_TRIANGLES (1 << 22)
#define PHC_RENDER_MESH_MIN_CROSS 1.0e-12f   /* m^2: |e1 x e2| at or below it = degenerate, never hit */
typedef struct {
    float lo[3];
    int32_t skip;                     /* node after this subtree, -1 = end of the mesh */
    float hi[3];
    int32_t leaf;                     /* < 0 interior (first child = this + 1); else 16 * first triangle + count */
} phc_bvh_node_t;                     /* 32 bytes, read as two 16-byte loads: the array must be 16-byte aligned */
typedef struct {
    int32_t owner;                    /* body that carries the instance */
    int32_t root;                     /* root node of its mesh */
    float pos[3], quat[4];            /* geom frame in the owner's body frame (xyzw) */
    float center[3], radius;          /* bounding sphere of the mesh, mesh frame */
    float rgb[3];                     /* base colour, linear 0..1 */
} phc_mesh_instance_t;                /* 64 bytes */
typedef struct {
    int32_t num_vertices, num_triangles, num_nodes, num_instances;   /* NV, NT, NN, I */
    const float* vertices;            /* device [NV, 3], mesh frames */
    const int32_t* triangles;         /* device [NT, 3] vertex indices, in leaf order */
    const int32_t* tri_perm;          /* device [NT]: index of triangle k in the caller's original order */
    const phc_bvh_node_t* nodes;      /* device [NN] */
    const phc_mesh_instance_t* instances;       /* HOST [I]: read by the argument checks */
    const phc_mesh_instance_t* instances_dev;   /* device copy of the same [I]: read by the kernel */
} phc_render_meshes_t;
int32_t phc_render_mesh(const phc_render_scene_t* scene /* host */, const phc_render_meshes_t* meshes /* host; nullable */,
                        const phc_camera_t* cameras /* host, [views] */, int32_t views, int32_t width, int32_t height, uint8_t* rgba, float* depth,
                        int32_t* hit_id, int32_t* tri_id /* nullable */, void* stream);

/* Evaluation sweep: tracking metrics accumulated on the device (csrc/phc_eval.hip; an addition to ABI 37, which stays 37).  One launch per env
 * step of a sweep batch replaces the host path's second reference lookup, its two [N, NB, 3] device-to-host copies and the numpy metric pass of
 * learning/im_eval.py (compute_metrics_per_clip).  One lane per body, 32-lane groups up to 32 bodies (64 above), 256-thread blocks.  Per env i:
 *   gt_j   = position of body j of clip motion_ids[i] at t = progress_buf[i] * dt + motion_start_times[i] + motion_start_times_offset[i], plus
 *            global_offset[i]: bit-equal to phc_motion_state's rg_pos (same loads, same blend); written to gt_out when that is given;
 *   pred_j = position of body j in rigid_body_state.  Only the NB simulated bodies take part (no extended reference bodies);
 *   mpjpe_step[i] = mean_j |pred_j - gt_j| (metres), every launch;
 *   while step < clip_steps[i] - 1 (the frames the host path counts; a termination or a reset in mid-batch does not stop it):
 *     count[i] += 1 and sums[i][0..4] += sum_j of, in this order,
 *       |pred_j - gt_j|; the same after subtracting body root_idx from both; the same after the similarity alignment (centre both, proper rotation
 *       with the det sign fix, scale (s1 + s2 + d s3) / sum |p|^2) of the root-relative pred onto the root-relative gt;
 *       the second difference in time of (pred_j - gt_j) (from the third counted frame on); its first difference (from the second on).
 *     Nothing is divided: metric = sums / (frames * NB) with frames = n, n, n, n - 2, n - 1 for count n.
 *   failed[i] |= terminate_buf[i] != 0 && step <= clip_steps[i] - 1   (a termination after the clip's last frame is not a failure);
 *   status[0] = number of envs with failed == 0 after this launch; status[1] = max clip_steps[i] over those of them with i < bound (0: none).
 *     The entry point clears status on `stream` before the kernel; blocks reduce in LDS and add one integer atomic per word.
 * `step` counts the launches of a batch from 0.  history holds the two previous frames (ring slot = step & 1), so the launches of one batch must
 * run in order on one stream; all state is the caller's (zeroed at the start of a batch), nothing is kept in the library.
 * PHC_EINVAL: a null lib / args / required pointer, num_envs < 0, num_bodies outside [1, PHC_MAX_BODIES] or != lib->num_bodies, root_idx outside
 * [0, num_bodies), step < 0, bound outside [0, num_envs]. */
typedef struct {
    int32_t num_envs, num_bodies;             /* N, NB */
    int32_t root_idx;
    int32_t step;                             /* index of this launch within the batch, from 0 */
    int32_t bound;                            /* status[1] only looks at envs below it */
    float dt;                                 /* env step, seconds */
    const float* rigid_body_state;            /* [N, NB, 13] */
    const int64_t* progress_buf;              /* [N] */
    const int64_t* terminate_buf;             /* [N] */
    const int64_t* motion_ids;                /* [N]; nullable = the env's own index */
    const float* motion_start_times;          /* [N] */
    const float* motion_start_times_offset;   /* [N] */
    const float* global_offset;               /* [N, 3] */
    const int32_t* clip_steps;                /* [N] env steps of the env's clip */
    float* history;                           /* [N, 2 slots, 2 (pred, gt), NB, 3] */
    double* sums;                             /* [N, 5] */
    int32_t* count;                           /* [N] */
    int32_t* failed;                          /* [N] */
    int32_t* status;                          /* [2] */
    float* mpjpe_step;                        /* [N] */
    float* gt_out;                            /* [N, NB, 3]; nullable */
} phc_eval_args_t;
int32_t phc_eval_accumulate(const phc_motion_lib_t* lib, const phc_eval_args_t* args /* host */, void* stream);

/* Push schedule on the device (csrc/phc_push.hip, per-lane code csrc/phc_push.h; an addition to ABI 37, which stays 37): one launch is one
 * `advance()` of the schedule of phc_amd/perturb.py -- all state and all random draws live on the device, so a captured launch moves on with
 * every replay.  One lane per env, 256-thread blocks.  Per env i, with k = k[i] the env's own launch count:
 *   u[0..4] = push_draws(key, env_offset + i, k): pause, magnitude, azimuth, height, body -- counter-based hashes, nothing is kept between launches;
 *   reset   = k == 0 (the schedule's first step) or progress_buf[i] == 0 (the env was reset since the last step): the running push ends and
 *             countdown = pause = pause_lo + min(floor(u[0] (pause_hi - pause_lo + 1)), pause_hi - pause_lo);
 *   a push starts when remaining == 0 && countdown <= 0: remaining = duration, started[i] += 1, and row bodies[min(floor(u[4] num_listed),
 *             num_listed - 1)] of force[i] becomes (force_lo + u[1] (force_hi - force_lo)) d with d = (cos az, sin az, 0), az = 2 pi u[2]
 *             (direction 0) or d uniform on the sphere, z = 2 u[3] - 1 (direction 1);
 *   while remaining > 0 the row keeps that value; in the first launch after the push's last step (or at a reset) the row is cleared.  A launch
 *             writes at most two rows of force[i] (the cleared one and the new one) and no other element: the buffer starts as zeros;
 *   then remaining = max(remaining - 1, 0), countdown = pause where the push's last step was this one, countdown - 1 while no push runs,
 *             k[i] += 1.  body[i] is the row that holds a force, -1 for none.
 * After the launch `force` holds what acts during this env step (phc_sim_step_wrench reads it).  The integer state is bit-equal to the host build
 * of phc_push.h; the force differs by the sinf / cosf / sqrtf implementations only.
 * PHC_EINVAL before any device work for: a null args / bodies / state / force pointer, num_envs < 0, num_bodies outside [1, PHC_MAX_BODIES],
 * num_listed outside [1, PHC_MAX_BODIES], pause_lo < 0, pause_hi < pause_lo or > 2^24, duration < 1, a direction other than 0 / 1, a force range that is
 * not 0 <= force_lo <= force_hi < inf, env_offset < 0 or env_offset + num_envs > 2^32.  The entries of `bodies` are device memory: the caller
 * guarantees 0 <= bodies[j] < num_bodies (phc_amd/perturb.py checks them before the upload).  num_envs == 0 returns 0 without a launch. */
typedef struct {
    int32_t num_envs, num_bodies;             /* N, NB */
    int32_t num_listed;                       /* entries of `bodies` */
    int32_t pause_lo, pause_hi;               /* env steps between the end of a push and the next one */
    int32_t duration;                         /* env steps a push lasts */
    int32_t direction;                        /* 0 = horizontal, 1 = any */
    float force_lo, force_hi;                 /* newtons */
    uint64_t key;                             /* stream key (the caller folds its seed into it) */
    int64_t env_offset;                       /* global index of env 0: the ranks of one run draw disjoint streams from one key */
    const int32_t* bodies;                    /* device [num_listed] */
    const int64_t* progress_buf;              /* [N]; nullable = no env was reset */
    int32_t* remaining;                       /* [N] env steps the running push still lasts */
    int32_t* countdown;                       /* [N] force-free env steps before the next push */
    int32_t* body;                            /* [N] the row of force[i] that is non-zero, or -1 */
    int32_t* k;                               /* [N] launches this env has seen (the draw counter) */
    int32_t* started;                         /* [N] pushes started; their sum is the schedule's push count */
    float* force;                             /* [N, NB, 3] */
} phc_push_args_t;
int32_t phc_push_advance(const phc_push_args_t* args /* host */, void* stream);

/* Thrown projectiles (csrc/phc_proj.hip, per-lane code and the rules line by line csrc/phc_proj.h; an addition to ABI 37, which stays 37): config group
 * `projectile` (phc_amd/projectile.py).  One launch is one env step of `count` spheres per env, in front of the stepper: flight, ground bounce, collision test
 * against every collision capsule of the model, and the impulse of a hit as a force and a torque on the struck body, which phc_sim_step_wrench holds over the
 * env step.  A projectile is a point mass of radius `radius` without spin; its contact with the bodies is frictionless; projectiles do not touch each other.
 * State per slot p < count and env i, arrays [P, N] (pos, vel: [P, N, 3]): life (env steps left, 0 = parked at z = -1000), countdown, thrown, hits, last_hit
 * (the shape struck in this env step, -1 none), pos, vel, mass; k[i] is the env's launch count.  One lane group of 32 (num_shapes <= 32) or 64 lanes per env,
 * lane s owns shape s and row s of force[i] / torque[i]; the winner of a sub-interval is a group-wide arg-min over (gap, shape index).  Per slot:
 *   u[0..7] = proj_draws(key, env_offset + i, k, p): pause, body, mass, speed, distance, azimuth, elevation, spare -- counter-based hashes;
 *   reset   = k == 0 or progress_buf[i] == 0: life = 0, countdown = pause = pause_lo + min(floor(u[0] (pause_hi - pause_lo + 1)), pause_hi - pause_lo), parked;
 *   parked with countdown > 0: countdown -= 1.  Parked with countdown <= 0: a throw at body bodies[min(floor(u[1] num_listed), num_listed - 1)]:
 *             m, speed s, distance d, elevation el uniform in their ranges, azimuth az = 2 pi u[5]; x_t, v_t the body's centre of mass and its velocity
 *             (origin velocity + w x R com); t_f = d / s; x0 = x_t + d (cos el cos az, cos el sin az, sin el) with x0.z >= radius + 0.01;
 *             v0 = (x_t + v_t t_f - x0) / t_f - 0.5 g t_f; life = life_steps, thrown += 1; flight starts in this launch;
 *   flight (life > 0): `substeps` sub-intervals h = dt / substeps, each: v += g h; x += v h; then the ground: where x.z < radius and v.z < 0 the tangential
 *             velocity shrinks by min(friction (1 + e) |v.z|, |v_t|), v.z = -e v.z, x.z = radius; then the bodies, unless the slot has struck in this launch:
 *             every capsule (radius r_c > 0) is posed at the start of the step from its owner's row of rigid_body_state, its endpoints moved at first order
 *             to the end of the sub-interval (t = (i + 1) h, endpoint velocity v_b + w x (a - x_b)); c = closest point of the segment, n = (x - c) / |x - c|
 *             (z^ where they coincide), gap = |x - c| - radius - r_c, vn = (v - v_c) . n with v_c the endpoint velocities interpolated at c; candidates have
 *             gap < 0 and vn < 0; the least gap wins, a tie goes to the lowest shape index; with r from the owner's centre of mass (moved to t at first order) to
 *             the contact point c + r_c n and I_w^-1 = R I_b^-1 R^T:  j = -(1 + e) vn / (1/m + 1/m_b + n . ((I_w^-1 (r x n)) x r)),  v += j n / m,
 *             force[i, owner] += -j n / dt, torque[i, owner] += r x (-j n / dt), hits += 1, last_hit = shape;
 *   end of the launch: life -= 1, at 0 the slot parks and countdown = pause.  k[i] += 1.
 * force / torque [N, NB, 3] hold exactly what acts in this env step: every row of every env is written once per launch, zero where nothing struck; two slots
 * that strike one body add, in slot order.  No atomics, no two lanes store to one address: the launch is deterministic.  Integer state and floats equal the host
 * build of phc_proj.h up to the sinf / cosf of the throw.
 * PHC_EINVAL before any device work for: a null args or a null pointer in it other than progress_buf; num_envs < 0; num_bodies outside [1, PHC_MAX_BODIES];
 * num_shapes outside [num_bodies, PHC_PROJ_MAX_SHAPES]; num_listed outside [1, PHC_MAX_BODIES]; count outside [1, PHC_PROJ_MAX_SLOTS]; pause_lo < 0, pause_hi <
 * pause_lo or > 2^24; life_steps outside [1, 2^24]; substeps outside [1, 64]; dt or radius not positive and finite; gravity_z positive or not finite; restitution
 * outside [0, 1]; friction negative or not finite; a mass, speed or distance range that is not 0 < lo <= hi < inf; an elevation range outside
 * -pi/2 <= lo <= hi <= pi/2; env_offset < 0 or env_offset + num_envs > 2^32.  `bodies` and `owner` are device memory: the caller guarantees entries in
 * [0, num_bodies) (phc_amd/projectile.py checks them before the upload).  num_envs == 0 returns 0 without a launch. */
#define PHC_PROJ_MAX_SLOTS 4
#define PHC_PROJ_MAX_SHAPES 64
typedef struct {
    int32_t num_envs, num_bodies, num_shapes; /* N, NB, collision shapes (primary capsules first, then the extra ones) */
    int32_t num_listed;                       /* entries of `bodies` */
    int32_t count;                            /* P: projectile slots per env */
    int32_t pause_lo, pause_hi;               /* env steps between parking and the next throw */
    int32_t life_steps;                       /* env steps a thrown projectile lives */
    int32_t substeps;                         /* sub-intervals of the env step */
    float dt, gravity_z;                      /* env step (s); gravity along z (<= 0) */
    float radius, restitution, friction;      /* sphere radius (m); restitution e of ground and bodies; the plane's friction */
    float mass_lo, mass_hi, speed_lo, speed_hi, dist_lo, dist_hi, elev_lo, elev_hi;   /* kg, m/s, m, radians */
    uint64_t key;                             /* stream key */
    int64_t env_offset;                       /* global index of env 0 */
    const int32_t* bodies;                    /* device [num_listed] target bodies */
    const float* capsules;                    /* [num_shapes, 7] a3, b3 in the owner's frame, radius (<= 0: no shape) */
    const int32_t* owner;                     /* [num_shapes] */
    const float* body_com;                    /* [NB, 3] centre of mass, body frame */
    const float* body_inv_mass;               /* [NB] */
    const float* body_inv_inertia;            /* [NB, 9] inverse inertia about the centre of mass, body frame, row-major */
    const float* rigid_body_state;            /* [N, NB, 13] */
    const int64_t* progress_buf;              /* [N]; nullable = no env was reset */
    int32_t* life;                            /* [P, N] */
    int32_t* countdown;                       /* [P, N] */
    int32_t* thrown;                          /* [P, N] */
    int32_t* hits;                            /* [P, N] */
    int32_t* last_hit;                        /* [P, N] */
    int32_t* k;                               /* [N] */
    float* pos;                               /* [P, N, 3] */
    float* vel;                               /* [P, N, 3] */
    float* mass;                              /* [P, N] */
    float* force;                             /* [N, NB, 3] */
    float* torque;                            /* [N, NB, 3] */
} phc_proj_args_t;
int32_t phc_proj_advance(const phc_proj_args_t* args /* host */, void* stream);

/* The two row copies that keep a task with projectiles bit-equal to the same task without them wherever nothing struck (csrc/phc_proj.hip).  The task steps
 * its simulator tensors through the launch it would take without the group (phc_sim_step), steps a shadow copy of them through phc_sim_step_wrench with the
 * wrench of phc_proj_advance, and takes the shadow's rows for the struck envs only.  One launch each, one 256-thread block per env, over num_sets tensor
 * pairs of `width[s]` floats per env:
 *   PHC_PROJ_SNAPSHOT  shadow[s][env] = base[s][env] for every env (before the two stepper launches);
 *   PHC_PROJ_SELECT    base[s][env] = shadow[s][env] for every env with last_hit[p, env] >= 0 in any slot p < count; no other element is written.
 * PHC_EINVAL before any device work: a null args, num_envs < 0, num_sets outside [1, PHC_PROJ_MAX_ROWSETS], a mode other than the two, a null base / shadow
 * pointer or a width < 1 in a used set, and with PHC_PROJ_SELECT a null last_hit or count outside [1, PHC_PROJ_MAX_SLOTS].  num_envs == 0: no launch. */
#define PHC_PROJ_MAX_ROWSETS 8
#define PHC_PROJ_SNAPSHOT 0
#define PHC_PROJ_SELECT 1
typedef struct {
    int32_t num_envs, count, num_sets, mode;
    const int32_t* last_hit;                  /* [P, N] of phc_proj_args_t; read by PHC_PROJ_SELECT only */
    float* base[PHC_PROJ_MAX_ROWSETS];        /* [N, width[s]] */
    float* shadow[PHC_PROJ_MAX_ROWSETS];      /* [N, width[s]] */
    int32_t width[PHC_PROJ_MAX_ROWSETS];
} phc_proj_rows_t;
int32_t phc_proj_rows(const phc_proj_rows_t* args /* host */, void* stream);

/* The getup task's episode draws on the device (csrc/phc_getup.hip, per-env code and the rules in full csrc/phc_getup.h; additions to ABI 37, which stays 37):
 * `+env.task_rng=device`.  phc_getup_assign is the device form of HumanoidImGetup._reset_envs(reset_buf.nonzero()) up to the reset launches -- same rules as
 * humanoid_im_getup.py:131-196, its own numbers.  For every env i with reset_buf[i] != 0:
 *   release   avail[assign[i]] = 0 (an env that never held a fall state has assign[i] == 0 and releases slot 0, as the reference does; an assign[i] outside
 *             [0, N) releases nothing);
 *   draw      u[0..1] = getup_draws(key, env_offset + i, k[i]); k[i] += 1;
 *   decide    kind[i] = 2 (RECOVERY) when u[0] < prob[0] and terminate_buf[i] == 1, else 3 (FALL) when u[1] < prob[1], else 1 (NORMAL); 0 for an env not done;
 *   slots     FALL env of rank r (env order) takes pick = free[pi(r)], free[0 .. F) = the slots with avail == 0 after all releases, in slot order, pi a keyed
 *             bijection of [0, F) (cycle-walking four-round Feistel network) that depends on (key, *launch_count, F) alone; *launch_count += 1 per launch.
 *             FALL envs of rank >= F (impossible while every held slot has one holder) become NORMAL;
 *   teleport  root_states[i] = fall_root[pick], dof_state[i, :, 0] = fall_dof_pos[pick], dof_state[i, :, 1] = 0; avail[pick] = 1, assign[i] = pick;
 *   counters  recovery_counter[i] = recovery_steps for FALL and RECOVERY envs;
 *   publish   normal_flag[i] = kind[i] == 1; fall_list[0 .. n_f) = the FALL envs in env order, every other entry N.
 * One workgroup of 1024 threads, block scans over tiles of 1024 envs, no atomics: the result is a function of (key, counters, inputs) alone and bit-equal to the
 * host build of phc_getup.h.  All lanes read *launch_count before the first barrier of the launch, lane 0 writes it after the last.
 * PHC_EINVAL before any device work for: a null args or any null pointer in it (prob included), num_envs < 0, num_dof < 1, recovery_steps < 0, env_offset < 0 or
 * env_offset + num_envs > 2^32.  PHC_EUNSUPPORTED: num_envs > 2^20.  num_envs == 0 returns 0 without a launch.  No lane reads or writes outside the stated sizes
 * whatever the device arrays hold. */
typedef struct {
    int32_t num_envs, num_dof;                /* N (envs == fall-state slots), D */
    int32_t recovery_steps;
    int32_t reserved;
    uint64_t key;                             /* stream key (the caller folds its seed into it) */
    int64_t env_offset;                       /* global index of env 0 */
    const float* prob;                        /* device [2]: p_recovery, p_fall */
    const int64_t* reset_buf;                 /* [N] */
    const int64_t* terminate_buf;             /* [N] */
    const float* fall_root;                   /* [N, 13] */
    const float* fall_dof_pos;                /* [N, D] */
    float* root_states;                       /* [N, 13] */
    float* dof_state;                         /* [N, D, 2] */
    int64_t* avail;                           /* [N] 1 = the slot is held */
    int64_t* assign;                          /* [N] the slot env i took last */
    int32_t* recovery_counter;                /* [N] phc_im_buffers_t.recovery_counter */
    int32_t* k;                               /* [N] draws this env has made */
    int64_t* launch_count;                    /* [1] launches so far (the permutation's counter) */
    int32_t* kind;                            /* [N] out */
    int64_t* normal_flag;                     /* [N] out */
    int64_t* fall_list;                       /* [N] out */
    int32_t* free_list;                       /* [N] scratch */
} phc_getup_args_t;
int32_t phc_getup_assign(const phc_getup_args_t* args /* host */, void* stream);

/* The resets behind phc_getup_assign, masked instead of listed.
 * phc_refresh_body_state_masked: phc_refresh_body_state_indexed over `fall_list` [num_envs] in DEVICE memory whose entries are env ids or num_envs (= skip this
 *   slot): the list phc_getup_assign publishes, so the stepper's kernel is launched as it is, over num_envs slots.  The caller guarantees 0 <= entry <= num_envs.
 * phc_im_reset_from_state_masked: phc_im_reset_from_state for the envs with kind[i] == 3 (fill_history = 1) and kind[i] == 2 (fill_history = 0), the same
 *   per-lane code; every other env is untouched.  PHC_EINVAL for a null `kind`, otherwise the checks of phc_im_reset_from_state. */
int32_t phc_refresh_body_state_masked(const phc_model_t* model, const phc_sim_state_t* sim, const int64_t* fall_list, void* stream);
int32_t phc_im_reset_from_state_masked(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                                       const phc_im_buffers_t* buf, const int32_t* kind, void* stream);

/* The per-step uniforms of cycle_motion / far starts (csrc/phc_getup.hip): one lane per env, u[0..2] = task_draws(key, env_offset + i, k[i]) -> cycle_phase[i],
 * offset_rand[i, 0..1] (each nullable), k[i] += 1 for EVERY env.  PHC_EINVAL: num_envs < 0, a null k, env_offset < 0 or env_offset + num_envs > 2^32. */
int32_t phc_task_draws(int32_t num_envs, uint64_t key, int64_t env_offset, int32_t* k, float* cycle_phase /*[N]*/, float* offset_rand /*[N, 2]*/, void* stream);

/* Observation noise and reference-sample dropout as one launch (csrc/phc_obs_aug.hip, per-lane code and the rules in full csrc/phc_obs_aug.h; additions to ABI 37,
 * which stays 37): `+env.task_rng=device` with env.add_obs_noise / env.fut_tracks_dropout.  Same rules as HumanoidIm._fut_dropout + _add_obs_noise
 * (humanoid_im.py:824-830, then :710-711), its own numbers.  For every SELECTED row i of obs [N, num_obs], with so = self_obs_size, T = num_samples,
 * W = (num_obs - so) / T, P = (num_obs + 1) / 2:
 *   dropout   T > 1 and dropout_p > 0: for each t < T with u(P + t, 0) < dropout_p, 0.0f into columns so + t W .. so + (t + 1) W - 1;
 *   noise     noise_std > 0: every column c becomes obs[c] + noise_std * z[c] (the zeroed ones included), (z[2 j], z[2 j + 1]) the Box-Muller pair of the
 *             uniforms a = u(j, 0), b = u(j, 1): r = sqrtf(-2 logf(1 - a)), theta = 2 pi b, r cosf(theta), r sinf(theta);
 *   counter   k[i] += 1.
 *   u(index, which) = hash_u01(splitmix64(key ^ (((k[i] << 16 | index) << 1 | which) * 0x9E6C63D0876A9A47)), env_offset + i).
 * An unselected row is untouched and its counter stays.  Selection, exactly one form: all rows (row_flag and env_ids NULL); row_flag [N] int64, non-zero =
 * selected; env_ids [n_ids] int64 in DEVICE memory, distinct ids in [0, N) (an id outside selects nothing; the same id twice is the caller's error).
 * One workgroup per row, lanes along the columns; counters, dropout decisions and every stored 0.0f are bit-equal to the host build of phc_obs_aug.h, a noised
 * element differs by the device's logf / sinf / cosf / sqrtf alone.
 * PHC_EINVAL before any device work for: a null args / obs / k, num_envs / num_obs / num_samples / n_ids < 0, self_obs_size outside [0, num_obs], num_samples >= 1
 * that does not divide num_obs - self_obs_size, both row_flag and env_ids, n_ids != 0 without env_ids, n_ids > num_envs, env_offset < 0 or env_offset + num_envs > 2^32, dropout_p
 * outside [0, 1], noise_std < 0 (a NaN fails either).  PHC_EUNSUPPORTED: num_obs > 65536, num_samples > 1024.  num_envs == 0, or env_ids with n_ids == 0: 0 without a launch. */
typedef struct {
    int32_t num_envs, num_obs;                /* N, columns of a row */
    int32_t self_obs_size, num_samples;       /* so, T */
    float dropout_p, noise_std;
    uint64_t key;                             /* stream key (the caller folds its seed into it) */
    int64_t env_offset;                       /* global index of env 0 */
    float* obs;                               /* [N, num_obs] contiguous */
    int32_t* k;                               /* [N] calls that selected this env (the draw counter) */
    const int64_t* row_flag;                  /* [N], nullable */
    const int64_t* env_ids;                   /* [n_ids], nullable */
    int64_t n_ids;
} phc_obs_aug_args_t;
int32_t phc_obs_augment(const phc_obs_aug_args_t* args /* host */, void* stream);

/* The occlusion schedule of env.occl_training as one launch (csrc/phc_obs_aug.hip; rules: csrc/phc_obs_aug.h), the device form of
 * HumanoidIm._update_occl_training (humanoid_im.py:1081-1092).  One lane per env i, for j = 0 .. J - 1, u = u(j, 0), v = u(j, 1) as above:
 *   start = j != 0 && u < prob;  span = min(span_lo + floor(v * (span_hi - span_lo)), span_hi - 1);
 *   count[i, j] = max((start ? span : count[i, j]) - 1, 0);  mask[i, j] = !(9 <= j && j < 24) (the reference overwrites the mask it derives from the counts:
 *   the schedule never reaches the mask);  k[i] += 1 for EVERY env.  Bit-equal to the host build.
 * PHC_EINVAL: a null k / count / mask, num_envs < 0, J < 0, env_offset < 0 or env_offset + num_envs > 2^32, prob outside [0, 1], span_hi <= span_lo.
 * PHC_EUNSUPPORTED: J > 64.  num_envs == 0 returns 0 without a launch. */
int32_t phc_occl_advance(int32_t num_envs, int32_t J, uint64_t key, int64_t env_offset, int32_t* k, float prob, int32_t span_lo, int32_t span_hi,
                         int64_t* count /*[N, J]*/, uint8_t* mask /*[N, J]*/, void* stream);

/* Domain randomisation in the stepper (csrc/phc_sim_dr.hip, the DR instantiations of the stepper's kernel; per-lane code csrc/phc_dr.h; additions to ABI 37, which
 * stays 37): phc_sim_step with PER-ENV physics.  With `dr` NULL, or both of its tensors NULL, and a model phc_sim_step accepts, the call IS phc_sim_step: same
 * checks, same launch, same bits.
 *   model blocks   model->num_shapes > 1 with sim->env_shape is accepted for BOTH joint families here (phc_sim_step keeps refusing revolute models): env i steps
 *                  with block env_shape[i] of the int / float tables -- its own masses, centres of mass, inertias, gains.  The blocks share topology and geometry;
 *                  the caller guarantees that (the check cannot read device memory);
 *   env_friction   env i's Coulomb coefficient max(env_friction[i], 0) replaces params->friction in every place the stepper reads it (penalty points, rigid
 *                  contact, force sensors);
 *   torque_noise   revolute models under control_mode 1 / 2: at the first sub-step of simulate call c of the launch, DoF d of env i steps with the PD target
 *                  target + u amp[i, d] / kp, u = dr_noise_u(key, k[i], c, (env_offset + i) D + d) in [-1, 1) -- a torque u amp added in front of the effort
 *                  clip (and of mode 2's saturation test).  kp is the env's block's; a DoF with kp == 0 gets none.  The published pd_target stays the un-noised one.
 * PHC_EUNSUPPORTED: lane_mapping 3; torque_noise on a spherical model or with control_mode 0.  PHC_EINVAL: torque_noise without k, env_offset < 0 or
 * (env_offset + N) D > 2^32, num_shapes > 1 without env_shape; then everything phc_sim_step refuses.  No external wrench in this launch. */
typedef struct {
    const float*   env_friction;   /* [N]; nullable */
    const float*   torque_noise;   /* [N, D] amplitude in N m; nullable */
    const int32_t* k;              /* [N] env-step counter of each env (written by phc_dr_advance); required with torque_noise */
    uint64_t       key;            /* stream key */
    int64_t        env_offset;     /* global index of env 0 (ranks of one run draw disjoint streams) */
} phc_sim_dr_t;
int32_t phc_sim_step_dr(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                        const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask, int32_t num_sim_calls,
                        const phc_sim_dr_t* dr /* host; nullable */, void* stream);

/* The per-env-step part of domain randomisation (csrc/phc_dr.hip, per-lane code csrc/phc_dr.h; an addition to ABI 37): control delay and velocity pushes, one
 * launch per env step AHEAD of the stepper, one lane per env.  All state and draws live on the device: a captured launch moves on with every replay.  Per env i,
 * with k = k[i] and Q = delay_hi + 1:
 *   reset  = k == 0 or progress_buf[i] == 0: the env's Q rows of the queue are zeroed and delay[i] = delay_lo + min(floor(u (delay_hi - delay_lo + 1)),
 *            delay_hi - delay_lo) is drawn anew;
 *   actions[i] goes to row k mod Q, row (k - delay[i]) mod Q goes to delayed_actions[i] (delay_hi == 0: delayed_actions[i] = actions[i], no queue);
 *   push_interval > 0, k > 0, k % push_interval == 0 and the env was not just reset: root_states[i, 7:9] = two draws of U(-max_push_vel_xy, max_push_vel_xy);
 *   k[i] += 1.
 * Integer state and draws are bit-equal to the host build of phc_dr.h.  PHC_EINVAL before any device work: a null args / actions / delayed_actions / delay / k,
 * a null action_queue with delay_hi > 0, a null root_states with push_interval > 0, num_envs < 0, num_dof < 1, delay_lo < 0, delay_hi < delay_lo or > 1023,
 * push_interval < 0, max_push_vel_xy negative or not finite, env_offset < 0 or env_offset + num_envs > 2^32.  num_envs == 0 returns 0 without a launch. */
typedef struct {
    int32_t num_envs, num_dof;
    int32_t delay_lo, delay_hi;          /* env steps, inclusive */
    int32_t push_interval;               /* env steps; 0 = no velocity push */
    float   max_push_vel_xy;
    uint64_t key;
    int64_t env_offset;
    const int64_t* progress_buf;         /* [N]; nullable = no env was reset */
    const float* actions;                /* [N, D] */
    float*   action_queue;               /* [Q, N, D] ring */
    int32_t* delay;                      /* [N] */
    int32_t* k;                          /* [N] launches the env has seen */
    float*   delayed_actions;            /* [N, D] out: what the stepper is given */
    float*   root_states;                /* [N, 13]; nullable unless push_interval > 0 */
} phc_dr_args_t;
int32_t phc_dr_advance(const phc_dr_args_t* args /* host */, void* stream);

/* Clip processing on the device (csrc/phc_clip.hip, per-lane code csrc/phc_clip.h; an addition to ABI 37, which stays 37): `process_clip` of
 * phc_amd/motion_lib.py for U concatenated clips of the SMPL family -- forward kinematics with the normalised local rotations, np.gradient and
 * finite-difference angular velocities, the gaussian filter (sigma 2, radius 8, `nearest` clamped to each clip's own first and last frame), the joint
 * velocities -- in fp64, rounded once to the fp32 records of phc_motion_lib_t (spherical layout, no extended bodies; pad floats written as 0).
 * Two launches on `stream`, 256-thread blocks:
 *   1. one lane per (frame, body) over tiles of up to 16 frames: the lane walks its own ancestor chain from the root; positions, both rotations and
 *      the joint velocities go through an LDS image of the tile's records to coalesced stores; the fp64 positions and raw angular velocities go to
 *      `scratch`, and one lane per frame records the frame's clip there;
 *   2. one lane per velocity float of a record: the 17-tap filter over the scratch rows of the lane's clip.
 * No lane loops over a clip's frames.  phc_clip_scratch_bytes(F, J) = 48 F J + 4 F rounded up to 8 (negative arguments: PHC_EINVAL).
 * Before any device work, PHC_EINVAL for: a null args or pointer field, num_clips / num_bodies / num_trees < 1, num_frames < 2 num_clips,
 * frame_stride != 20 num_bodies, scratch_bytes below phc_clip_scratch_bytes, an f64 / i64 array or the scratch not 8-byte aligned, an i32 / f32 array not
 * 4-byte aligned; PHC_EUNSUPPORTED for num_bodies > PHC_MAX_BODIES and for a num_frames that does not fit the launch grids (6 num_bodies num_frames > (2^31 - 1) 256, or more than
 * 2^31 - 1 tiles).
 * The contents of the device arrays are the caller's duty (phc_amd/motion_lib.py validates them before the upload): clips of at least 2 frames,
 * clip_start ascending from 0 to num_frames, clip_tree in [0, num_trees), parents[j] < j with exactly the entries < 0 as roots.  Whatever they hold, no
 * lane reads or writes outside the arrays' stated sizes. */
typedef struct {
    int32_t num_clips, num_bodies, num_trees; /* U, J, trees */
    int32_t frame_stride;                     /* floats per record: 20 J */
    int64_t num_frames;                       /* F, all clips together */
    const int32_t* parents;                   /* [J] */
    const double*  local_translation;         /* [num_trees, J, 3] */
    const int32_t* clip_tree;                 /* [U] */
    const int64_t* clip_start;                /* [U + 1] frame offsets; the last entry is F */
    const double*  clip_dt;                   /* [U] 1 / fps */
    const double*  quat;                      /* [F, J, 4] global rotations, xyzw */
    const double*  trans;                     /* [F, 3] root translation */
    void*          scratch;                   /* phc_clip_scratch_bytes(F, J) bytes */
    int64_t        scratch_bytes;
    float*         frames;                    /* [F, frame_stride] out */
} phc_clip_args_t;
int64_t phc_clip_scratch_bytes(int64_t num_frames, int32_t num_bodies);
int32_t phc_clip_process(const phc_clip_args_t* args /* host; all pointers device memory */, void* stream);

/* Clip processing on the device for the robots (csrc/phc_clip_real.hip, per-lane code csrc/phc_clip_real.h; an addition to ABI 37, which stays 37): the robot
 * branch of `_run_clip_job` of phc_amd/motion_lib.py for U concatenated clips of one all-revolute model with NB simulated and E extended bodies -- the height
 * fix, `Humanoid_Batch`'s matrix forward kinematics (`robot_fk`: axis-angle -> quaternion -> matrix per body, wmat = wmat_parent (rest_mat pm), the best-
 * conditioned of the four matrix -> quaternion candidates taken as is), np.gradient and finite-difference angular velocities with the gaussian filter of
 * phc_clip_process, dof_pos as the row sum of pose_aa, dvs as its finite difference (the clip's LAST frame takes the difference of frames T-3 and T-2, as the
 * reference does) -- in fp64, rounded once to the fp32 records of phc_motion_lib_t (revolute layout: gts 3(NB+E) | grs 4(NB+E) | gvs 3NB | gavs 3NB |
 * dof_pos NB-1 | dvs NB-1 | pad floats written as 0).  Launches on `stream`, 256-thread blocks:
 *   0. (fix_height != 0 only) one block per clip: the FK of the clip's first frame, z = wpos_z + wmat[2, :] . contact_pos - contact_radius over the C contact
 *      points, clip_dz[c] = their minimum into `scratch`; the root translation of every frame of the clip is lowered by it;
 *   1. one lane per (frame, body in NB+E) over tiles of up to 16 frames: the lane walks its own ancestor chain from the root, for frame f and (simulated
 *      bodies, for the angular velocity) for frame f + 1; positions, rotations, dof_pos and dvs go through an LDS image of the tile's records to coalesced
 *      stores; the fp64 positions and raw angular velocities of the NB simulated bodies go to `scratch`, and one lane per frame records the frame's clip there;
 *   2. one lane per velocity float of a record (6 NB, at column 7 (NB+E)): the 17-tap filter over the scratch rows of the lane's clip.
 * No lane loops over a clip's frames.  phc_clip_real_scratch_bytes(F, NB, E, U) = 48 F NB + 8 U + 4 F rounded up to 8 (F < 0, NB < 1, E < 0, U < 1: PHC_EINVAL).
 * Before any device work, PHC_EINVAL for: a null args or pointer field (the three contact arrays only with fix_height), num_clips / num_bodies < 1,
 * num_ext < 0, num_contacts < 1 with fix_height, num_frames < 3 num_clips, frame_stride != the revolute record's, scratch_bytes below
 * phc_clip_real_scratch_bytes, an f64 / i64 array or the scratch not 8-byte aligned, an i32 / f32 array not 4-byte aligned; PHC_EUNSUPPORTED for
 * num_bodies + num_ext > PHC_MAX_BODIES and for a num_frames that does not fit the launch grids (6 num_bodies num_frames > (2^31 - 1) 256, or more than 2^31 - 1 tiles).
 * The contents of the device arrays are the caller's duty (phc_amd/motion_lib.py validates them before the upload): clips of at least 3 frames, clip_start
 * ascending from 0 to num_frames, parents[j] < j with exactly the entries < 0 as roots, contact_body in [0, NB).  Whatever they hold, no lane reads or
 * writes outside the arrays' stated sizes. */
typedef struct {
    int32_t num_clips, num_bodies, num_ext, num_contacts; /* U, NB, E, C */
    int32_t frame_stride;                     /* floats per record: 7 (NB+E) + 6 NB + 2 (NB-1) rounded up to a multiple of 4 */
    int32_t fix_height;                       /* 0: no height fix (launch 0 is skipped, the contact arrays are not read) */
    int64_t num_frames;                       /* F, all clips together */
    const int32_t* parents;                   /* [NB+E] the extended bodies appended */
    const double*  offsets;                   /* [NB+E, 3] translation to the parent */
    const double*  rest_mat;                  /* [NB+E, 3, 3] rest rotations, row-major matrices */
    const double*  pose_aa;                   /* [F, NB+E, 3] axis-angle per body */
    const double*  trans;                     /* [F, 3] root translation */
    const int64_t* clip_start;                /* [U + 1] frame offsets; the last entry is F */
    const double*  clip_dt;                   /* [U] 1 / fps */
    const int32_t* contact_body;              /* [C] */
    const double*  contact_pos;               /* [C, 3] in the body's frame */
    const double*  contact_radius;            /* [C] */
    void*          scratch;                   /* phc_clip_real_scratch_bytes(F, NB, E, U) bytes */
    int64_t        scratch_bytes;
    float*         frames;                    /* [F, frame_stride] out */
} phc_clip_real_args_t;
int64_t phc_clip_real_scratch_bytes(int64_t num_frames, int32_t num_bodies, int32_t num_ext, int32_t num_clips);
int32_t phc_clip_process_real(const phc_clip_real_args_t* args /* host; all pointers device memory */, void* stream);

/* HumanoidTeleop's regularisation rewards and its recovery window after a velocity push (csrc/phc_teleop.hip, per-env code csrc/phc_teleop.h; an addition to
 * ABI 37, which stays 37; reference: phc/env/tasks/humanoid_teleop.py:95-101,167-307).  One launch per env step AFTER phc_im_post_physics on the same stream;
 * a group of 32 lanes per env, lanes along a DoF row, 256-thread blocks; every sum is a fixed-order butterfly over the group (no atomics): the same inputs
 * give the same bits at any num_envs.  Per env i, with R = popcount(term_mask) and C = num_im_cols:
 *   (a) the terms of term_mask (bit PHC_TELEOP_*), tau = dof_force, (q, qd) = dof_state, a = actions, F = contact_force and v, rot = rigid_body_state of the
 *       bodies feet[0 .. num_feet):
 *         DOF_POS_LIMITS  sum_d max(lo_d - q_d, 0) + max(q_d - hi_d, 0)          TORQUE_LIMITS  sum_d max(|tau_d| - torque_limits_d, 0)
 *         TORQUES         sum_d tau_d^2                                          DOF_VEL        sum_d qd_d^2
 *         DOF_ACC         sum_d ((last_dof_vel_d - qd_d) / dt)^2                 ACTION_RATE    sum_d (last_actions_d - a_d)^2
 *         SLIPPAGE        sum_f |v_f| [|F_f| > 1]                                FEET_CONTACT_FORCES  sum_f max(|F_f| - max_contact_force, 0)
 *         STUMBLE         1 if any_f |F_f,xy| > 5 |F_f,z| else 0
 *         FEET_AIR_TIME   contact_f = F_f,z > 1; filt_f = contact_f or last_contacts_f; last_contacts_f = contact_f; first_f = feet_air_time_f > 0 and filt_f;
 *                         feet_air_time_f += dt; value = sum_f (feet_air_time_f - 0.25) first_f; feet_air_time_f = 0 where filt_f; value *= [|ref root v_xy| > 0.1],
 *                         the reference root velocity looked up in `lib` at the imitation reward's own time: progress_buf[i] (+ 1 where recovery_counter[i] > 0:
 *                         phc_im_post_physics held the progress of a gated env) x dt + motion_start_times[i] + motion_start_times_offset[i];
 *         FEET_ORI        |g_xy| of foot 0 + |g_xy| of foot 1, g = (0, 0, -1) rotated into the foot's frame;
 *   (b) column r of the new ones is the term order[r] times scale[order[r]] (the caller's reward_specs value x dt); rew_buf[i] += the columns in their order;
 *       reward_raw[i] = reward_im[i, 0 .. C) followed by the R columns (phc_im_post_physics writes its own C columns with a row stride of C: reward_im is
 *       that tensor, reward_raw the public [N, C + R] one);
 *   (c) last_actions[i] = actions[i], last_dof_vel[i] = qd (each where the pointer is given); feet_air_time / last_contacts as under FEET_AIR_TIME.  None of
 *       them is cleared by an env reset (the reference does not clear them either);
 *   (d) push_interval > 0: with k = dr_k[i] (phc_dr_advance has already counted this step), where k > 0 and k % push_interval == 0 -- phc_dr_advance pushes the
 *       env at the START of the next step -- recovery_counter[i] = recovery_steps + 1: phc_im_post_physics decrements first and gates while the result is
 *       positive, so the env is neither reset nor advanced for recovery_steps steps from the pushed one on.  An env reset in between is not pushed and its
 *       counter is zeroed by the reset launch.
 * A term that is off reads none of its inputs: every input below is nullable unless a term of the mask (or a state array that is given) needs it.
 * PHC_EINVAL before any device work: a null args / rew_buf / reward_raw; reward_im null with num_im_cols > 0; a null input that a term of the mask or a given
 * state array needs (dof_state: DOF_POS_LIMITS, DOF_VEL, DOF_ACC, last_dof_vel; dof_limits_lower / upper: DOF_POS_LIMITS; dof_force: TORQUE_LIMITS, TORQUES;
 * torque_limits: TORQUE_LIMITS; last_dof_vel: DOF_ACC; actions: ACTION_RATE, last_actions; last_actions: ACTION_RATE; contact_force: SLIPPAGE,
 * FEET_CONTACT_FORCES, STUMBLE, FEET_AIR_TIME; rigid_body_state: SLIPPAGE, FEET_ORI; feet_air_time, last_contacts, progress_buf, motion_start_times,
 * motion_start_times_offset: FEET_AIR_TIME; dr_k, recovery_counter: push_interval > 0); num_envs < 0, num_dof < 1, num_feet outside [0, PHC_TELEOP_MAX_FEET],
 * num_bodies outside [1, PHC_MAX_BODIES] or a foot outside [0, num_bodies) when num_feet > 0, num_im_cols outside [0, 8], FEET_ORI with fewer than two feet,
 * FEET_AIR_TIME without a motion library (lib null, or without frames or clip tables), a term_mask with bits at or above
 * PHC_TELEOP_NUM_TERMS, an `order` that is not the mask's terms each once, dt not positive and finite, push_interval < 0 or recovery_steps < 0.
 * PHC_EUNSUPPORTED: (none).  num_envs == 0 returns 0 without a launch. */
#define PHC_TELEOP_DOF_POS_LIMITS 0
#define PHC_TELEOP_TORQUE_LIMITS 1
#define PHC_TELEOP_TORQUES 2
#define PHC_TELEOP_DOF_VEL 3
#define PHC_TELEOP_DOF_ACC 4
#define PHC_TELEOP_ACTION_RATE 5
#define PHC_TELEOP_SLIPPAGE 6
#define PHC_TELEOP_FEET_CONTACT_FORCES 7
#define PHC_TELEOP_STUMBLE 8
#define PHC_TELEOP_FEET_AIR_TIME 9
#define PHC_TELEOP_FEET_ORI 10
#define PHC_TELEOP_NUM_TERMS 11
#define PHC_TELEOP_MAX_FEET 8
typedef struct {
    int32_t num_envs, num_dof, num_bodies, num_feet;
    int32_t num_im_cols;                          /* C: the columns phc_im_post_physics wrote (4, or 5 with the power reward) */
    uint32_t term_mask;                           /* bit t = term t is on */
    int32_t order[PHC_TELEOP_NUM_TERMS];          /* order[r] = the term of new column r, r < popcount(term_mask) */
    float   scale[PHC_TELEOP_NUM_TERMS];          /* by term: reward_specs value x dt */
    int32_t feet[PHC_TELEOP_MAX_FEET];            /* body indices, the config's order */
    float   dt, max_contact_force;
    int32_t push_interval, recovery_steps;        /* env steps; push_interval 0 = no recovery window */
    const float* dof_state;                       /* [N, D, 2] position, velocity */
    const float* dof_limits_lower;                /* [D] */
    const float* dof_limits_upper;                /* [D] */
    const float* torque_limits;                   /* [D] */
    const float* dof_force;                       /* [N, D] */
    const float* actions;                         /* [N, D] the policy's action, not the delayed one */
    const float* contact_force;                   /* [N, NB, 3] */
    const float* rigid_body_state;                /* [N, NB, 13] */
    const int64_t* progress_buf;                  /* [N] as phc_im_post_physics left it */
    const float* motion_start_times;              /* [N] */
    const float* motion_start_times_offset;       /* [N] */
    const int64_t* sampled_motion_ids;            /* [N]; nullable = env i plays clip i */
    const int32_t* dr_k;                          /* [N] phc_dr_args_t.k after this step's phc_dr_advance */
    int32_t* recovery_counter;                    /* [N] phc_im_buffers_t.recovery_counter */
    float*   last_actions;                        /* [N, D] state */
    float*   last_dof_vel;                        /* [N, D] state */
    float*   feet_air_time;                       /* [N, num_feet] state */
    uint8_t* last_contacts;                       /* [N, num_feet] state, 0 / 1 */
    float*   rew_buf;                             /* [N] in / out */
    const float* reward_im;                       /* [N, C] */
    float*   reward_raw;                          /* [N, C + R] out */
} phc_teleop_args_t;
int32_t phc_teleop_rewards(const phc_motion_lib_t* lib /* host; nullable without FEET_AIR_TIME */, const phc_teleop_args_t* args /* host */, void* stream);

/* Tracking of streamed keypoints: the per-step work of HumanoidImDemo / HumanoidImMCPDemo (csrc/phc_stream.hip, per-lane code csrc/phc_stream.h; an addition
 * to ABI 37, which stays 37; reference: phc/env/tasks/humanoid_im_mcp_demo.py:252-321).  One launch per env step AFTER phc_im_post_physics on the same stream
 * (mode PHC_STREAM_ADVANCE) and one after every reset launch (mode PHC_STREAM_OBSERVE); a group of 32 lanes per env, lanes along the bodies (bodies l, l + 32),
 * 256-thread blocks, no LDS, no atomics; sums over the group are phc_group.h's fixed-order butterfly: the same inputs give the same bits at any num_envs.
 * ADVANCE, per env i with W = window, the env's ring of W past samples, L = min(count[i] + 1, W):
 *   (1) p_j = frames[r, perm[j]] for body j (r = i, or 0 when frame_rows == 1; perm null = identity); q_j = p_j - p_0;
 *   (2) limb_scale: s = mean over the pairs k < num_pairs of |q_parent_k - q_child_k| / pair_length[k] (fp32, fixed order); q_j /= s;
 *   (3) q -> ring_body[i, head[i]], p_0 -> ring_root[i, head[i]]; head[i] = (head[i] + 1) % W; count[i] = L;
 *   (4) with the L samples oldest first x_0 .. x_{L-1}: Q_j = sum_k fold[3][L-1][k] q_j,k and T_c = sum_k fold[c][L-1][k] p_0,k,c for the axes c = 0, 1, 2
 *       (fold[s][L-1][k]: fp64 [4, fold_window, fold_window]; the value AT THE NEWEST SAMPLE of a gaussian filter with mirrored ends over L samples; rows
 *       0..2 the root translation's axes, row 3 the bodies; the caller builds it, phc_amd/stream.py);
 *   (5) ref_j = frame_mat (Q_j + T) (row-major 3 x 3, i.e. (Q + T) @ M^T); vel_j = (ref_j - cur_ref[i, j]) / dt where has_prev[i], else 0; has_prev[i] = 1;
 *       sums and the difference in fp64, rounded once; cur_ref[i, j] = ref_j, cur_vel[i, j] = vel_j.
 * OBSERVE skips (1) - (5): ref = cur_ref, vel = cur_vel; rings, head, count and has_prev are not touched.
 * Both modes then, for the tracked bodies (prm->track_slot): with d = |root body pos - ref of the body in track slot 0 (track_root_body)| and where
 * prm->zero_out_far: d > close_distance: targets of the slots >= 1 := the body's own position, every target velocity := the body's; d > far_distance: the
 * slot-0 target := body + (ref - body) / d x far_distance (humanoid_im_mcp_demo.py:296-306; the distances are this struct's, not prm's); the obs_v 7 task
 * observation of that target into obs_buf[i, num_self_obs ..) (root rotation with prm->remove_base_rot); reset_buf[i] = terminate_buf[i] = 0 (where given);
 * track_err[i] = mean over the tracked bodies of |body pos - ref| (the ungated ref).
 * PHC_EINVAL before any device work: a null model / prm / args / prm->track_slot / cur_ref / cur_vel / rigid_body_state / obs_buf / track_err; num_envs < 0;
 * model->num_bodies outside [1, PHC_MAX_BODIES]; prm->num_track_bodies outside [1, num_bodies]; track_root_body outside [0, num_bodies); a mode other than the two;
 * in ADVANCE: window outside [1, PHC_STREAM_MAX_WINDOW], fold_window < window, a null frames / fold / ring_body / ring_root / head / count / has_prev,
 * frame_rows other than 1 or num_envs, num_pairs outside [0, PHC_STREAM_MAX_PAIRS] (limb_scale: outside [1, ..]), a pair index outside [0, num_bodies), a
 * pair_length or dt that is not positive and finite.  PHC_EUNSUPPORTED: prm->obs_v other than 7, prm->num_traj_samples > 1.  num_envs == 0 returns 0 without
 * a launch. */
#define PHC_STREAM_ADVANCE 0
#define PHC_STREAM_OBSERVE 1
#define PHC_STREAM_MAX_WINDOW 64
#define PHC_STREAM_MAX_PAIRS 8
typedef struct {
    int32_t num_envs, mode;
    int32_t window, fold_window;                  /* W; the side of the fold table (>= W) */
    int32_t frame_rows;                           /* 1: one staged frame for all envs; else num_envs */
    int32_t limb_scale, num_pairs;
    int32_t pair_parent[PHC_STREAM_MAX_PAIRS], pair_child[PHC_STREAM_MAX_PAIRS];   /* body indices (after perm) */
    float   pair_length[PHC_STREAM_MAX_PAIRS];
    float   frame_mat[9];                         /* row-major M: ref = M x */
    float   dt, close_distance, far_distance;
    int32_t track_root_body;                      /* the body in track slot 0 */
    const float*   frames;                        /* [frame_rows, NB, 3] staged keypoints, the source's joint order */
    const int32_t* perm;                          /* [NB] body j reads joint perm[j]; nullable = identity */
    const double*  fold;                          /* [4, fold_window, fold_window] */
    float*   ring_body;                           /* [N, W, NB, 3] state */
    float*   ring_root;                           /* [N, W, 3] state */
    int32_t* head;                                /* [N] state: the slot the next sample takes */
    int32_t* count;                               /* [N] state: samples held, <= W */
    uint8_t* has_prev;                            /* [N] state: cur_ref holds a previous frame */
    float*   cur_ref;                             /* [N, NB, 3] state / out: the task's ref_body_pos */
    float*   cur_vel;                             /* [N, NB, 3] out: the task's ref_body_vel */
    const float* rigid_body_state;                /* [N, NB, 13] */
    float*   obs_buf;                             /* [N, num_self_obs + num_task_obs]: the task block is written */
    int64_t* reset_buf;                           /* [N] out, nullable */
    int64_t* terminate_buf;                       /* [N] out, nullable */
    float*   track_err;                           /* [N] out */
} phc_stream_args_t;
int32_t phc_stream_track(const phc_model_t* model /* host */, const phc_im_params_t* prm /* host */, const phc_stream_args_t* args /* host */, void* stream);

/* ---- Distilling a composed controller into one MLP (csrc/phc_distill.hip; additive, ABI 37 unchanged) ------------------------------------------------------
 * phc_dataset_record: the evaluation sweep's `collect_dataset` (im_amp_players.py:95-99,132-151), ONE launch per env step behind the post-physics launch.
 * Env i with step < rows[i] stores, at row row_start[i] + step of the clip-major batch block, the observation it acted on (obs_prev[i]), clean_actions[i],
 * actions[i] and reset_buf[i]; rows at or past `capacity` are never written.  Then obs_prev[i] = obs_buf[i] for EVERY env.  rows = max(num_steps - 1, 0) and
 * row_start = its exclusive prefix sum give the layout of the reference's np.concatenate of the per-clip slices.
 * PHC_EINVAL before any device work: a null args or pointer field, num_envs / obs_dim / num_actions / capacity < 1, step < 0. */
typedef struct {
    int32_t num_envs, obs_dim, num_actions, step;
    int64_t capacity;                 /* R: rows of the batch block */
    const float*   obs_buf;           /* [N, obs_dim] the task's observation after this step */
    float*         obs_prev;          /* [N, obs_dim] state: the observation before this step */
    const float*   clean_actions;     /* [N, A] */
    const float*   actions;           /* [N, A] what the task received */
    const int64_t* reset_buf;         /* [N] after the step */
    const int64_t* rows;              /* [N] */
    const int64_t* row_start;         /* [N] */
    float*   obs;                     /* [R, obs_dim] out */
    float*   clean;                   /* [R, A] out */
    float*   env;                     /* [R, A] out */
    int64_t* reset;                   /* [R] out */
} phc_record_args_t;
int32_t phc_dataset_record(const phc_record_args_t* args /* host */, void* stream);

/* y = z / (1 + exp(-z)) on bf16 [rows, cols] (contiguous), evaluated in fp32, stored as bf16; finite for every finite z (-0 at the negative end). */
int32_t phc_silu_bf16(const void* z, int64_t rows, int32_t cols, void* y, void* stream);
/* gz = gy s (1 + z (1 - s)), s = sigmoid(z), stored as bf16 (gz must not alias gy / z), and the fp32 column sums of the unrounded products: the contract of
 * phc_colsum_relu_bf16 (workspace phc_colsum_workspace(rows, cols); out == NULL runs the first stage only and leaves phc_colsum_chunks(rows) partials for
 * phc_colsum_finish_batch; bit-reproducible). */
int32_t phc_colsum_silu_bf16(const void* gy, const void* z, int64_t rows, int32_t cols, void* gz, float* out, float* workspace, void* stream);
/* nn.MSELoss(): loss_out[0] = mean over batch x dim of (pred[r, d] - target[q, d])^2 with q = row_index[r] (NULL: q = r), grad = 2 (pred - target) / (batch dim)
 * in pred's type (bf16 when is_bf16, else fp32); target fp32 [*, dim].  Sums in a fixed order (fp64 per-block partials, one finishing block): two runs give
 * the same bits.  workspace: phc_mse_loss_workspace() bytes.  PHC_EINVAL: a null pred / target / grad / loss_out / workspace, batch or dim < 1. */
int64_t phc_mse_loss_workspace(void);
int32_t phc_mse_loss(const void* pred, int32_t is_bf16, const float* target, const int64_t* row_index, int64_t batch, int32_t dim, void* grad, float* loss_out,
                     double* workspace, void* stream);

/* Retargeting fit on the device (csrc/phc_fit.hip, per-lane code csrc/phc_fit.h; an addition to ABI 37, which stays 37): `iterations` trips of the loop of
 * `fit_clip` (phc_amd/utils/fit_robot_motion.py <- reference scripts/data_process/fit_smpl_motion.py:101-150) for C concatenated clips at once, fp32 throughout.
 * Clip c owns frames clip_start[c] .. clip_start[c + 1] - 1 (T_c of them); with NB simulated bodies, E extended ones, ND = NB - 1 revolute joints and M matched
 * bodies one trip is
 *   1. FK as RobotFK: root rotation = Rodrigues(root_rot[t]) (series branch for |r|^2 < 1e-8), joint j = Rodrigues(axis_j dof[t, j]), extended bodies do not
 *      rotate, root position = root_trans_offset[t] + root_off[c];
 *   2. loss_c = mean_{t,m} |p - g| + 0.01 mean_{t,j} dof^2 over the clip's own frames, and its analytic gradient: with u = (p - g) / |p - g| (0 where the
 *      residual is exactly 0), joint j gets sum_{m in subtree(j)} a_j . ((p_m - p_j) x u_m) / (T_c M) + 0.02 dof_j / (T_c ND) (a_j the joint's axis in the
 *      world), the root rotation vector J_l(r)^T sum_m (p_m - p_root) x u_m / (T_c M) (J_l the exponential map's left Jacobian, with its series branch),
 *      root_off[c] sum_t sum_m u / (T_c M);
 *   3. torch.optim.Adam's step (betas 0.9 / 0.999, eps 1e-8, no weight decay; denom = sqrt(v) / sqrt(1 - b2^k) + eps, step = lr / (1 - b1^k), k = step[c] + 1)
 *      on dof, root_rot and root_off; step[c] = k;
 *   4. dof clamped to `range`;
 *   5. the clamped dof smoothed along time by the normalised 5-tap gaussian (sigma 0.75), replicate-padded at the clip's own two ends.
 * Two launches per trip on `stream` (plus one per call that lays out the tiles), 256-thread blocks, no atomics: (a) a group of 32 lanes per frame (64 when
 * NB + E > 32), one lane per body, over tiles of 8 (4) frames that never span two clips: steps 1-4, the clamped dof into `scratch`, one partial sum of the
 * root_off gradient and of the loss per tile; (b) step 5 from `scratch` into `dof`, and per clip the partial sums added in tile order, root_off's Adam step,
 * loss[c] and step[c].  Every sum has a fixed order that does not depend on the clip's place in the batch: a clip's state after any number of trips has the
 * same bits alone, first, last or between other clips, and iterations = a then = b give the bits of a + b.  iterations == 0 checks the arguments and launches
 * nothing.  phc_fit_scratch_bytes(F, C, NB + E): negative F, C < 1 or NB + E outside [1, PHC_MAX_BODIES]: PHC_EINVAL.
 * Before any device work, PHC_EINVAL for: a null args or pointer field, num_clips / num_bodies / num_matched / num_frames < 1, num_ext < 0, a NaN lr, iterations < 0, clip_start_host
 * not starting at 0, not strictly increasing (a clip has at least one frame) or not ending at num_frames, a scratch below phc_fit_scratch_bytes, a pointer not
 * 4-byte (clip_start: 8-byte; scratch: 16-byte) aligned; PHC_EUNSUPPORTED for num_bodies + num_ext > PHC_MAX_BODIES, num_matched > PHC_FIT_MAX_MATCHED and more than
 * 2^31 - 1 tiles.  clip_start_host is the caller's host copy of the device array clip_start: the checks and the launch grid read it, the kernels read the
 * device array.  The contents of the other device arrays are the caller's duty (parents[b] < b with the root alone at -1, match_body in [0, NB + E),
 * match_slot in [0, M)); whatever they hold, no lane reads or writes outside the arrays' stated sizes. */
#define PHC_FIT_MAX_MATCHED 32
typedef struct {
    int32_t num_bodies, num_ext;              /* NB, E */
    int32_t num_matched, num_clips;           /* M, C */
    int64_t num_frames;                       /* F, all clips together */
    double  lr;                               /* torch.optim.Adam's lr (a python float there) */
    const int32_t*  parents;                  /* [NB + E]; an extended body's parent is a simulated body */
    const float*    offsets;                  /* [NB + E, 3] position in the parent's frame */
    const float*    rest;                     /* [NB + E, 9] rest rotation in the parent's frame, row-major matrices */
    const float*    axis;                     /* [ND, 3] joint axis of body j + 1 in its own frame */
    const float*    range;                    /* [ND, 2] lower, upper */
    const int32_t*  match_body;               /* [M] the matched body */
    const int32_t*  match_slot;               /* [M] its column of `target` */
    const uint32_t* subtree;                  /* [NB] bit m: matched entry m lies in the subtree of body j (bit set for match_body[m] == j too) */
    const int64_t*  clip_start;               /* [C + 1] frame offsets (device) */
    const int64_t*  clip_start_host;          /* [C + 1] the same values in host memory */
    const float*    target;                   /* [F, M, 3] */
    const float*    root_trans_offset;        /* [F, 3] */
    float *dof, *dof_m, *dof_v;               /* [F, ND] state: parameter, Adam's first and second moment */
    float *root_rot, *root_rot_m, *root_rot_v;/* [F, 3] */
    float *root_off, *root_off_m, *root_off_v;/* [C, 3] */
    int32_t* step;                            /* [C] Adam steps taken */
    float*   loss;                            /* [C] out: the loss the last trip evaluated (before its step) */
    void*    scratch;                         /* phc_fit_scratch_bytes(F, C, NB + E) bytes */
    int64_t  scratch_bytes;
} phc_fit_args_t;
int64_t phc_fit_scratch_bytes(int64_t num_frames, int32_t num_clips, int32_t num_bodies_ext);
int32_t phc_fit_iterate(const phc_fit_args_t* args /* host; pointers device memory except clip_start_host */, int32_t iterations, void* stream);

/* Keypoint fit of the all-spherical SMPL family on the device (csrc/phc_fit_sph.hip, per-lane code csrc/phc_fit_sph.h over csrc/phc_fit.h; an addition to
 * ABI 37, which stays 37): `iterations` trips of the loop of `fit_keypoint_clips` (phc_amd/utils/fit_keypoints.py) for C concatenated clips at once, fp32
 * throughout.  It takes phc_fit_args_t as it is, read for spherical joints: with ND = 3 (NB - 1), `dof`, `dof_m`, `dof_v` are [F, ND] -- body b's rotation
 * vector in its parent's frame at columns 3 (b - 1) .. 3 (b - 1) + 2 --, `range` is [ND, 2], the scratch rows are ND floats wide, `axis` is not read and may
 * be null, and num_ext is 0.  One trip is
 *   1. FK: R_0 = exp(root_rot), p_0 = root_trans_offset + root_off[c]; R_b = R_parent rest_b exp(rot_b), p_b = p_parent + R_parent offset_b;
 *   2. loss_c = mean_{t, m} |p[match_body[m]] - target[:, match_slot[m]]| + 0.01 mean(dof^2) (the regulariser over T_c ND values) -> loss[c];
 *   3. its analytic gradient: for a joint, with tau the torque of its subtree's matched entries in the joint's own frame,
 *      (tau + B r x tau + C r x (r x tau)) / (T_c M) + 0.02 r / (T_c ND) (the transposed right Jacobian of exp at r); the root rotation vector and root_off as
 *      in phc_fit_iterate;
 *   4. Adam with the clip's own step counter, as phc_fit_iterate; every component of dof clamped to `range`;
 *   5. dof smoothed along the clip's own frames by the normalised 5-tap gaussian of sigma 0.75 with replicate padding.  The root rotation is neither clamped
 *      nor smoothed.
 * Two launches per trip behind phc_fit_iterate's table launch, on `stream`, capturable in a graph: (a) one block per tile of 8 frames, a group of 32 lanes a
 * frame, a lane a body: steps 1-4 into the scratch rows, the partial sums per tile; (b) step 5 from `scratch` into `dof`, and per clip the partial sums added
 * in tile order, root_off's Adam step, loss[c] and step[c].  The sums' orders are phc_fit_iterate's: a clip's state after any number of trips has the same
 * bits alone, first, last or between other clips, and iterations = a then = b give the bits of a + b.  iterations == 0 checks the arguments and launches
 * nothing; a refused call writes nothing.  phc_fit_sph_scratch_bytes(F, C, NB): negative F, C < 1 or NB outside [1, 32]: PHC_EINVAL.
 * The checks are phc_fit_iterate's (with `axis` exempt from the null check and the scratch at least phc_fit_sph_scratch_bytes), then PHC_EUNSUPPORTED for
 * num_bodies > 32 (no all-spherical model above 32 bodies ships: there is no 64-lane instantiation) and for num_ext != 0; num_matched > PHC_FIT_MAX_MATCHED is
 * PHC_EUNSUPPORTED as there.  Whatever the device arrays hold, no lane reads or writes outside the arrays' stated sizes. */
int64_t phc_fit_sph_scratch_bytes(int64_t num_frames, int32_t num_clips, int32_t num_bodies);
int32_t phc_fit_sph_iterate(const phc_fit_args_t* args /* host; pointers device memory except clip_start_host */, int32_t iterations, void* stream);

/* ---- Recording the simulated motion (csrc/phc_record.hip, per-lane code and the rules csrc/phc_record.h; an addition to ABI 37, which stays 37) ------------
 * phc_motion_record: ONE launch per call, behind the post-physics launch on the same stream.  For every env i it appends one frame row to env i's block
 * [cap, W] of the caller-owned `frames` [N, cap, W] (fp32) and one header row to `header` [N, cap, 4] (int32).  With NB simulated bodies, E extended
 * (reference-only) ones and D DoFs a frame row is, in this order,
 *   root_pos 3 | body_quat_global NB x 4 (rigid_body_state's rotations, xyzw, bit for bit: no hemisphere flip) | pose_aa (NB + E) x 3 |
 *   dof_pos D | root linear and angular velocity 6 | reference time 1 | ref_body_pos NB x 3 (only with PHC_RECORD_REF)
 * so W = phc_motion_record_width(NB, E, D, flags) = 3 + 4 NB + 3 (NB + E) + D + 7 (+ 3 NB).  pose_aa row 0 is quat_to_exp_map(root rotation) (phc_math.h), the
 * row of a body on a spherical joint its three dof_pos values as they are (the DoF state already is the exp map), of a body on a revolute joint axis x dof_pos
 * (axis from phc_model_t's body floats; shape block 0), of every other body -- the extended ones included -- zero.  The reference time is
 * progress_buf dt + motion_start_times + motion_start_times_offset, the time post_physics_step looks up.  A header row is (segment id, progress_buf, motion id,
 * the frame's flag).
 * Per-env device state, all int32 [N]: len (frames held), seg (segment id), closed, dropped.  Row rule for env i with f = len[i]:
 *   1. closed[i], or f >= min(cap, limit[i]) (limit nullable: cap): nothing is written; in the second case, unless closed[i], dropped[i] += 1;
 *   2. otherwise the row is written at f and len[i] = f + 1;
 *   3. then, if flag[i] != 0 (the caller passes terminate_buf in the sweep, reset_buf in play): closed[i] = 1 with PHC_RECORD_ONE_SEGMENT, else seg[i] += 1
 *      (whether or not step 2 wrote the row, so that a segment cut short by `cap` still ends where the episode did).
 * With PHC_RECORD_SEED steps 1 and 2 alone run and the stored flag is 0: the current state becomes a frame whatever `flag` holds (used right after a reset, so
 * that frame 0 is the reset state).  Every decision is taken from device memory: no host read per call.
 * PHC_EINVAL before any device access: a null model / args / model table / required pointer (ref_body_pos is required with PHC_RECORD_REF only, limit never),
 * num_envs / num_bodies / num_dof / cap < 1, num_ext < 0, num_bodies / num_dof other than the model's, num_dof > 3 PHC_MAX_BODIES, a width other than phc_motion_record_width, dt not positive and finite, unknown flag bits;
 * PHC_EUNSUPPORTED: num_bodies + num_ext > PHC_MAX_BODIES. */
#define PHC_RECORD_REF 1
#define PHC_RECORD_SEED 2
#define PHC_RECORD_ONE_SEGMENT 4
typedef struct {
    int32_t num_envs, num_bodies, num_ext, num_dof;   /* N, NB, E, D */
    int32_t cap, width;                       /* frames per env block; W */
    int32_t flags;                            /* PHC_RECORD_* */
    float   dt;
    const float*   root_states;               /* [N, 13] */
    const float*   dof_state;                 /* [N, D, 2] */
    const float*   rigid_body_state;          /* [N, NB, 13] */
    const int64_t* progress_buf;              /* [N] */
    const int64_t* flag;                      /* [N] terminate_buf or reset_buf of this frame */
    const int64_t* motion_ids;                /* [N] sampled motion ids */
    const float*   motion_start_times;        /* [N] */
    const float*   motion_start_times_offset; /* [N] */
    const float*   ref_body_pos;              /* [N, NB, 3]; with PHC_RECORD_REF */
    const int32_t* limit;                     /* [N] per-env frame limit; nullable */
    float*   frames;                          /* [N, cap, W] out; 4-byte alignment suffices */
    int32_t* header;                          /* [N, cap, 4] out */
    int32_t* len;                             /* [N] state */
    int32_t* seg;                             /* [N] state */
    int32_t* closed;                          /* [N] state */
    int32_t* dropped;                         /* [N] state */
} phc_motion_record_args_t;
int32_t phc_motion_record_width(int32_t num_bodies, int32_t num_ext, int32_t num_dof, int32_t flags);
int32_t phc_motion_record(const phc_model_t* model /* host */, const phc_motion_record_args_t* args /* host */, void* stream);

/* ---- Video output: baseline JPEG scans of device frames (csrc/phc_jpeg.hip, per-block / per-segment code, the worst-case derivation and the scratch layout
 * csrc/phc_jpeg.h; additions to ABI 37, which stays 37) -------------------------------------------------------------------------------------------------------
 * `+render.format=avi` (phc_amd/video.py): the renderer's frames leave the device as the entropy-coded scans of a Motion-JPEG stream instead of 1.2 MB of
 * pixels each.  One call codes F frames rgba u8 [F, H, W, 4] (rows row_stride bytes apart, frames frame_stride bytes apart; alpha is ignored) into F
 * contiguous byte runs out[f * out_stride .. + length[f]): the complete scan of frame f, from the first entropy-coded byte to the last, RSTn markers included.
 * The host puts the frame header (SOI .. SOS: phc_amd/video.py jpeg_header) in front and EOI behind.  The stream is ISO/IEC 10918-1 baseline sequential, 8-bit,
 * three components, one interleaved scan:
 *   colour     JFIF full-range BT.601 of 8-bit R, G, B:  Y = 0.299 R + 0.587 G + 0.114 B,  Cb = -0.168735892 R - 0.331264108 G + 0.5 B + 128,
 *              Cr = 0.5 R - 0.418687589 G - 0.081312411 B + 128; level shift 128.  The frame is extended to multiples of 16 by replicating its last column and
 *              row (SOF0 carries the true size); chroma is 4:2:0, a sample = the mean of its 2 x 2 pixel group of the extended frame.  The MCU is 16 x 16
 *              pixels: Y00 Y01 Y10 Y11 Cb Cr, MCUs in raster order.
 *   transform  the orthonormal 8 x 8 DCT-II of A.3.3, S(v,u) = C(u) C(v) / 4 sum_y sum_x s(y,x) cos((2x+1) u pi / 16) cos((2y+1) v pi / 16), in fp32 as two
 *              passes of eight-term sums.  Quantisation: sign(S) floor(|S| / q + 0.5) with the caller's table entry q, in zigzag order (Figure A.6); the
 *              result is clamped to [-1023, 1023] (DC: [-1024, 1023]), which 8-bit input never reaches.
 *   qtab       u8 [2][64], HOST memory, zigzag order as DQT carries them: luminance, chrominance.  The caller scales Tables K.1 / K.2 (libjpeg's rule:
 *              s = quality < 50 ? 5000 / quality : 200 - 2 quality; clamp((t s + 50) / 100, 1, 255)); the kernels have no notion of quality.
 *   entropy    the typical Huffman tables K.3 - K.6 (the header emits them as DHT).  DC: the difference to the previous block of the same component, category
 *              SSSS + SSSS extra bits; AC: run / size symbols, ZRL for every 16 zeros in front of a non-zero coefficient, EOB behind the last non-zero one unless
 *              that is coefficient 63 (F.1.2).  A negative value's extra bits are those of value - 1.
 *   restarts   a segment is restart_interval MCUs (the last one of a frame may be shorter; an interval above the frame's MCU count is one segment); DRI says
 *              so.  The DC predictors are 0 at the start of every segment, its last byte is padded with 1-bits, every 0xFF byte of entropy-coded data is
 *              followed by 0x00, and segment i, unless it is the frame's last, is followed by the marker RST(i mod 8).
 * Segments are independent, so they are coded in parallel, each into a slot of worst-case size in `scratch`, and then moved to their places by a sum over the
 * segment lengths: no atomics, the bytes depend on the input alone and repeats are byte-identical.  phc_jpeg_frame_bound is the most a frame can take (1660 bits
 * per block, doubled for stuffing, + 2 per segment: phc_jpeg.h) and the least out_stride; no input makes a kernel write outside out [F, out_stride], length [F],
 * coef and scratch [scratch_bytes].
 * coef (nullable): i16 [F, 6 M, 64], M = ceil(W / 16) ceil(H / 16) -- the quantised coefficients in zigzag order, per component plane in raster block order:
 * the Y plane's 4 M blocks (a grid 2 ceil(W / 16) wide), then Cb's M, then Cr's M.
 * PHC_EINVAL before any device work for: args or rgba / qtab / out / length / scratch NULL, width or height outside 1 .. 65535, num_frames < 0, a quantiser entry
 * of 0, restart_interval < 1, row_stride < 4 width or not a multiple of 4, frame_stride < height row_stride or not a multiple of 4, rgba not 4-byte or coef /
 * scratch not 16-byte aligned, out_stride < phc_jpeg_frame_bound, scratch_bytes < phc_jpeg_scratch_bytes.  PHC_EUNSUPPORTED where a frame's bound passes 2^31 - 1
 * (its offsets are 32-bit).  num_frames == 0 returns 0 without a launch.  The two size functions return PHC_EINVAL for sizes the call would refuse. */
typedef struct {
    int32_t num_frames;                       /* F */
    int32_t width, height;                    /* W, H */
    int32_t restart_interval;                 /* MCUs per segment */
    int64_t row_stride, frame_stride;         /* bytes */
    const uint8_t* rgba;
    const uint8_t* qtab;                      /* host, [2][64] */
    uint8_t* out;                             /* [F, out_stride] */
    int64_t  out_stride;
    int32_t* length;                          /* [F] out */
    int16_t* coef;                            /* [F, 6 M, 64] out; nullable */
    void*    scratch;
    int64_t  scratch_bytes;
} phc_jpeg_args_t;
int64_t phc_jpeg_frame_bound(int32_t width, int32_t height, int32_t restart_interval);
int64_t phc_jpeg_scratch_bytes(int64_t num_frames, int32_t width, int32_t height, int32_t restart_interval);
int32_t phc_jpeg_encode(const phc_jpeg_args_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHC_AMD_H */
