// phc_kernels_plain.hip -- the PLAIN instantiations of the two task kernels (phc_task_kernel.h): the default SMPL task's feature set (phc_im_plain.h) as
// compile-time constants, <DPJ = 3, G = 32> only.  A translation unit of their own, compiled with phc_kernels.hip's flags (phc_amd/build.py), so that the generic
// kernels of phc_kernels.hip -- which launches these through task_launch when im_is_plain holds -- stay what they are.
#include "phc_task_kernel.h"

template __global__ void k_im_post_physics<3, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int);
template __global__ void k_im_reset<3, false, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int, const int64_t* __restrict__,
                                                        const float* __restrict__, int, uint64_t);
template __global__ void k_im_reset<3, true, 32, true>(phc_model_t, phc_motion_lib_t, phc_im_params_t, phc_sim_state_t, phc_im_buffers_t, int, const int64_t* __restrict__,
                                                       const float* __restrict__, int, uint64_t);
