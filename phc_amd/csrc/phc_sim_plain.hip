// phc_sim_plain.hip -- the PLAIN instantiation of k_sim_step (phc_sim_kernel.h): the default SMPL task's launch (phc_sim_plain.h) with its options, nullable pointers
// and tree constants as compile-time constants and the launch-invariant drive terms formed once.  A translation unit of its own, compiled with phc_sim.hip's flags
// (phc_amd/build.py), so that the generic kernels of phc_sim.hip -- whose chooser launches this one when sim_is_plain holds -- stay what they are.
#include "phc_sim_kernel.h"

template __global__ void k_sim_step<true, PHC_JT_SPHERICAL, 32, false, false, 2, true, false, true>(phc_model_t, phc_sim_params_t, phc_sim_state_t, const float* __restrict__,
                                                                                                    const float* __restrict__, const float* __restrict__,
                                                                                                    const int32_t* __restrict__, int, const int64_t* __restrict__, int,
                                                                                                    WrenchArgs<false>, DrArgs<false>);
