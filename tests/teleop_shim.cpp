// Host build of phc_amd/csrc/phc_teleop.h for tests/test_teleop_cpu.py and tests/test_teleop_gpu.py: the argument check and a whole launch of
// phc_teleop_rewards as a loop over the envs (all pointers are host memory here).
#include "phc_teleop.h"

extern "C" {

int teleop_args_check_of(const phc_motion_lib_t* lib, const phc_teleop_args_t* a) { return phc::teleop_args_check(lib, a); }

// phc_teleop_rewards on the host: the entry point's check, then the same per-lane functions and the same group sums over all envs
int teleop_rewards_host(const phc_motion_lib_t* lib, const phc_teleop_args_t* a) {
    const int rc = phc::teleop_args_check(lib, a);
    if (rc) return rc;
    phc_motion_lib_t l = {};
    if (lib) l = *lib;
    for (int64_t e = 0; e < a->num_envs; ++e) phc::teleop_env_host(l, *a, e);
    return 0;
}

}
