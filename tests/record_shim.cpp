// Host build of phc_amd/csrc/phc_record.h for tests/test_motion_record_cpu.py and tests/test_motion_record_gpu.py: the sizes, the argument check and whole
// launches of phc_motion_record as plain loops (all pointers, the model's tables included, are host memory here).
#include "phc_record.h"

extern "C" {

int record_sizeof_args() { return (int)sizeof(phc_motion_record_args_t); }
int record_block() { return phc::RECORD_BLOCK; }
int record_width_of(int nb, int ne, int nd, int flags) { return phc::record_width(nb, ne, nd, flags); }
int record_group_of(int nb, int ne) { return phc::record_group(nb, ne); }

int motion_record_check_of(const phc_model_t* m, const phc_motion_record_args_t* a) { return phc::motion_record_check(m, a); }
void motion_record_host_of(const phc_model_t* m, const phc_motion_record_args_t* a) { phc::motion_record_host(*m, *a); }

}
