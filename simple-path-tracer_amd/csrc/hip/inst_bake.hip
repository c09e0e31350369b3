// spt_bake's kernels (bake_kernels.h): k_bake_intake<kLds>, k_bake_intake_stream and k_bake_finish, a unit of its own like the groups of kernel_list.h
#define SPT_INSTANTIATE_GROUP_BAKE 1
#include "bake_kernels.h"
