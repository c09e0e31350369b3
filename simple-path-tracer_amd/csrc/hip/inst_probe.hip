// spt_probe's kernels (probe_kernels.h): k_probe_intake<kLds>, k_probe_intake_stream and k_probe_finish, a unit of its own like inst_bake.hip
#define SPT_INSTANTIATE_GROUP_PROBE 1
#include "probe_kernels.h"
