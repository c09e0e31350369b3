// spt_occluded and spt_ao's kernels (visibility_kernels.h): k_occluded<kLds>, k_occluded_stream, k_ao<kLds> and k_ao_stream, a unit of its own like inst_bake.hip
#define SPT_INSTANTIATE_GROUP_VISIBILITY 1
#include "visibility_kernels.h"
