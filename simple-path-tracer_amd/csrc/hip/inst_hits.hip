// spt_hits' kernels (hits_kernels.h): k_hits<kLds, kAll>, a unit of its own like inst_visibility.hip
#define SPT_INSTANTIATE_GROUP_HITS 1
#include "hits_kernels.h"
