// one group of kernel instantiations (see kernel_list.h): spt_gbuffer's k_gbuffer<kTex, kPndf> (gbuffer_kernels.h)
#define SPT_INSTANTIATE_GROUP_GBUFFER 1
#include "kernel_list.h"
