// one group of kernel instantiations (see kernel_list.h)
#define SPT_INSTANTIATE_GROUP_SHADE0_ORIGIN 1
#include "kernel_list.h"
