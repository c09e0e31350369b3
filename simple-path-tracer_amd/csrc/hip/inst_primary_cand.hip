// one group of kernel instantiations (see kernel_list.h)
#define SPT_INSTANTIATE_GROUP_PRIMARY_CAND 1
#include "kernel_list.h"
