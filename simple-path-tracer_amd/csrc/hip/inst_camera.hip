// the instantiations of k_primary_cam (camera_kernels.h), a unit of its own like the groups of kernel_list.h
#define SPT_INSTANTIATE_GROUP_CAMERA 1
#include "camera_kernels.h"
