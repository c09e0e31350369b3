// spt_camera_rays' and spt_camera_gbuffer's kernels (camera_device_kernels.h): k_camera_rays, k_gbuffer_image<kTex, kPndf> and
// k_gbuffer_image_finish, a unit of its own like inst_visibility.hip
#define SPT_INSTANTIATE_GROUP_CAMERA_DEVICE 1
#include "camera_device_kernels.h"
