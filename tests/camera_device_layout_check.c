/* Prints the layout of the spt_camera_rays / spt_camera_gbuffer job structs as this compiler sees include/spt_abi.h: "name value" per
 * line.  tests/test_camera_device_abi.py compiles it and compares the numbers with the binding's ctypes declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_camera_rays_job);
    OFF(spt_camera_rays_job, size); OFF(spt_camera_rays_job, flags); OFF(spt_camera_rays_job, model); OFF(spt_camera_rays_job, plan);
    OFF(spt_camera_rays_job, first); OFF(spt_camera_rays_job, count); OFF(spt_camera_rays_job, rays); OFF(spt_camera_rays_job, aux);
    OFF(spt_camera_rays_job, rays_per_pass); OFF(spt_camera_rays_job, pad);
    SIZE(spt_camera_gbuffer_job);
    OFF(spt_camera_gbuffer_job, size); OFF(spt_camera_gbuffer_job, flags); OFF(spt_camera_gbuffer_job, model); OFF(spt_camera_gbuffer_job, plan);
    OFF(spt_camera_gbuffer_job, first); OFF(spt_camera_gbuffer_job, count); OFF(spt_camera_gbuffer_job, albedo); OFF(spt_camera_gbuffer_job, normal);
    OFF(spt_camera_gbuffer_job, depth); OFF(spt_camera_gbuffer_job, coverage); OFF(spt_camera_gbuffer_job, rays_per_pass); OFF(spt_camera_gbuffer_job, pad);
    SIZE(spt_path_ray);
    SIZE(spt_ray_aux);
    SIZE(spt_camera_model);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_CAMERA_RAYS_DEVICE_POINTERS %u\n", (unsigned)SPT_CAMERA_RAYS_DEVICE_POINTERS);
    printf("SPT_CAMERA_GBUFFER_DEVICE_POINTERS %u\n", (unsigned)SPT_CAMERA_GBUFFER_DEVICE_POINTERS);
    return 0;
}
