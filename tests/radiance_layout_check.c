/* Prints the layout of the spt_radiance structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_radiance_abi.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_path_ray);
    OFF(spt_path_ray, o); OFF(spt_path_ray, t_min); OFF(spt_path_ray, d); OFF(spt_path_ray, stream_a); OFF(spt_path_ray, stream_b); OFF(spt_path_ray, pad);
    SIZE(spt_ray_aux);
    OFF(spt_ray_aux, rx_o); OFF(spt_ray_aux, rx_d); OFF(spt_ray_aux, ry_o); OFF(spt_ray_aux, ry_d);
    SIZE(spt_radiance_job);
    OFF(spt_radiance_job, size); OFF(spt_radiance_job, flags); OFF(spt_radiance_job, n_rays); OFF(spt_radiance_job, rays); OFF(spt_radiance_job, aux);
    OFF(spt_radiance_job, repeats); OFF(spt_radiance_job, max_depth); OFF(spt_radiance_job, seed); OFF(spt_radiance_job, rng_skip);
    OFF(spt_radiance_job, rays_per_pass); OFF(spt_radiance_job, rgb_out); OFF(spt_radiance_job, hits_out);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_RADIANCE_DEVICE_POINTERS %u\n", (unsigned)SPT_RADIANCE_DEVICE_POINTERS);
    return 0;
}
