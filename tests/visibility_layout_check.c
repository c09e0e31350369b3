/* Prints the layout of the spt_occluded / spt_ao structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_visibility_abi.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_ray);
    OFF(spt_ray, o); OFF(spt_ray, t_min); OFF(spt_ray, d); OFF(spt_ray, t_max);
    SIZE(spt_occluded_job);
    OFF(spt_occluded_job, size); OFF(spt_occluded_job, flags); OFF(spt_occluded_job, n_rays); OFF(spt_occluded_job, rays); OFF(spt_occluded_job, out);
    OFF(spt_occluded_job, rays_per_pass); OFF(spt_occluded_job, pad);
    SIZE(spt_ao_rec);
    OFF(spt_ao_rec, sum); OFF(spt_ao_rec, open); OFF(spt_ao_rec, bent); OFF(spt_ao_rec, count);
    SIZE(spt_ao_job);
    OFF(spt_ao_job, size); OFF(spt_ao_job, flags); OFF(spt_ao_job, kind); OFF(spt_ao_job, pad); OFF(spt_ao_job, n_points); OFF(spt_ao_job, points);
    OFF(spt_ao_job, out); OFF(spt_ao_job, samples); OFF(spt_ao_job, max_distance); OFF(spt_ao_job, seed); OFF(spt_ao_job, first_point);
    OFF(spt_ao_job, first_sample); OFF(spt_ao_job, points_per_pass); OFF(spt_ao_job, pad1);
    SIZE(spt_bake_point);
    SIZE(spt_bake_world_point);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_OCCLUDED_DEVICE_POINTERS %u\n", (unsigned)SPT_OCCLUDED_DEVICE_POINTERS);
    printf("SPT_OCCLUDED_PACKED %u\n", (unsigned)SPT_OCCLUDED_PACKED);
    printf("SPT_AO_DEVICE_POINTERS %u\n", (unsigned)SPT_AO_DEVICE_POINTERS);
    printf("SPT_AO_FLIP %u\n", (unsigned)SPT_AO_FLIP);
    printf("SPT_BAKE_FLIP %u\n", (unsigned)SPT_BAKE_FLIP);
    return 0;
}
