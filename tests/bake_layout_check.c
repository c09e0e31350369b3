/* Prints the layout of the spt_bake structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_bake_host.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_bake_point);
    OFF(spt_bake_point, instance); OFF(spt_bake_point, prim); OFF(spt_bake_point, v); OFF(spt_bake_point, w);
    SIZE(spt_bake_world_point);
    OFF(spt_bake_world_point, p); OFF(spt_bake_world_point, pad0); OFF(spt_bake_world_point, n); OFF(spt_bake_world_point, pad1);
    SIZE(spt_bake_job);
    OFF(spt_bake_job, size); OFF(spt_bake_job, flags); OFF(spt_bake_job, kind); OFF(spt_bake_job, pad); OFF(spt_bake_job, n_points);
    OFF(spt_bake_job, points); OFF(spt_bake_job, rgb_out); OFF(spt_bake_job, samples); OFF(spt_bake_job, max_depth); OFF(spt_bake_job, seed);
    OFF(spt_bake_job, first_point); OFF(spt_bake_job, first_sample); OFF(spt_bake_job, points_per_pass); OFF(spt_bake_job, pad1);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_BAKE_DEVICE_POINTERS %u\n", (unsigned)SPT_BAKE_DEVICE_POINTERS);
    printf("SPT_BAKE_FLIP %u\n", (unsigned)SPT_BAKE_FLIP);
    printf("SPT_BAKE_POINTS_WORLD %u\n", (unsigned)SPT_BAKE_POINTS_WORLD);
    return 0;
}
