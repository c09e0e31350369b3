/* Prints the layout of the spt_gbuffer structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_gbuffer_abi.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_gbuffer_rec);
    OFF(spt_gbuffer_rec, p); OFF(spt_gbuffer_rec, t); OFF(spt_gbuffer_rec, n); OFF(spt_gbuffer_rec, instance); OFF(spt_gbuffer_rec, albedo);
    OFF(spt_gbuffer_rec, prim); OFF(spt_gbuffer_rec, v); OFF(spt_gbuffer_rec, w); OFF(spt_gbuffer_rec, surface); OFF(spt_gbuffer_rec, flags);
    SIZE(spt_gbuffer_job);
    OFF(spt_gbuffer_job, size); OFF(spt_gbuffer_job, flags); OFF(spt_gbuffer_job, n_rays); OFF(spt_gbuffer_job, rays); OFF(spt_gbuffer_job, aux);
    OFF(spt_gbuffer_job, rays_per_pass); OFF(spt_gbuffer_job, pad); OFF(spt_gbuffer_job, out);
    SIZE(spt_path_ray);
    SIZE(spt_ray_aux);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_GBUFFER_DEVICE_POINTERS %u\n", (unsigned)SPT_GBUFFER_DEVICE_POINTERS);
    printf("SPT_GBUF_BACKFACING %u\n", (unsigned)SPT_GBUF_BACKFACING);
    printf("SPT_GBUF_LIGHT %u\n", (unsigned)SPT_GBUF_LIGHT);
    return 0;
}
