/* Prints the layout of the spt_hits structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_hits_abi.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_ray);
    OFF(spt_ray, o); OFF(spt_ray, t_min); OFF(spt_ray, d); OFF(spt_ray, t_max);
    SIZE(spt_hit_rec);
    OFF(spt_hit_rec, t); OFF(spt_hit_rec, instance); OFF(spt_hit_rec, prim); OFF(spt_hit_rec, flags); OFF(spt_hit_rec, v); OFF(spt_hit_rec, w);
    OFF(spt_hit_rec, pad);
    SIZE(spt_hit_count);
    OFF(spt_hit_count, total); OFF(spt_hit_count, back);
    SIZE(spt_hits_job);
    OFF(spt_hits_job, size); OFF(spt_hits_job, flags); OFF(spt_hits_job, n_rays); OFF(spt_hits_job, rays); OFF(spt_hits_job, hits);
    OFF(spt_hits_job, counts); OFF(spt_hits_job, max_hits); OFF(spt_hits_job, rays_per_pass);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_HITS_DEVICE_POINTERS %u\n", (unsigned)SPT_HITS_DEVICE_POINTERS);
    printf("SPT_HITS_COUNT_ALL %u\n", (unsigned)SPT_HITS_COUNT_ALL);
    printf("SPT_HIT_BACKFACING %u\n", (unsigned)SPT_HIT_BACKFACING);
    printf("SPT_GBUF_BACKFACING %u\n", (unsigned)SPT_GBUF_BACKFACING);
    printf("SPT_PRIM_MESH %u\n", (unsigned)SPT_PRIM_MESH);
    printf("SPT_PRIM_SPHERE %u\n", (unsigned)SPT_PRIM_SPHERE);
    return 0;
}
