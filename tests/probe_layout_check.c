/* Prints the layout of the spt_probe structs as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_probe_host.py compiles it and compares the numbers with the binding's ctypes / numpy declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_probe_point);
    OFF(spt_probe_point, p); OFF(spt_probe_point, pad);
    SIZE(spt_probe_job);
    OFF(spt_probe_job, size); OFF(spt_probe_job, flags); OFF(spt_probe_job, n_points); OFF(spt_probe_job, points); OFF(spt_probe_job, sh_out);
    OFF(spt_probe_job, aux_out); OFF(spt_probe_job, samples); OFF(spt_probe_job, max_depth); OFF(spt_probe_job, seed); OFF(spt_probe_job, first_point);
    OFF(spt_probe_job, first_sample); OFF(spt_probe_job, points_per_pass); OFF(spt_probe_job, pad);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_PROBE_DEVICE_POINTERS %u\n", (unsigned)SPT_PROBE_DEVICE_POINTERS);
    return 0;
}
