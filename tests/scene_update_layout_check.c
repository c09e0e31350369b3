/* Prints the layout of spt_scene_update_desc as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_scene_update_host.py compiles it and compares the numbers with the binding's ctypes declaration. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_scene_update_desc);
    OFF(spt_scene_update_desc, size); OFF(spt_scene_update_desc, flags);
    OFF(spt_scene_update_desc, n_tlas_nodes); OFF(spt_scene_update_desc, tlas_nodes);
    OFF(spt_scene_update_desc, n_instances); OFF(spt_scene_update_desc, instances);
    OFF(spt_scene_update_desc, n_lights); OFF(spt_scene_update_desc, lights);
    OFF(spt_scene_update_desc, light_alias);
    SIZE(spt_alias_table);
    SIZE(spt_instance);
    SIZE(spt_light);
    SIZE(spt_bvh_node);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    return 0;
}
