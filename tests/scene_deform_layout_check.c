/* Prints the layout of spt_mesh_deform as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_scene_deform_host.py compiles it and compares the numbers with the binding's ctypes declaration. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_mesh_deform);
    OFF(spt_mesh_deform, mesh); OFF(spt_mesh_deform, tri_count);
    OFF(spt_mesh_deform, tri_pos); OFF(spt_mesh_deform, tri_attr);
    SIZE(spt_tri_pos);
    SIZE(spt_tri_attr);
    SIZE(spt_scene_update_desc);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    return 0;
}
