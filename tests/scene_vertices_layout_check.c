/* Prints the layout of spt_mesh_topology and spt_mesh_vertices as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_scene_vertices_host.py compiles it and compares the numbers with the binding's ctypes declarations. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_mesh_topology);
    OFF(spt_mesh_topology, size); OFF(spt_mesh_topology, mesh);
    OFF(spt_mesh_topology, n_vertices); OFF(spt_mesh_topology, tri_count);
    OFF(spt_mesh_topology, indices); OFF(spt_mesh_topology, face_of_tri);
    OFF(spt_mesh_topology, uv); OFF(spt_mesh_topology, normals);
    SIZE(spt_mesh_vertices);
    OFF(spt_mesh_vertices, mesh); OFF(spt_mesh_vertices, n_vertices);
    OFF(spt_mesh_vertices, positions); OFF(spt_mesh_vertices, normals);
    SIZE(spt_scene_update_desc);
    SIZE(spt_mesh_deform);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    return 0;
}
