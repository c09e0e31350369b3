/* Prints the layout of spt_camera_model as this compiler sees include/spt_abi.h: "name value" per line.
 * tests/test_camera_models.py compiles it and compares the numbers with the binding's ctypes declaration. */
#include <stddef.h>
#include <stdio.h>

#include "spt_abi.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))

int main(void) {
    SIZE(spt_camera);
    SIZE(spt_camera_model);
    OFF(spt_camera_model, size); OFF(spt_camera_model, type); OFF(spt_camera_model, base); OFF(spt_camera_model, lens_radius);
    OFF(spt_camera_model, focus_distance); OFF(spt_camera_model, view_height); OFF(spt_camera_model, pad);
    printf("SPT_ABI_VERSION %d\n", (int)SPT_ABI_VERSION);
    printf("SPT_CAMERA_PERSPECTIVE %d\n", (int)SPT_CAMERA_PERSPECTIVE);
    printf("SPT_CAMERA_THIN_LENS %d\n", (int)SPT_CAMERA_THIN_LENS);
    printf("SPT_CAMERA_ORTHOGRAPHIC %d\n", (int)SPT_CAMERA_ORTHOGRAPHIC);
    printf("SPT_CAMERA_PANORAMA %d\n", (int)SPT_CAMERA_PANORAMA);
    printf("SPT_CAMERA_SEED_SALT_HI %llu\n", (unsigned long long)(SPT_CAMERA_SEED_SALT >> 32));
    printf("SPT_CAMERA_SEED_SALT_LO %llu\n", (unsigned long long)(SPT_CAMERA_SEED_SALT & 0xffffffffull));
    return 0;
}
