// The constants the host-side scene builder (scene_build.h) shares with the kernels: no device code here, so that the builder
// compiles without a kernel header.  What each of them means is explained where the kernels use it.
#pragma once
#include <cstddef>
#include <cstdint>

// a leaf ref of the wide nodes: kLeaf | count << 27 | first item (trace.h, "wide nodes")
constexpr uint32_t kLeaf = 0x80000000u;

// the traversal stack: levels of a lane in LDS, and the private entries behind them (trace.h, TStack)
constexpr uint32_t kLdsStack = 8;
constexpr uint32_t kSpillStack = 40;

constexpr uint32_t kBlock = 256;
constexpr size_t kStackBytes = (size_t)kLdsStack * 2 * kBlock * sizeof(uint32_t);   // (ref, t0) per LDS level

constexpr uint32_t kFlatBudget = 32;         // triangle tests per ray up to which a scene is walked exhaustively (flat.h)

// the instructions of a texture's postfix program (shading.h, "textures")
enum { TEXOP_SCALAR = 0, TEXOP_IMAGE = 1, TEXOP_ADD = 2, TEXOP_SUB = 3, TEXOP_MUL = 4, TEXOP_DIV = 5, TEXOP_SRGB = 6 };
