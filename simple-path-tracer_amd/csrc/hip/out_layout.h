// Where the floats of a shard's packed film go in the caller's buffer, and how k_finish_host cuts that into stores.
// Shared by the kernel (film_kernels.h), by spt_render (spt_hip.hip) and by tests/out_layout_check.cpp, which runs the same
// functions on the CPU against a plain loop over rows.  Plain C++: no HIP type, no library call.
//
// spt_render's destination: local row r of the shard starts at byte (r / strip_rows) * out_strip_stride + (r % strip_rows) * row_bytes,
// so the rows of one strip are contiguous.  A *segment* is one strip's floats (all of the shard's when the layout is packed);
// segment s reads the film at float s * seg_floats and starts at destination float s * seg_stride.  Every segment is cut into
// *windows*: the 16-byte-aligned groups of four destination floats it touches.  A window that lies wholly inside its segment is
// one 16-byte store, a ragged one (the first and the last of a segment whose ends are not 16-byte aligned) is dword stores.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SPT_OUT_HD __host__ __device__ inline
#else
#define SPT_OUT_HD inline
#endif

struct OutLayout {
    uint64_t n_floats;      // of the shard: own_rows * width * 3
    uint64_t seg_floats;    // floats per (full) segment; the last may be shorter
    uint64_t seg_stride;    // destination floats from one segment's start to the next
    uint64_t n_segments;
    uint64_t seg_windows;   // windows per segment, an upper bound that holds for every misalignment
    uint32_t base_mis;      // (destination address / 4) & 3: floats by which the first segment is off a 16-byte boundary
};

// One window's work: `count` floats from film[src ..] to dst[dst ..] (float offsets from the first segment's start, which the
// caller adds to the destination address).  count == 4 means dst is 16-byte aligned: one 16-byte store.  count == 0: nothing.
struct OutWindow {
    uint64_t src, dst;
    uint32_t count;
};

// out_strip_stride in bytes, 0 = packed.  The caller has checked that a non-zero stride is no smaller than a strip and a multiple of 4.
SPT_OUT_HD OutLayout out_layout(uint64_t own_rows, uint64_t width, uint64_t strip_rows, uint64_t out_strip_stride, uint64_t dst_address) {
    OutLayout L;
    const uint64_t row_floats = width * 3u, strip_floats = strip_rows * row_floats;
    L.n_floats = own_rows * row_floats;
    const bool packed = out_strip_stride == 0u || out_strip_stride == strip_floats * 4u;
    L.seg_floats = packed ? L.n_floats : strip_floats;
    L.seg_stride = packed ? L.n_floats : out_strip_stride / 4u;
    L.n_segments = L.seg_floats ? (L.n_floats + L.seg_floats - 1u) / L.seg_floats : 0u;
    L.seg_windows = (L.seg_floats + 3u + 3u) / 4u;   // up to 3 floats of misalignment ahead, rounded up
    L.base_mis = (uint32_t)((dst_address >> 2) & 3u);
    return L;
}

SPT_OUT_HD uint64_t out_layout_items(const OutLayout& L) { return L.n_segments * L.seg_windows; }

// The last destination float's offset + 1: the span of the caller's buffer that the shard writes, in floats
SPT_OUT_HD uint64_t out_layout_span(const OutLayout& L) {
    if (L.n_segments == 0u) return 0u;
    return (L.n_segments - 1u) * L.seg_stride + (L.n_floats - (L.n_segments - 1u) * L.seg_floats);
}

SPT_OUT_HD OutWindow out_window(const OutLayout& L, uint64_t item) {
    const uint64_t seg = item / L.seg_windows, w = item - seg * L.seg_windows;
    const uint64_t src0 = seg * L.seg_floats, dst0 = seg * L.seg_stride;
    const uint64_t len = L.n_floats - src0 < L.seg_floats ? L.n_floats - src0 : L.seg_floats;
    const uint64_t mis = (L.base_mis + dst0) & 3u;   // this segment's first float within its 16-byte window
    // the window holds the segment's floats [4w - mis, 4w - mis + 4), cut to [0, len)
    const uint64_t lo = 4u * w > mis ? 4u * w - mis : 0u;
    uint64_t hi = 4u * w + 4u - mis;
    if (hi > len) hi = len;
    OutWindow o;
    o.src = src0 + lo;
    o.dst = dst0 + lo;
    o.count = hi > lo ? (uint32_t)(hi - lo) : 0u;
    return o;
}
