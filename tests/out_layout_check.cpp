// csrc/hip/out_layout.h on the CPU: the windows k_finish_host walks, against a plain loop over rows.
//
// For every shape the destination is a byte buffer with guard bytes either side.  The program plays the kernel's stores into it
// (one 16-byte store for a window of four, dword stores otherwise) and checks that
//   * a 16-byte store is 16-byte aligned at the address the device would see;
//   * every destination float is written exactly once, with the film float the plain loop puts there:
//     local row r -> byte (r / strip_rows) * out_strip_stride + (r % strip_rows) * row_bytes;
//   * nothing outside those floats is written (guards, the gaps between a shard's strips), and the span the host checks for
//     pinning ends with the last float.
// Built with -fsanitize=address,undefined (`make out-layout-check`), so a store past the buffer is a report, not a wrong byte.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../simple-path-tracer_amd/csrc/hip/out_layout.h"

namespace {

int g_failures = 0;

void fail(const char* what, uint64_t rows, uint64_t width, uint64_t strip_rows, uint64_t stride, uint64_t mis) {
    std::fprintf(stderr, "out_layout: %s (rows %llu, width %llu, strip_rows %llu, stride %llu, base misaligned by %llu floats)\n", what,
                 (unsigned long long)rows, (unsigned long long)width, (unsigned long long)strip_rows, (unsigned long long)stride, (unsigned long long)mis);
    ++g_failures;
}

// own_rows rows of `width` pixels in strips of strip_rows, out_strip_stride bytes apart (0: packed); the destination starts
// `mis` floats past a 16-byte boundary
void check(uint64_t own_rows, uint64_t width, uint64_t strip_rows, uint64_t stride, uint64_t mis) {
    const uint64_t row_floats = width * 3, n = own_rows * row_floats, guard = 64;
    const uint64_t eff_stride = stride ? stride : strip_rows * row_floats * 4;
    const uint64_t n_strips = (own_rows + strip_rows - 1) / strip_rows;
    const uint64_t span_bytes = n_strips ? (n_strips - 1) * eff_stride + (own_rows - (n_strips - 1) * strip_rows) * row_floats * 4 : 0;
    // expected[k]: the film index destination float k holds, or -1
    std::vector<int64_t> expected(span_bytes / 4, -1);
    for (uint64_t r = 0; r < own_rows; ++r)
        for (uint64_t c = 0; c < row_floats; ++c)
            expected[((r / strip_rows) * eff_stride + (r % strip_rows) * row_floats * 4) / 4 + c] = (int64_t)(r * row_floats + c);

    // a buffer whose first destination float sits `mis` floats past a 16-byte boundary, guards around the span
    std::vector<uint32_t> storage(guard + 4 + span_bytes / 4 + guard + 4, 0xdeadbeefu);
    uint64_t first = guard;
    while ((((uintptr_t)&storage[first] >> 2) & 3u) != mis) ++first;
    uint32_t* dst = &storage[first];
    std::vector<uint8_t> writes(span_bytes / 4, 0);

    const OutLayout L = out_layout(own_rows, width, strip_rows, stride, (uint64_t)(uintptr_t)dst);
    if (out_layout_span(L) * 4 != span_bytes) fail("span differs from the plain loop's", own_rows, width, strip_rows, stride, mis);
    if (L.n_floats != n) fail("n_floats", own_rows, width, strip_rows, stride, mis);
    const uint64_t items = out_layout_items(L);
    uint64_t vec_stores = 0;
    for (uint64_t item = 0; item < items; ++item) {
        const OutWindow w = out_window(L, item);
        if (w.count > 4u) { fail("a window of more than four floats", own_rows, width, strip_rows, stride, mis); return; }
        if (w.count == 0u) continue;
        if (w.src + w.count > n) { fail("reads past the film", own_rows, width, strip_rows, stride, mis); return; }
        if (w.dst + w.count > span_bytes / 4) { fail("writes past the span", own_rows, width, strip_rows, stride, mis); return; }
        if (w.count == 4u) {
            if (((uintptr_t)(dst + w.dst) & 15u) != 0u) { fail("a 16-byte store that is not 16-byte aligned", own_rows, width, strip_rows, stride, mis); return; }
            ++vec_stores;
        }
        for (uint32_t k = 0; k < w.count; ++k) {
            dst[w.dst + k] = (uint32_t)(w.src + k);   // (the sanitizer watches this store)
            ++writes[w.dst + k];
        }
    }
    for (uint64_t k = 0; k < expected.size(); ++k) {
        if (expected[k] < 0) {
            if (writes[k] != 0 || dst[k] != 0xdeadbeefu) { fail("a float between the shard's strips was written", own_rows, width, strip_rows, stride, mis); return; }
        } else if (writes[k] != 1 || dst[k] != (uint32_t)expected[k]) {
            fail("a float is missing, written twice or holds another film float", own_rows, width, strip_rows, stride, mis);
            return;
        }
    }
    for (uint64_t k = 0; k < storage.size(); ++k)
        if ((k < first || k >= first + span_bytes / 4) && storage[k] != 0xdeadbeefu) { fail("a guard word was written", own_rows, width, strip_rows, stride, mis); return; }
    // all but the ragged ends of each segment go out as 16-byte stores
    if (n >= 16 && vec_stores + 2 * L.n_segments < n / 4) fail("too few 16-byte stores", own_rows, width, strip_rows, stride, mis);
}

}  // namespace

int main() {
    for (uint64_t mis = 0; mis < 4; ++mis) {
        check(80, 96, 16, 0, mis);                      // packed 96 x 80
        check(33, 97, 16, 0, mis);                      // ragged rows: 1164 bytes each
        check(33, 97, 16, 16 * 97 * 12, mis);           // the same with the stride of a packed film spelled out
        check(1, 1, 1, 0, mis);                         // three floats
        check(5, 2, 2, 2 * 2 * 12 + 4, mis);            // strips 4 bytes apart more than their size: every strip's alignment differs
        for (uint64_t shard = 0; shard < 3; ++shard) {  // 96 x 80 in strips of 4 over 3 shards: 20 strips, shards own 7, 7 and 6
            const uint64_t strips = (20 - shard + 2) / 3;
            check(strips * 4, 96, 4, 3 * 4 * 96 * 12, mis);
        }
        check(27, 97, 4, 3 * 4 * 97 * 12, mis);         // ragged rows, strided, a short last strip (27 = 6 * 4 + 3)
        check(7, 97, 16, 5 * 16 * 97 * 12, mis);        // a single short strip
    }
    check(0, 96, 16, 0, 0);                             // a shard without rows
    if (g_failures) return 1;
    std::puts("out_layout_check ok");
    return 0;
}
