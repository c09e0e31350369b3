// Film / filter kernels and the small test seams: cheap to compile, only spt_hip.hip includes this file (the heavy
// kernel templates of kernels.h are instantiated in their own translation units, see kernel_list.h).
#pragma once
#include "kernels.h"
#include "out_layout.h"

// ---------------------------------------------------------------------------- resolve
// k_resolve for passes of the chunked k_primary (slot bits; the only form the headline workload runs).
// Only the samples marked in slot_bits own a slot; the others were black and add nothing (film.rs:87 adds +0 for them: the
// same sum).  The additions of a pixel are sequential, so what the kernel waits for is memory latency, once per batch:
// kBatch samples = their mask bytes + 3 kBatch slot loads are requested TOGETHER - the slot loads do not wait for the mask; an
// unmarked slot is read (whatever it holds) and not added.  With the per-row spans nearly every live sample is marked, so the
// extra reads are few.  (Round 2's form - mask first, then the marked slots of one byte at a time - took one round trip per 8
// samples: 0.07 ms per launch whatever the shard size, 0.17 of the 0.6 ms step of an 8-GPU rank.)
//
// kMoments (a film object with SPT_FILM_MOMENTS, spt_film_*): the one extra argument is the film's Q, and every added sample x also
// gives Q = Q + x * x per channel in the same pass over the slots.  Without kMoments there is no extra argument: the signature, and
// with it the kernel's code, stay those of the plain resolve (the Q pointer does not go into RenderCtx, which every hot kernel
// takes by value).
template <uint32_t kResolveBatch, bool kMoments = false, class... Sq>
__global__ void __launch_bounds__(256, 3) k_resolve_bits(RenderCtx rc, Sq... sq_arg) {
    static_assert(sizeof...(Sq) == (kMoments ? 1u : 0u), "k_resolve_bits<., true> takes the film's Q pointer, <., false> nothing more");
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= rc.n_pixels) return;
    if (rc.first_slot[lp] >= rc.pass_samples) return;
    const size_t plane = rc.rad_plane;
    const float* rp = rc.rad + lp;
    const uint8_t* bp = rc.slot_bits + lp;
    f3 sum = mk3(rc.film[3 * lp], rc.film[3 * lp + 1], rc.film[3 * lp + 2]);
    float* sq = nullptr;
    f3 sum_sq = mk3(0, 0, 0);
    if constexpr (kMoments) {
        sq = (sq_arg, ...);
        sum_sq = mk3(sq[3 * lp], sq[3 * lp + 1], sq[3 * lp + 2]);
    }
    for (uint32_t s0 = 0; s0 < rc.pass_samples; s0 += kResolveBatch) {
        uint32_t m = 0u;
        float r[kResolveBatch], g[kResolveBatch], b[kResolveBatch];
#pragma unroll
        for (uint32_t q = 0; q < kResolveBatch / 8u; ++q)
            if (s0 + 8u * q < rc.pass_samples) m |= (uint32_t)bp[(size_t)((s0 >> 3) + q) * rc.n_pixels] << (8u * q);
#pragma unroll
        for (uint32_t k = 0; k < kResolveBatch; ++k) {
            if (s0 + k < rc.pass_samples) {
                const size_t ri = (size_t)(s0 + k) * rc.n_pixels;
                r[k] = rp[ri]; g[k] = rp[plane + ri]; b[k] = rp[2 * plane + ri];
            }
        }
        if (m == 0u) continue;
#pragma unroll
        for (uint32_t k = 0; k < kResolveBatch; ++k)
            if ((m >> k) & 1u) {
                const f3 x = mk3(r[k], g[k], b[k]);
                sum = sum + x;
                if (kMoments) sum_sq = sum_sq + x * x;
            }
    }
    rc.film[3 * lp] = sum.x; rc.film[3 * lp + 1] = sum.y; rc.film[3 * lp + 2] = sum.z;
    if constexpr (kMoments) { sq[3 * lp] = sum_sq.x; sq[3 * lp + 1] = sum_sq.y; sq[3 * lp + 2] = sum_sq.z; }
}

// kMoments: as in k_resolve_bits.  The samples before `first` went into the film in k_primary: misses, black unless the scene has an
// environment, and a film with moments of such a scene takes the chunked path (k_resolve_bits), so Q misses nothing here.
template <bool kMoments = false, class... Sq>
__global__ void __launch_bounds__(256) k_resolve(RenderCtx rc, Sq... sq_arg) {
    static_assert(sizeof...(Sq) == (kMoments ? 1u : 0u), "k_resolve<true> takes the film's Q pointer, <false> nothing more");
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= rc.n_pixels) return;
    const uint32_t first = rc.first_slot[lp];
    if (first >= rc.pass_samples) return;
    const size_t plane = rc.rad_plane;
    f3 sum = mk3(rc.film[3 * lp], rc.film[3 * lp + 1], rc.film[3 * lp + 2]);
    float* sq = nullptr;
    f3 sum_sq = mk3(0, 0, 0);
    if constexpr (kMoments) {
        sq = (sq_arg, ...);
        sum_sq = mk3(sq[3 * lp], sq[3 * lp + 1], sq[3 * lp + 2]);
    }
    // the additions are sequential (sample order = the reference's, film.rs:87), the loads are not: 8 samples
    // (24 loads) in flight per lane, which matters when a narrow shard leaves few pixels to hide latency with
    uint32_t s = first;
    for (; s + 8u <= rc.pass_samples; s += 8u) {
        float r[8], g[8], b[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const size_t ri = (size_t)(s + k) * rc.n_pixels + lp;
            r[k] = rc.rad[ri]; g[k] = rc.rad[plane + ri]; b[k] = rc.rad[2 * plane + ri];
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const f3 x = mk3(r[k], g[k], b[k]);
            sum = sum + x;
            if (kMoments) sum_sq = sum_sq + x * x;
        }
    }
    for (; s < rc.pass_samples; ++s) {
        const size_t ri = (size_t)s * rc.n_pixels + lp;
        const f3 x = mk3(rc.rad[ri], rc.rad[plane + ri], rc.rad[2 * plane + ri]);
        sum = sum + x;  // film.rs:87
        if (kMoments) sum_sq = sum_sq + x * x;
    }
    rc.film[3 * lp] = sum.x; rc.film[3 * lp + 1] = sum.y; rc.film[3 * lp + 2] = sum.z;
    if constexpr (kMoments) { sq[3 * lp] = sum_sq.x; sq[3 * lp + 1] = sum_sq.y; sq[3 * lp + 2] = sum_sq.z; }
}

// The bucket sums of a bucketed film (spt_film_buckets), after the resolve of the same pass and over the same radiance slots: one
// lane per pixel.  Sample s of the pass has the plan index rc.pass_first + s and belongs to bucket (rc.pass_first + s) % K, so the
// samples of bucket j are s_j, s_j + K, ... in increasing s, and the additions of one bucket are sequential in that order.
// Different buckets do not depend on each other: the lane takes a group of up to kBucketGroup buckets at once (K <= 8: all of
// them; else two groups of about K / 2), loads their sums together, then walks the rounds - round m holds the m-th sample of each
// bucket of the group - requesting the slots of a round (kBits: their raw mask bytes too) together before it adds them, each to
// its own register (every register index is a compile-time one; the bucket number only enters addresses), and stores the group
// back.  Every slot is read once, with up to 8 samples (24 loads) in flight per lane, as in k_resolve.
// kBits: after a chunked primary, where only the samples marked in slot_bits own a slot (the others were black and add
// nothing); else after an un-chunked one, where the samples before first_slot were black (a bucketed film of a scene with an
// environment takes the chunked primary, as a film with moments does) and every later one owns a slot.  An unmarked slot is
// read (whatever it holds) and not added, as in k_resolve_bits.  A pixel that the pass did not trace (outside the screen bound,
// or retired in an adaptive film) has first_slot == pass_samples and is left alone; a bucket without a sample in the pass too.
// K, the bucket array and its plane stride (floats per bucket) are arguments of this kernel only: RenderCtx does not grow.
constexpr uint32_t kBucketGroup = 8;

template <bool kBits>
__global__ void __launch_bounds__(256) k_resolve_buckets(RenderCtx rc, uint32_t K, float* buckets, size_t bucket_plane) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= rc.n_pixels) return;
    const uint32_t first = rc.first_slot[lp];
    const uint32_t n = rc.pass_samples;
    if (first >= n) return;
    const size_t plane = rc.rad_plane, np = rc.n_pixels;
    const float* rp = rc.rad + lp;
    const uint8_t* bp = kBits ? rc.slot_bits + lp : nullptr;
    const uint32_t phase = rc.pass_first % K;
    const uint32_t n_groups = (K + kBucketGroup - 1u) / kBucketGroup, group = (K + n_groups - 1u) / n_groups;
    for (uint32_t j0 = 0; j0 < K; j0 += group) {
        const uint32_t in_group = min(group, K - j0);
        // Straight-line code between the loads: a slot of the group that has no bucket (c >= in_group) or no sample left reads a
        // clamped address (bucket K - 1, the pass's last sample) and its value is not used, so no branch separates the loads
        // and all of a round's are requested before the first wait.
        uint32_t s[kBucketGroup];     // the next sample of the pass in bucket j0 + c; >= n: none (left)
        f3 sum[kBucketGroup];
        uint32_t touched = 0u;
#pragma unroll
        for (uint32_t c = 0; c < kBucketGroup; ++c) {
            const uint32_t j = j0 + c;
            s[c] = c < in_group ? (j >= phase ? j - phase : j + K - phase) : n;
            const float* bj = buckets + (size_t)min(j, K - 1u) * bucket_plane + 3 * (size_t)lp;
            sum[c] = mk3(bj[0], bj[1], bj[2]);
            if (s[c] < n) touched |= 1u << c;
        }
        uint32_t pending = touched;
        // One round.  It is called once ahead of the loop, so that the first round's loads are requested together with the
        // sums' loads above (one dependent round trip per round, the sums' included in the first).
        auto round = [&]() {
            float r[kBucketGroup], g[kBucketGroup], b[kBucketGroup];
            uint32_t mb[kBucketGroup];   // kBits: the raw mask byte; the bit is taken in the add loop, as k_resolve_bits does
#pragma unroll
            for (uint32_t c = 0; c < kBucketGroup; ++c) {
                const uint32_t sl = min(s[c], n - 1u);
                const size_t ri = (size_t)sl * np;
                mb[c] = kBits ? (uint32_t)bp[(size_t)(sl >> 3) * np] : 0u;
                r[c] = rp[ri]; g[c] = rp[plane + ri]; b[c] = rp[2 * plane + ri];
            }
#pragma unroll
            for (uint32_t c = 0; c < kBucketGroup; ++c) {
                const bool live = s[c] < n;
                const bool marked = live && (kBits ? ((mb[c] >> (s[c] & 7u)) & 1u) != 0u : s[c] >= first);
                if (marked) sum[c] = sum[c] + mk3(r[c], g[c], b[c]);
                if (live) s[c] += K;
                if (s[c] >= n) pending &= ~(1u << c);
            }
        };
        if (pending != 0u) round();
        while (pending != 0u) round();
#pragma unroll
        for (uint32_t c = 0; c < kBucketGroup; ++c)
            if ((touched >> c) & 1u) {
                float* bj = buckets + (size_t)(j0 + c) * bucket_plane + 3 * (size_t)lp;
                bj[0] = sum[c].x; bj[1] = sum[c].y; bj[2] = sum[c].z;
            }
    }
}

// film.rs:91: color / weight_sum  (Color / f32 = Color * (1/f32))
__global__ void __launch_bounds__(256) k_finish(RenderCtx rc, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rc.n_pixels * 3u) return;
    out[i] = rc.film[i] * rc.spp_inv;
}

// k_finish with the caller's buffer as its destination: `dst` is the device-visible address of spt_render's rgb_mean_out (pinned
// host memory, checked per call by spt_render), so the image needs neither the scene's `out` buffer nor the runtime's copy, whose
// blit kernel holds up the k_primary beside it for as long as it runs (profiles/r05_copy_probe.md).  The same product for every
// float; out_layout.h says where a float goes (packed, or strip by strip in a larger film) and cuts the destination into
// 16-byte stores with dword stores at the ragged ends of a segment.  Grid-stride over the windows.
// kFinishHostGrid: FEW workgroups on purpose.  MEASURED (profiles/r05_copy_probe.md, a k_primary-shaped kernel of 0.55 ms beside a copy kernel of
// 12.6 MB into pinned memory): 256 or 4096 workgroups lengthen it to 0.72 ms, as the runtime's blit kernel does; 32 to 0.62 - 0.65; 4 leave it at
// 0.55 and take 0.6 - 0.76 ms themselves, which the film stream has.  Plain against non-temporal stores: no difference beyond the ranges; plain.
constexpr uint32_t kFinishHostGrid = 4;
constexpr bool kFinishHostNonTemporal = false;
typedef float finish_v4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_finish_host(RenderCtx rc, OutLayout lay, float* dst) {
    const uint64_t items = out_layout_items(lay);
    for (uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += (uint64_t)gridDim.x * blockDim.x) {
        const OutWindow w = out_window(lay, item);
        const float* src = rc.film + w.src;
        if (w.count == 4u) {
            const finish_v4 v = {src[0] * rc.spp_inv, src[1] * rc.spp_inv, src[2] * rc.spp_inv, src[3] * rc.spp_inv};
            finish_v4* to = reinterpret_cast<finish_v4*>(dst + w.dst);
            if (kFinishHostNonTemporal) __builtin_nontemporal_store(v, to);
            else *to = v;
        } else {
            for (uint32_t k = 0; k < w.count; ++k) {
                const float v = src[k] * rc.spp_inv;
                if (kFinishHostNonTemporal) __builtin_nontemporal_store(v, dst + w.dst + k);
                else dst[w.dst + k] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------- general box filter
// BoxFilter::weight (src/filter/boxf.rs:27-33) of sample s of `pixel` seen from a pixel (di, dj) away: the film keeps
// (offset - 0.5) per sample (pt.rs:278) and filter_pixel adds the pixel distance (film.rs:84-85).  The offsets are the
// sampler's first draws of the sample's stream, so they are recomputed here instead of being stored.
SPT_DEV float box_weight(const RenderCtx& rc, uint32_t pixel, uint32_t s, int32_t di, int32_t dj, float radius) {
    DRng rng;
    rng.s.state = 0ull;
    if (rc.sampler != SPT_SAMPLER_RECURRENCE) rng.s = spt_rng_seed(rc.seed, pixel, s);
    float ox, oy;
    pixel_offset(rc, pixel, s, rng, &ox, &oy);
    const float wx = (float)di + (ox - 0.5f), wy = (float)dj + (oy - 0.5f);
    return (fabsf(wx) <= radius && fabsf(wy) <= radius) ? 1.0f : 0.0f;
}

// radius_int <= 0 (radius <= 0.5): the colour is the pixel's own in-order sum (rc.film), the weight sum counts the
// samples whose offset lies inside the box (all of them at radius 0.5, which is k_finish).  radius_int < 0
// (radius <= -0.5) leaves both loops of filter_pixel empty: 0 * (1 / 0).
// The film holds the samples [s_first, s_first + s_count) of the plan: spt_render passes [0, spp), a film object what it covers.
__global__ void __launch_bounds__(256) k_finish_box(RenderCtx rc, float* out, float radius, int32_t R, uint32_t s_first, uint32_t s_count) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= rc.n_pixels) return;
    f3 sum = mk3(0, 0, 0);
    float wsum = 0.0f;
    if (R == 0) {
        const uint32_t row_local = lp / rc.width, col = lp - row_local * rc.width;
        const uint32_t pixel = global_row(rc, row_local) * rc.width + col;
        sum = mk3(rc.film[3 * lp], rc.film[3 * lp + 1], rc.film[3 * lp + 2]);
        for (uint32_t s = s_first; s < s_first + s_count; ++s) wsum += box_weight(rc, pixel, s, 0, 0, radius);
    }
    const f3 c = sum * (1.0f / wsum);   // film.rs:91, Color / f32 = Color * (1 / f32) (color.rs:125-131)
    out[3 * lp] = c.x; out[3 * lp + 1] = c.y; out[3 * lp + 2] = c.z;
}

// Read-out of a film object (spt_film_read) for radius 0.5, one lane per float: SPT_FILM_MEAN is S * (1 / n), the operation of
// k_finish; SPT_FILM_VAR_OF_MEAN is the variance of that mean from the moments, m = S * (1/n), v = (Q * (1/n) - m * m) * (1/(n - 1)),
// clamped at 0 (a NaN stays one) and +inf for one sample.  The reciprocals come from the host, as rc.spp_inv does for k_finish.
// The variance of the mean of one channel from its mean m = S * (1/n), n >= 2 samples: the one formula of SPT_FILM_VAR_OF_MEAN and of
// spt_film_adapt's criterion.
SPT_DEV float film_var_of_mean(float m, float q, float inv_n, float inv_n1) {
    const float v = (q * inv_n - m * m) * inv_n1;
    return v < 0.0f ? 0.0f : v;
}

__global__ void __launch_bounds__(256) k_film_read(uint32_t what, uint32_t n_floats, const float* sum, const float* sum_sq, uint32_t n,
                                                   float inv_n, float inv_n1, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    const float m = sum[i] * inv_n;
    if (what == SPT_FILM_MEAN) { out[i] = m; return; }
    if (n == 1u) { out[i] = __builtin_huge_valf(); return; }
    out[i] = film_var_of_mean(m, sum_sq[i], inv_n, inv_n1);
}

// k_film_read of an adaptive film: pixel p covers n_p samples, `done` while it is active (mask 1), counts[p] once retired.  The
// reciprocals come from the host's table inv[k] = 1.0f / (float)k, k = 0 .. spp (no device division), so MEAN and VAR_OF_MEAN
// are those of a plain film read at n_p samples, bit for bit.
__global__ void __launch_bounds__(256) k_film_read_counts(uint32_t what, uint32_t n_floats, const float* sum, const float* sum_sq,
                                                          const uint8_t* mask, const uint32_t* counts, uint32_t done, const float* inv,
                                                          float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    const uint32_t px = i / 3u;
    const uint32_t n = mask[px] ? done : counts[px];
    const float inv_n = inv[n];
    const float m = sum[i] * inv_n;
    if (what == SPT_FILM_MEAN) { out[i] = m; return; }
    if (n == 1u) { out[i] = __builtin_huge_valf(); return; }
    out[i] = film_var_of_mean(m, sum_sq[i], inv_n, inv[n - 1u]);
}

// spt_film_read_robust: the median of the bucket means (SPT_ROBUST_MON) or their Gini-adaptive trimmed mean (SPT_ROBUST_GMON) of
// a bucketed film, one lane per float (pixel and channel); the arithmetic is spelled out in spt_abi.h and every operation below
// is one rounded f32 operation in that order.  The keys live in a fixed array of kMaxBuckets registers whose slots from K on hold
// +inf: every index is a compile-time one (the loops are unrolled, K only enters as a predicate), and the sorting network -
// odd-even transposition, kMaxBuckets rounds of compare and select - leaves the K keys in a[0 .. K - 1] in ascending order,
// because nothing sorts behind a +inf.  A key is never a NaN nor -0, so the order is total and the sorted keys are unique.
// The film covers [first, first + n) at the pixel: n = done (kCounts: while the pixel is active, else counts[px]), and bucket j
// holds n_j = c(first + n) - c(first) samples with c(x) = x / K + (x % K > j), integer arithmetic.  The reciprocals come from the
// host's table inv[k] = 1.0f / (float)k, k = 0 .. spp; kf = (float)K, gk = (float)(K + 1) / (float)K and hf = (float)((K - 1) / 2)
// are rounded by the host too.
constexpr uint32_t kMaxBuckets = 15;

template <bool kCounts>
__global__ void __launch_bounds__(256) k_film_read_robust(uint32_t estimator, uint32_t n_floats, uint32_t K, const float* sum, const float* buckets,
                                                          size_t bucket_plane, uint32_t first, uint32_t done, const uint8_t* mask,
                                                          const uint32_t* counts, const float* inv, float kf, float gk, float hf, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    uint32_t n = done;
    if constexpr (kCounts) {
        const uint32_t px = i / 3u;
        n = mask[px] ? done : counts[px];
    }
    if (n < K) { out[i] = sum[i] * inv[n]; return; }   // some bucket is empty: the plain mean
    const uint32_t q0 = first / K, r0 = first % K, q1 = (first + n) / K, r1 = (first + n) % K;
    // All loads first, without a branch between them.  n_j is d - 1, d or d + 1 with d = q1 - q0 (n >= K, so d >= 1), so three
    // reciprocals of the table serve every bucket (the index d + 1 is clamped to n: n_j <= n); a slot from K on reads bucket
    // K - 1 once more and its value is not used.  kMaxBuckets + 3 loads are requested together, the keys come after one wait.
    const uint32_t d = q1 - q0;
    float r_lo = inv[d - 1u], r_mid = inv[d], r_hi = inv[min(d + 1u, n)];
    float a[kMaxBuckets], bsum[kMaxBuckets];
#pragma unroll
    for (uint32_t j = 0; j < kMaxBuckets; ++j) bsum[j] = buckets[(size_t)min(j, K - 1u) * bucket_plane + i];
    // (one empty statement that names every loaded value: the scheduler otherwise holds some of the loads back until earlier
    //  ones have been consumed, four dependent round trips instead of one)
    asm volatile("" : "+v"(bsum[0]), "+v"(bsum[1]), "+v"(bsum[2]), "+v"(bsum[3]), "+v"(bsum[4]), "+v"(bsum[5]), "+v"(bsum[6]), "+v"(bsum[7]),
                      "+v"(bsum[8]), "+v"(bsum[9]), "+v"(bsum[10]), "+v"(bsum[11]), "+v"(bsum[12]), "+v"(bsum[13]), "+v"(bsum[14]));
    static_assert(kMaxBuckets == 15, "the statement above names 15 values");
#pragma unroll
    for (uint32_t j = 0; j < kMaxBuckets; ++j) {
        const uint32_t up = r1 > j ? 1u : 0u, down = r0 > j ? 1u : 0u;   // n_j = d + up - down
        const float rcp = up == down ? r_mid : (up != 0u ? r_hi : r_lo);
        const float mu = bsum[j] * rcp;
        a[j] = (j < K && spt_is_finite(mu)) ? mu + 0.0f : __builtin_huge_valf();
    }
#pragma unroll
    for (uint32_t round = 0; round < kMaxBuckets; ++round) {
#pragma unroll
        for (uint32_t j = round & 1u; j + 1u < kMaxBuckets; j += 2u) {
            const float lo = a[j], hi = a[j + 1u];
            const bool swap = hi < lo;
            a[j] = swap ? hi : lo;
            a[j + 1u] = swap ? lo : hi;
        }
    }
    const uint32_t h = (K - 1u) / 2u;
    uint32_t t = h;
    if (estimator == SPT_ROBUST_GMON) {
        float num = 0.0f, den = 0.0f, top = 0.0f;
#pragma unroll
        for (uint32_t j = 0; j < kMaxBuckets; ++j)
            if (j < K) {
                num = num + (float)(j + 1u) * a[j];
                den = den + a[j];
                top = a[j];
            }
        if (top != __builtin_huge_valf()) {   // (a key is finite or +inf)
            t = 0u;
            if (den > 0.0f) {
                const float G = (2.0f * num) / (kf * den) - gk;
                if (G > 0.0f) t = (G * hf >= hf) ? h : (uint32_t)(G * hf);
            }
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < kMaxBuckets; ++j)
        if (j >= t && j + t < K) acc = acc + a[j];
    // MON (and t == h): the one key a[h], which the sum above holds exactly (0 + a is a: no key is -0) and inv[1] is 1
    out[i] = acc * inv[K - 2u * t];
}

// spt_film_adapt: one 256-lane block per 16x16 tile of the shard, k_primary's numbering (tile = tx + tiles_x * ty over the packed
// rows).  An active pixel whose variance of the mean meets v_c <= (rel * |m_c| + floor)^2 in all three channels (n = done samples,
// exact f32, no sqrt: a NaN never retires) is retired: mask 0, counts = n.  The block's active count goes to tile_active[tile]
// (plain store); totals[0] += active pixels, totals[1] += 1 if the tile keeps any (the host zeroes both first).
__global__ void __launch_bounds__(256) k_film_adapt(uint32_t width, uint32_t rows, uint32_t tiles_x, const float* sum, const float* sum_sq,
                                                    uint8_t* mask, uint32_t* counts, uint32_t* tile_active, uint32_t* totals, uint32_t n,
                                                    float inv_n, float inv_n1, float rel_error, float abs_floor) {
    __shared__ uint32_t wave_active[256 / 64];
    const uint32_t tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const uint32_t i = tx * 16u + (threadIdx.x % 16u), row_local = ty * 16u + (threadIdx.x / 16u);
    bool active = false;
    if (i < width && row_local < rows) {
        const uint32_t lp = row_local * width + i;
        active = mask[lp] != 0u;
        if (active) {
            bool retire = true;
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) {
                const float m = sum[3 * lp + c] * inv_n;
                const float v = film_var_of_mean(m, sum_sq[3 * lp + c], inv_n, inv_n1);
                const float tol = rel_error * fabsf(m) + abs_floor;
                retire = retire && (v <= tol * tol);
            }
            if (retire) {
                mask[lp] = 0u;
                counts[lp] = n;
                active = false;
            }
        }
    }
    const unsigned long long b = __ballot(active);
    if ((threadIdx.x & 63u) == 0u) wave_active[threadIdx.x / 64u] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0u;
        for (uint32_t w = 0; w < 256u / 64u; ++w) t += wave_active[w];
        tile_active[tile] = t;
        if (t != 0u) {
            atomicAdd(&totals[0], t);
            atomicAdd(&totals[1], 1u);
        }
    }
}

// ---------------------------------------------------------------------------- denoiser (spt_film_denoise)
// An edge-aware 5x5 a-trous wavelet filter (B3 spline) over a film's mean, guided by the variance of that mean and, optionally,
// by a second film (the guide: e.g. first-hit normals) and ITS variance.  The arithmetic is spelled out in spt_abi.h; every
// operation below is one rounded f32 operation in that order, so a float32 restatement on the host gives the same bits.
//
// What the filter reads of one film: its sums and how many samples each pixel covers (mask == nullptr: `done` for all, the
// reciprocals from the host; else an adaptive film's mask / counts / inv table, as in k_film_read_counts).
struct DenoiseFilm {
    const float* sum;
    const float* sum_sq;
    const uint8_t* mask;
    const uint32_t* counts;
    const float* inv;
    uint32_t done;
    float inv_n, inv_n1;
};

// SPT_FILM_MEAN and SPT_FILM_VAR_OF_MEAN of pixel lp, the operations of k_film_read / k_film_read_counts.
SPT_DEV void denoise_film_pixel(const DenoiseFilm& f, uint32_t lp, f3* m_out, f3* v_out) {
    uint32_t n = f.done;
    float inv_n = f.inv_n, inv_n1 = f.inv_n1;
    if (f.mask) {
        n = f.mask[lp] ? f.done : f.counts[lp];
        inv_n = f.inv[n];
        inv_n1 = f.inv[n - 1u];
    }
    const f3 s = mk3(f.sum[3 * lp], f.sum[3 * lp + 1], f.sum[3 * lp + 2]);
    const f3 q = mk3(f.sum_sq[3 * lp], f.sum_sq[3 * lp + 1], f.sum_sq[3 * lp + 2]);
    const f3 m = mk3(s.x * inv_n, s.y * inv_n, s.z * inv_n);
    *m_out = m;
    if (n == 1u) { *v_out = mk3(__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()); return; }
    *v_out = mk3(film_var_of_mean(m.x, q.x, inv_n, inv_n1), film_var_of_mean(m.y, q.y, inv_n, inv_n1), film_var_of_mean(m.z, q.z, inv_n, inv_n1));
}

// One lane per pixel: colour (r, g, b, lv) with lv the variance of the mean's luminance, and - kGuide - guide (gx, gy, gz, gv)
// with gv the summed variance of the guide's channels.  One 16-byte store per pixel and array.
template <bool kGuide>
__global__ void __launch_bounds__(256) k_denoise_pack(uint32_t n_pixels, DenoiseFilm film, DenoiseFilm guide, float4* color_out, float4* guide_out) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= n_pixels) return;
    f3 m, v;
    denoise_film_pixel(film, lp, &m, &v);
    const float lv = ((0.299f * 0.299f) * v.x + (0.587f * 0.587f) * v.y) + (0.114f * 0.114f) * v.z;
    color_out[lp] = make_float4(m.x, m.y, m.z, lv);
    if constexpr (kGuide) {
        f3 g, u;
        denoise_film_pixel(guide, lp, &g, &u);
        guide_out[lp] = make_float4(g.x, g.y, g.z, (u.x + u.y) + u.z);
    }
}

// ok(q) of the specification: a pixel whose colour or luminance variance is not finite neither filters nor is filtered.
SPT_DEV bool denoise_ok(const float4& c) { return spt_is_finite(c.x) && spt_is_finite(c.y) && spt_is_finite(c.z) && spt_is_finite(c.w); }

struct DenoiseArgs {
    uint32_t width, rows, tiles_x;
    int32_t step;                     // 1 << k
    float kc2, kg2, eps_c, eps_g;     // k_color^2, k_guide^2 (multiplied by the host), the two epsilons
};

// The distance d of one tap before the cut-off: the luminance term and - kGuide - the guide's term (pixel q seen from pixel p).
template <bool kGuide>
SPT_DEV float denoise_dist(const DenoiseArgs& a, const float4& cp, const float4& gp, float l_p, const float4& cq, const float4& gq) {
    const float dl = l_p - luminance(mk3(cq.x, cq.y, cq.z));
    float d = (dl * dl) / (a.kc2 * (cp.w + cq.w) + a.eps_c);
    if constexpr (kGuide) {
        const float ex = gp.x - gq.x, ey = gp.y - gq.y, ez = gp.z - gq.z;
        d = d + ((ex * ex + ey * ey) + ez * ez) / (a.kg2 * (gp.w + gq.w) + a.eps_g);
    }
    return d;
}

// A tap at distance d with spline weight hw, added to p's three sums.
SPT_DEV void denoise_add(float d, const float4& cq, float hw, f3& acc, float& ws, float& va) {
    if (!(d < 87.0f)) return;   // (also a NaN; spt_exp(-d) is 0 beyond)
    const float w = hw * spt_exp(-d);
    acc = mk3(acc.x + w * cq.x, acc.y + w * cq.y, acc.z + w * cq.z);
    ws = ws + w;
    va = va + (w * w) * cq.w;
}

// One tap of the filter: pixel q (colour record cq, guide record gq, spline weight hw) seen from pixel p, added to p's three sums.
template <bool kGuide>
SPT_DEV void denoise_tap(const DenoiseArgs& a, const float4& cp, const float4& gp, float l_p, const float4& cq, const float4& gq, float hw,
                         f3& acc, float& ws, float& va) {
    if (!denoise_ok(cq)) return;
    denoise_add(denoise_dist<kGuide>(a, cp, gp, l_p, cq, gq), cq, hw, acc, ws, va);
}

// What a pixel becomes after its 25 taps; kLast: packed RGB f32 (the film's read-out staging buffer), the variance is dropped.
template <bool kLast>
SPT_DEV void denoise_store(uint32_t lp, const float4& cp, const f3& acc, float ws, float va, float4* color_out, float* rgb_out) {
    float4 r = cp;   // a pixel that is not ok passes through
    if (denoise_ok(cp)) r = make_float4(acc.x / ws, acc.y / ws, acc.z / ws, va / (ws * ws));
    if constexpr (kLast) {
        rgb_out[3 * lp] = r.x; rgb_out[3 * lp + 1] = r.y; rgb_out[3 * lp + 2] = r.z;
    } else {
        color_out[lp] = r;
    }
}

SPT_DEV float denoise_h(int32_t d) { return d == 0 ? 3.0f / 8.0f : ((d == -1 || d == 1) ? 1.0f / 4.0f : 1.0f / 16.0f); }   // the B3 spline

// One a-trous iteration: one 256-lane block per 16x16 tile (k_primary's numbering), one lane per pixel, 25 taps at distance
// `step`, rows top to bottom and left to right within a row: the order of the sums.  A tap is one 16-byte load of the colour record
// and - kGuide - one of the guide record; the taps are independent, and one row of five (10 loads) is requested before its
// arithmetic starts, which keeps the kernel under 128 VGPRs.  The re-reads of the neighbours hit L1 / L2: per iteration the kernel
// moves 48 bytes per pixel with a guide (32 read + 16 written), 32 without.  A tap outside the image reads the lane's own pixel
// and is not added.  The kernel is bound by its arithmetic (two divisions and one spt_exp per tap), not by these loads: staging the
// tile's footprint in LDS for steps 1 and 2 was measured and changed nothing ("Denoising").
template <bool kGuide, bool kLast>
__global__ void __launch_bounds__(256) k_denoise_atrous(DenoiseArgs a, const float4* __restrict__ color_in, const float4* __restrict__ guide,
                                                        float4* __restrict__ color_out, float* __restrict__ rgb_out) {
    const uint32_t tile = blockIdx.x, tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int32_t x = (int32_t)(tx * 16u + (threadIdx.x % 16u)), y = (int32_t)(ty * 16u + (threadIdx.x / 16u));
    if (x >= (int32_t)a.width || y >= (int32_t)a.rows) return;
    const uint32_t lp = (uint32_t)y * a.width + (uint32_t)x;
    const float4 cp = color_in[lp];
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (kGuide) gp = guide[lp];
    const float l_p = luminance(mk3(cp.x, cp.y, cp.z));
    f3 acc = mk3(0, 0, 0);
    float ws = 0.0f, va = 0.0f;
#pragma unroll 1
    for (int32_t dy = -2; dy <= 2; ++dy) {
        const int32_t qy = y + a.step * dy;
        const bool row_in = qy >= 0 && qy < (int32_t)a.rows;
        float4 cq[5], gq[5];
        bool in[5];
#pragma unroll
        for (int32_t k = 0; k < 5; ++k) {
            const int32_t qx = x + a.step * (k - 2);
            in[k] = row_in && qx >= 0 && qx < (int32_t)a.width;
            const uint32_t lq = in[k] ? (uint32_t)qy * a.width + (uint32_t)qx : lp;
            cq[k] = color_in[lq];
            gq[k] = gp;
            if constexpr (kGuide) gq[k] = guide[lq];
        }
        const float hy = denoise_h(dy);
#pragma unroll
        for (int32_t k = 0; k < 5; ++k)
            if (in[k]) denoise_tap<kGuide>(a, cp, gp, l_p, cq[k], gq[k], hy * denoise_h(k - 2), acc, ws, va);
    }
    denoise_store<kLast>(lp, cp, acc, ws, va, color_out, rgb_out);
}

// ---- the albedo variants (spt_film_denoise_job with an albedo film) ----------------------------------------------------------
// A third record per pixel, (al.r, al.g, al.b, av): the albedo film's mean and the summed variance of that mean.  Its term joins d
// behind the guide's; with `demodulate` the colour record holds m / dem and the variance v / (dem * dem), dem = max(al, eps_demod)
// per channel (a NaN albedo gives the floor), and the last iteration multiplies dem back.  spt_abi.h has the arithmetic.
struct DenoiseAlbedo {
    float ka2, eps_a, eps_d;   // k_albedo^2 (multiplied by the host), eps_albedo, eps_demod
    uint32_t demodulate;
};

SPT_DEV f3 denoise_dem(const float4& al, float eps_d) {
    return mk3(al.x > eps_d ? al.x : eps_d, al.y > eps_d ? al.y : eps_d, al.z > eps_d ? al.z : eps_d);
}

template <bool kGuide>
__global__ void __launch_bounds__(256) k_denoise_pack_albedo(uint32_t n_pixels, DenoiseFilm film, DenoiseFilm guide, DenoiseFilm albedo, DenoiseAlbedo b,
                                                             float4* color_out, float4* guide_out, float4* albedo_out) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= n_pixels) return;
    f3 m, v, al, ua;
    denoise_film_pixel(film, lp, &m, &v);
    denoise_film_pixel(albedo, lp, &al, &ua);
    const float4 ar = make_float4(al.x, al.y, al.z, (ua.x + ua.y) + ua.z);
    if (b.demodulate != 0u) {
        const f3 dem = denoise_dem(ar, b.eps_d);
        m = mk3(m.x / dem.x, m.y / dem.y, m.z / dem.z);
        v = mk3(v.x / (dem.x * dem.x), v.y / (dem.y * dem.y), v.z / (dem.z * dem.z));
    }
    const float lv = ((0.299f * 0.299f) * v.x + (0.587f * 0.587f) * v.y) + (0.114f * 0.114f) * v.z;
    color_out[lp] = make_float4(m.x, m.y, m.z, lv);
    albedo_out[lp] = ar;
    if constexpr (kGuide) {
        f3 g, u;
        denoise_film_pixel(guide, lp, &g, &u);
        guide_out[lp] = make_float4(g.x, g.y, g.z, (u.x + u.y) + u.z);
    }
}

// The same records from caller-provided images (spt_denoise_image): planar RGB triplets as SPT_FILM_MEAN / SPT_FILM_VAR_OF_MEAN
// return them, one array per quantity, instead of a film's sums.  One lane per pixel: one 12-byte load per array (the compiler
// joins the triplet into a global_load_dwordx3; consecutive lanes read consecutive triplets, so a wave's load covers 768
// contiguous bytes), the operations of k_denoise_pack / k_denoise_pack_albedo in their order, one 16-byte store per record.
// The four instantiations take 9, 18, 22 and 24 VGPRs and no scratch.  The kernel moves 24 bytes in and 16 out per pixel and
// array pair and does at most six divisions.  From those byte counts it should be bound by memory and small next to an a-trous
// iteration (25 taps with two divisions and an exponential each); its time has not been measured.
struct DenoiseImage {
    const float* mean;          // m
    const float* var;           // v
    const float* guide_mean;    // g   (kGuide)
    const float* guide_var;     // u
    const float* albedo_mean;   // al  (kAlbedo)
    const float* albedo_var;    // ua
};

SPT_DEV f3 denoise_image_rgb(const float* a, uint32_t lp) {
    const size_t i = 3 * (size_t)lp;
    return mk3(a[i], a[i + 1], a[i + 2]);
}

template <bool kGuide, bool kAlbedo>
__global__ void __launch_bounds__(256) k_denoise_pack_image(uint32_t n_pixels, DenoiseImage in, DenoiseAlbedo b, float4* color_out,
                                                            float4* guide_out, float4* albedo_out) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= n_pixels) return;
    f3 m = denoise_image_rgb(in.mean, lp), v = denoise_image_rgb(in.var, lp);
    if constexpr (kAlbedo) {
        const f3 al = denoise_image_rgb(in.albedo_mean, lp), ua = denoise_image_rgb(in.albedo_var, lp);
        const float4 ar = make_float4(al.x, al.y, al.z, (ua.x + ua.y) + ua.z);
        if (b.demodulate != 0u) {
            const f3 dem = denoise_dem(ar, b.eps_d);
            m = mk3(m.x / dem.x, m.y / dem.y, m.z / dem.z);
            v = mk3(v.x / (dem.x * dem.x), v.y / (dem.y * dem.y), v.z / (dem.z * dem.z));
        }
        albedo_out[lp] = ar;
    }
    const float lv = ((0.299f * 0.299f) * v.x + (0.587f * 0.587f) * v.y) + (0.114f * 0.114f) * v.z;
    color_out[lp] = make_float4(m.x, m.y, m.z, lv);
    if constexpr (kGuide) {
        const f3 g = denoise_image_rgb(in.guide_mean, lp), u = denoise_image_rgb(in.guide_var, lp);
        guide_out[lp] = make_float4(g.x, g.y, g.z, (u.x + u.y) + u.z);
    }
}

// k_denoise_atrous with the albedo record: one more 16-byte load per tap (a row of five is 15 loads with a guide), the same order
// of the sums.  kLast: the demodulated colour is multiplied by dem in the store, pass-through pixels included.
template <bool kGuide, bool kLast>
__global__ void __launch_bounds__(256) k_denoise_atrous_albedo(DenoiseArgs a, DenoiseAlbedo b, const float4* __restrict__ color_in,
                                                               const float4* __restrict__ guide, const float4* __restrict__ albedo,
                                                               float4* __restrict__ color_out, float* __restrict__ rgb_out) {
    const uint32_t tile = blockIdx.x, tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int32_t x = (int32_t)(tx * 16u + (threadIdx.x % 16u)), y = (int32_t)(ty * 16u + (threadIdx.x / 16u));
    if (x >= (int32_t)a.width || y >= (int32_t)a.rows) return;
    const uint32_t lp = (uint32_t)y * a.width + (uint32_t)x;
    const float4 cp = color_in[lp], ap = albedo[lp];
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (kGuide) gp = guide[lp];
    const float l_p = luminance(mk3(cp.x, cp.y, cp.z));
    f3 acc = mk3(0, 0, 0);
    float ws = 0.0f, va = 0.0f;
#pragma unroll 1
    for (int32_t dy = -2; dy <= 2; ++dy) {
        const int32_t qy = y + a.step * dy;
        const bool row_in = qy >= 0 && qy < (int32_t)a.rows;
        float4 cq[5], gq[5], aq[5];
        bool in[5];
#pragma unroll
        for (int32_t k = 0; k < 5; ++k) {
            const int32_t qx = x + a.step * (k - 2);
            in[k] = row_in && qx >= 0 && qx < (int32_t)a.width;
            const uint32_t lq = in[k] ? (uint32_t)qy * a.width + (uint32_t)qx : lp;
            cq[k] = color_in[lq];
            aq[k] = albedo[lq];
            gq[k] = gp;
            if constexpr (kGuide) gq[k] = guide[lq];
        }
        const float hy = denoise_h(dy);
#pragma unroll
        for (int32_t k = 0; k < 5; ++k)
            if (in[k] && denoise_ok(cq[k])) {
                float d = denoise_dist<kGuide>(a, cp, gp, l_p, cq[k], gq[k]);
                const float ex = ap.x - aq[k].x, ey = ap.y - aq[k].y, ez = ap.z - aq[k].z;
                d = d + ((ex * ex + ey * ey) + ez * ez) / (b.ka2 * (ap.w + aq[k].w) + b.eps_a);
                denoise_add(d, cq[k], hy * denoise_h(k - 2), acc, ws, va);
            }
    }
    float4 r = cp;   // a pixel that is not ok passes through
    if (denoise_ok(cp)) r = make_float4(acc.x / ws, acc.y / ws, acc.z / ws, va / (ws * ws));
    if constexpr (kLast) {
        if (b.demodulate != 0u) {
            const f3 dem = denoise_dem(ap, b.eps_d);
            r.x = r.x * dem.x; r.y = r.y * dem.y; r.z = r.z * dem.z;
        }
        rgb_out[3 * lp] = r.x; rgb_out[3 * lp + 1] = r.y; rgb_out[3 * lp + 2] = r.z;
    } else {
        color_out[lp] = r;
    }
}

// radius_int >= 1: Film::filter_pixel (film.rs:71-92) over the kept samples of a band of whole rows.  Rows j, then
// columns i, then the samples of that pixel in the order they were added, one running colour sum (the colour is NOT
// weighted - film.rs:87 adds sample.color as is - only weight_sum looks at the offsets).
struct BoxJob {
    const float* rad;               // 3 planes [c][sample][band pixel]
    uint32_t band_base, band_rows;  // image rows held by the planes
    uint32_t out_j0, out_rows;      // image rows to filter
    float* out;                     // first pixel of row out_j0 in the packed output of the shard
    int32_t R;
    float radius;
};
__global__ void __launch_bounds__(256) k_filter_box(RenderCtx rc, BoxJob job) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= job.out_rows * rc.width) return;
    const uint32_t row = idx / rc.width, x = idx - row * rc.width;
    const int32_t y = (int32_t)(job.out_j0 + row);
    const size_t n_band = (size_t)job.band_rows * rc.width, plane = n_band * rc.spp;
    f3 sum = mk3(0, 0, 0);
    float wsum = 0.0f;
    for (int32_t dj = -job.R; dj <= job.R; ++dj) {
        const int32_t jj = y + dj;
        if (jj < 0 || jj >= (int32_t)rc.height) continue;
        for (int32_t di = -job.R; di <= job.R; ++di) {
            const int32_t ii = (int32_t)x + di;
            if (ii < 0 || ii >= (int32_t)rc.width) continue;
            const uint32_t pixel = (uint32_t)jj * rc.width + (uint32_t)ii;
            const size_t lp = (size_t)((uint32_t)jj - job.band_base) * rc.width + (uint32_t)ii;
            for (uint32_t s = 0; s < rc.spp; ++s) {
                const size_t ri = (size_t)s * n_band + lp;
                sum = sum + mk3(job.rad[ri], job.rad[plane + ri], job.rad[2 * plane + ri]);
                wsum += box_weight(rc, pixel, s, di, dj, job.radius);
            }
        }
    }
    const f3 c = sum * (1.0f / wsum);
    job.out[3 * (size_t)idx] = c.x; job.out[3 * (size_t)idx + 1] = c.y; job.out[3 * (size_t)idx + 2] = c.z;
}

// ---------------------------------------------------------------------------- sample-keeping films (SPT_FILM_KEEP_SAMPLES)
// A film that keeps its samples owns, per run of consecutive own rows, the radiance of every covered sample of the run's stored
// rows (the own rows and R halo rows each way): one chunk per wavefront pass, three planes [c][sample in pass][stored pixel] as the
// pass wrote them.  The chunks of a run cover the film's samples in increasing plan index without gaps.
struct KeptChunk {
    const float* rad;   // 3 planes of `count` samples, count * stored pixels floats apart
    uint32_t first;     // plan index of the chunk's first sample
    uint32_t count;     // its samples
};

struct KeptJob {
    const KeptChunk* chunks;        // the run's chunk table, on the device
    uint32_t n_chunks;
    uint32_t band_base, band_rows;  // image rows the chunks hold
    uint32_t out_j0, out_rows;      // image rows to filter
    float* out;                     // first pixel of row out_j0 in the packed output of the shard
    int32_t R;
    float radius;
    uint32_t mean;                  // 1: colour * (1 / weight_sum) (SPT_FILM_MEAN); 0: the colour (SPT_FILM_SUM)
};

// The read-out of a sample-keeping film: Film::filter_pixel (film.rs:71-92) over the kept samples, the loops of k_filter_box with
// the samples of a pixel walked chunk by chunk (increasing plan index).  One lane per output pixel; consecutive lanes read
// consecutive floats of every plane.  The colour chain is sequential by specification, the loads are not: kBatch samples (3 kBatch
// loads) are requested together before the first is added, as in k_resolve; the host picks kBatch by R.
// weight_sum adds 0.0f or 1.0f per sample, which in f32 is min(count, 2^24) whatever the order: the kernel counts in integers.
// Every sample's offset is derived again per neighbour that reads it, as k_filter_box does.  (The measurements behind kBatch, and
// the count table that was tried instead of the RNG: DESIGN.md, "Films that keep their samples".)
template <uint32_t kBatch>
__global__ void __launch_bounds__(256) k_film_filter_box(RenderCtx rc, KeptJob job) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= job.out_rows * rc.width) return;
    const uint32_t row = idx / rc.width, x = idx - row * rc.width;
    const int32_t y = (int32_t)(job.out_j0 + row);
    const size_t n_band = (size_t)job.band_rows * rc.width;
    f3 sum = mk3(0, 0, 0);
    unsigned long long inside = 0ull;
    for (int32_t dj = -job.R; dj <= job.R; ++dj) {
        const int32_t jj = y + dj;
        if (jj < 0 || jj >= (int32_t)rc.height) continue;
        for (int32_t di = -job.R; di <= job.R; ++di) {
            const int32_t ii = (int32_t)x + di;
            if (ii < 0 || ii >= (int32_t)rc.width) continue;
            const uint32_t pixel = (uint32_t)jj * rc.width + (uint32_t)ii;
            const size_t lp = (size_t)((uint32_t)jj - job.band_base) * rc.width + (uint32_t)ii;
            for (uint32_t c = 0; c < job.n_chunks; ++c) {
                const KeptChunk ch = job.chunks[c];
                const size_t plane = (size_t)ch.count * n_band;
                const float* rp = ch.rad + lp;
                uint32_t s = 0;
                for (; s + kBatch <= ch.count; s += kBatch) {
                    float r[kBatch], g[kBatch], b[kBatch];
#pragma unroll
                    for (uint32_t k = 0; k < kBatch; ++k) {
                        const size_t ri = (size_t)(s + k) * n_band;
                        r[k] = rp[ri]; g[k] = rp[plane + ri]; b[k] = rp[2 * plane + ri];
                    }
#pragma unroll
                    for (uint32_t k = 0; k < kBatch; ++k) {
                        sum = sum + mk3(r[k], g[k], b[k]);
                        if (box_weight(rc, pixel, ch.first + s + k, di, dj, job.radius) != 0.0f) ++inside;
                    }
                }
                for (; s < ch.count; ++s) {
                    const size_t ri = (size_t)s * n_band;
                    sum = sum + mk3(rp[ri], rp[plane + ri], rp[2 * plane + ri]);
                    if (box_weight(rc, pixel, ch.first + s, di, dj, job.radius) != 0.0f) ++inside;
                }
            }
        }
    }
    f3 c = sum;
    if (job.mean) {
        const float wsum = (float)(inside < (1ull << 24) ? inside : (1ull << 24));
        c = sum * (1.0f / wsum);
    }
    job.out[3 * (size_t)idx] = c.x; job.out[3 * (size_t)idx + 1] = c.y; job.out[3 * (size_t)idx + 2] = c.z;
}

// ---- weighted reconstruction filters over the kept samples (spt_film_filter) ----
// What a filter's f(a) reads besides the radius: GAUSSIAN a[0] = alpha, a[1] = e_r = spt_exp(-(alpha * (r * r))), made on the host
// (spt_exp has the same bits there); MITCHELL a[0..3] = c3, c2, c1, c0 and a[4..6] = q3, q2, q0, rounded once from double.
struct FilterCoef {
    float a[7];
};

// f(a) of include/spt_abi.h ("reconstruction filters"), 0 <= a <= r, one rounded operation at a time
template <uint32_t kType>
SPT_DEV float filter_f(const FilterCoef& fc, float r, float a) {
    if constexpr (kType == SPT_FILTER_TENT) {
        return r - a;
    } else if constexpr (kType == SPT_FILTER_GAUSSIAN) {
        const float g = spt_exp(-(fc.a[0] * (a * a))) - fc.a[1];
        return g < 0.0f ? 0.0f : g;
    } else {
        const float t = (2.0f * a) / r;
        if (t > 1.0f) return ((fc.a[0] * t + fc.a[1]) * t + fc.a[2]) * t + fc.a[3];
        return ((fc.a[4] * t + fc.a[5]) * t) * t + fc.a[6];
    }
}

// The weight of sample s of `pixel` seen from a pixel (di, dj) away, 0.0f for a sample outside the support: the offsets as
// box_weight derives them, the support test before any filter evaluation.
template <uint32_t kType>
SPT_DEV float filter_weight(const RenderCtx& rc, const FilterCoef& fc, uint32_t pixel, uint32_t s, int32_t di, int32_t dj, float r) {
    DRng rng;
    rng.s.state = 0ull;
    if (rc.sampler != SPT_SAMPLER_RECURRENCE) rng.s = spt_rng_seed(rc.seed, pixel, s);
    float ox, oy;
    pixel_offset(rc, pixel, s, rng, &ox, &oy);
    const float ax = fabsf((float)di + (ox - 0.5f)), ay = fabsf((float)dj + (oy - 0.5f));
    if (!(ax <= r && ay <= r)) return 0.0f;
    return filter_f<kType>(fc, r, ax) * filter_f<kType>(fc, r, ay);
}

// The read-out of a sample-keeping film under a weighted filter: the loops of k_film_filter_box over job.R = Rf rings, job.radius = r.
// One lane per output pixel; consecutive lanes read consecutive floats of every plane.  The colour and wsum chains are sequential by
// specification; per batch of kBatch samples the 3 kBatch loads are requested together and the kBatch weights (offset derivation,
// support test, two filter evaluations) are made before the first sample enters the chain, so the chain itself is one multiply
// and one add per channel.  A sample of weight 0 (outside the support included) enters neither sum.
// Every sample's offset is derived again per tap with the RNG, as the box does: a per-read table of offsets (stored pixels x
// samples x 8 B, filled by a kernel of its own) was measured and lost by 1.6 - 1.7 x, and kBatch 4 is level with 8 and ahead of 1
// for the filters that do arithmetic ("Reconstruction filters").
template <uint32_t kType, uint32_t kBatch>
__global__ void __launch_bounds__(256) k_film_filter_weighted(RenderCtx rc, KeptJob job, FilterCoef fc) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= job.out_rows * rc.width) return;
    const uint32_t row = idx / rc.width, x = idx - row * rc.width;
    const int32_t y = (int32_t)(job.out_j0 + row);
    const size_t n_band = (size_t)job.band_rows * rc.width;
    const float rad = job.radius;
    f3 sum = mk3(0, 0, 0);
    float wsum = 0.0f;
    for (int32_t dj = -job.R; dj <= job.R; ++dj) {
        const int32_t jj = y + dj;
        if (jj < 0 || jj >= (int32_t)rc.height) continue;
        for (int32_t di = -job.R; di <= job.R; ++di) {
            const int32_t ii = (int32_t)x + di;
            if (ii < 0 || ii >= (int32_t)rc.width) continue;
            const uint32_t pixel = (uint32_t)jj * rc.width + (uint32_t)ii;
            const size_t lp = (size_t)((uint32_t)jj - job.band_base) * rc.width + (uint32_t)ii;
            for (uint32_t c = 0; c < job.n_chunks; ++c) {
                const KeptChunk ch = job.chunks[c];
                const size_t plane = (size_t)ch.count * n_band;
                const float* rp = ch.rad + lp;
                uint32_t s = 0;
                for (; s + kBatch <= ch.count; s += kBatch) {
                    float r[kBatch], g[kBatch], b[kBatch], w[kBatch];
#pragma unroll
                    for (uint32_t k = 0; k < kBatch; ++k) {
                        const size_t ri = (size_t)(s + k) * n_band;
                        r[k] = rp[ri]; g[k] = rp[plane + ri]; b[k] = rp[2 * plane + ri];
                    }
#pragma unroll
                    for (uint32_t k = 0; k < kBatch; ++k) w[k] = filter_weight<kType>(rc, fc, pixel, ch.first + s + k, di, dj, rad);
#pragma unroll
                    for (uint32_t k = 0; k < kBatch; ++k)
                        if (w[k] != 0.0f) {
                            sum.x = sum.x + w[k] * r[k]; sum.y = sum.y + w[k] * g[k]; sum.z = sum.z + w[k] * b[k];
                            wsum = wsum + w[k];
                        }
                }
                for (; s < ch.count; ++s) {
                    const size_t ri = (size_t)s * n_band;
                    const float w = filter_weight<kType>(rc, fc, pixel, ch.first + s, di, dj, rad);
                    if (w != 0.0f) {
                        sum.x = sum.x + w * rp[ri]; sum.y = sum.y + w * rp[plane + ri]; sum.z = sum.z + w * rp[2 * plane + ri];
                        wsum = wsum + w;
                    }
                }
            }
        }
    }
    f3 c = sum;
    if (job.mean) c = sum * (1.0f / wsum);
    job.out[3 * (size_t)idx] = c.x; job.out[3 * (size_t)idx + 1] = c.y; job.out[3 * (size_t)idx + 2] = c.z;
}

// spt_film_read_samples: the own rows of `count` kept samples from plan index `first`, [k][own row][x][3].  One lane per float of
// one sample plane; blockIdx.y walks the samples.  The chunk holding sample first + k is found by a walk over the (short) table.
__global__ void __launch_bounds__(256) k_film_read_kept(KeptJob job, uint32_t width, uint32_t first, size_t out_plane) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)job.out_rows * width * 3u) return;
    const uint32_t s = first + blockIdx.y;
    const size_t px = i / 3u, c = i - 3u * px;
    const size_t n_band = (size_t)job.band_rows * width;
    const size_t lp = (size_t)(job.out_j0 - job.band_base) * width + px;
    float v = 0.0f;
    for (uint32_t k = 0; k < job.n_chunks; ++k) {
        const KeptChunk ch = job.chunks[k];
        if (s >= ch.first && s - ch.first < ch.count) { v = ch.rad[(size_t)c * ch.count * n_band + (size_t)(s - ch.first) * n_band + lp]; break; }
    }
    job.out[(size_t)blockIdx.y * out_plane + i] = v;
}

// ---------------------------------------------------------------------------- RGB8 output
// color_to_rgb (film.rs:94-99) of one channel, the arithmetic of spt_host_film_to_rgb8, one rounded operation at a time: Rust's
// clamp keeps a NaN and `NaN as u8` is 0; +inf gives 255, -inf and -0 give 0; the conversion truncates.
SPT_DEV uint32_t rgb8_byte(float x) {
    const float c = x * 255.0f;
    const float cl = c < 0.0f ? 0.0f : (c > 255.0f ? 255.0f : c);
    return (cl != cl) ? 0u : (uint32_t)cl;
}

// The 8-bit image of a packed float buffer (spt_film_read_rgb8): a pass of its own behind the
// read-out kernels, whose code stays what it was.  One lane takes four consecutive floats: one 16-byte load, four conversions,
// one dword store (both buffers come from the allocator, so 16 * i and 4 * i are aligned).  The last lane of a buffer whose
// length is no multiple of 4 takes its one to three elements singly.
__global__ void __launch_bounds__(256) k_pack_rgb8(uint32_t n_floats, const float* in, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (n_floats + 3u) / 4u) return;   // (n_floats <= 2^32 - 4: the grid's lane count fits 32 bits)
    const uint32_t base = 4u * i;
    if (n_floats - base >= 4u) {
        const float4 v = *reinterpret_cast<const float4*>(in + base);
        *reinterpret_cast<uint32_t*>(out + base) = rgb8_byte(v.x) | (rgb8_byte(v.y) << 8) | (rgb8_byte(v.z) << 16) | (rgb8_byte(v.w) << 24);
    } else {
        for (uint32_t k = base; k < n_floats; ++k) out[k] = (uint8_t)rgb8_byte(in[k]);
    }
}

// ---------------------------------------------------------------------------- test seams
template <bool kLds>
__global__ void __launch_bounds__(256) k_trace_closest(DScene sc, uint32_t n, const spt_ray* rays, spt_hit* hits) {
    stage_geometry<kLds>(sc);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const spt_ray in = rays[active ? i : 0u];
    DRay r;
    r.o = mk3(in.o); r.d = mk3(in.d); r.t_min = in.t_min;
    DHit h;
    if (kLds && sc.flat) h = flat_closest(sc, r, in.t_max, active);   // (whole waves, see flat.h)
    if (!active) return;
    if (!(kLds && sc.flat)) h = trace_closest<kLds>(sc, r, in.t_max);
    const bool hit = h.inst >= 0;
    hits[i].t = hit ? h.t : SPT_F32_MAX;
    hits[i].instance = h.inst;
    hits[i].prim = hit ? h.prim : -1;
    hits[i].v = hit ? h.v : 0.0f;
    hits[i].w = hit ? h.w : 0.0f;
}
template <bool kLds>
__global__ void __launch_bounds__(256) k_trace_any(DScene sc, uint32_t n, const spt_ray* rays, uint8_t* occluded) {
    stage_geometry<kLds>(sc);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const spt_ray in = rays[active ? i : 0u];
    DRay r;
    r.o = mk3(in.o); r.d = mk3(in.d); r.t_min = in.t_min;
    bool occ = false;
    if (kLds && sc.flat) occ = flat_any(sc, r, in.t_max, active);
    if (!active) return;
    if (!(kLds && sc.flat)) occ = trace_any<kLds>(sc, r, in.t_max);
    occluded[i] = occ ? 1 : 0;
}

// the same seams through the streaming walker (scenes that do not fit LDS): one ray per lane, no refill
__global__ void __launch_bounds__(256) k_trace_closest_stream(DScene sc, uint32_t n, const spt_ray* rays, spt_hit* hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint2 spill_mem[kSpillStack];
    SWalker<true, false> wk;
    wk.done = true;
    wk.cur = kNoRef;
    if (i < n) {
        DRay r;
        r.o = mk3(rays[i].o); r.d = mk3(rays[i].d); r.t_min = rays[i].t_min;
        wk.begin(sc, r, rays[i].t_max);
    }
    for (uint32_t guard = 0; guard < (1u << 20) && __ballot(!wk.done) != 0ull; ++guard) wk.run(sc, 8u, spill_mem);
    if (i >= n) return;
    const bool hit = wk.h.inst >= 0;
    hits[i].t = hit ? wk.h.t : SPT_F32_MAX;
    hits[i].instance = wk.h.inst;
    hits[i].prim = hit ? wk.h.prim : -1;
    hits[i].v = hit ? wk.h.v : 0.0f;
    hits[i].w = hit ? wk.h.w : 0.0f;
}
__global__ void __launch_bounds__(256) k_trace_any_stream(DScene sc, uint32_t n, const spt_ray* rays, uint8_t* occluded) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint2 spill_mem[kSpillStack];
    SWalker<false, false> wk;
    wk.done = true;
    wk.cur = kNoRef;
    if (i < n) {
        DRay r;
        r.o = mk3(rays[i].o); r.d = mk3(rays[i].d); r.t_min = rays[i].t_min;
        wk.begin(sc, r, rays[i].t_max);
    }
    for (uint32_t guard = 0; guard < (1u << 20) && __ballot(!wk.done) != 0ull; ++guard) wk.run(sc, 8u, spill_mem);
    if (i < n) occluded[i] = wk.h.inst >= 0 ? 1 : 0;
}

__global__ void k_detmath(uint32_t fn, uint32_t n, const float* a, const float* b, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b[i], r;
    switch (fn) {
    case 0: r = spt_sin(x); break;
    case 1: r = spt_cos(x); break;
    case 2: r = spt_log(x); break;
    case 3: r = spt_exp(x); break;
    case 4: r = spt_acos(x); break;
    case 5: r = spt_atan2(x, y); break;
    case 6: r = spt_asin(x); break;
    case 7: r = spt_round(x); break;
    case 8: r = spt_floor(x); break;
    case 9: r = spt_sqrt(x); break;
    case 10: r = x / y; break;
    case 11: r = spt_max(x, y); break;
    case 12: r = spt_min(x, y); break;
    case 13: r = spt_pow(x, y); break;
    case 14: r = spt_log2(x); break;
    case 15: r = spt_trunc(x); break;
    case 16: r = spt_fract(x); break;
    default: r = 0.0f; break;
    }
    out[i] = r;
}

// Test seam behind spt_debug_bxdf: BxdfT::{sample, bxdf, pdf} (src/bxdf/mod.rs:80-90) of one material record, one lane per input.
// op 0: sample(wo, rng stream) -> (wi, f, pdf, transmit); op 1: bxdf(wo, wi), pdf(wo, wi).  kScene: the record may be a
// position-normal-distribution lobe (SPT_BXDF_PNDF_*), whose tables are read from the scene.
template <bool kScene>
__global__ void k_debug_bxdf(DScene sc, DMat m, uint32_t op, uint32_t n, const float* wo_in, const float* wi_in, const uint64_t* rng_state,
                             float* wi_out, float* f_out, float* pdf_out, int32_t* dir_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 wo = mk3(wo_in[3 * i], wo_in[3 * i + 1], wo_in[3 * i + 2]);
    if (op == 0u) {
        DRng rng;
        rng.s.state = rng_state[i];
        DSubsurfaceIo io;
        io.has = false;
        const DBxdfSample s = mat_sample<false, false, false, kScene>(m, wo, rng, &sc, &io);
        wi_out[3 * i] = s.wi.x; wi_out[3 * i + 1] = s.wi.y; wi_out[3 * i + 2] = s.wi.z;
        f_out[3 * i] = s.f.x; f_out[3 * i + 1] = s.f.y; f_out[3 * i + 2] = s.f.z;
        pdf_out[i] = s.pdf;
        dir_out[i] = s.transmit ? 1 : 0;
    } else {
        const f3 wi = mk3(wi_in[3 * i], wi_in[3 * i + 1], wi_in[3 * i + 2]);
        const f3 f = mat_eval<kScene>(m, wo, wi, &sc);
        f_out[3 * i] = f.x; f_out[3 * i + 1] = f.y; f_out[3 * i + 2] = f.z;
        pdf_out[i] = mat_pdf<kScene>(m, wo, wi, &sc);
    }
}
