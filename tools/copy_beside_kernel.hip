// What does a device-to-host copy of one film cost the kernel that runs beside it, by the route the copy takes?
//
// One victim kernel on stream A; once its first workgroup has raised a flag in host-visible memory, one copy of 12 582 912 bytes
// (a 1024 x 1024 RGB f32 film) from device memory to pinned host memory:
//   M0  hipMemcpyAsync on stream B (the runtime's choice: a blit kernel or an SDMA engine)
//   M0k the same behind a one-workgroup kernel on stream B, as the library's copy follows its finish kernel (beyond the
//       issue's list: on an idle stream the runtime sent M0 to an SDMA engine, behind a kernel it may not)
//   M1  a copy kernel of this file on stream B: 16-byte loads from the device buffer, 16-byte stores straight into the pinned
//       buffer; grid-stride over G workgroups; plain stores or __builtin_nontemporal_store
//   M2  hsa_amd_memory_async_copy_on_engine on a free SDMA engine (entry points by dlsym, no link-time dependency on HSA)
// against both kinds of pinned memory: hipHostMalloc and malloc + hipHostRegister (device-side address by hipHostGetDevicePointer).
// Victims: V1, a VALU loop that streams ~1 GB of 16-byte records to HBM (k_primary's shape); V2, the same loop without memory
// traffic; none (the copy alone).  One JSON line per cell: medians and min - max over 20 runs after 3 warm-ups, ms, HIP events
// (M2's copy time: host clock from the call to the completion signal, it is on no HIP stream).
//
// build: hipcc -O3 --offload-arch=gfx950 -o copy_beside_kernel tools/copy_beside_kernel.hip -ldl
// usage: copy_beside_kernel [loop_count=0 (calibrate V1 and V2 to ~0.6 ms alone)] [reps=20] [warmups=3]
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr size_t kCopyBytes = 12582912;               // 1024 * 1024 * 3 * 4
constexpr uint32_t kBlock = 256, kVictimGrid = 32768; // ~k_primary's dispatch
constexpr uint32_t kRecords = 8;                      // per thread: 32768 * 256 * 8 * 16 B = 1 GiB
constexpr double kTargetMs = 0.6;

// `iters` dependent FMAs per record, kRecords records per thread; kStore: each record goes to HBM, coalesced over the grid
template <bool kStore>
__global__ void __launch_bounds__(256) k_victim(v4f* rec, uint32_t iters, float seed, uint32_t* started) {
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(started, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, n = (size_t)gridDim.x * kBlock;
    float a = seed + (float)threadIdx.x, b = seed * 0.5f;
    for (uint32_t r = 0; r < kRecords; ++r) {
        for (uint32_t i = 0; i < iters; ++i) { a = __builtin_fmaf(a, 0.999f, b); b = __builtin_fmaf(b, 1.001f, -a); }
        const v4f v = {a, b, a + b, (float)r};
        if (kStore) rec[r * n + tid] = v;
        else if (a == 1.2345e30f && b == -a) rec[tid] = v;   // (never: keeps the loop alive)
    }
}

__global__ void __launch_bounds__(256) k_touch(v4f* rec) {   // what M0k puts ahead of its copy
    if (threadIdx.x == 0) rec[0] = v4f{1.0f, 2.0f, 3.0f, 4.0f};
}

template <bool kNonTemporal>
__global__ void __launch_bounds__(256) k_copy(const v4f* __restrict__ src, v4f* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const v4f v = src[i];
        if (kNonTemporal) __builtin_nontemporal_store(v, &dst[i]);
        else dst[i] = v;
    }
}

// ---------------------------------------------------------------------------- HSA, by dlsym from the library HIP has loaded
struct Hsa {
    decltype(&hsa_iterate_agents) iterate_agents = nullptr;
    decltype(&hsa_agent_get_info) agent_get_info = nullptr;
    decltype(&hsa_signal_create) signal_create = nullptr;
    decltype(&hsa_signal_store_relaxed) signal_store = nullptr;
    decltype(&hsa_signal_wait_scacquire) signal_wait = nullptr;
    decltype(&hsa_signal_destroy) signal_destroy = nullptr;
    decltype(&hsa_amd_memory_copy_engine_status) engine_status = nullptr;
    decltype(&hsa_amd_memory_async_copy_on_engine) copy_on_engine = nullptr;
    hsa_agent_t gpu{}, cpu{};
    hsa_signal_t done{};
    bool ok = false;
    std::string why;
};

struct AgentSearch { Hsa* h; uint32_t bdf; bool gpu_found, cpu_found; };

static hsa_status_t on_agent(hsa_agent_t agent, void* data) {
    AgentSearch* s = (AgentSearch*)data;
    hsa_device_type_t type;
    if (s->h->agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (type == HSA_DEVICE_TYPE_CPU && !s->cpu_found) { s->h->cpu = agent; s->cpu_found = true; }
    if (type == HSA_DEVICE_TYPE_GPU && !s->gpu_found) {
        uint32_t bdf = 0;
        if (s->h->agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS && (bdf & 0xffffu) == s->bdf) {
            s->h->gpu = agent;
            s->gpu_found = true;
        }
    }
    return HSA_STATUS_SUCCESS;
}

static void hsa_open(Hsa& h, int device) {
    void* lib = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) { h.why = "libhsa-runtime64.so.1 is not loaded"; return; }
#define SYM(field, name) h.field = (decltype(h.field))dlsym(lib, #name); if (!h.field) { h.why = "missing " #name; return; }
    SYM(iterate_agents, hsa_iterate_agents) SYM(agent_get_info, hsa_agent_get_info) SYM(signal_create, hsa_signal_create)
    SYM(signal_store, hsa_signal_store_relaxed) SYM(signal_wait, hsa_signal_wait_scacquire) SYM(signal_destroy, hsa_signal_destroy)
    SYM(engine_status, hsa_amd_memory_copy_engine_status) SYM(copy_on_engine, hsa_amd_memory_async_copy_on_engine)
#undef SYM
    char id[64] = {};
    CHECK(hipDeviceGetPCIBusId(id, sizeof id, device));
    unsigned dom = 0, bus = 0, dev = 0, fn = 0;
    if (std::sscanf(id, "%x:%x:%x.%x", &dom, &bus, &dev, &fn) != 4) { h.why = std::string("unparsed bus id ") + id; return; }
    AgentSearch s{&h, (bus << 8) | (dev << 3) | fn, false, false};
    h.iterate_agents(on_agent, &s);
    if (!s.gpu_found || !s.cpu_found) { h.why = std::string("no HSA agent with the bus id ") + id; return; }
    if (h.signal_create(1, 0, nullptr, &h.done) != HSA_STATUS_SUCCESS) { h.why = "hsa_signal_create failed"; return; }
    h.ok = true;
}

// ---------------------------------------------------------------------------- one cell
struct Stat { double med, lo, hi; };
static Stat stat_of(std::vector<double> v) {
    if (v.empty()) return {0, 0, 0};
    std::sort(v.begin(), v.end());
    return {v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]), v.front(), v.back()};
}

struct Copy { const char* mech; int g; bool nt; };   // mech: "none", "M0", "M0k", "M1", "M2"

struct Probe {
    hipStream_t sa, sb;
    hipEvent_t a0, a1, b0, b1;
    v4f* rec;                 // 1 GiB, the victims' records
    v4f* src;                 // the film on the device
    v4f* touch;               // 16 bytes for k_touch
    volatile uint32_t* flag;  // host-visible, raised by the victim's first workgroup
    uint32_t* flag_dev;
    Hsa hsa;
    uint32_t engine_used = 0;
    int reps, warm;
};

// victim: 0 none, 1 V1, 2 V2.  Returns false when the cell could not run (M2 without HSA or without a free engine).
static bool run_cell(Probe& p, int victim, uint32_t iters, const Copy& c, void* dst_host, void* dst_dev, std::vector<double>& vt, std::vector<double>& ct) {
    const size_t n16 = kCopyBytes / 16;
    for (int it = 0; it < p.warm + p.reps; ++it) {
        *p.flag = 0u;
        double copy_ms = 0.0;
        if (victim) {
            CHECK(hipEventRecord(p.a0, p.sa));
            if (victim == 1) hipLaunchKernelGGL(k_victim<true>, dim3(kVictimGrid), dim3(kBlock), 0, p.sa, p.rec, iters, 1.0f + it, p.flag_dev);
            else hipLaunchKernelGGL(k_victim<false>, dim3(kVictimGrid), dim3(kBlock), 0, p.sa, p.rec, iters, 1.0f + it, p.flag_dev);
            CHECK(hipEventRecord(p.a1, p.sa));
            const auto t0 = std::chrono::steady_clock::now();
            while (*p.flag == 0u)
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) { std::fprintf(stderr, "the victim never raised its flag\n"); std::exit(3); }
        }
        if (!std::strcmp(c.mech, "M0") || !std::strcmp(c.mech, "M0k")) {
            if (c.mech[2] == 'k') hipLaunchKernelGGL(k_touch, dim3(1), dim3(kBlock), 0, p.sb, p.touch);
            CHECK(hipEventRecord(p.b0, p.sb));
            CHECK(hipMemcpyAsync(dst_host, p.src, kCopyBytes, hipMemcpyDeviceToHost, p.sb));
            CHECK(hipEventRecord(p.b1, p.sb));
        } else if (!std::strcmp(c.mech, "M1")) {
            CHECK(hipEventRecord(p.b0, p.sb));
            if (c.nt) hipLaunchKernelGGL(k_copy<true>, dim3(c.g), dim3(kBlock), 0, p.sb, p.src, (v4f*)dst_dev, n16);
            else hipLaunchKernelGGL(k_copy<false>, dim3(c.g), dim3(kBlock), 0, p.sb, p.src, (v4f*)dst_dev, n16);
            CHECK(hipEventRecord(p.b1, p.sb));
        } else if (!std::strcmp(c.mech, "M2")) {
            if (!p.hsa.ok) return false;
            uint32_t mask = 0;
            if (p.hsa.engine_status(p.hsa.cpu, p.hsa.gpu, &mask) != HSA_STATUS_SUCCESS || mask == 0u) { p.hsa.why = "no free SDMA engine"; return false; }
            const uint32_t engine = mask & (0u - mask);
            p.engine_used = engine;
            p.hsa.signal_store(p.hsa.done, 1);
            const auto t0 = std::chrono::steady_clock::now();
            const hsa_status_t st = p.hsa.copy_on_engine(dst_dev, p.hsa.cpu, p.src, p.hsa.gpu, kCopyBytes, 0, nullptr, p.hsa.done, (hsa_amd_sdma_engine_id_t)engine, false);
            if (st != HSA_STATUS_SUCCESS) { p.hsa.why = "hsa_amd_memory_async_copy_on_engine failed, status " + std::to_string((int)st); CHECK(hipDeviceSynchronize()); return false; }
            if (p.hsa.signal_wait(p.hsa.done, HSA_SIGNAL_CONDITION_LT, 1, 2000000000ull, HSA_WAIT_STATE_BLOCKED) >= 1) { std::fprintf(stderr, "the SDMA copy did not complete\n"); std::exit(3); }
            copy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        CHECK(hipStreamSynchronize(p.sa));
        CHECK(hipStreamSynchronize(p.sb));
        CHECK(hipGetLastError());
        float ms = 0.0f;
        if (victim) CHECK(hipEventElapsedTime(&ms, p.a0, p.a1));
        if (c.mech[0] == 'M' && c.mech[1] != '2') { float k = 0.0f; CHECK(hipEventElapsedTime(&k, p.b0, p.b1)); copy_ms = k; }
        if (it >= p.warm) { vt.push_back(ms); ct.push_back(copy_ms); }
    }
    return true;
}

int main(int argc, char** argv) {
    uint32_t loop_count = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 0u;
    Probe p;
    p.reps = argc > 2 ? std::atoi(argv[2]) : 20;
    p.warm = argc > 3 ? std::atoi(argv[3]) : 3;
    CHECK(hipSetDevice(0));
    CHECK(hipStreamCreateWithFlags(&p.sa, hipStreamNonBlocking));
    CHECK(hipStreamCreateWithFlags(&p.sb, hipStreamNonBlocking));
    for (hipEvent_t* e : {&p.a0, &p.a1, &p.b0, &p.b1}) CHECK(hipEventCreate(e));
    CHECK(hipMalloc(&p.rec, (size_t)kVictimGrid * kBlock * kRecords * sizeof(v4f)));
    CHECK(hipMalloc(&p.src, kCopyBytes));
    CHECK(hipMalloc(&p.touch, sizeof(v4f)));
    std::vector<float> film(kCopyBytes / 4);
    for (size_t i = 0; i < film.size(); ++i) film[i] = (float)(i % 9973u);
    CHECK(hipMemcpy(p.src, film.data(), kCopyBytes, hipMemcpyHostToDevice));
    uint32_t* flag_host = nullptr;
    CHECK(hipHostMalloc(&flag_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    p.flag = flag_host;
    CHECK(hipHostGetDevicePointer((void**)&p.flag_dev, flag_host, 0));
    hsa_open(p.hsa, 0);

    // the two kinds of pinned memory
    void* host[2] = {nullptr, nullptr};
    void* dev[2] = {nullptr, nullptr};
    CHECK(hipHostMalloc(&host[0], kCopyBytes, hipHostMallocDefault));
    void* raw = nullptr;
    if (posix_memalign(&raw, 4096, kCopyBytes)) return 2;
    host[1] = raw;
    std::memset(host[1], 0, kCopyBytes);
    CHECK(hipHostRegister(host[1], kCopyBytes, hipHostRegisterPortable));
    for (int k = 0; k < 2; ++k) CHECK(hipHostGetDevicePointer(&dev[k], host[k], 0));
    const char* kind_name[2] = {"hipHostMalloc", "hipHostRegister"};

    // loop counts: given, or scaled until each victim takes ~0.6 ms alone
    uint32_t iters[3] = {0u, loop_count, loop_count};
    const Copy none{"none", 0, false};
    for (int v = 1; v <= 2 && loop_count == 0u; ++v) {
        iters[v] = 64u;
        for (int round = 0; round < 4; ++round) {
            std::vector<double> vt, ct;
            const int reps = p.reps, warm = p.warm;
            p.reps = 5; p.warm = 1;
            run_cell(p, v, iters[v], none, nullptr, nullptr, vt, ct);
            p.reps = reps; p.warm = warm;
            const double med = stat_of(vt).med;
            // (V1 has a floor: its stores; the loop count only matters above it)
            const double scaled = (double)iters[v] * kTargetMs / std::max(med, 1e-3);
            const uint32_t next = (uint32_t)std::min(std::max(scaled, 1.0), 100000.0);
            if (next == iters[v] || (med > 0.97 * kTargetMs && med < 1.03 * kTargetMs)) break;
            iters[v] = next;
        }
    }

    std::vector<Copy> copies = {none, {"M0", 0, false}, {"M0k", 0, false}};
    for (int nt = 0; nt < 2; ++nt)
        for (int g : {4, 8, 16, 32, 256, 4096}) copies.push_back({"M1", g, nt != 0});
    copies.push_back({"M2", 0, false});
    const char* victim_name[3] = {"none", "V1", "V2"};
    int bad = 0;
    for (int kind = 0; kind < 2; ++kind)
        for (int v = 0; v <= 2; ++v)
            for (const Copy& c : copies) {
                if (v == 0 && !std::strcmp(c.mech, "none")) continue;
                // (the victim alone does not depend on the destination: its second cell shows how far "alone" drifts within a call)
                std::memset(host[kind], 0xff, kCopyBytes);
                std::vector<double> vt, ct;
                const bool ran = run_cell(p, v, iters[v], c, host[kind], dev[kind], vt, ct);
                if (!ran) {
                    std::printf("{\"victim\": \"%s\", \"copy\": \"%s\", \"pinned\": \"%s\", \"skipped\": \"%s\"}\n", victim_name[v], c.mech, kind_name[kind], p.hsa.why.c_str());
                    continue;
                }
                const bool same = std::strcmp(c.mech, "none") == 0 || std::memcmp(host[kind], film.data(), kCopyBytes) == 0;
                if (!same) ++bad;
                const Stat sv = stat_of(vt), sc = stat_of(ct);
                std::printf("{\"victim\": \"%s\", \"loop_count\": %u, \"copy\": \"%s\", \"G\": %d, \"nontemporal\": %s, \"pinned\": \"%s\", "
                            "\"victim_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"copy_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
                            "\"sdma_engine_mask\": %u, \"bytes_right\": %s}\n",
                            victim_name[v], iters[v], c.mech, c.g, c.nt ? "true" : "false", kind_name[kind], sv.med, sv.lo, sv.hi, sc.med, sc.lo, sc.hi,
                            !std::strcmp(c.mech, "M2") ? p.engine_used : 0u, same ? "true" : "false");
                std::fflush(stdout);
            }
    if (p.hsa.ok) p.hsa.signal_destroy(p.hsa.done);
    CHECK(hipHostUnregister(host[1]));
    std::free(raw);
    return bad ? 1 : 0;
}
