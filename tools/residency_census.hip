// residency_census.hip -- how many 256-thread workgroups a CU of the MI355X really keeps resident, as a function of the
// kernel's SGPR count.  Developer tool (not part of the product):
//   hipcc --offload-arch=gfx950 -O2 -Rpass-analysis=kernel-resource-usage tools/residency_census.hip -o tools/residency_census
//   tools/residency_census [dynamic LDS bytes per workgroup, default 4096] [blocks per CU, default 16]
// The compiler's occupancy line and hipOccupancyMaxActiveBlocksPerMultiprocessor answer 8 for both kernels below; the
// hardware admits workgroups by SGPR granule (16 registers plus a fixed 16 per wave out of 800 per SIMD).  Two kernels that
// differ ONLY in the highest SGPR they name -- s87 (.sgpr_count 94, the render kernel's) and s71 (.sgpr_count 78) -- with the
// sphere render kernel's VGPR granule (v55 named: .vgpr_count 56) and its dynamic LDS.  The remarks of the compile line
// above show the counts the build really has; keep them next to the output (profiles/r15/census.txt does).
// Each workgroup, on entry: one lane adds 1 to the counter of its CU (keyed by XCC_ID and HW_ID's SE / SH / CU fields),
// records the largest value it saw, holds for a BOUNDED time (s_memtime ticks, with a hard cap on the iterations; it waits
// for nobody), then subtracts 1; the other waves sit at the barrier meanwhile, so the whole workgroup stays resident.
// Printed per kernel: over the CUs that ran a workgroup, the smallest / median / largest peak.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIP_OK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

constexpr unsigned N_SLOTS = 8 * 256;            // XCC_ID (3 bits used) x HW_ID[15:8] (CU 4 bits, SH 1, SE 3)
constexpr unsigned HOLD_TICKS = 20000;           // s_memtime runs at 100 MHz: 200 us
constexpr int HOLD_CAP = 4096;                   // iterations of an s_sleep of ~1 us: the hold ends after a few ms at the latest

#define CENSUS_KERNEL(NAME, TOP_SGPR)                                                                            \
    __global__ __launch_bounds__(256) void NAME(unsigned *now, unsigned *peak) {                                 \
        extern __shared__ unsigned dyn_lds[];                                                                    \
        asm volatile("" ::: TOP_SGPR, "v55");                                                                    \
        if (threadIdx.x == 0) {                                                                                  \
            unsigned hw, xcc;                                                                                    \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                     \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                   \
            const unsigned slot = ((xcc & 7u) << 8) | ((hw >> 8) & 0xffu);       /* < N_SLOTS */                 \
            dyn_lds[0] = slot;                                                                                   \
            const unsigned mine = atomicAdd(&now[slot], 1u) + 1u;                                                \
            atomicMax(&peak[slot], mine);                                                                        \
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();                                          \
            for (int i = 0; i < HOLD_CAP; ++i) {                                                                 \
                __builtin_amdgcn_s_sleep(32);                                                                    \
                if (__builtin_amdgcn_s_memtime() - t0 >= HOLD_TICKS) break;                                      \
            }                                                                                                    \
            atomicSub(&now[slot], 1u);                                                                           \
        }                                                                                                        \
        __syncthreads();                                                                                         \
    }

CENSUS_KERNEL(census_sgpr94, "s87")
CENSUS_KERNEL(census_sgpr78, "s71")

static int run(const char *name, void (*k)(unsigned *, unsigned *), unsigned grid, size_t lds, unsigned *d_now, unsigned *d_peak) {
    HIP_OK(hipMemset(d_now, 0, sizeof(unsigned) * N_SLOTS));
    HIP_OK(hipMemset(d_peak, 0, sizeof(unsigned) * N_SLOTS));
    int api = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, k, 256, lds));
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, 0, d_now, d_peak);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned> peak(N_SLOTS), now(N_SLOTS);
    HIP_OK(hipMemcpy(peak.data(), d_peak, sizeof(unsigned) * N_SLOTS, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(now.data(), d_now, sizeof(unsigned) * N_SLOTS, hipMemcpyDeviceToHost));
    std::vector<unsigned> seen;
    unsigned left = 0;
    for (unsigned i = 0; i < N_SLOTS; ++i) {
        if (peak[i]) seen.push_back(peak[i]);
        left += now[i];
    }
    if (seen.empty()) { fprintf(stderr, "%s: no workgroup ran\n", name); return 1; }
    std::sort(seen.begin(), seen.end());
    printf("%-14s grid %u, dynamic LDS %zu B, occupancy API %d per CU: %zu CUs seen, peak resident workgroups per CU min %u median %u max %u"
           " (counters back at %u)\n", name, grid, lds, api, seen.size(), seen.front(), seen[seen.size() / 2], seen.back(), left);
    return 0;
}

int main(int argc, char **argv) {
    const size_t lds = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    const unsigned per_cu = argc > 2 ? (unsigned)atoi(argv[2]) : 16;
    if (lds < 64 || lds > 48 * 1024 || per_cu == 0 || per_cu > 64) { fprintf(stderr, "LDS 64 ... 49152 bytes, 1 ... 64 blocks per CU\n"); return 2; }
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    const unsigned grid = (unsigned)prop.multiProcessorCount * per_cu;
    printf("%s, %d CUs; kernels name s87 / s71 and v55 (see the build's resource remarks for .sgpr_count / .vgpr_count)\n",
           prop.name, prop.multiProcessorCount);
    unsigned *d_now = nullptr, *d_peak = nullptr;
    HIP_OK(hipMalloc((void **)&d_now, sizeof(unsigned) * N_SLOTS));
    HIP_OK(hipMalloc((void **)&d_peak, sizeof(unsigned) * N_SLOTS));
    int rc = run("census_sgpr94", census_sgpr94, grid, lds, d_now, d_peak);
    if (rc == 0) rc = run("census_sgpr78", census_sgpr78, grid, lds, d_now, d_peak);
    if (rc == 0) rc = run("census_sgpr94", census_sgpr94, grid, lds, d_now, d_peak);      // (again: the order of the runs does not matter)
    (void)hipFree(d_now);
    (void)hipFree(d_peak);
    return rc;
}
