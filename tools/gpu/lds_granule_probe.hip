// How many single-wave workgroups of a given LDS size are resident per CU at once: the LDS allocation granule of the
// device, measured.  Every workgroup counts itself in, records the largest count it sees, waits about 40 us on the
// 100 MHz wall clock (bounded) and counts itself out; the grid is several times what can be resident, so the largest
// count is the chip's capacity for that LDS size.  Behind DESIGN.md section 6 (lk_kernel's 12 992 B per wave).
// build: hipcc -O2 --offload-arch=gfx950 lds_granule_probe.hip -o lds_granule_probe.bin ; usage: lds_granule_probe.bin [bytes ...]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(64) void probe(int *count, int *peak, uint32_t *sink)
{
    extern __shared__ uint32_t lds[];
    if (threadIdx.x == 0) {
        lds[0] = blockIdx.x;
        const int now = atomicAdd(count, 1) + 1;
        atomicMax(peak, now);
        const unsigned long long t0 = wall_clock64();
        for (int i = 0; i < 100000 && wall_clock64() - t0 < 4000ull; i++) __builtin_amdgcn_s_sleep(32);
        atomicSub(count, 1);
        if (lds[0] == 0xffffffffu) *sink = 1;
    }
}

int main(int argc, char **argv)
{
    int *d, h[2];
    uint32_t *sink;
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    CK(hipMalloc(&d, 2 * sizeof(int)));
    CK(hipMalloc(&sink, sizeof(uint32_t)));
    printf("%s: %d CUs\n", p.name, p.multiProcessorCount);
    for (int i = 1; i < argc; i++) {
        const int bytes = atoi(argv[i]);
        if (bytes < 4 || bytes > 65536) continue;
        CK(hipMemset(d, 0, 2 * sizeof(int)));
        hipLaunchKernelGGL(probe, dim3(p.multiProcessorCount * 64), dim3(64), bytes, 0, d, d + 1, sink);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
        printf("LDS %6d B per single-wave workgroup: at most %5d resident = %.2f per CU (left at the end: %d)\n", bytes, h[1],
               (double)h[1] / p.multiProcessorCount, h[0]);
    }
    return 0;
}
