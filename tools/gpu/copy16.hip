// copy16.hip -- the yardstick of tools/bench_ingest.py: a plain device-to-device copy, 16 bytes per lane, grid-stride.
// Built by the tool:  hipcc -O3 --offload-arch=gfx950 -shared -fPIC -o tools/gpu/copy16.so tools/gpu/copy16.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void copy16_kernel(const uint4 *__restrict__ s, uint4 *__restrict__ d, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) d[i] = s[i];
}

// bytes: a multiple of 16; both pointers 16-byte aligned.  Returns the hipError_t of the launch.
extern "C" int copy16(const void *src, void *dst, size_t bytes, void *stream)
{
    const size_t n16 = bytes / 16;
    if (n16 == 0) return 0;
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint4 *)src, (uint4 *)dst, n16);
    return (int)hipGetLastError();
}
