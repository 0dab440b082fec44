// Micro-benchmark: v_fma_f64 rate of the vector unit (the SSIM kernel of csrc/metrics.hip is a float64 FMA loop; AMD's
// specification gives 78.6 TFLOP/s of vector float64).  Every workgroup runs `iters` rounds of 16 independent dependent-chain
// FMAs per lane; WAVES waves per SIMD (1, 2, 4).  Prints lane-FMAs per clock per CU at the 2.4 GHz peak clock and TFLOP/s.
#include <hip/hip_runtime.h>
#include <cstdio>

template <int THREADS>
__global__ void __launch_bounds__(THREADS) k(double *out, int iters, double a, double b)
{
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = a * (threadIdx.x + i);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = __builtin_fma(acc[i], a, b);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc[i];
    out[(size_t)blockIdx.x * THREADS + threadIdx.x] = s;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <int THREADS>
int run(double *out, int blocks, int iters)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    k<THREADS><<<blocks, THREADS>>>(out, iters, 0.999999, 1e-9);
    CK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 5; ++r) {
        CK(hipEventRecord(e0));
        k<THREADS><<<blocks, THREADS>>>(out, iters, 0.999999, 1e-9);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best;
    }
    const double fmas = (double)blocks * THREADS * 16.0 * iters;
    printf("%d waves/SIMD: %.3f ms, %.2f TFLOP/s f64, %.1f lane-FMAs/clk/CU at 2.4 GHz\n", THREADS / 256, best,
           2.0 * fmas / (best * 1e-3) * 1e-12, fmas / (best * 1e-3) / 2.4e9 / blocks);
    return 0;
}

int main()
{
    const int blocks = 256, iters = 20000;              // one workgroup per CU
    double *out;
    CK(hipMalloc(&out, sizeof(double) * blocks * 1024));
    if (run<256>(out, blocks, iters) || run<512>(out, blocks, iters) || run<1024>(out, blocks, iters)) return 1;
    CK(hipFree(out));
    return 0;
}
