// The spherical-Gaussian environment of section V step 3 of include/esr_hip.h, for the kernels that evaluate it on the surface:
// the lobe table in LDS (unit lobes [J,3], mus [J,3], |lambda| [J], each at a stride of ESR_SURFACE_ENV_MAX_SG lobes) and its
// evaluation along a direction, binary32, every operation rounded on its own, in the order of lts_combine_kernel.
#pragma once
#include "esr_common.h"

namespace {

constexpr int SG_TABLE_FLOATS = 7 * ESR_SURFACE_ENV_MAX_SG;

// fill the table from the raw model parameters; every lane of the block calls it, the caller synchronises
__device__ __forceinline__ void sg_table_fill(float *sg, const float *mus, const float *lambdas, const float *lobes, int J, int threads)
{
#pragma clang fp contract(off)
    for (int j = threadIdx.x; j < J; j += threads) {
        const float lx = lobes[3 * j], ly = lobes[3 * j + 1], lz = lobes[3 * j + 2];
        const float nn = fmaxf(sqrtf((lx * lx + ly * ly) + lz * lz), 1e-12f);
        sg[3 * j] = lx / nn, sg[3 * j + 1] = ly / nn, sg[3 * j + 2] = lz / nn;
#pragma unroll
        for (int c = 0; c < 3; ++c) sg[3 * ESR_SURFACE_ENV_MAX_SG + 3 * j + c] = mus[3 * j + c];
        sg[6 * ESR_SURFACE_ENV_MAX_SG + j] = fabsf(lambdas[j]);
    }
}

// the environment along the unit direction w
__device__ __forceinline__ void sg_environment(const float *sg, int J, const float w[3], float L[3])
{
#pragma clang fp contract(off)
    float pre[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < J; ++j) {
        const float dtl = (w[0] * sg[3 * j] + w[1] * sg[3 * j + 1]) + w[2] * sg[3 * j + 2];
        const float e = expf(sg[6 * ESR_SURFACE_ENV_MAX_SG + j] * (dtl - 1.f));
        const float *mu = sg + 3 * ESR_SURFACE_ENV_MAX_SG + 3 * j;
        pre[0] = pre[0] + mu[0] * e, pre[1] = pre[1] + mu[1] * e, pre[2] = pre[2] + mu[2] * e;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = esr_softplus(pre[c]);
}

}  // namespace
