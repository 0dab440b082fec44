// The Disney reflection of the light-transport stages (reference: app/utils/pbr/functions.py:108-173, disney_reflection), binary32:
// the one owner of the BRDF.  lts.hip differentiates it in the light-transport combine, surflight.hip evaluates it forward on the
// exported surface.
#pragma once
#include "esr_common.h"

namespace {

constexpr float kPi = 3.14159265358979323846f;

struct Disney {
    float R[3];
    float dR_da[3];      // d R[c] / d albedo[c]
    float dR_dro[3], dR_dm[3];
};

// (fd + fs) * (wi.n) * 2 pi with the clamps of the reference; gradients w.r.t. albedo, roughness, metallic
__device__ __forceinline__ Disney disney_eval(const float a[3], float ro, float m, const float n[3],
                                              const float wi[3], const float wo[3])
{
    const float EPS = 1e-7f;
    float hv[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float hn = fmaxf(sqrtf(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]), 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; ++k) hv[k] /= hn;
    const float noh = fmaxf(n[0] * hv[0] + n[1] * hv[1] + n[2] * hv[2], 0.f);
    const float ooh = fmaxf(wo[0] * hv[0] + wo[1] * hv[1] + wo[2] * hv[2], 0.f);
    const float ion = fmaxf(wi[0] * n[0] + wi[1] * n[1] + wi[2] * n[2], 0.f);
    const float oon = fmaxf(wo[0] * n[0] + wo[1] * n[1] + wo[2] * n[2], 0.f);
    const float r2raw = ro * ro;
    const float r2 = fmaxf(r2raw, EPS);
    const float D = 1.f / (r2 * kPi) * expf(2.f / r2 * (noh - 1.f));
    const float dD_dr2 = D * (-1.f / r2 - 2.f * (noh - 1.f) / (r2 * r2));
    const float dr2_dro = (r2raw >= EPS) ? 2.f * ro : 0.f;          // clamp(min) passes the gradient at equality
    const float om = 1.f - ooh;
    const float t5 = om * om * om * om * om;
    const float k = (1.f + ro) * (1.f + ro) / 8.f, dk_dro = (1.f + ro) / 4.f;
    const float den_i = ion * (1.f - k) + k, den_o = oon * (1.f - k) + k;
    const float Vi = 0.5f / fmaxf(den_i, EPS), Vo = 0.5f / fmaxf(den_o, EPS);
    const float dVi_dk = (den_i >= EPS) ? -0.5f / (den_i * den_i) * (1.f - ion) : 0.f;
    const float dVo_dk = (den_o >= EPS) ? -0.5f / (den_o * den_o) * (1.f - oon) : 0.f;
    const float V = Vi * Vo;
    const float dV_dro = (dVi_dk * Vo + Vi * dVo_dk) * dk_dro;
    const float lam = ion * kPi * 2.f;
    Disney o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float F0 = 0.04f * (1.f - m) + a[c] * m;
        const float Fr = F0 + (1.f - F0) * t5;
        const float fd = (1.f - m) * a[c] / kPi;
        o.R[c] = (fd + D * Fr * V) * lam;
        o.dR_da[c] = ((1.f - m) / kPi + D * V * m * (1.f - t5)) * lam;
        o.dR_dm[c] = (-a[c] / kPi + D * V * (a[c] - 0.04f) * (1.f - t5)) * lam;
        o.dR_dro[c] = Fr * (dD_dr2 * dr2_dro * V + D * dV_dro) * lam;
    }
    return o;
}

}  // namespace
