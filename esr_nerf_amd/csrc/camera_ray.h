// The single source of a camera ray: every kernel that makes a ray from (view, pixel) calls esr_camera_ray -- the dense, batch
// and bounds kernels of camera.hip and the camera instantiation of the training-ray filter (rayfilter.hip).
//
// Reference (paths under the reference tree): data/esrnerf/esrnerf.py:48-59,252-259 and data/dtu/dtu.py:74-86,207-211
// (pixelcoord and pose2ray), F.normalize of esrnerf.py:238 / dtu.py:194.
//   pixel p of a width x height image: i = p % width, j = p / width
//   px = ((i + 0.5) - cx) / fx,  py = ((j + 0.5) - cy) / fy,  pz = 1       binary32, true (correctly rounded) division
//   d[a] = (R[a][0] * px + R[a][1] * py) + R[a][2]                          R | t = the view's 3x4 camera-to-world matrix
//   o = t,  viewdir = d / max(|d|, 1e-12),  |d| = sqrt((dx dx + dy dy) + dz dz)
// Every operation is a separately rounded binary32 operation (contraction off), so a ray does not depend on which kernel
// asked for it.  i + 0.5 and j + 0.5 are exact for every image a 32-bit row index admits.
#pragma once
#include "esr_common.h"

// (ray origin, direction, unit direction) of pixel `pixel` (< width * height) under the pose `m` (12 floats, row-major 3x4)
__device__ __forceinline__ void esr_camera_ray(const esr_camera_t &cam, const float m[12], int pixel, float o[3], float d[3],
                                               float vd[3])
{
#pragma clang fp contract(off)
    const int j = pixel / cam.width, i = pixel - j * cam.width;
    const float px = __fdiv_rn(((float)i + 0.5f) - cam.cx, cam.fx);
    const float py = __fdiv_rn(((float)j + 0.5f) - cam.cy, cam.fy);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (m[4 * a] * px + m[4 * a + 1] * py) + m[4 * a + 2];
        o[a] = m[4 * a + 3];
    }
    const float nrm = fmaxf(esr_ray_norm(d), 1e-12f);
#pragma unroll
    for (int a = 0; a < 3; ++a) vd[a] = __fdiv_rn(d[a], nrm);
}

// the same from a pose table in memory (global or LDS)
__device__ __forceinline__ void esr_camera_ray_at(const esr_camera_t &cam, const float *__restrict__ poses, int view, int pixel,
                                                  float o[3], float d[3], float vd[3])
{
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * view + k];
    esr_camera_ray(cam, m, pixel, o, d, vd);
}
