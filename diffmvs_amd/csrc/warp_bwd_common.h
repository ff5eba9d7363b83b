// Shared by every feature-gradient kernel of the warps (warp_bwd.hip per pixel; warp_bwd_win.hip and warp_init_bwd_win.hip
// through warp_tile.h): the pixel's ray and the depth of a GetCost hypothesis.  No kernels here, so any translation unit may
// include it.  Everything is file-local to the including translation unit (anonymous namespace).
#pragma once
#include "dmvs_common.h"

namespace {

// reference pixel (x, y) seen from a source view: point(depth) = r * depth + t  (m = the view's 3x3 rotation | translation)
struct Ray {
    float rx, ry, rz, tx, ty, tz;
    __device__ __forceinline__ void init(const float* m, float x, float y) {
        rx = m[0] * x + m[1] * y + m[2];
        ry = m[3] * x + m[4] * y + m[5];
        rz = m[6] * x + m[7] * y + m[8];
        tx = m[9]; ty = m[10]; tz = m[11];
    }
};

// hypothesis k of a pixel whose inverse-depth hypotheses are lo + k * step (reference module.py:259-276)
__device__ __forceinline__ float hyp_depth(int k, float lo, float step, float dmin, float dmax) {
    float sk = (float)k * step;
    sk += lo;
    return dmvs_disp_to_depth(fminf(fmaxf(sk, 0.0f), 1.0f), dmin, dmax);
}

}  // namespace
