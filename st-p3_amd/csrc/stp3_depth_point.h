// stp3_depth_point.h -- the LiDAR point side shared by stp3_depth.hip and stp3_depth_augment.hip: the devkit's
// map_pointcloud_to_image restated (the arithmetic is defined in the header of stp3_depth.hip, (a)) and the frame look-up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if !defined(__HIPCC__)
// host build of the kernels (tests/hipcpu): its stand-in runtime has atomicAdd only
inline int atomicMax(int* p, int v) { return __atomic_fetch_max(p, v, __ATOMIC_SEQ_CST); }
#endif

namespace {

struct Cloud {
    const float* points;                     // [n_total][3]
    const int* offsets;                      // [F + 1]
    const double* steps;                     // [F][N][4][12]: rotation (row-major), translation
    const double* intrinsics;                // [F][N][3][3]
    int before;                              // bit s: step s translates before it rotates
};

struct Xyz { float x, y, z; };

// LidarPointCloud.rotate / .translate of the four steps on one point (float32 storage after every call)
__device__ __forceinline__ Xyz transform_point(const float* __restrict__ pt, const double* __restrict__ st, int before) {
    float x = pt[0], y = pt[1], z = pt[2];
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const double* r = st + 12 * s;
        const bool first = (before >> s) & 1;
        if (first) {
            x = (float)((double)x + r[9]);
            y = (float)((double)y + r[10]);
            z = (float)((double)z + r[11]);
        }
        const double dx = x, dy = y, dz = z;
        x = (float)(r[0] * dx + r[1] * dy + r[2] * dz);
        y = (float)(r[3] * dx + r[4] * dy + r[5] * dz);
        z = (float)(r[6] * dx + r[7] * dy + r[8] * dz);
        if (!first) {
            x = (float)((double)x + r[9]);
            y = (float)((double)y + r[10]);
            z = (float)((double)z + r[11]);
        }
    }
    Xyz o;
    o.x = x; o.y = y; o.z = z;
    return o;
}

struct Hit {
    int px, py;                              // truncated (u, v); 0 when the point is not kept
    float depth;
    bool keep;
};

__device__ __forceinline__ Hit project_point(const float* __restrict__ pt, const double* __restrict__ st, int before,
                                             const double* __restrict__ k, int H, int W) {
    const Xyz c = transform_point(pt, st, before);
    const double x = c.x, y = c.y, z = c.z;
    const double p0 = k[0] * x + k[1] * y + k[2] * z;
    const double p1 = k[3] * x + k[4] * y + k[5] * z;
    const double p2 = k[6] * x + k[7] * y + k[8] * z;
    const double u = p0 / p2, v = p1 / p2;
    Hit h;
    h.depth = c.z;
    h.keep = c.z > 1.0f && u > 1.0 && u < (double)(W - 1) && v > 1.0 && v < (double)(H - 1);
    h.px = h.keep ? (int)u : 0;
    h.py = h.keep ? (int)v : 0;
    return h;
}

// the frame whose range holds point p, or -1
__device__ __forceinline__ int frame_of(const int* __restrict__ offsets, int F, int n_total, int p) {
    int lo = 0, hi = F;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= p) lo = mid; else hi = mid;
    }
    const int a = offsets[lo], b = offsets[lo + 1];
    return (a >= 0 && a <= p && p < b && b <= n_total) ? lo : -1;
}

}  // namespace
