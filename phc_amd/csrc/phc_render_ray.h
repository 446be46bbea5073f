// Per-ray code shared by the two renderer kernels (phc_render.hip: capsules, markers, ground; phc_render_mesh.hip: the same plus triangle
// meshes): the small vector type, the LDS record of a capsule / marker and the shape-centred capsule solve.  See phc_render.hip for the
// precision argument of the shape-centred solve.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/phc_amd.h"

#define RD_VIEWS 16                                       // views per launch: their cameras ride in the kernel arguments
#define RD_TILE 16                                        // pixel tile of a workgroup (4 waves of 8 x 8)
#define RD_THREADS 256
#define RD_MAX_PRIMS (PHC_RENDER_MAX_SHAPES + PHC_RENDER_MAX_MARKERS)
#define RD_SHADOW_OFFSET 1.0e-3f                          // shadow-ray origin: hit point + 1 mm along the normal

struct RenderViews {
    phc_camera_t cam[RD_VIEWS];
};

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 unit(V3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }
__device__ __forceinline__ V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }

// v rotated by the xyzw quaternion q: v + 2 w (q x v) + 2 q x (q x v)
__device__ __forceinline__ V3 quat_rotate(V3 q, float w, V3 v) {
    const V3 t = 2.0f * cross(q, v);
    return v + w * t + cross(q, t);
}

// LDS record of one primitive: P0 = (centre, radius), P1 = (half axis, bounding radius; < 0 = not drawn), P2 = (colour, hit id bits).
// A marker is a capsule with a zero half axis.
struct Prims {
    float4 p0[RD_MAX_PRIMS], p1[RD_MAX_PRIMS], p2[RD_MAX_PRIMS];
};

// First entry s (along the unit ray, relative to tc) of the capsule {x : dist(x, [-h, h]) <= r} from the shape-centred origin p; INFINITY if
// the ray misses it or enters it at t = tc + s <= 0.  The capsule is the union of the lateral cylinder (|y| <= |h|^2) and the two end spheres:
// its first entry is the smallest first entry of the three pieces.
__device__ __forceinline__ float capsule_entry(V3 p, V3 d, V3 h, float r, float tc) {
    float best = INFINITY;
    const float rr = r * r;
    const float hh = dot(h, h);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (e == 1 && hh == 0.0f) break;
        const V3 q = e == 0 ? p - h : p + h;
        const float b = dot(q, d), c = dot(q, q) - rr;
        const float disc = b * b - c;
        if (disc >= 0.0f) {
            const float s = -b - sqrtf(disc);
            if (tc + s > 0.0f) best = fminf(best, s);
        }
    }
    if (hh > 0.0f) {
        const float hd = dot(h, d), hp = dot(h, p), pd = dot(p, d);
        const float A = hh - hd * hd;
        if (A > 1.0e-12f * hh) {
            const float B = hh * pd - hp * hd;
            const float C = hh * (dot(p, p) - rr) - hp * hp;
            const float disc = B * B - A * C;
            if (disc >= 0.0f) {
                const float s = (-B - sqrtf(disc)) / A;
                const float y = hp + s * hd;
                if (fabsf(y) <= hh && tc + s > 0.0f) best = fminf(best, s);
            }
        }
    }
    return best;
}
