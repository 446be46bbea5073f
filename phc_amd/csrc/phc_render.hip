// Offscreen renderer of the articulated humanoids (include/phc_amd.h `phc_render`): one ray per pixel against the env's collision capsules,
// the marker spheres and the checkered ground, Lambert + ambient shading under one directional light and one shadow ray per lit pixel.
// Replaces the reference player's camera sensor (phc/env/tasks/base_task.py:176-195,405-437); it is not on the training path.
//
// Work split: one workgroup = (view, 16 x 16 pixel tile); its four waves take one 8 x 8 block each, so the 64 rays of a wave are neighbours and
// mostly take the same branches.  The workgroup first poses its env's capsules and markers in world space into LDS (one transform per shape,
// not per pixel); every lane then walks that list in the same order (LDS broadcast reads) with a bounding-sphere reject in front of the exact test.
//
// Precision: every intersection is solved in coordinates centred on the shape.  The ray origin is first advanced to tc = (c - o) . d, the
// projection of the shape's centre c, and the quadratic is formed from p = o + tc d - c (|p| <= the shape's bounding radius after the reject):
// the coefficients are products of numbers of the shape's own size, so the root carries errors of a few ulps of the shape's size plus the
// rounding of tc, instead of the cancellation of a camera-origin quadratic (|o - c|^2 - r^2 at metres for a centimetre-scale silhouette).
#include "phc_render_ray.h"   // V3, Prims, capsule_entry: shared with phc_render_mesh.hip

__global__ void __launch_bounds__(RD_THREADS) k_render(phc_render_scene_t sc, RenderViews views, int32_t v0, int32_t W, int32_t H,
                                                        int32_t tiles_x, uint8_t* __restrict__ rgba, float* __restrict__ depth,
                                                        int32_t* __restrict__ hit_id) {
    __shared__ Prims P;
    const int vl = blockIdx.y;
    const phc_camera_t& cam = views.cam[vl];
    const int env = cam.env;
    const int S = sc.num_capsules, M = sc.num_markers, NP = S + M;

    // ---- pose the env's shapes in world space, one thread per shape ----
    int block = 0;
    if (sc.env_shape != nullptr && sc.num_shape_blocks > 1) {
        block = sc.env_shape[env];
        if (block < 0 || block >= sc.num_shape_blocks) block = 0;
    }
    const float* caps = sc.capsules + (int64_t)block * sc.capsule_stride;
    for (int i = threadIdx.x; i < NP; i += RD_THREADS) {
        V3 c = v3(0.f, 0.f, 0.f), h = v3(0.f, 0.f, 0.f), col = v3(0.f, 0.f, 0.f);
        float r = 0.0f, R = -1.0f;
        int id;
        if (i < S) {
            const float* cp = caps + 8 * i;
            const int owner = (int)cp[7];
            r = cp[6];
            id = i;
            if (r > 0.0f && owner >= 0 && owner < sc.num_bodies) {
                const float* bs = sc.body_state + ((int64_t)env * sc.num_bodies + owner) * 13;
                const V3 q = ld3(bs + 3);
                const float w = bs[6];
                const V3 a = ld3(cp), b = ld3(cp + 3);
                c = ld3(bs) + quat_rotate(q, w, 0.5f * (a + b));
                h = quat_rotate(q, w, 0.5f * (b - a));
                R = sqrtf(dot(h, h)) + r;
                const float* pc = sc.palette[owner % PHC_RENDER_PALETTE];
                col = ld3(pc);
            }
        } else {
            const int m = i - S;
            c = ld3(sc.markers + ((int64_t)env * M + m) * 3);
            r = sc.marker_radii ? sc.marker_radii[m] : sc.marker_radius;             // (per-marker radius / colour: nullable, see include/phc_amd.h)
            R = r > 0.0f ? r : -1.0f;
            col = sc.marker_colors ? ld3(sc.marker_colors + 3 * m) : ld3(sc.marker_color);
            id = PHC_RENDER_MARKER_ID + m;
        }
        P.p0[i] = make_float4(c.x, c.y, c.z, r);
        P.p1[i] = make_float4(h.x, h.y, h.z, R * 1.0001f);   // (a margin on the reject only: the exact test decides)
        P.p2[i] = make_float4(col.x, col.y, col.z, __int_as_float(id));
    }
    __syncthreads();

    // ---- this lane's pixel: wave w takes the 8 x 8 block (w & 1, w >> 1) of the tile ----
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int px = tx * RD_TILE + (wave & 1) * 8 + (lane & 7);
    const int py = ty * RD_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (px >= W || py >= H) return;   // (no barrier below)

    const V3 eye = ld3(cam.eye);
    const V3 f = unit(ld3(cam.target) - eye);
    const V3 rt = unit(cross(f, ld3(cam.up)));
    const V3 up = cross(rt, f);
    const float th = tanf(0.5f * cam.fov_y);
    const float sx = (2.0f * ((float)px + 0.5f) / (float)W - 1.0f) * th * ((float)W / (float)H);
    const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)H) * th;
    const V3 d = unit(f + sx * rt + sy * up);

    // ---- primary ray ----
    float best_t = INFINITY, best_s = 0.0f;
    int best = -1;
    for (int i = 0; i < NP; ++i) {
        const float4 a = P.p0[i], b = P.p1[i];
        if (b.w < 0.0f) continue;
        const V3 c = v3(a.x, a.y, a.z);
        const float tc = dot(c - eye, d);
        if (tc + b.w < 0.0f) continue;                    // wholly behind the camera
        const V3 p = (eye - c) + tc * d;
        if (dot(p, p) > b.w * b.w) continue;              // bounding sphere
        const float s = capsule_entry(p, d, v3(b.x, b.y, b.z), a.w, tc);
        if (tc + s < best_t) {
            best_t = tc + s;
            best_s = s;
            best = i;
        }
    }
    int id = -1;
    V3 n = v3(0.f, 0.f, 1.f), col = ld3(sc.sky_color), hitp = v3(0.f, 0.f, 0.f);
    if (d.z < 0.0f && eye.z > 0.0f) {
        const float tg = -eye.z / d.z;
        if (tg < best_t) {
            best_t = tg;
            best = -1;
            id = -2;
            hitp = eye + tg * d;
            const long long cx = (long long)floorf(hitp.x), cy = (long long)floorf(hitp.y);
            col = ld3(sc.ground_color[(cx + cy) & 1]);
            hitp.z = 0.0f;
        }
    }
    if (best >= 0) {
        const float4 a = P.p0[best], b = P.p1[best], e = P.p2[best];
        const V3 c = v3(a.x, a.y, a.z), h = v3(b.x, b.y, b.z);
        const float tc = dot(c - eye, d);
        const V3 x = ((eye - c) + tc * d) + best_s * d;   // the hit, relative to the centre
        const float hh = dot(h, h);
        const float y = hh > 0.0f ? fminf(fmaxf(dot(x, h) / hh, -1.0f), 1.0f) : 0.0f;
        n = unit(x - y * h);
        hitp = c + x;
        col = v3(e.x, e.y, e.z);
        id = __float_as_int(e.w);
    }

    // ---- shading ----
    float shade = 1.0f;
    if (id != -1) {
        const V3 L = ld3(sc.light_dir);
        float lit = fmaxf(dot(n, L), 0.0f);
        if (lit > 0.0f) {
            const V3 o = hitp + RD_SHADOW_OFFSET * n;
            for (int i = 0; i < NP; ++i) {
                const float4 a = P.p0[i], b = P.p1[i];
                if (b.w < 0.0f) continue;
                const V3 c = v3(a.x, a.y, a.z);
                const float tc = dot(c - o, L);
                if (tc + b.w < 0.0f) continue;
                const V3 p = (o - c) + tc * L;
                if (dot(p, p) > b.w * b.w) continue;
                if (capsule_entry(p, L, v3(b.x, b.y, b.z), a.w, tc) < INFINITY) {
                    lit = 0.0f;
                    break;
                }
            }
        }
        shade = sc.ambient + sc.diffuse * lit;
    }
    const float rgb[3] = {col.x * shade, col.y * shade, col.z * shade};
    uint32_t word = 0xff000000u;
#pragma unroll
    for (int k = 0; k < 3; ++k) word |= (uint32_t)floorf(fminf(fmaxf(rgb[k], 0.0f), 1.0f) * 255.0f + 0.5f) << (8 * k);
    const int64_t pix = ((int64_t)(v0 + vl) * H + py) * W + px;
    reinterpret_cast<uint32_t*>(rgba)[pix] = word;
    if (depth) depth[pix] = id == -1 ? INFINITY : best_t;
    if (hit_id) hit_id[pix] = id;
}

extern "C" int32_t phc_render(const phc_render_scene_t* scene, const phc_camera_t* cameras, int32_t views, int32_t width, int32_t height,
                              uint8_t* rgba, float* depth, int32_t* hit_id, void* stream) {
    if (!scene || !cameras || !rgba || views <= 0 || width <= 0 || height <= 0) return PHC_EINVAL;
    if ((int64_t)width * height > PHC_RENDER_MAX_PIXELS) return PHC_EINVAL;
    const phc_render_scene_t& sc = *scene;
    if (!sc.body_state || !sc.capsules || sc.num_envs <= 0 || sc.num_bodies < 1 || sc.num_bodies > PHC_MAX_BODIES) return PHC_EINVAL;
    if (sc.num_capsules < 1 || sc.num_capsules > PHC_RENDER_MAX_SHAPES || sc.num_shape_blocks < 1 || sc.capsule_stride < 8 * (int64_t)sc.num_capsules)
        return PHC_EINVAL;
    if (sc.num_markers < 0 || sc.num_markers > PHC_RENDER_MAX_MARKERS || (sc.num_markers > 0 && !sc.markers)) return PHC_EINVAL;
    if (((uintptr_t)rgba | (uintptr_t)depth | (uintptr_t)hit_id) & 3) return PHC_EINVAL;   // one 32-bit store per pixel and output
    for (int32_t v = 0; v < views; ++v)
        if (cameras[v].env < 0 || cameras[v].env >= sc.num_envs) return PHC_EINVAL;
    const int32_t tiles_x = (width + RD_TILE - 1) / RD_TILE, tiles_y = (height + RD_TILE - 1) / RD_TILE;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t v0 = 0; v0 < views; v0 += RD_VIEWS) {
        RenderViews vw = {};
        const int32_t nv = views - v0 < RD_VIEWS ? views - v0 : RD_VIEWS;
        for (int32_t k = 0; k < nv; ++k) vw.cam[k] = cameras[v0 + k];
        hipLaunchKernelGGL(k_render, dim3((unsigned)(tiles_x * tiles_y), (unsigned)nv), dim3(RD_THREADS), 0, st, sc, vw, v0, width, height, tiles_x,
                           rgba, depth, hit_id);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
