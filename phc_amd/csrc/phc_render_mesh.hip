// Offscreen renderer with triangle meshes (include/phc_amd.h `phc_render_mesh`): phc_render's scene plus posed instances of triangle meshes
// (the robots' visual meshes), each behind a bounding-volume hierarchy.  Off the training path, opt-in (render.meshes).
//
// Work split: phc_render's.  One workgroup = (view, 16 x 16 pixel tile), one 8 x 8 block per wave.  The workgroup poses its env's capsules and
// markers into LDS as phc_render does and, next to them, its env's instances: the columns of the mesh-to-world rotation, the bounding
// sphere's centre in the world and in the mesh frame, the colour and the root node.  A ray rejects an instance by its bounding sphere before
// it touches the tree, and is taken into the mesh frame for the traversal; vertices are never moved.
//
// Traversal: the tree is stored depth-first with a skip link per node, so a lane walks it with node = hit ? node + 1 : skip: no stack, no LDS
// per lane, no scratch.  A node is two 16-byte loads.  The slab test takes a direction component of exactly 0 apart (the slab holds the whole
// ray or none of it: no 0 * inf) and compares near <= far with a few ulps of slack, so a box of zero thickness (near == far up to rounding)
// is entered.
//
// Precision: as for the capsules, the ray origin is first advanced to tc = (c - o) . d, the projection of the bounding sphere's centre c, and
// the mesh-frame origin is formed from p = o + tc d - c (|p| <= the sphere's radius): every number of the triangle solve is of the mesh's
// size, and t = tc + s inherits the rounding of tc once.
#include "phc_render_ray.h"

#define RM_SLAB_SLACK 1.0e-6f   // relative slack of the near <= far comparison (each side carries <= 3 roundings of 2^-24)

// LDS record of one instance: m0..m2 = (column j of the mesh-to-world rotation, world centre[j]), m3 = (mesh-frame centre, bounding radius with
// the reject margin; < 0 = not drawn), m4 = (colour, root node bits).
struct Insts {
    float4 m0[PHC_RENDER_MAX_INSTANCES], m1[PHC_RENDER_MAX_INSTANCES], m2[PHC_RENDER_MAX_INSTANCES], m3[PHC_RENDER_MAX_INSTANCES],
        m4[PHC_RENDER_MAX_INSTANCES];
};

struct MeshArrays {
    const float* __restrict__ vertices;
    const int32_t* __restrict__ triangles;
    const float4* __restrict__ nodes;
    int32_t num_vertices, num_triangles, num_nodes;
};

// The three corners of triangle k, or false when k or one of its vertex indices lies outside the arrays.
__device__ __forceinline__ bool load_triangle(const MeshArrays& ms, int k, V3& v0, V3& v1, V3& v2) {
    if ((unsigned)k >= (unsigned)ms.num_triangles) return false;
    const int32_t* t = ms.triangles + 3 * (int64_t)k;
    const unsigned i0 = (unsigned)t[0], i1 = (unsigned)t[1], i2 = (unsigned)t[2], nv = (unsigned)ms.num_vertices;
    if (i0 >= nv || i1 >= nv || i2 >= nv) return false;
    v0 = ld3(ms.vertices + 3 * (int64_t)i0);
    v1 = ld3(ms.vertices + 3 * (int64_t)i1);
    v2 = ld3(ms.vertices + 3 * (int64_t)i2);
    return true;
}

// Walks the tree under `node` along the mesh-frame ray o + s d for hits with s in (smin, best): on return best / tri hold the nearest one (the
// first in traversal order among equal s).  ANY: stop at the first hit found (shadow rays).  -> whether a hit was found.
template <bool ANY>
__device__ __forceinline__ bool mesh_trace(const MeshArrays& ms, int node, V3 o, V3 d, float smin, float& best, int& tri) {
    const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;   // (inf for a zero component: not used then)
    bool found = false;
    while ((unsigned)node < (unsigned)ms.num_nodes) {
        const float4 a = ms.nodes[2 * (int64_t)node], b = ms.nodes[2 * (int64_t)node + 1];
        const int skip = __float_as_int(a.w), leaf = __float_as_int(b.w);
        float nr = smin, fr = best;
        {
            const float t0 = (a.x - o.x) * ix, t1 = (b.x - o.x) * ix;
            const bool in = a.x <= o.x && o.x <= b.x;
            nr = fmaxf(nr, d.x == 0.0f ? (in ? -INFINITY : INFINITY) : fminf(t0, t1));
            fr = fminf(fr, d.x == 0.0f ? INFINITY : fmaxf(t0, t1));
        }
        {
            const float t0 = (a.y - o.y) * iy, t1 = (b.y - o.y) * iy;
            const bool in = a.y <= o.y && o.y <= b.y;
            nr = fmaxf(nr, d.y == 0.0f ? (in ? -INFINITY : INFINITY) : fminf(t0, t1));
            fr = fminf(fr, d.y == 0.0f ? INFINITY : fmaxf(t0, t1));
        }
        {
            const float t0 = (a.z - o.z) * iz, t1 = (b.z - o.z) * iz;
            const bool in = a.z <= o.z && o.z <= b.z;
            nr = fmaxf(nr, d.z == 0.0f ? (in ? -INFINITY : INFINITY) : fminf(t0, t1));
            fr = fminf(fr, d.z == 0.0f ? INFINITY : fmaxf(t0, t1));
        }
        const bool hit = nr < INFINITY && nr - fr <= RM_SLAB_SLACK * (fabsf(nr) + fabsf(fr));   // (nr = inf: parallel to a slab and outside it)
        int next = skip;
        if (hit) {
            if (leaf < 0) {
                next = node + 1;
            } else {
                const int first = leaf >> 4, count = leaf & 15;
                for (int k = first; k < first + count; ++k) {
                    V3 v0, v1, v2;
                    if (!load_triangle(ms, k, v0, v1, v2)) continue;
                    const V3 e1 = v1 - v0, e2 = v2 - v0;
                    const V3 g = cross(e1, e2);
                    if (dot(g, g) <= PHC_RENDER_MESH_MIN_CROSS * PHC_RENDER_MESH_MIN_CROSS) continue;
                    const V3 pv = cross(d, e2);
                    const float det = dot(e1, pv);                  // = -d . g
                    if (det == 0.0f) continue;
                    const float inv = 1.0f / det;
                    const V3 tv = o - v0;
                    const float u = dot(tv, pv) * inv;
                    const V3 qv = cross(tv, e1);
                    const float v = dot(d, qv) * inv;
                    const float s = dot(e2, qv) * inv;
                    if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && s > smin && s < best) {
                        best = s;
                        tri = k;
                        found = true;
                        if (ANY) return true;
                    }
                }
            }
        }
        if (next <= node) break;   // -1: done; a link that steps backwards would never end
        node = next;
    }
    return found;
}

__global__ void __launch_bounds__(RD_THREADS) k_render_mesh(phc_render_scene_t sc, MeshArrays ms, const phc_mesh_instance_t* __restrict__ inst,
                                                             int32_t NI, uint64_t meshed_bodies, const int32_t* __restrict__ tri_perm,
                                                             RenderViews views, int32_t v0, int32_t W, int32_t H, int32_t tiles_x,
                                                             uint8_t* __restrict__ rgba, float* __restrict__ depth, int32_t* __restrict__ hit_id,
                                                             int32_t* __restrict__ tri_id) {
    __shared__ Prims P;
    __shared__ Insts M;
    const int vl = blockIdx.y;
    const phc_camera_t& cam = views.cam[vl];
    const int env = cam.env;
    const int S = sc.num_capsules, NM = sc.num_markers, NP = S + NM;

    // ---- pose the env's shapes in world space, one thread per shape (phc_render's, minus the capsules of bodies that carry a mesh) ----
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
            if (r > 0.0f && owner >= 0 && owner < sc.num_bodies && !((meshed_bodies >> owner) & 1)) {
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
            c = ld3(sc.markers + ((int64_t)env * NM + m) * 3);
            r = sc.marker_radii ? sc.marker_radii[m] : sc.marker_radius;
            R = r > 0.0f ? r : -1.0f;
            col = sc.marker_colors ? ld3(sc.marker_colors + 3 * m) : ld3(sc.marker_color);
            id = PHC_RENDER_MARKER_ID + m;
        }
        P.p0[i] = make_float4(c.x, c.y, c.z, r);
        P.p1[i] = make_float4(h.x, h.y, h.z, R * 1.0001f);   // (a margin on the reject only: the exact test decides)
        P.p2[i] = make_float4(col.x, col.y, col.z, __int_as_float(id));
    }
    // ---- pose the instances: mesh frame = body frame o geom frame ----
    for (int i = threadIdx.x; i < NI; i += RD_THREADS) {
        const phc_mesh_instance_t in = inst[i];
        const float* bs = sc.body_state + ((int64_t)env * sc.num_bodies + in.owner) * 13;   // (owner checked on the host)
        const V3 qb = ld3(bs + 3), qi = ld3(in.quat);
        const float wb = bs[6], wi = in.quat[3];
        V3 q = wb * qi + wi * qb + cross(qb, qi);
        float w = wb * wi - dot(qb, qi);
        const float qn = 1.0f / sqrtf(dot(q, q) + w * w);
        q = qn * q;
        w = qn * w;
        const V3 org = ld3(bs) + quat_rotate(qb, wb, ld3(in.pos));
        const V3 cm = ld3(in.center);
        const V3 cw = org + quat_rotate(q, w, cm);
        const V3 c0 = quat_rotate(q, w, v3(1.f, 0.f, 0.f)), c1 = quat_rotate(q, w, v3(0.f, 1.f, 0.f)), c2 = quat_rotate(q, w, v3(0.f, 0.f, 1.f));
        M.m0[i] = make_float4(c0.x, c0.y, c0.z, cw.x);
        M.m1[i] = make_float4(c1.x, c1.y, c1.z, cw.y);
        M.m2[i] = make_float4(c2.x, c2.y, c2.z, cw.z);
        M.m3[i] = make_float4(cm.x, cm.y, cm.z, in.radius > 0.0f ? in.radius * 1.0001f : -1.0f);
        M.m4[i] = make_float4(in.rgb[0], in.rgb[1], in.rgb[2], __int_as_float(in.root));
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

    // ---- primary ray: capsules and markers, then the instances ----
    float best_t = INFINITY, best_s = 0.0f;
    int best = -1, best_inst = -1, best_tri = -1;
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
    for (int i = 0; i < NI; ++i) {
        const float4 a0 = M.m0[i], a1 = M.m1[i], a2 = M.m2[i], a3 = M.m3[i];
        if (a3.w < 0.0f) continue;
        const V3 c = v3(a0.w, a1.w, a2.w);
        const float tc = dot(c - eye, d);
        if (tc + a3.w < 0.0f) continue;
        const V3 p = (eye - c) + tc * d;
        if (dot(p, p) > a3.w * a3.w) continue;
        const V3 c0 = v3(a0.x, a0.y, a0.z), c1 = v3(a1.x, a1.y, a1.z), c2 = v3(a2.x, a2.y, a2.z);
        const V3 om = v3(dot(c0, p), dot(c1, p), dot(c2, p)) + v3(a3.x, a3.y, a3.z);
        const V3 dm = v3(dot(c0, d), dot(c1, d), dot(c2, d));
        float s = best_t - tc;                            // only hits in front of the best so far (t = tc + s < best_t)
        int tri = -1;
        if (mesh_trace<false>(ms, __float_as_int(M.m4[i].w), om, dm, -tc, s, tri) && tc + s < best_t) {
            best_t = tc + s;
            best_s = s;
            best = -1;
            best_inst = i;
            best_tri = tri;
        }
    }
    int id = -1, tid = -1;
    V3 n = v3(0.f, 0.f, 1.f), col = ld3(sc.sky_color), hitp = v3(0.f, 0.f, 0.f);
    if (d.z < 0.0f && eye.z > 0.0f) {
        const float tg = -eye.z / d.z;
        if (tg < best_t) {
            best_t = tg;
            best = -1;
            best_inst = -1;
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
    } else if (best_inst >= 0) {
        const float4 a0 = M.m0[best_inst], a1 = M.m1[best_inst], a2 = M.m2[best_inst], e = M.m4[best_inst];
        const V3 c = v3(a0.w, a1.w, a2.w);
        const float tc = dot(c - eye, d);
        const V3 x = ((eye - c) + tc * d) + best_s * d;   // the hit, relative to the sphere's centre
        V3 t0, t1, t2;
        load_triangle(ms, best_tri, t0, t1, t2);          // (it was loaded before: the indices are in range)
        const V3 g = unit(cross(t1 - t0, t2 - t0));
        n = g.x * v3(a0.x, a0.y, a0.z) + g.y * v3(a1.x, a1.y, a1.z) + g.z * v3(a2.x, a2.y, a2.z);
        if (dot(n, d) > 0.0f) n = -1.0f * n;
        hitp = c + x;
        col = v3(e.x, e.y, e.z);
        id = PHC_RENDER_MESH_ID + best_inst;
        tid = tri_perm[best_tri];
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
            for (int i = 0; i < NI && lit > 0.0f; ++i) {
                const float4 a0 = M.m0[i], a1 = M.m1[i], a2 = M.m2[i], a3 = M.m3[i];
                if (a3.w < 0.0f) continue;
                const V3 c = v3(a0.w, a1.w, a2.w);
                const float tc = dot(c - o, L);
                if (tc + a3.w < 0.0f) continue;
                const V3 p = (o - c) + tc * L;
                if (dot(p, p) > a3.w * a3.w) continue;
                const V3 c0 = v3(a0.x, a0.y, a0.z), c1 = v3(a1.x, a1.y, a1.z), c2 = v3(a2.x, a2.y, a2.z);
                const V3 om = v3(dot(c0, p), dot(c1, p), dot(c2, p)) + v3(a3.x, a3.y, a3.z);
                const V3 dm = v3(dot(c0, L), dot(c1, L), dot(c2, L));
                float s = INFINITY;
                int tri = -1;
                if (mesh_trace<true>(ms, __float_as_int(M.m4[i].w), om, dm, -tc, s, tri)) lit = 0.0f;
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
    if (tri_id) tri_id[pix] = tid;
}

extern "C" int32_t phc_render_mesh(const phc_render_scene_t* scene, const phc_render_meshes_t* meshes, const phc_camera_t* cameras, int32_t views,
                                   int32_t width, int32_t height, uint8_t* rgba, float* depth, int32_t* hit_id, int32_t* tri_id, void* stream) {
    // phc_render's own checks (it repeats them when it runs, on the no-mesh path)
    if (!scene || !cameras || !rgba || views <= 0 || width <= 0 || height <= 0) return PHC_EINVAL;
    if ((int64_t)width * height > PHC_RENDER_MAX_PIXELS) return PHC_EINVAL;
    const phc_render_scene_t& sc = *scene;
    if (!sc.body_state || !sc.capsules || sc.num_envs <= 0 || sc.num_bodies < 1 || sc.num_bodies > PHC_MAX_BODIES) return PHC_EINVAL;
    if (sc.num_capsules < 1 || sc.num_capsules > PHC_RENDER_MAX_SHAPES || sc.num_shape_blocks < 1 || sc.capsule_stride < 8 * (int64_t)sc.num_capsules)
        return PHC_EINVAL;
    if (sc.num_markers < 0 || sc.num_markers > PHC_RENDER_MAX_MARKERS || (sc.num_markers > 0 && !sc.markers)) return PHC_EINVAL;
    if (((uintptr_t)rgba | (uintptr_t)depth | (uintptr_t)hit_id | (uintptr_t)tri_id) & 3) return PHC_EINVAL;
    for (int32_t v = 0; v < views; ++v)
        if (cameras[v].env < 0 || cameras[v].env >= sc.num_envs) return PHC_EINVAL;
    uint64_t meshed = 0;
    if (meshes) {
        const phc_render_meshes_t& m = *meshes;
        if (m.num_instances < 0 || m.num_instances > PHC_RENDER_MAX_INSTANCES) return PHC_EINVAL;
        if (m.num_instances > 0) {
            if (!m.instances || !m.instances_dev || !m.vertices || !m.triangles || !m.tri_perm || !m.nodes) return PHC_EINVAL;
            if (m.num_vertices < 1 || m.num_triangles < 1 || m.num_triangles > PHC_RENDER_MAX_TRIANGLES || m.num_nodes < 1 ||
                m.num_nodes > 2 * PHC_RENDER_MAX_TRIANGLES || ((uintptr_t)m.nodes & 15))
                return PHC_EINVAL;
            for (int32_t i = 0; i < m.num_instances; ++i) {
                const phc_mesh_instance_t& in = m.instances[i];
                if (in.owner < 0 || in.owner >= sc.num_bodies || in.root < 0 || in.root >= m.num_nodes) return PHC_EINVAL;
                meshed |= (uint64_t)1 << in.owner;
            }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (!meshes || meshes->num_instances == 0) {   // the capsule kernel itself: the same bytes
        const int32_t rc = phc_render(scene, cameras, views, width, height, rgba, depth, hit_id, stream);
        if (rc != 0 || !tri_id) return rc;
        hipError_t e = hipMemsetAsync(tri_id, 0xff, (size_t)views * height * width * sizeof(int32_t), st);
        return e == hipSuccess ? 0 : (int32_t)e;
    }
    const MeshArrays ms = {meshes->vertices, meshes->triangles, reinterpret_cast<const float4*>(meshes->nodes), meshes->num_vertices,
                           meshes->num_triangles, meshes->num_nodes};
    const int32_t tiles_x = (width + RD_TILE - 1) / RD_TILE, tiles_y = (height + RD_TILE - 1) / RD_TILE;
    for (int32_t v0 = 0; v0 < views; v0 += RD_VIEWS) {
        RenderViews vw = {};
        const int32_t nv = views - v0 < RD_VIEWS ? views - v0 : RD_VIEWS;
        for (int32_t k = 0; k < nv; ++k) vw.cam[k] = cameras[v0 + k];
        hipLaunchKernelGGL(k_render_mesh, dim3((unsigned)(tiles_x * tiles_y), (unsigned)nv), dim3(RD_THREADS), 0, st, sc, ms, meshes->instances_dev,
                           meshes->num_instances, meshed, meshes->tri_perm, vw, v0, width, height, tiles_x, rgba, depth, hit_id, tri_id);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
