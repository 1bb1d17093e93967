// rt_views.hip — the read-only viewers and queries of a radiance map: the radiance-map view
// (k_sarsa_view), the irradiance render on the k nearest volumes (k_sarsa_irr) and the two query
// kernels (k_sarsa_nearest, k_sarsa_knn).  They search the map as the learning render does
// (rt_sarsa_search.hpp) and change nothing in it; the two views stand on the camera-hit frame of
// rt_view.hpp (k_sarsa_view in view_frame, k_sarsa_irr with its loop written out on the pieces).
// The learning render itself is rt_sarsa.hip.
#include <float.h>

#include "rt_sarsa_search.hpp"
#include "rt_view.hpp"

namespace rt {

namespace {

// normal class of a query normal (queries without a surface index)
__device__ int sarsa_class_of(const SarsaMap& m, f3 nrm) {
    for (int c = 0; c < m.n_class; ++c) {
        const float4 n4 = m.class_nrm[c];
        if (nrm.x == n4.x && nrm.y == n4.y && nrm.z == n4.z) return c;
    }
    return -1;
}

// nearest-volume queries alone (KD parity): pos/nrm [n][3]
__global__ __launch_bounds__(256) void k_sarsa_nearest(const SarsaMap m, const float* __restrict__ pos,
                                                       const float* __restrict__ nrm, int n, int32_t* out) {
    __shared__ int kd_stack[kKdStack * 256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 + (threadIdx.x & ~63) >= n) return;  // (whole waves past the end)
    const bool in = i < n;
    const f3 p = in ? make3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]) : make3(0.f, 0.f, 0.f);
    const f3 nr = in ? make3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]) : make3(0.f, 0.f, 0.f);
    int v = -1;
    if (m.use_grid) {  // as k_sarsa_render_pq searches
        if (in) v = sarsa_nearest_grid(m, sarsa_class_of(m, nr), p, nr);
        sarsa_resolve_walks(m, p, nr, &v, kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64), kd_stack_of(kd_stack),
                            threadIdx.x & 63);
    } else if (in) {
        v = sarsa_nearest(m, p, nr, kd_stack_of(kd_stack));
    }
    if (in) out[i] = v;
}

// The radiance-map view (the reference's PATH_TRACING_METHOD 2: GPU/path_tracing/
// voronoi_trace.cu:6-41, RadianceMap::get_voronoi_colour, radiance_map.cu:218-225): per
// sample the camera ray of k_sarsa_render_pq (sample index a.sample_base + s), its closest hit,
// the nearest volume of a surface hit as the render searches it, and that volume's entry of
// the colour table; (1, 1, 1) for a light or a miss.  The lane layout, the cull, the trips and
// the chunk fold are rt_view.hpp's; the k-d walks of the grid's undecided queries are shared by
// the wave (sarsa_resolve_walks), so every lane searches in every trip, with or without a
// query.  Reads the map only (grid_fallbacks counts its undecided queries as in the render).
// cull: the camera rays take the cull of the wave's pixel rectangle (launch_sarsa_view).
// out_tri / out_vol / out_pos (each may be null): triangle (-1: miss), volume (-1: no
// surface) and hit point (zeros: no surface) of sample a.sample_base, by output pixel.
template <int RULE>
__global__ __launch_bounds__(256) void k_sarsa_view(const RenderLaunch a, const SarsaMap m,
                                                    const float4* __restrict__ colours, int cull,
                                                    int32_t* __restrict__ out_tri, int32_t* __restrict__ out_vol,
                                                    float* __restrict__ out_pos) {
    __shared__ int kd_stack[kKdStack * 256];
    ViewLane v;
    if (!view_lane(a, &v)) return;
    int* const st = kd_stack_of(kd_stack);
    int* const blk_ws = kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64);
    const f3 o = make3(a.cam_x, a.cam_y, a.cam_z);
    uint64_t cm[kRenderCullWords];
    view_cull<RULE>(a, v, cull, cm);
    view_frame(a, v, [&](int s, bool first) {
        f3 d;
        const Hit h = view_camera_hit<RULE, false>(a, v, s, cull, cm, o, nullptr, &d);
        const bool is_surf = view_is_surf(a, v, h);
        f3 pos = o;
        f3 nrm = make3(0.f, 0.f, 0.f);
        if (is_surf) {
            pos = view_hit_point(a, h, o, d);
            nrm = view_normal(a, h.tri);
        }
        int rv = -1;
        if (is_surf) rv = m.use_grid ? sarsa_nearest_grid_tri(m, h.tri, pos, nrm) : kNeedWalk;
        if (m.use_grid)  // the whole wave, with or without a query
            sarsa_resolve_walks(m, pos, nrm, &rv, blk_ws, st, v.lane);
        else if (rv == kNeedWalk)
            rv = sarsa_nearest(m, pos, nrm, st);
        float4 c = make_float4(1.f, 1.f, 1.f, 0.f);
        if (rv >= 0) c = colours[rv];
        if (first) {
            const size_t op = v.op(a);
            view_write_tri(op, out_tri, h.tri);
            if (out_vol != nullptr) out_vol[op] = rv;
            if (out_pos != nullptr) {  // (view_write_pos, written out: it costs this kernel scalar spills)
                out_pos[3 * op + 0] = is_surf ? pos.x : 0.0f;
                out_pos[3 * op + 1] = is_surf ? pos.y : 0.0f;
                out_pos[3 * op + 2] = is_surf ? pos.z : 0.0f;
            }
        }
        return make3(c.x, c.y, c.z);
    });
}

// ---- the k nearest volumes (rt_sarsa_knn) and the irradiance render on them ----
//
// RadianceTree::find_closest_radiance_volumes (Old_CPU_Rendering_Engine/Source/radiance_volumes/
// radiance_tree.cpp:111-177) with an exact range test: of the volumes whose normal equals the
// query's and whose len3 distance d is below radius, the k smallest by (d, volume index).
// The per-normal grid answers it without a walk: every class volume closer than grid_h to the
// query is in the list of the query's clamped cell (rt_sarsa_host.cpp NearestGrid), so
// radius <= grid_h (host-checked) makes the cell's list a superset of the answer.

constexpr int kKnnMax = 8;  // RT_SARSA_KNN_MAX

// The best kKnnMax candidates, ascending by (d, v); an empty slot is (+inf, -1).  The slots
// are named members, not an array: a select chain over array elements is folded into a
// run-time index by the compiler, which moves the whole set out of registers.
struct KnnSet {
    float d0, d1, d2, d3, d4, d5, d6, d7;
    int v0, v1, v2, v3, v4, v5, v6, v7;
};
static_assert(kKnnMax == 8, "KnnSet names its slots");
#define KNN_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

__device__ __forceinline__ void knn_clear(KnnSet& s) {
#define KNN_X(i)     \
    s.d##i = INFINITY; \
    s.v##i = -1;
    KNN_SLOTS(KNN_X)
#undef KNN_X
}

// insertion of (d, v), d finite: b_i = it sorts before slot i (monotone in i, the slots being
// sorted); slot i takes its left neighbour where that one moves, the candidate where only
// itself moves
__device__ __forceinline__ void knn_insert(KnnSet& s, float d, int v) {
#define KNN_X(i) const bool b##i = (d < s.d##i) | ((d == s.d##i) & (v < s.v##i));
    KNN_SLOTS(KNN_X)
#undef KNN_X
#define KNN_MOVE(i, j)                                 \
    s.d##i = b##j ? s.d##j : (b##i ? d : s.d##i); \
    s.v##i = b##j ? s.v##j : (b##i ? v : s.v##i);
    KNN_MOVE(7, 6)
    KNN_MOVE(6, 5)
    KNN_MOVE(5, 4)
    KNN_MOVE(4, 3)
    KNN_MOVE(3, 2)
    KNN_MOVE(2, 1)
    KNN_MOVE(1, 0)
#undef KNN_MOVE
    s.d0 = b0 ? d : s.d0;
    s.v0 = b0 ? v : s.v0;
}

// slot k - 1 (k in [1, kKnnMax], wave-uniform): the distance a candidate has to beat or tie
__device__ __forceinline__ float knn_kth(const KnnSet& s, int k) {
    float r = s.d7;
#define KNN_X(i) r = (k == i + 1) ? s.d##i : r;
    KNN_SLOTS(KNN_X)
#undef KNN_X
    return r;
}

// The search in the class grid (G, D) as sarsa_nearest_grid_gd finds its cell.  The set keeps
// the best kKnnMax candidates whatever k is; its first k slots are the answer: the scan stops
// at the first listed entry L with d(C, L) > min(radius, k-th distance) + d(q, C) (the list
// ascends in d(C, L); the 2^-12 margin as in sarsa_nearest_grid_gd), which can neither enter
// the first k slots nor tie with them, and neither can any entry after it.
__device__ __forceinline__ void sarsa_knn_gd(const SarsaMap& m, float4 G, int4 D, f3 pos, int k, float radius,
                                             KnnSet& s) {
    if (!(__builtin_isfinite(pos.x) && __builtin_isfinite(pos.y) && __builtin_isfinite(pos.z))) return;
    const float ic = m.grid_inv_cs;
    const int ix = (int)floorf(fminf(fmaxf((pos.x - G.x) * ic, 0.0f), (float)(D.x - 1)));
    const int iy = (int)floorf(fminf(fmaxf((pos.y - G.y) * ic, 0.0f), (float)(D.y - 1)));
    const int iz = (int)floorf(fminf(fmaxf((pos.z - G.z) * ic, 0.0f), (float)(D.z - 1)));
    const uint32_t c = __float_as_uint(G.w) + (uint32_t)((iz * D.y + iy) * D.x + ix);
    const uint2 r = m.cell_range[c];
    const uint32_t e = r.y;
    const float cx = G.x + ((float)ix + 0.5f) * m.grid_cs;
    const float cy = G.y + ((float)iy + 0.5f) * m.grid_cs;
    const float cz = G.z + ((float)iz + 0.5f) * m.grid_cs;
    const float qx = pos.x - cx, qy = pos.y - cy, qz = pos.z - cz;
    const float dq = __builtin_sqrtf((qx * qx + qy * qy) + qz * qz);
    for (uint32_t j = r.x; j < e; j += 4) {  // 4 candidate loads in flight
        float4 L[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) L[u] = m.grid_leaf[min(j + (uint32_t)u, e - 1u)];
        const float lim = (fminf(radius, knn_kth(s, k)) + dq) * (1.0f + 0x1p-12f) + 1e-6f;
        const float lim2 = lim * lim;
        bool done = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float ex = L[u].x - cx, ey = L[u].y - cy, ez = L[u].z - cz;
            done = done || ((ex * ex + ey * ey) + ez * ez > lim2);
            const float d = len3(L[u].x - pos.x, L[u].y - pos.y, L[u].z - pos.z);
            if (!done && j + (uint32_t)u < e && d < radius) knn_insert(s, d, __float_as_int(L[u].w));
        }
        if (done) break;
    }
}

// rt_sarsa_knn: one lane per query; no LDS, no wave-level operation.  Slots past the count
// hold -1 / +inf.
__global__ __launch_bounds__(256) void k_sarsa_knn(const SarsaMap m, const float* __restrict__ pos,
                                                   const float* __restrict__ nrm, int n, int k, float radius,
                                                   int32_t* __restrict__ out_vol, float* __restrict__ out_dist,
                                                   int32_t* __restrict__ out_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f3 p = make3(pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
    const f3 nr = make3(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2]);
    KnnSet s;
    knn_clear(s);
    const int cls = sarsa_class_of(m, nr);
    if (cls >= 0) sarsa_knn_gd(m, m.class_org[cls], m.class_dim[cls], p, k, radius, s);
    int count = 0;
#define KNN_X(u)                                                            \
    if (u < k) {                                                            \
        count += s.v##u >= 0 ? 1 : 0;                                       \
        out_vol[(size_t)i * k + u] = s.v##u;                                \
        if (out_dist != nullptr) out_dist[(size_t)i * k + u] = s.d##u; \
    }
    KNN_SLOTS(KNN_X)
#undef KNN_X
    if (out_count != nullptr) out_count[i] = count;
}

// rt_render_irradiance's options on the device (rt_irr_opts, host-checked)
struct IrrOpts {
    int k;
    float radius;
    int cone;  // RT_IRR_CONE: weights 1 - d / radius (0: the plain mean)
    int tint;
};

// The map's irradiance estimate at a surface point, interpolated over its first k volumes
// (RadianceMap::get_irradiance_estimate, radiance_map.cpp:93-128): e = accum * kIrrScale per
// volume, nearest first; the mean, or the cone-weighted mean (the mean where the weights sum
// to 0); 0 with no volume in range.
__device__ __forceinline__ float irr_estimate(const SarsaMap& m, const KnnSet& s, const IrrOpts& o) {
    int count = 0;
    float sum = 0.0f, wsum = 0.0f, wtot = 0.0f;
#define KNN_X(u)                                        \
    if (u < o.k && s.v##u >= 0) {                       \
        const float e = m.accum[s.v##u] * kIrrScale;    \
        const float w = 1.f - s.d##u / o.radius;        \
        const float we = w * e;                         \
        sum = count == 0 ? e : sum + e;                 \
        wsum = count == 0 ? we : wsum + we;             \
        wtot = count == 0 ? w : wtot + w;               \
        ++count;                                        \
    }
    KNN_SLOTS(KNN_X)
#undef KNN_X
    if (count == 0) return 0.0f;
    if (o.cone && wtot != 0.0f) return wsum / wtot;
    return sum / (float)count;
}

// The irradiance render of the map (the CPU engine's draw_radiance_map_path_tracing,
// path_tracing/precompute_irradiance_path_tracing.cpp:3-53): per sample the camera ray and
// closest hit of the view frame (rt_view.hpp), and at a surface hit the map's interpolated
// estimate (irr_estimate) of the hit point under the surface's stored normal -- grey, or (tint)
// times the surface's albedo over its luminance; a light gives its emission, a miss env_light.
// No k-d walk, so no LDS.  Reads the map only.
// out_tri / out_pos as k_sarsa_view's; out_vol / out_dist [pixel][k]: the volumes found for
// sample a.sample_base and their distances (-1 / +inf: none, or no surface hit).
template <int RULE>
__global__ __launch_bounds__(256) void k_sarsa_irr(const RenderLaunch a, const SarsaMap m, const IrrOpts o, int cull,
                                                   int32_t* __restrict__ out_tri, float* __restrict__ out_pos,
                                                   int32_t* __restrict__ out_vol, float* __restrict__ out_dist) {
    ViewLane v;
    if (!view_lane(a, &v)) return;
    const float4* __restrict__ shade = a.scene.shade;
    const f3 o3 = make3(a.cam_x, a.cam_y, a.cam_z);
    uint64_t cm[kRenderCullWords];
    view_cull<RULE>(a, v, cull, cm);
    // (the trips written out on the frame's pieces, not through view_frame: DESIGN.md section 7)
    f3 acc = make3(0.f, 0.f, 0.f);
    for (int t = 0; t < a.per_chunk; ++t) {
        f3 d;
        const Hit h = view_camera_hit<RULE, false>(a, v, v.chunk * a.per_chunk + t, cull, cm, o3, nullptr, &d);
        const bool is_surf = view_is_surf(a, v, h);
        f3 pos = o3;
        KnnSet ks;
        knn_clear(ks);
        f3 c = make3(a.env_light, a.env_light, a.env_light);  // a miss
        if (is_surf) {
            pos = view_hit_point(a, h, o3, d);
            const float4 G = m.tri_grid[2 * h.tri];
            const float4 Df = m.tri_grid[2 * h.tri + 1];
            const int4 D = make_int4(__float_as_int(Df.x), __float_as_int(Df.y), __float_as_int(Df.z),
                                     __float_as_int(Df.w));
            if (D.w >= 0) sarsa_knn_gd(m, G, D, pos, o.k, o.radius, ks);
            const float L = irr_estimate(m, ks, o);
            c = make3(L, L, L);
            if (o.tint) {
                const float4 alb = shade[h.tri * kShadeF4 + 4];
                const float lum = m.tri_lum[h.tri];
                const float g = L / lum;
                c = lum == 0.0f ? make3(0.f, 0.f, 0.f) : make3(alb.x * g, alb.y * g, alb.z * g);
            }
        } else if (h.tri >= 0) {  // a light: its emission
            const float4 em = shade[h.tri * kShadeF4 + 3];
            c = make3(em.x, em.y, em.z);
        }
        acc.x = acc.x + c.x;
        acc.y = acc.y + c.y;
        acc.z = acc.z + c.z;
        if (t == 0 && v.chunk == 0 && v.valid) {
            const size_t op = v.op(a);
            view_write_tri(op, out_tri, h.tri);
            view_write_pos(op, out_pos, is_surf, pos);
#define KNN_X(u)                                                          \
    if (u < o.k) {                                                        \
        if (out_vol != nullptr) out_vol[op * o.k + u] = ks.v##u;      \
        if (out_dist != nullptr) out_dist[op * o.k + u] = ks.d##u; \
    }
            KNN_SLOTS(KNN_X)
#undef KNN_X
        }
    }
    view_fold_store(a, v, acc);
}

}  // namespace

hipError_t launch_sarsa_knn(const SarsaMap& m, const float* pos, const float* nrm, int n, int k, float radius,
                            int32_t* out_vol, float* out_dist, int32_t* out_count, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (m.grid_leaf == nullptr || k < 1 || k > kKnnMax || !(radius > 0.0f && radius <= m.grid_h) || out_vol == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sarsa_knn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, pos, nrm, n, k, radius,
                       out_vol, out_dist, out_count);
    return hipGetLastError();
}

hipError_t launch_sarsa_irr(const RenderLaunch& a, const SarsaMap& m, int k, float radius, int cone, int tint,
                            int32_t* out_tri, float* out_pos, int32_t* out_vol, float* out_dist, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    if (a.out == nullptr || m.grid_leaf == nullptr || k < 1 || k > kKnnMax || !(radius > 0.0f && radius <= m.grid_h))
        return hipErrorInvalidValue;
    if (!view_split_ok(a)) return hipErrorInvalidValue;
    const int cull = view_cull_wanted(a);
    const IrrOpts o{k, radius, cone, tint};
    const dim3 grid((unsigned)(a.n_blocks * a.split));
    if (a.hit_rule == 0)
        hipLaunchKernelGGL((k_sarsa_irr<0>), grid, dim3(256), 0, stream, a, m, o, cull, out_tri, out_pos, out_vol, out_dist);
    else
        hipLaunchKernelGGL((k_sarsa_irr<1>), grid, dim3(256), 0, stream, a, m, o, cull, out_tri, out_pos, out_vol, out_dist);
    return hipGetLastError();
}

// the camera rays take the rectangle cull where view_cull_wanted says (rt_internal.hpp)
hipError_t launch_sarsa_view(const RenderLaunch& a, const SarsaMap& m, const float4* colours, int32_t* out_tri,
                             int32_t* out_vol, float* out_pos, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    if (colours == nullptr || a.out == nullptr) return hipErrorInvalidValue;
    if (!view_split_ok(a)) return hipErrorInvalidValue;
    const int cull = view_cull_wanted(a);
    const dim3 grid((unsigned)(a.n_blocks * a.split));
    KernelTimer kt(KT_SARSA_VIEW, stream);
    if (a.hit_rule == 0)
        hipLaunchKernelGGL((k_sarsa_view<0>), grid, dim3(256), 0, stream, a, m, colours, cull, out_tri, out_vol, out_pos);
    else
        hipLaunchKernelGGL((k_sarsa_view<1>), grid, dim3(256), 0, stream, a, m, colours, cull, out_tri, out_vol, out_pos);
    return hipGetLastError();
}

hipError_t launch_sarsa_nearest(const SarsaMap& m, const float* pos, const float* nrm, int n, int32_t* out,
                                hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    KernelTimer kt(KT_SARSA_NEAREST, stream);
    hipLaunchKernelGGL(k_sarsa_nearest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, pos, nrm, n, out);
    return hipGetLastError();
}

}  // namespace rt
