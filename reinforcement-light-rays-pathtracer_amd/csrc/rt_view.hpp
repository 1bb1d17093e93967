// rt_view.hpp — the frame of a camera-hit view: what k_sarsa_view, k_sarsa_irr (rt_views.hip) and
// k_glyph_view (rt_glyph.hip) share.  One lane per (pixel, chunk) in k_render's layout -- a
// wave covers 16 x 4 pixels at split 1 -- per trip the camera ray of sample a.sample_base + s and
// its closest hit, the view's own colour of that hit (the kernel's body), and the fold of the
// chunk sums in chunk order.  Every lane of a wave that has a pixel runs all per_chunk trips and
// calls the body in each: a lane outside the image or the tile casts nothing, but stays for the
// cull's ballots, the body's wave-level work (sarsa_resolve_walks) and the fold's shuffles.  The
// host's half -- view_split_ok, view_cull_wanted, fill_view_launch -- is in rt_internal.hpp.
#pragma once

#include "rt_trace.hpp"

namespace rt {

// ---- the lane layout of a (pixel, chunk) launch ----
struct ViewLane {
    BlockDesc blk;
    int part, q, chunk, lane;  // the block's part of this workgroup; the pixel of the block; the lane's chunk
    int lx, ly, px, py;
    bool valid;    // the pixel lies inside the clip
    uint32_t pix;  // the RNG key
    // the output pixel index (a.out's layout: the AOVs and the image)
    __device__ __forceinline__ size_t op(const RenderLaunch& a) const {
        return (size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx);
    }
};
// false: the whole wave lies outside the image (the kernel returns; the only early exit)
__device__ __forceinline__ bool view_lane(const RenderLaunch& a, ViewLane* v) {
    const int lg = a.split_log2;
    v->blk = a.blocks[blockIdx.x >> lg];
    v->part = blockIdx.x & (a.split - 1);
    v->q = (v->part << (8 - lg)) + ((int)threadIdx.x >> lg);
    v->chunk = threadIdx.x & (a.split - 1);
    v->lane = threadIdx.x & 63;
    v->lx = v->q & 15;
    v->ly = v->q >> 4;
    v->px = v->blk.px0 + v->lx;
    v->py = v->blk.py0 + v->ly;
    v->valid = (v->px < a.clip_x1) && (v->py < a.clip_y1);
    v->pix = (uint32_t)v->py * (uint32_t)a.width + (uint32_t)v->px;
    return __ballot(v->valid) != 0ull;
}

// the cull of the wave's pixel rectangle where the launcher asked for it (view_cull_wanted)
template <int RULE>
__device__ __forceinline__ void view_cull(const RenderLaunch& a, const ViewLane& v, int cull, uint64_t* cm) {
#pragma unroll
    for (int k = 0; k < kRenderCullWords; ++k) cm[k] = 0ull;
    if (cull) wave_candidates<RULE>(a, v.valid, v.px, v.py, v.lane, cm);
}

// ---- the camera sample of a trip ----
// Sample s of the lane's pixel: the GPU preset's camera ray (*d) and its closest hit in the scene,
// by the exact BVH (SBVH; stk: the lane's stack column), the wave's cull (cm) or the scan.  A lane
// without a pixel casts nothing (no hit).
template <int RULE, bool SBVH>
__device__ __forceinline__ Hit view_camera_hit(const RenderLaunch& a, const ViewLane& v, int s, int cull,
                                               const uint64_t* cm, f3 o, int* stk, f3* d) {
    Hit h;
    h.t = 0.0f;
    h.tri = -1;
    *d = make3(0.f, 0.f, 1.f);
    if (v.valid) {
        float r1, r2;
        draw2(v.pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
        camera_ray<1>(a, v.px, v.py, r1, r2, d);
        if constexpr (SBVH)
            h = closest_hit_bvh<RULE>(a.scene, o, *d, a.t_scale, stk);
        else
            h = cull ? view_hit_culled<RULE>(a.scene, cm, o, *d, a.t_scale)
                     : closest_hit<RULE>(a.scene.isect, a.scene.n_tri, o, *d, a.t_scale);
    }
    return h;
}

// ---- the surface hit's point and stored normal (taken inside the kernel's own is-a-surface branch: ----
// ---- computed ahead of it they cost k_sarsa_irr three VGPRs)                                        ----
// h is a surface hit of a lane with a pixel
__device__ __forceinline__ bool view_is_surf(const RenderLaunch& a, const ViewLane& v, const Hit& h) {
    return v.valid && (h.tri >= 0) && (h.tri < a.scene.n_surf);
}
__device__ __forceinline__ f3 view_hit_point(const RenderLaunch& a, const Hit& h, f3 o, f3 d) {
    const float Dx = d.x * a.t_scale, Dy = d.y * a.t_scale, Dz = d.z * a.t_scale;
    return make3(o.x + h.t * Dx, o.y + h.t * Dy, o.z + h.t * Dz);
}
__device__ __forceinline__ f3 view_normal(const RenderLaunch& a, int tri) {
    const float4 N4 = a.scene.shade[tri * kShadeF4 + 0];
    return make3(N4.x, N4.y, N4.z);
}

// ---- the AOVs every surface view has (each may be null): triangle (-1: miss), hit point (zeros: no surface) ----
__device__ __forceinline__ void view_write_tri(size_t op, int32_t* __restrict__ out_tri, int tri) {
    if (out_tri != nullptr) out_tri[op] = tri;
}
// (k_sarsa_view keeps these three stores written out: through this function, in any form tried,
// it spills three to five more scalar registers -- DESIGN.md section 7)
__device__ __forceinline__ void view_write_pos(size_t op, float* __restrict__ out_pos, bool is_surf, f3 pos) {
    if (out_pos != nullptr) {
        out_pos[3 * op + 0] = is_surf ? pos.x : 0.0f;
        out_pos[3 * op + 1] = is_surf ? pos.y : 0.0f;
        out_pos[3 * op + 2] = is_surf ? pos.z : 0.0f;
    }
}

// ---- the chunk fold and store: ((P0 + P1) + P2) + ... of the pixel's chunk sums, / spp ----
__device__ __forceinline__ void view_fold_store(const RenderLaunch& a, const ViewLane& v, f3 acc) {
    const int base = v.lane & ~(a.split - 1);
    f3 tot = acc;
    for (int k = 1; k < a.split; ++k) {
        const float vx = __shfl(acc.x, base + k, 64);
        const float vy = __shfl(acc.y, base + k, 64);
        const float vz = __shfl(acc.z, base + k, 64);
        tot.x = tot.x + vx;
        tot.y = tot.y + vy;
        tot.z = tot.z + vz;
    }
    if (v.valid && v.chunk == 0) {
        const float fs = (float)a.spp;
        store_rgb(a.out + v.op(a) * 3, tot.x / fs, tot.y / fs, tot.z / fs);
    }
}

// ---- the frame ----
// The lane's per_chunk trips, then the fold.  body(s, first) -> f3: the colour of sample s;
// first: this lane writes the view's AOVs (those of sample a.sample_base).  The sum starts at 0
// and takes one add per trip, in sample order.
template <class Body>
__device__ __forceinline__ void view_frame(const RenderLaunch& a, const ViewLane& v, Body&& body) {
    f3 acc = make3(0.f, 0.f, 0.f);
    for (int k = 0; k < a.per_chunk; ++k) {
        const f3 c = body(v.chunk * a.per_chunk + k, k == 0 && v.chunk == 0 && v.valid);
        acc.x = acc.x + c.x;
        acc.y = acc.y + c.y;
        acc.z = acc.z + c.z;
    }
    view_fold_store(a, v, acc);
}

}  // namespace rt
