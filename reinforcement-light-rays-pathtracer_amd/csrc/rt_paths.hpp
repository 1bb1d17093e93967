// rt_paths.hpp — what the GPU preset's path kernels share: the preset's surface step (k_render,
// k_render_pq, k_probe, k_bake), the first ray of a (point, sector, sample) and the cast routes of
// a ray that leaves a known surface (k_probe, k_bake, k_sweep).  The host's half -- the route
// choice, the argument checks, the error text -- is in rt_internal.hpp / rt_capi.cpp.
#pragma once

#include "rt_trace.hpp"

namespace rt {

// ---- the GPU preset's surface step ----
// The direction sampled in surface tri's shading frame by event 1 + depth of Philox counter
// (pix, s); returns cos(theta) of the direction.
template <int SAMPLER>
__device__ __forceinline__ float bounce_direction_at(int tri, const float4* __restrict__ shade, uint32_t pix,
                                                     uint32_t s, int depth, uint32_t seed_lo, uint32_t seed_hi, f3* sd) {
    const float4 N = shade[tri * kShadeF4 + 0];
    const float4 T = shade[tri * kShadeF4 + 1];
    const float4 B = shade[tri * kShadeF4 + 2];
    float r1, r2;
    draw2(pix, s, 1u + (uint32_t)depth, seed_lo, seed_hi, &r1, &r2);
    float cos_theta, sin_theta;
    if (SAMPLER == 0) {
        cos_theta = r1;
        sin_theta = sqrtf(1.0f - r1 * r1);
    } else {
        cos_theta = sqrtf(r1);
        sin_theta = sqrtf(1.0f - r1);
    }
    float sphi, cphi;
    sincos_turn(r2, &sphi, &cphi);
    const float sx = sin_theta * cphi, sz = sin_theta * sphi;
    *sd = make3((sx * B.x + cos_theta * N.x) + sz * T.x, (sx * B.y + cos_theta * N.y) + sz * T.y,
                (sx * B.z + cos_theta * N.z) + sz * T.z);
    return cos_theta;
}
// The hit position, and bounce_direction_at of the hit surface.
template <int SAMPLER>
__device__ __forceinline__ float bounce_direction(const Hit& h, f3 o, f3 d, float t_scale,
                                                  const float4* __restrict__ shade, uint32_t pix, uint32_t s,
                                                  int depth, uint32_t seed_lo, uint32_t seed_hi, f3* pos, f3* sd) {
    const float Dx = d.x * t_scale, Dy = d.y * t_scale, Dz = d.z * t_scale;
    *pos = make3(o.x + h.t * Dx, o.y + h.t * Dy, o.z + h.t * Dz);
    return bounce_direction_at<SAMPLER>(h.tri, shade, pix, s, depth, seed_lo, seed_hi, sd);
}
// the throughput past surface tri, left along a direction of cos_theta
template <int SAMPLER>
__device__ __forceinline__ f3 bounce_throughput(f3 tp, const float4* __restrict__ shade, int tri, float cos_theta) {
    if (SAMPLER == 0) {
        const float4 c = shade[tri * kShadeF4 + 3];
        return make3(div_rho((tp.x * c.x) * cos_theta), div_rho((tp.y * c.y) * cos_theta),
                     div_rho((tp.z * c.z) * cos_theta));
    }
    const float4 c = shade[tri * kShadeF4 + 4];
    return make3(tp.x * c.x, tp.y * c.y, tp.z * c.z);
}
// The whole step at a surface hit h of the ray (o, d): the new ray, the new throughput; returns
// the surface the new ray leaves.
template <int SAMPLER>
__device__ __forceinline__ int surface_step(const Hit& h, f3& o, f3& d, f3& tp, float t_scale,
                                            const float4* __restrict__ shade, uint32_t pix, uint32_t s, int depth,
                                            uint32_t seed_lo, uint32_t seed_hi) {
    f3 pos, sd;
    const float cos_theta = bounce_direction<SAMPLER>(h, o, d, t_scale, shade, pix, s, depth, seed_lo, seed_hi, &pos, &sd);
    tp = bounce_throughput<SAMPLER>(tp, shade, h.tri, cos_theta);
    o = make3(pos.x + kEps * sd.x, pos.y + kEps * sd.y, pos.z + kEps * sd.z);
    d = normalize(sd);
    return h.tri;
}

// surface_step for a caller that holds the hit position pos on surface tri (k_render_nee, whose
// shadow cast lies between the hit and the bounce): the same ray and throughput.
template <int SAMPLER>
__device__ __forceinline__ void surface_step_at(f3 pos, int tri, f3& o, f3& d, f3& tp, const float4* __restrict__ shade,
                                                uint32_t pix, uint32_t s, int depth, uint32_t seed_lo, uint32_t seed_hi) {
    f3 sd;
    const float cos_theta = bounce_direction_at<SAMPLER>(tri, shade, pix, s, depth, seed_lo, seed_hi, &sd);
    tp = bounce_throughput<SAMPLER>(tp, shade, tri, cos_theta);
    o = make3(pos.x + kEps * sd.x, pos.y + kEps * sd.y, pos.z + kEps * sd.z);
    d = normalize(sd);
}

// ---- the first ray of (point, sector, sample) ----
// Sample s draws the DQN sampler's jittered direction inside the sector of the 12 x 12 grid laid
// out in the frame N / T / B at pos: Philox counter (pix, s, 1, 73), pix = id * 144 + sector.
// Returns the unnormalised direction; the ray is o = pos + dir * kEps along d = normalize(dir).
__device__ __forceinline__ f3 sector_first_ray(uint32_t pix, uint32_t s, int sector, f3 N, f3 T, f3 B, f3 pos,
                                               uint32_t seed_lo, uint32_t seed_hi, f3* o, f3* d) {
    uint32_t w[4];
    philox4x32_10(pix, s, 1u, 1u + kDqnActions / 2, seed_lo, seed_hi, w);
    const int gx = sector / kDqnGrid, gy = sector - gx * kDqnGrid;
    const f3 dir = grid_direction((float)gx + u01(w[0]), (float)gy + u01(w[1]), N, T, B, pos);
    *o = make3(pos.x + dir.x * kEps, pos.y + dir.y * kEps, pos.z + dir.z * kEps);
    *d = normalize(dir);
    return dir;
}

// ---- the cast routes of a ray that leaves surface surf (the same hit, bit for bit) ----
// the scene's bounce-ray candidate table (wave-level: every lane calls, wl the wave's exact-phase
// LDS), the exact BVH (stk: the lane's stack column of stride STRIDE), else the two-phase filter
// (use_filter, and the origin inside its bound) or the scan.  An inactive lane gets no hit.
// (kRouteSel / kRouteTable / kRouteBvh: rt_internal.hpp, with the host's choice leaving_route)
template <int RULE, int ROUTE, int NW, int STRIDE = 256>
__device__ __forceinline__ Hit closest_hit_route(const DeviceScene& sc, int use_filter, int surf, f3 o, f3 d,
                                                 float t_scale, bool active, float* wl, int* stk) {
    Hit h;
    h.t = 0.0f;
    h.tri = -1;
    if constexpr (ROUTE == kRouteTable) {
        h = closest_hit_ctab<RULE, NW>(sc, sc.ctab[RULE], surf, o, d, t_scale, active, wl);
    } else if constexpr (ROUTE == kRouteBvh) {
        if (active) h = closest_hit_bvh<RULE, STRIDE>(sc, o, d, t_scale, stk);
    } else if (active) {
        // the filter's bounds hold for origins within origin_bound (a caller's point may lie anywhere)
        const float om = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
        h = closest_hit_sel<RULE>(sc, use_filter && om <= sc.origin_bound, o, d, t_scale);
    }
    return h;
}

}  // namespace rt
