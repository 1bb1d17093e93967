// rt_nee.hip — next-event estimation for the GPU preset (rt_render_nee in rtmi.h, where the
// estimator is defined line by line): rt_render's paths with a shadow ray towards one sampled
// point of one light at every surface hit.
//
// k_render_nee: a persistent grid over the launch-wide queue of (pixel, chunk) items, as
// k_render_pq / k_probe: a wave claims 64 items per atomic and hands them to its lanes by ballot
// rank; a lane sums its chunk in sample order, stores the chunk sum and claims the next.
// k_nee_fold adds each pixel's chunk sums in chunk order and divides by spp.
// One cast site per loop trip: a lane's ray in a trip is a camera ray (surf < 0), a shadow ray or a
// bounce ray (both leave surface surf).  On the table route the camera ray takes every triangle
// of the scene as its candidates and the other two the table's masks for surf; on the BVH and
// scan routes all three are the same call.  All give the scan's hit bit for bit
// (closest_hit_route, rt_paths.hpp).  A lane that took a direct term carries over its shadow
// trip the hit point, the three pre-multiplied channel factors and the light; the surface, the
// throughput and the depth stay where the path keeps them, and the bounce direction is drawn
// after the shadow trip (counter based: it needs no carried state).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_hostframe.hpp"
#include "rt_nee.hpp"
#include "rt_paths.hpp"

namespace rt {
namespace {

// Waves per SIMD the launch bounds ask for.  The table route's casts wait on two dependent
// lookups and gain from occupancy, as k_probe's, so each instantiation asks for the most it
// holds without scratch (tools/kernel_resources.py): under the GPU rule 6
// waves with one mask word (73-76 VGPRs) and 5 with four (85; 6 spill 1), under the CPU rule 5
// (93; 6 spill 10) and 4 (99; 6 spill 33).  The shadow trip's carried state costs one step against
// k_probe's 7 / 6 / 6 / 5.  The scan and the BVH are bound by their own loops.
__host__ __device__ constexpr int nee_waves(int route, int rule, int nw) {
    return route != kRouteTable ? 4 : (rule == 1 ? 5 : 4) + (nw == 1 ? 1 : 0);
}

struct NeeLaunch {
    RenderLaunch r;  // rt_render's launch: scene (the route's view), camera, blocks, clip, csum, work, casts
    NeeLights lights;
    int direct_only;
    unsigned long long* stats;  // [2] paths, zero-contribution paths: accumulated into, or null
};

template <int SAMPLER, int RULE, int ROUTE, int NW>
__global__ __launch_bounds__(256, nee_waves(ROUTE, RULE, NW)) void k_render_nee(const NeeLaunch a) {
    __shared__ __attribute__((aligned(16))) float s_mfw[ROUTE == kRouteTable ? 4 * kMfWaveFloats : 1];
    __shared__ int s_stk[ROUTE == kRouteBvh ? kBvhMaxDepth * 256 : 1];
    float* const wl = s_mfw + (ROUTE == kRouteTable ? ((int)threadIdx.x >> 6) * kMfWaveFloats : 0);
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.r.scene.shade;
    const float4* __restrict__ isect = a.r.scene.isect;
    const int n_surf = a.r.scene.n_surf;
    const long long total = (long long)a.r.n_blocks * 256 * a.r.split;
    const f3 cam = make3(a.r.cam_x, a.r.cam_y, a.r.cam_z);
    long long qb = 0, qe = 0;  // wave-uniform: the wave's claimed, not yet handed out items
    bool exhausted = false;     // wave-uniform: the launch's queue is empty
    bool have = false;          // the lane holds a chunk
    long long item = 0;
    int s = 0, s_end = 0, px = 0, py = 0;
    uint32_t pix = 0;
    int depth = 0;
    int surf = -1;        // the surface the ray leaves, -1: a camera ray
    bool shadow = false;  // the ray is a shadow ray towards light lsel
    int lsel = 0;
    f3 o = cam, d = make3(0.0f, 0.0f, 1.0f), tp = make3(1.0f, 1.0f, 1.0f);
    f3 pos = make3(0.0f, 0.0f, 0.0f), fac = make3(0.0f, 0.0f, 0.0f);  // the shadow trip's hit point and factors
    f3 L = make3(0.0f, 0.0f, 0.0f), acc = make3(0.0f, 0.0f, 0.0f);
    unsigned n_casts = 0, n_paths = 0, n_zero = 0;
    auto camera = [&]() {
        float r1, r2;
        draw2(pix, (uint32_t)s, 0u, a.r.seed_lo, a.r.seed_hi, &r1, &r2);
        camera_ray<1>(a.r, px, py, r1, r2, &d);
        o = cam;
        tp = make3(1.0f, 1.0f, 1.0f);
        L = make3(0.0f, 0.0f, 0.0f);
        depth = 0;
        surf = -1;
        shadow = false;
    };
    for (;;) {
        // lanes without a chunk take the next items of the queue
        if (!exhausted) {
            const uint64_t need = __ballot(!have);
            if (need != 0ull) {
                const int n_need = __builtin_popcountll(need);
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                const long long avail = qe - qb;
                long long nb = 0;
                if (n_need > avail) {  // (wave-uniform) 64 more items
                    unsigned long long v = 0;
                    if (lane == 0) v = atomicAdd(a.r.work, 64ull);
                    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
                    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                    nb = (long long)(((unsigned long long)hi << 32) | lo);
                }
                if (!have) {
                    const long long j = rank < avail ? qb + rank : nb + (rank - avail);
                    if (j < total) {
                        item = j;
                        const long long p = j >> a.r.split_log2;
                        const int c = (int)(j & (a.r.split - 1));
                        const BlockDesc blk = a.r.blocks[p >> 8];
                        const int q = (int)(p & 255);
                        px = blk.px0 + (q & 15);
                        py = blk.py0 + (q >> 4);
                        if (px < a.r.clip_x1 && py < a.r.clip_y1) {  // (a clipped pixel's chunks: nothing)
                            pix = (uint32_t)py * (uint32_t)a.r.width + (uint32_t)px;
                            s = c * a.r.per_chunk;
                            s_end = s + a.r.per_chunk;
                            acc = make3(0.0f, 0.0f, 0.0f);
                            have = true;
                            camera();
                        }
                    }
                }
                if (n_need > avail) {
                    qb = nb + (n_need - avail);
                    qe = nb + 64;
                } else {
                    qb += n_need;
                }
                if (qb >= total) exhausted = true;
            }
        }
        const bool active = have;
        if (__ballot(active) == 0ull) {
            if (exhausted) break;
            continue;  // (every claimed item was a clipped pixel's)
        }
        // the trip's cast
        Hit h;
        if constexpr (ROUTE == kRouteTable) {
            uint64_t F[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) F[k] = 0ull;
            if (active && surf < 0) {
#pragma unroll
                for (int k = 0; k < NW; ++k) F[k] = tri_mask(a.r.scene.n_tri, k);
            } else if (active) {
                ctab_candidates<NW>(a.r.scene.ctab[RULE], a.r.scene.n_tri, n_surf, surf, o, d, F);
            }
            h = closest_hit_cand<RULE, NW>(a.r.scene, F, o, d, a.r.t_scale, wl);
        } else {
            h = closest_hit_route<RULE, ROUTE, NW>(a.r.scene, a.r.use_filter, surf, o, d, a.r.t_scale, active, wl,
                                                   ROUTE == kRouteBvh ? s_stk + threadIdx.x : nullptr);
        }
        if (!active) continue;
        ++n_casts;
        bool end = false, bounce = false;
        if (shadow) {
            // visible iff the closest hit is the sampled light's triangle
            if (h.tri == n_surf + lsel) {
                L.x = L.x + fac.x;
                L.y = L.y + fac.y;
                L.z = L.z + fac.z;
            }
            shadow = false;
            if (a.direct_only)
                end = true;
            else
                bounce = true;
        } else if (h.tri < 0) {
            end = true;
            L.x = L.x + tp.x * a.r.env_light;
            L.y = L.y + tp.y * a.r.env_light;
            L.z = L.z + tp.z * a.r.env_light;
        } else if (h.tri >= n_surf) {
            end = true;
            if (depth == 0) {  // the camera sees the light; deeper, the previous surface sampled it
                const float4 e = shade[h.tri * kShadeF4 + 3];
                L.x = L.x + tp.x * e.x;
                L.y = L.y + tp.y * e.y;
                L.z = L.z + tp.z * e.z;
            }
        } else if (depth + 1 == a.r.max_bounces) {
            end = true;  // no next cast: no direct light either
        } else {
            const float Dx = d.x * a.r.t_scale, Dy = d.y * a.r.t_scale, Dz = d.z * a.r.t_scale;
            pos = make3(o.x + h.t * Dx, o.y + h.t * Dy, o.z + h.t * Dz);
            surf = h.tri;
            // the direct term
            if (a.lights.last >= 0) {
                uint32_t w[4];
                philox4x32_10(pix, (uint32_t)s, 1u + (uint32_t)depth, kNeeCounterWord, a.r.seed_lo, a.r.seed_hi, w);
                const int l = nee_pick(a.lights.cdf, a.lights.last, u01(w[0]));
                const int lt = n_surf + l;
                const float4 v0 = isect[lt * kIsectF4 + 0], e1 = isect[lt * kIsectF4 + 1], e2 = isect[lt * kIsectF4 + 2];
                const f3 y = nee_point(make3(v0.x, v0.y, v0.z), make3(e1.x, e1.y, e1.z), make3(e2.x, e2.y, e2.z),
                                       u01(w[1]), u01(w[2]));
                const float4 N = shade[surf * kShadeF4 + 0];
                const float4 Nl = shade[lt * kShadeF4 + 0];
                f3 sd;
                float g;
                if (nee_geometry(pos, make3(N.x, N.y, N.z), y, make3(Nl.x, Nl.y, Nl.z), &sd, &g)) {
                    g = g * a.lights.k[l];
                    const float4 brdf = shade[surf * kShadeF4 + 3];
                    const float4 le = shade[lt * kShadeF4 + 3];
                    fac = make3(((tp.x * brdf.x) * le.x) * g, ((tp.y * brdf.y) * le.y) * g, ((tp.z * brdf.z) * le.z) * g);
                    o = make3(pos.x + kEps * sd.x, pos.y + kEps * sd.y, pos.z + kEps * sd.z);
                    d = sd;
                    lsel = l;
                    shadow = true;
                }
            }
            if (!shadow) {
                if (a.direct_only)
                    end = true;
                else
                    bounce = true;
            }
        }
        if (bounce) {
            surface_step_at<SAMPLER>(pos, surf, o, d, tp, shade, pix, (uint32_t)s, depth, a.r.seed_lo, a.r.seed_hi);
            ++depth;
        }
        if (end) {
            acc.x = acc.x + L.x;
            acc.y = acc.y + L.y;
            acc.z = acc.z + L.z;
            ++n_paths;
            if (L.x == 0.0f && L.y == 0.0f && L.z == 0.0f) ++n_zero;
            ++s;
            if (s < s_end) {
                camera();
            } else {
                store_rgb(a.r.csum + (size_t)item * 3, acc.x, acc.y, acc.z);
                have = false;
            }
        }
    }
    if (a.r.casts != nullptr) {
        const unsigned tot = wave_sum(n_casts);
        if (lane == 0 && tot != 0u) atomicAdd(a.r.casts, (unsigned long long)tot);
    }
    if (a.stats != nullptr) {
        const unsigned tp_ = wave_sum(n_paths), tz = wave_sum(n_zero);
        if (lane == 0 && tp_ != 0u) atomicAdd(a.stats + 0, (unsigned long long)tp_);
        if (lane == 0 && tz != 0u) atomicAdd(a.stats + 1, (unsigned long long)tz);
    }
}

// the pixels of k_render_nee's launch: chunk sums in chunk order, / spp (k_render's fold)
__global__ __launch_bounds__(256) void k_nee_fold(const RenderLaunch a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)a.n_blocks * 256) return;
    const BlockDesc blk = a.blocks[p >> 8];
    const int q = (int)(p & 255), lx = q & 15, ly = q >> 4;
    if (blk.px0 + lx >= a.clip_x1 || blk.py0 + ly >= a.clip_y1) return;
    const float* c = a.csum + (size_t)p * a.split * 3;
    f3 tot = make3(c[0], c[1], c[2]);
    for (int k = 1; k < a.split; ++k) {
        tot.x = tot.x + c[3 * k + 0];
        tot.y = tot.y + c[3 * k + 1];
        tot.z = tot.z + c[3 * k + 2];
    }
    const float fs = (float)a.spp;
    float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
    store_rgb(dst, tot.x / fs, tot.y / fs, tot.z / fs);
}

template <int SAMPLER, int RULE>
void launch_nee_t(const NeeLaunch& a, int route, hipStream_t stream) {
    const long long items = (long long)a.r.n_blocks * 256 * a.r.split;
    const long long wanted = (items + 255) / 256;
    const int nw = a.r.scene.n_tri <= 64 ? 1 : 4;
    const int waves = nee_waves(route, RULE, nw);
    const unsigned wgs = (unsigned)std::min<long long>(wanted, (long long)waves * device_cu_count());
    (void)hipMemsetAsync(a.r.work, 0, sizeof(unsigned long long), stream);
    if (route == kRouteTable && nw == 1)
        hipLaunchKernelGGL((k_render_nee<SAMPLER, RULE, kRouteTable, 1>), dim3(wgs), dim3(256), 0, stream, a);
    else if (route == kRouteTable)
        hipLaunchKernelGGL((k_render_nee<SAMPLER, RULE, kRouteTable, 4>), dim3(wgs), dim3(256), 0, stream, a);
    else if (route == kRouteBvh)
        hipLaunchKernelGGL((k_render_nee<SAMPLER, RULE, kRouteBvh, 1>), dim3(wgs), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((k_render_nee<SAMPLER, RULE, kRouteSel, 1>), dim3(wgs), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_nee_fold, dim3((unsigned)a.r.n_blocks), dim3(256), 0, stream, a.r);
}

hipError_t launch_nee(const NeeLaunch& a, int route, hipStream_t stream) {
    switch (a.r.sampler * 2 + a.r.hit_rule) {
        case 0: launch_nee_t<0, 0>(a, route, stream); break;
        case 1: launch_nee_t<0, 1>(a, route, stream); break;
        case 2: launch_nee_t<1, 0>(a, route, stream); break;
        case 3: launch_nee_t<1, 1>(a, route, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// what both entries check after their pointers: rt_render's parameter checks, the flags, the preset
int check_nee(const rt_params* p, int flags) {
    const int rc = check_render_params(p);
    if (rc != RT_OK) return rc;
    if (flags != 0 && flags != RT_NEE_DIRECT_ONLY) return errorf(RT_E_INVALID, "bad flags %d", flags);
    if (p->preset != RT_PRESET_GPU) return errorf(RT_E_UNSUPPORTED, "next-event estimation renders the GPU preset only");
    return RT_OK;
}

// the launch of either entry, less its blocks and outputs: the cast route (with the candidate
// table built on first use) and the scene's light table
int nee_launch(const rt_scene* scene, const rt_camera* cam, const rt_params* p, int flags, NeeLaunch* a, int* route) {
    a->r = render_launch(scene, cam, p);
    *route = leaving_route(scene, p, &a->r.scene);
    if (*route < 0) return *route;
    const int rc = scene_nee_lights(scene, &a->lights);
    if (rc != RT_OK) return rc;
    a->direct_only = (flags & RT_NEE_DIRECT_ONLY) ? 1 : 0;
    a->stats = nullptr;
    return RT_OK;
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_render_nee(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params, int flags,
                  int x0, int y0, int w, int h, float* out_rgb, uint64_t* out_ray_casts, uint64_t* out_stats) {
    using namespace rt;
    if (!ctx || !scene || !cam || !out_rgb) return errorf(RT_E_INVALID, "NULL argument");
    int rc = check_nee(params, flags);
    if (rc != RT_OK) return rc;
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 + w > params->width || y0 + h > params->height)
        return errorf(RT_E_INVALID, "rectangle outside the image");
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    NeeLaunch a;
    int route = 0;
    rc = nee_launch(scene, cam, params, flags, &a, &route);
    if (rc != RT_OK) return rc;
    float* d_out;
    unsigned long long *d_casts, *d_stats;
    unsigned long long casts = 0, stats[2] = {0, 0};
    HostFrame f(x0, y0, w, h);
    f.out(&d_out, out_rgb, sizeof(float) * 3 * (size_t)w * (size_t)h);
    f.out(&d_casts, &casts, sizeof(casts), 0);
    f.out(&d_stats, stats, sizeof(stats), 0);
    e = f.begin();
    if (e == hipSuccess) {
        a.r.blocks = f.blocks();
        a.r.n_blocks = f.n_blocks();
        a.r.clip_x1 = x0 + w;
        a.r.clip_y1 = y0 + h;
        a.r.out_pitch = w;
        a.r.out = d_out;
        a.r.casts = d_casts;
        a.stats = d_stats;
        if (ctx_chunks(ctx, &a.r) != RT_OK) e = hipErrorOutOfMemory;
        if (e == hipSuccess) e = launch_nee(a, route, 0);
    }
    rc = f.finish(RT_OK, e, "rt_render_nee");
    if (rc == RT_OK && out_ray_casts) *out_ray_casts = casts;
    if (rc == RT_OK && out_stats) {
        out_stats[0] = stats[0];
        out_stats[1] = stats[1];
    }
    return rc;
}

int rt_render_nee_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params,
                               int flags, const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                               uint64_t* d_casts, uint64_t* d_stats, void* stream) {
    using namespace rt;
    if (!ctx || !scene || !cam) return errorf(RT_E_INVALID, "NULL argument");
    int rc = check_nee(params, flags);
    if (rc != RT_OK) return rc;
    if (n_tiles < 0) return errorf(RT_E_INVALID, "n_tiles < 0");
    if (n_tiles == 0) return RT_OK;
    if (!tiles || !d_out) return errorf(RT_E_INVALID, "NULL tiles/out");
    if (tile_size <= 0 || tile_size % 16 != 0) return errorf(RT_E_INVALID, "tile_size must be a positive multiple of 16");
    for (int k = 0; k < n_tiles; ++k) {
        const int tx = tiles[2 * k], ty = tiles[2 * k + 1];
        if (tx < 0 || ty < 0 || tx >= params->width || ty >= params->height)
            return errorf(RT_E_INVALID, "tile %d origin (%d,%d) outside the image", k, tx, ty);
    }
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    const BlockDesc* d_blocks = nullptr;
    int n_blocks = 0;
    rc = ctx_blocks(ctx, tiles, n_tiles, tile_size, params->width, params->height, &d_blocks, &n_blocks);
    if (rc != RT_OK) return rc;
    NeeLaunch a;
    int route = 0;
    rc = nee_launch(scene, cam, params, flags, &a, &route);
    if (rc != RT_OK) return rc;
    a.r.blocks = d_blocks;
    a.r.n_blocks = n_blocks;
    a.r.clip_x1 = params->width;
    a.r.clip_y1 = params->height;
    a.r.out_pitch = tile_size;
    a.r.out = d_out;
    a.r.casts = reinterpret_cast<unsigned long long*>(d_casts);
    a.stats = reinterpret_cast<unsigned long long*>(d_stats);
    rc = ctx_chunks(ctx, &a.r);
    if (rc != RT_OK) return rc;
    e = launch_nee(a, route, (hipStream_t)stream);
    if (e != hipSuccess) return errorf(RT_E_HIP, "rt_render_nee_tiles_device: %s", hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
