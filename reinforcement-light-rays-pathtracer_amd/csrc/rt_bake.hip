// rt_bake.hip — fill a radiance map's volumes from ground truth (rt_sarsa_bake in rtmi.h).
// The reference's CPU engine samples the incoming radiance of every sector when it builds its
// map (Old_CPU_Rendering_Engine/Source/radiance_volumes/radiance_map.cpp, radiance_volume.cpp)
// and then importance-samples it with no learning step; here the same for the GPU engine's
// 12 x 12 scalar grid.  For volume v and sector k, rad is what rt_probe_radiance (rt_probe.hip)
// gives for the point {pos = the volume's position, tri = its surface, ids = v}: sample s draws
// the DQN sampler's jittered direction of the sector (Philox counter (v * 144 + k, s, 1, 73)),
// and the GPU preset's path follows from depth 1; spp_split chunks summed in sample order,
// folded in chunk order, / spp.  Then
//   Q[v][k] = max(vol_brdf[v] * ((rad.r + rad.g) + rad.b) / 3, RADIANCE_THRESHOLD)   (NaN: the floor)
//   visits[v][k] = spp, the sector's pending TD sum and count = 0,
// the volume's irradiance estimate as rt_sarsa_load_q recomputes it (initialise_radiance_grid:
// double products summed into a float, in sector order) and its CDF, row ends and arg-max as
// rebuild_volume does (rt_sarsa.hip).
//
// The frame: a volume's sectors are laid out in normal_frame(N) of its surface normal N
// (rt_sarsa_host.cpp, rt_sarsa_create_density), the probe's in the scene's shading frame of the
// surface (rt_capi.cpp: normal_frame of the same stored normal), both with sector k = x * 12 + y
// through grid_direction: the probe's sector k is the volume's sector k, and both read the
// scene's frame.
//
// k_bake: a persistent grid over the launch-wide queue of (volume, sector, chunk) items (a wave
// claims 64 items per atomic and hands them to its lanes by ballot rank).  The sample's first ray
// (sector_first_ray), the cast on the route the host picked (closest_hit_route; leaving_route in
// rt_capi.cpp: the same hit, bit for bit, on each) and the preset's bounce (surface_step) are
// rt_paths.hpp's, shared with k_probe and k_sweep.  It keeps three chunk sums per item, reads
// positions and surfaces from the map, writes no rad / irr / dir arrays, and the result
// stays on the device: k_bake_fold (one lane per sector: fold, luminance, floor, visits),
// k_bake_irradiance (one lane per volume) and the ranged rebuild.  The entry walks its range in
// batches of a bounded chunk-sum workspace; a volume's result depends on neither the batching,
// v0, n nor the route.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "rt_paths.hpp"

namespace rt {
namespace {

static_assert(kSarsaSectors == kDqnActions && kSarsaSectors == kDqnGrid * kDqnGrid && kDqnGrid == kGridRes, "the map's sectors are the sampler's 12 x 12 cells");
// (volume * 144 + 143 fits 32 bits: maps hold at most 2^24 volumes, rt_sarsa_create_density)
constexpr float kRadianceThreshold = (1.f / ((float)kGridRes * (float)kGridRes)) * 0.8f;  // RADIANCE_THRESHOLD
constexpr size_t kBakeBatchFloats = (size_t)1 << 26;  // the chunk-sum workspace of one batch: 256 MiB

// Waves per SIMD the launch bounds ask for: k_probe's (rt_probe.hip probe_waves), whose path
// loop this is.  The table route's casts wait on two dependent lookups and gain from occupancy;
// the scan and the BVH are bound by their own loops.
__host__ __device__ constexpr int bake_waves(int route, int rule, int nw) {
    return route != kRouteTable ? 4 : (rule == 0 && nw == 4 ? 5 : 6);
}

struct BakeLaunch {
    DeviceScene scene;
    const float4* vol_pos;    // [n_vol] the map's volume positions
    const int32_t* vol_surf;  // [n_vol] and surfaces
    int v0, n;                // the batch: volumes [v0, v0 + n)
    uint32_t first_sample;
    int spp, split, per_chunk, max_bounces;
    uint32_t seed_lo, seed_hi;
    float t_scale, env_light;
    int use_filter;            // the scene's filter records hold at this t_scale (origins checked per cast)
    float* csum;               // [n * 144 * split][3]: the chunk sums of L
    unsigned long long* work;  // the queue's counter (zeroed by the launcher)
    unsigned long long* casts;  // accumulated into
};

template <int SAMPLER, int RULE, int ROUTE, int NW>
__global__ __launch_bounds__(256, bake_waves(ROUTE, RULE, NW)) void k_bake(const BakeLaunch a) {
    __shared__ __attribute__((aligned(16))) float s_mfw[ROUTE == kRouteTable ? 4 * kMfWaveFloats : 1];
    __shared__ int s_stk[ROUTE == kRouteBvh ? kBvhMaxDepth * 256 : 1];
    float* const wl = s_mfw + (ROUTE == kRouteTable ? ((int)threadIdx.x >> 6) * kMfWaveFloats : 0);
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const long long per_vol = (long long)kSarsaSectors * a.split;
    const long long total = (long long)a.n * per_vol;
    long long qb = 0, qe = 0;  // wave-uniform: the wave's claimed, not yet handed out items
    bool exhausted = false;     // wave-uniform: the launch's queue is empty
    bool have = false;          // the lane holds a chunk
    long long item = 0;
    int vol = 0, tri0 = 0, sector = 0;
    uint32_t pix = 0, s = 0;
    int left = 0;   // samples of the chunk still to finish, the current one included
    int depth = 1;  // the volume stands for the path's first surface
    int surf = -1;  // the surface the ray leaves
    f3 o = make3(0.0f, 0.0f, 0.0f), d = make3(0.0f, 0.0f, 1.0f), tp = make3(1.0f, 1.0f, 1.0f);
    f3 acc = make3(0.0f, 0.0f, 0.0f);
    unsigned n_casts = 0;
    // the first ray of sample s: the sampler's jittered direction inside the sector
    auto begin = [&]() {
        const float4 N4 = shade[tri0 * kShadeF4 + 0];
        const float4 T4 = shade[tri0 * kShadeF4 + 1];
        const float4 B4 = shade[tri0 * kShadeF4 + 2];
        const float4 P4 = a.vol_pos[vol];
        const f3 pos = make3(P4.x, P4.y, P4.z);
        sector_first_ray(pix, s, sector, make3(N4.x, N4.y, N4.z), make3(T4.x, T4.y, T4.z), make3(B4.x, B4.y, B4.z), pos,
                         a.seed_lo, a.seed_hi, &o, &d);
        tp = make3(1.0f, 1.0f, 1.0f);
        depth = 1;
        surf = tri0;
    };
    auto finish = [&]() {
        store_rgb(a.csum + (size_t)item * 3, acc.x, acc.y, acc.z);
        have = false;
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
                    if (lane == 0) v = atomicAdd(a.work, 64ull);
                    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
                    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                    nb = (long long)(((unsigned long long)hi << 32) | lo);
                }
                if (!have) {
                    const long long j = rank < avail ? qb + rank : nb + (rank - avail);
                    if (j < total) {
                        item = j;
                        const long long p = j / per_vol;
                        const int r = (int)(j - p * per_vol);
                        sector = r / a.split;
                        const int c = r - sector * a.split;
                        vol = a.v0 + (int)p;
                        tri0 = a.vol_surf[vol];
                        acc = make3(0.0f, 0.0f, 0.0f);
                        // (a volume lies on a surface of the scene its map was made for; another
                        // scene's surface count is checked by the entry, and here again)
                        const bool ok = tri0 >= 0 && tri0 < n_surf;
                        have = true;
                        if (ok) {
                            pix = (uint32_t)vol * (uint32_t)kSarsaSectors + (uint32_t)sector;
                            s = a.first_sample + (uint32_t)(c * a.per_chunk);
                            left = a.per_chunk;
                            begin();
                        }
                        // depth 1 == max_bounces before the cast: every path ends with 0
                        if (!ok || a.max_bounces <= 1) finish();
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
            continue;  // (every claimed item ended without a cast)
        }
        const Hit h = closest_hit_route<RULE, ROUTE, NW>(a.scene, a.use_filter, surf, o, d, a.t_scale, active, wl,
                                                         ROUTE == kRouteBvh ? s_stk + threadIdx.x : nullptr);
        if (!active) continue;
        ++n_casts;
        bool terminal = false;
        f3 L = make3(0.0f, 0.0f, 0.0f);
        if (h.tri < 0) {
            terminal = true;
            L = make3(tp.x * a.env_light, tp.y * a.env_light, tp.z * a.env_light);
        } else if (h.tri >= n_surf) {
            terminal = true;
            const float4 e = shade[h.tri * kShadeF4 + 3];
            L = make3(tp.x * e.x, tp.y * e.y, tp.z * e.z);
        } else {
            surf = surface_step<SAMPLER>(h, o, d, tp, a.t_scale, shade, pix, s, depth, a.seed_lo, a.seed_hi);
            ++depth;
            if (depth == a.max_bounces) terminal = true;  // loop exhausted -> 0
        }
        if (terminal) {
            acc.x = acc.x + L.x;
            acc.y = acc.y + L.y;
            acc.z = acc.z + L.z;
            ++s;
            if (--left > 0)
                begin();
            else
                finish();
        }
    }
    const unsigned tot = wave_sum(n_casts);
    if (lane == 0 && tot != 0u) atomicAdd(a.casts, (unsigned long long)tot);
}

// one lane per (volume, sector) of the batch: the chunk sums in chunk order, / spp (k_probe_fold's
// rad), then the sector's Q, visits and cleared TD accumulators
__global__ __launch_bounds__(256) void k_bake_fold(const BakeLaunch a, const SarsaMap m) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // volume of the batch * 144 + sector
    if (q >= (long long)a.n * kSarsaSectors) return;
    const float* c = a.csum + (size_t)q * a.split * 3;
    f3 rad = make3(c[0], c[1], c[2]);
    for (int k = 1; k < a.split; ++k) {
        rad.x = rad.x + c[3 * k + 0];
        rad.y = rad.y + c[3 * k + 1];
        rad.z = rad.z + c[3 * k + 2];
    }
    const float fs = (float)a.spp;
    rad = make3(rad.x / fs, rad.y / fs, rad.z / fs);
    const int v = a.v0 + (int)(q / kSarsaSectors);
    const size_t e = (size_t)a.v0 * kSarsaSectors + (size_t)q;
    const float lum = ((rad.x + rad.y) + rad.z) / 3.0f;
    const float val = m.vol_brdf[v] * lum;
    m.Q[e] = val > kRadianceThreshold ? val : kRadianceThreshold;
    m.visits[e] = (uint32_t)a.spp;
    m.acc_sum[e] = 0ull;
    m.acc_cnt[e] = 0u;
}

// one lane per volume of the batch: rt_sarsa_load_q's irradiance estimate of the new Q
// (rt_sarsa_host.cpp initial_irradiance, the same operations in the same order)
__global__ __launch_bounds__(256) void k_bake_irradiance(const BakeLaunch a, const SarsaMap m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int v = a.v0 + i;
    const size_t b = (size_t)v * kSarsaSectors;
    const float lum = m.tri_lum[a.vol_surf[v]];
    float irr = 0.f;
    for (int k = 0; k < kSarsaSectors; ++k)
        irr = (float)((double)irr + ((double)m.cos_center[b + k] * ((double)lum / M_PI)) * (double)m.Q[b + k]);
    m.accum[v] = irr;
}

template <int SAMPLER, int RULE>
void launch_bake_t(const BakeLaunch& a, int route, hipStream_t stream) {
    const long long items = (long long)a.n * kSarsaSectors * a.split;
    const long long wanted = (items + 255) / 256;
    const int waves = bake_waves(route, RULE, a.scene.n_tri <= 64 ? 1 : 4);
    const unsigned wgs = (unsigned)std::min<long long>(wanted, (long long)waves * device_cu_count());
    (void)hipMemsetAsync(a.work, 0, sizeof(unsigned long long), stream);
    KernelTimer kt(KT_BAKE, stream);
    if (route == kRouteTable && a.scene.n_tri <= 64)
        hipLaunchKernelGGL((k_bake<SAMPLER, RULE, kRouteTable, 1>), dim3(wgs), dim3(256), 0, stream, a);
    else if (route == kRouteTable)
        hipLaunchKernelGGL((k_bake<SAMPLER, RULE, kRouteTable, 4>), dim3(wgs), dim3(256), 0, stream, a);
    else if (route == kRouteBvh)
        hipLaunchKernelGGL((k_bake<SAMPLER, RULE, kRouteBvh, 1>), dim3(wgs), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((k_bake<SAMPLER, RULE, kRouteSel, 1>), dim3(wgs), dim3(256), 0, stream, a);
}

// one batch: the paths, then the device-side finish of its volumes
hipError_t launch_bake(const BakeLaunch& a, const SarsaMap& m, int sampler, int rule, int route, hipStream_t stream) {
    switch (sampler * 2 + rule) {
        case 0: launch_bake_t<0, 0>(a, route, stream); break;
        case 1: launch_bake_t<0, 1>(a, route, stream); break;
        case 2: launch_bake_t<1, 0>(a, route, stream); break;
        case 3: launch_bake_t<1, 1>(a, route, stream); break;
        default: return hipErrorInvalidValue;
    }
    const long long sectors = (long long)a.n * kSarsaSectors;
    hipLaunchKernelGGL(k_bake_fold, dim3((unsigned)((sectors + 255) / 256)), dim3(256), 0, stream, a, m);
    hipLaunchKernelGGL(k_bake_irradiance, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a, m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sarsa_rebuild_range(m, a.v0, a.n, stream);
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_sarsa_bake(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sa, const rt_params* p, int v0, int n,
                  uint32_t first_sample, uint64_t* out_casts, void* stream_) {
    using namespace rt;
    if (ctx && scene && !sa) return errorf(RT_E_INVALID, "sarsa is NULL");  // (after ctx and scene, before params)
    int rc = check_leaving_args(ctx, scene, p, n);
    if (rc != RT_OK) return rc;
    const int split = p->spp_split <= 0 ? 1 : p->spp_split;
    if (p->spp % split != 0) return errorf(RT_E_INVALID, "spp_split %d does not divide spp %d", split, p->spp);
    if (p->max_bounces < 1) return errorf(RT_E_INVALID, "max_bounces must be >= 1 (got %d)", p->max_bounces);
    if (p->sampler != RT_SAMPLER_UNIFORM && p->sampler != RT_SAMPLER_COSINE)
        return errorf(RT_E_INVALID, "bad sampler %d", p->sampler);
    if (p->preset != RT_PRESET_GPU)
        return errorf(RT_E_UNSUPPORTED, "rt_sarsa_bake follows the GPU-engine preset's path (got preset %d)", p->preset);
    const int n_vol = sarsa_n_volumes(sa);
    if (v0 < 0 || n > n_vol - v0)
        return errorf(RT_E_INVALID, "volumes [%d, %lld) outside the map's [0, %d)", v0, (long long)v0 + n, n_vol);
    if (sarsa_device(sa) != ctx_device(ctx)) return errorf(RT_E_INVALID, "radiance map belongs to another device");
    if (n == 0) {
        if (out_casts) *out_casts = 0;
        return RT_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    BakeLaunch a;
    const int route = leaving_route(scene, p, &a.scene);
    if (route < 0) return route;
    const size_t per_vol = (size_t)kSarsaSectors * (size_t)split * 3;
    const int batch = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, kBakeBatchFloats / per_vol));
    SarsaBakeView view;
    rc = sarsa_bake_view(sa, (size_t)batch * per_vol, &view);
    if (rc != RT_OK) return rc;
    a.vol_pos = view.m.vol_pos;
    a.vol_surf = view.vol_surf;
    a.first_sample = first_sample;
    a.spp = p->spp;
    a.split = split;
    a.per_chunk = a.spp / a.split;
    a.max_bounces = p->max_bounces;
    a.seed_lo = (uint32_t)p->seed;
    a.seed_hi = (uint32_t)(p->seed >> 32);
    a.t_scale = p->t_scale;
    a.env_light = p->env_light;
    a.use_filter = filter_usable(a.scene, 0.0f, 0.0f, 0.0f, p->t_scale);
    a.csum = view.csum;
    a.work = view.work;
    a.casts = view.work + 1;
    e = hipMemsetAsync(a.casts, 0, sizeof(unsigned long long), stream);
    for (int b0 = 0; e == hipSuccess && b0 < n; b0 += batch) {
        a.v0 = v0 + b0;
        a.n = std::min(batch, n - b0);
        e = launch_bake(a, view.m, p->sampler, p->hit_rule, route, stream);
    }
    if (e != hipSuccess) return errorf(RT_E_HIP, "rt_sarsa_bake: %s", hipGetErrorString(e));
    if (out_casts) {
        unsigned long long casts = 0;
        e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = hipMemcpy(&casts, a.casts, sizeof(casts), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return errorf(RT_E_HIP, "rt_sarsa_bake: %s", hipGetErrorString(e));
        *out_casts = casts;
    }
    return RT_OK;
}

}  // extern "C"
