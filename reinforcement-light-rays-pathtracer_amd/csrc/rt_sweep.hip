// rt_sweep.hip — expected-value sweeps of a radiance map (rt_sarsa_sweep in rtmi.h).
// The Expected-SARSA target of a sector is one cast long: the emitted light, or the irradiance
// estimate the map holds at the point the cast lands on.  The render forms it along camera paths
// (rt_sarsa.hip sarsa_step); here it is formed from every volume's own position, which is value
// iteration over the map: for volume v, sector k and sample s
//   the first ray of rt_sarsa_bake's (v, k, s)  (sector_first_ray, rt_paths.hpp: Philox counter
//     (v * 144 + k, s, 1, 73), grid_direction in the surface's shading frame, o = pos + dir * 1e-5f,
//     d = normalize(dir)),
//   one closest hit under the hit rule and t_scale, on the route leaving_route picks
//     (closest_hit_route, rt_paths.hpp: the same hit, bit for bit, on each),
//   target = brdf * env_light (miss), brdf * tri_lum[hit] (light), (accum[u] * kIrrScale) * brdf
//     (surface), brdf = vol_brdf[v], u = the nearest volume the render finds for the hit point
//     o + t * (d * t_scale) with the hit surface's stored normal (the map's search mode),
//   and __float2ll_rn(target * 2^32) joins acc_sum[v * 144 + k], 1 joins acc_cnt[v * 144 + k]:
// the pending sums a tile render leaves with apply = 0, folded by k_sarsa_apply (rt_sarsa.hip).
// The kernel reads accum and writes the pending sums only, so a sweep never sees its own
// results (Jacobi).
//
// k_sweep: every item has the same trip count -- one cast per sample -- so there is no path loop
// and no queue: lane g of the launch is item (volume, chunk, sector) = (g / (144 chunks),
// g / 144 % chunks, g % 144), consecutive lanes on consecutive sectors of one volume, and runs
// the samples of its chunk.  Every lane of a wave stays for all per_chunk trips (the table
// route's exact phase and sarsa_resolve_walks are wave-cooperative, as in k_sarsa_view); a lane
// past the end of the range or of its chunk casts nothing and searches nothing.  A lane sums its
// chunk's fixed-point targets in a 64-bit register and deposits once, one 64-bit and one 32-bit
// atomic per item.  Integer sums are order-free: the chunking (chosen by the launcher from the
// size of the range) is not part of the result.  The k-d stack block of the search is the one
// LDS array of the kernel: between searches it serves the table route's exact phase and the
// BVH route's stack (as in k_sarsa_render_pq).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_paths.hpp"
#include "rt_sarsa_search.hpp"

namespace rt {
namespace {

static_assert(kSarsaSectors == kDqnActions && kSarsaSectors == kDqnGrid * kDqnGrid && kDqnGrid == kGridRes,
              "the map's sectors are the sampler's 12 x 12 cells");

// Waves per SIMD the launch bounds ask for.  The stack block (30 KB per workgroup) lets five
// workgroups share a CU; the BVH traversal's state wants the registers of four (k_sarsa_render_pq).
__host__ __device__ constexpr int sweep_waves(int route) { return route == kRouteBvh ? 4 : 5; }

struct SweepLaunch {
    DeviceScene scene;
    const int32_t* vol_surf;  // [n_vol] the surface each volume lies on
    int v0, n;                // volumes [v0, v0 + n)
    uint32_t first_sample;
    int spp, chunks, per_chunk;  // chunk c runs samples [c * per_chunk, min(spp, (c + 1) * per_chunk))
    uint32_t seed_lo, seed_hi;
    float t_scale, env_light;
    int use_filter;             // the scene's filter records hold at this t_scale (origins checked per cast)
    unsigned long long* casts;  // accumulated into
};

template <int RULE, int ROUTE, int NW>
__global__ __launch_bounds__(256, sweep_waves(ROUTE)) void k_sweep(const SweepLaunch a, const SarsaMap m) {
    __shared__ __attribute__((aligned(16))) int kd_stack[kKdStack * 256];
    static_assert(kKdStack * 64 >= kMfWaveFloats, "the exact phase's LDS fits a wave's stack block");
    static_assert(kKdStack >= kBvhMaxDepth, "the BVH stack fits the k-d stack column");
    int* const st = kd_stack_of(kd_stack);
    int* const blk_ws = kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64);  // the wave's block
    float* const wl = reinterpret_cast<float*>(blk_ws);
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const long long per_vol = (long long)kSarsaSectors * a.chunks;
    const long long total = (long long)a.n * per_vol;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g - lane >= total) return;  // (whole waves past the end)
    int vol = 0, sector = 0, tri0 = -1, count = 0;
    uint32_t s0 = a.first_sample;
    if (g < total) {
        const long long p = g / per_vol;
        const int r = (int)(g - p * per_vol);
        const int c = r / kSarsaSectors;
        sector = r - c * kSarsaSectors;
        vol = a.v0 + (int)p;
        tri0 = a.vol_surf[vol];
        // (a volume lies on a surface of the scene its map was made for; another scene's
        // surface is checked here: such a lane deposits nothing)
        if (tri0 >= 0 && tri0 < n_surf) {
            count = min(a.per_chunk, a.spp - c * a.per_chunk);
            count = count > 0 ? count : 0;
            s0 = a.first_sample + (uint32_t)(c * a.per_chunk);
        }
    }
    const uint32_t pix = (uint32_t)vol * (uint32_t)kSarsaSectors + (uint32_t)sector;
    f3 N = make3(0.f, 0.f, 1.f), T = make3(1.f, 0.f, 0.f), B = make3(0.f, 1.f, 0.f), vpos = make3(0.f, 0.f, 0.f);
    float brdf = 0.0f;
    if (count > 0) {
        const float4 N4 = shade[tri0 * kShadeF4 + 0];
        const float4 T4 = shade[tri0 * kShadeF4 + 1];
        const float4 B4 = shade[tri0 * kShadeF4 + 2];
        const float4 P4 = m.vol_pos[vol];
        N = make3(N4.x, N4.y, N4.z);
        T = make3(T4.x, T4.y, T4.z);
        B = make3(B4.x, B4.y, B4.z);
        vpos = make3(P4.x, P4.y, P4.z);
        brdf = m.vol_brdf[vol];
    }
    long long sum = 0;  // the chunk's targets, fixed point 2^-32
    for (int k = 0; k < a.per_chunk; ++k) {
        const bool active = k < count;
        f3 o = vpos, d = make3(0.f, 0.f, 1.f);
        if (active) sector_first_ray(pix, s0 + (uint32_t)k, sector, N, T, B, vpos, a.seed_lo, a.seed_hi, &o, &d);
        // (the table route's exact phase shares the stack block with the searches: the previous
        // search's stack accesses stay before it, and its LDS traffic before the next search)
        if constexpr (ROUTE == kRouteTable) wave_lds_sync();
        const Hit h = closest_hit_route<RULE, ROUTE, NW, 64>(a.scene, a.use_filter, tri0, o, d, a.t_scale, active, wl, st);
        if constexpr (ROUTE == kRouteTable) wave_lds_sync();
        // the nearest volume of a surface hit, as k_sarsa_render_pq searches it
        const bool is_surf = active && (h.tri >= 0) && (h.tri < n_surf);
        f3 pos = o;
        f3 nrm = make3(0.f, 0.f, 0.f);
        if (is_surf) {
            const float Dx = d.x * a.t_scale, Dy = d.y * a.t_scale, Dz = d.z * a.t_scale;
            pos = make3(o.x + h.t * Dx, o.y + h.t * Dy, o.z + h.t * Dz);
            const float4 N4 = shade[h.tri * kShadeF4 + 0];
            nrm = make3(N4.x, N4.y, N4.z);
        }
        int rv = -1;
        if (is_surf) rv = m.use_grid ? sarsa_nearest_grid_tri(m, h.tri, pos, nrm) : kNeedWalk;
        if (m.use_grid)  // the whole wave, with or without a query
            sarsa_resolve_walks(m, pos, nrm, &rv, blk_ws, st, lane);
        else if (rv == kNeedWalk)
            rv = sarsa_nearest(m, pos, nrm, st);
        if (active) {
            // sarsa_step's target (rt_sarsa.hip), cur_brdf = the volume's
            float target;
            if (h.tri < 0)
                target = brdf * a.env_light;
            else if (!is_surf)
                target = brdf * m.tri_lum[h.tri];
            else
                target = (m.accum[rv] * kIrrScale) * brdf;
            sum += __float2ll_rn(target * 4294967296.0f);  // td_event's fixed point
        }
    }
    if (count > 0) {
        const size_t e = (size_t)vol * kSarsaSectors + (size_t)sector;
        atomicAdd(&m.acc_sum[e], (unsigned long long)sum);
        atomicAdd(&m.acc_cnt[e], (uint32_t)count);
    }
    const unsigned tot = wave_sum((unsigned)count);
    if (lane == 0 && tot != 0u) atomicAdd(a.casts, (unsigned long long)tot);
}

template <int RULE>
void launch_sweep_t(const SweepLaunch& a, const SarsaMap& m, int route, hipStream_t stream) {
    const long long items = (long long)a.n * kSarsaSectors * a.chunks;
    const unsigned wgs = (unsigned)((items + 255) / 256);
    KernelTimer kt(KT_BAKE, stream);
    if (route == kRouteTable && a.scene.n_tri <= 64)
        hipLaunchKernelGGL((k_sweep<RULE, kRouteTable, 1>), dim3(wgs), dim3(256), 0, stream, a, m);
    else if (route == kRouteTable)
        hipLaunchKernelGGL((k_sweep<RULE, kRouteTable, 4>), dim3(wgs), dim3(256), 0, stream, a, m);
    else if (route == kRouteBvh)
        hipLaunchKernelGGL((k_sweep<RULE, kRouteBvh, 1>), dim3(wgs), dim3(256), 0, stream, a, m);
    else
        hipLaunchKernelGGL((k_sweep<RULE, kRouteSel, 1>), dim3(wgs), dim3(256), 0, stream, a, m);
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_sarsa_sweep(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sa, const rt_params* p, int v0, int n,
                   uint32_t first_sample, int apply, uint64_t* out_casts, void* stream_) {
    using namespace rt;
    // (spp_split, max_bounces and sampler are not used: not checked)
    if (ctx && scene && !sa) return errorf(RT_E_INVALID, "sarsa is NULL");  // (after ctx and scene, before params)
    int rc = check_leaving_args(ctx, scene, p, n);
    if (rc != RT_OK) return rc;
    if (p->preset != RT_PRESET_GPU)
        return errorf(RT_E_UNSUPPORTED, "rt_sarsa_sweep casts the GPU-engine preset's rays (got preset %d)", p->preset);
    const int n_vol = sarsa_n_volumes(sa);
    if (v0 < 0 || n > n_vol - v0)
        return errorf(RT_E_INVALID, "volumes [%d, %lld) outside the map's [0, %d)", v0, (long long)v0 + n, n_vol);
    if (sarsa_device(sa) != ctx_device(ctx)) return errorf(RT_E_INVALID, "radiance map belongs to another device");
    SarsaSweepView view;
    rc = sarsa_sweep_view(sa, &view);  // (refuses a map that is not in RT_SARSA_TD_FRAME)
    if (rc != RT_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) {
        if (out_casts) *out_casts = 0;
        if (apply) return rt_sarsa_apply(sa, stream_);
        return RT_OK;
    }
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    SweepLaunch a;
    const int route = leaving_route(scene, p, &a.scene);
    if (route < 0) return route;
    a.vol_surf = view.vol_surf;
    a.v0 = v0;
    a.n = n;
    a.first_sample = first_sample;
    a.spp = p->spp;
    // a small range is cut into chunks of samples until the launch fills the device twice over;
    // a large one keeps a sector's samples on one lane (one deposit per sector)
    const long long sectors = (long long)n * kSarsaSectors;
    const long long fill = 2ll * sweep_waves(route) * 256 * device_cu_count();
    a.chunks = (int)std::max<long long>(1, std::min<long long>(p->spp, (fill + sectors - 1) / sectors));
    a.per_chunk = (a.spp + a.chunks - 1) / a.chunks;
    a.chunks = (a.spp + a.per_chunk - 1) / a.per_chunk;  // (no chunk without a sample)
    a.seed_lo = (uint32_t)p->seed;
    a.seed_hi = (uint32_t)(p->seed >> 32);
    a.t_scale = p->t_scale;
    a.env_light = p->env_light;
    a.use_filter = filter_usable(a.scene, 0.0f, 0.0f, 0.0f, p->t_scale);
    a.casts = view.casts;
    e = hipMemsetAsync(a.casts, 0, sizeof(unsigned long long), stream);
    if (e == hipSuccess) {
        if (p->hit_rule == RT_HIT_RULE_CPU)
            launch_sweep_t<0>(a, view.m, route, stream);
        else
            launch_sweep_t<1>(a, view.m, route, stream);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return errorf(RT_E_HIP, "rt_sarsa_sweep: %s", hipGetErrorString(e));
    if (apply) {
        rc = rt_sarsa_apply(sa, stream_);
        if (rc != RT_OK) return rc;
    }
    if (out_casts) {
        unsigned long long casts = 0;
        e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = hipMemcpy(&casts, a.casts, sizeof(casts), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return errorf(RT_E_HIP, "rt_sarsa_sweep: %s", hipGetErrorString(e));
        *out_casts = casts;
    }
    return RT_OK;
}

}  // extern "C"
