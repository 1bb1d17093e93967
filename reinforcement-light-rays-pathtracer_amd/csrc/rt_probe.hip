// rt_probe.hip — ground-truth incident radiance at surface points (rt_probe_radiance in
// rtmi.h).  The thesis judges what a radiance map or a Q-network learned against "the true
// incident radiance distribution", "calculated by firing 4096 sampled light paths per sector
// and averaging their incident radiance approximation"
// (Descriptions/write_up/chapters/4_critical_evaluation.tex:92-110); the reference ships the
// picture, not the code.  Here: for point p on surface tri[p] and sector k of the 12 x 12
// grid, sample s draws a direction inside the sector (the DQN sampler's own cell jitter:
// Philox counter (ids[p] * 144 + k, s, 1, 73)), casts pos + dir * 1e-5 along normalize(dir)
// and follows the GPU preset's path from there (k_render's tail at depth 1: throughput
// (1, 1, 1), bounce events 1 + depth).  The sector's radiance is the mean of the paths'
// values L, its irradiance the mean of L * dot(N, d), both in the project's sum order
// (spp_split chunks summed in sample order, folded in chunk order, / spp).
//
// k_probe: a persistent grid over the launch-wide queue of (point, sector, chunk) items, as
// k_render_pq: a wave claims 64 items per atomic and hands them to its lanes by ballot rank;
// a lane sums its chunk in sample order, stores the two chunk sums and claims the next.
// Item j = (p * 144 + k) * split + c: the lanes of a wave share a point, and neighbouring
// lanes its sector (one candidate-table entry, one cube-map bin).  k_probe_fold adds each
// sector's chunk sums in chunk order and divides by spp.
// The sample's first ray (sector_first_ray), the cast on the route the host picked
// (closest_hit_route; leaving_route in rt_capi.cpp: the same hit, bit for bit, on each) and the
// preset's bounce (surface_step) are rt_paths.hpp's, shared with k_bake and k_sweep.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>

#include "rt_paths.hpp"

namespace rt {
namespace {

constexpr int kProbeSectors = RT_PROBE_SECTORS;
static_assert(kProbeSectors == kDqnActions && kProbeSectors == kDqnGrid * kDqnGrid, "the sampler's 12 x 12 cells");
constexpr uint32_t kProbeMaxId = (uint32_t)(((uint64_t)1 << 32) / kProbeSectors);  // ids below: id * 144 + 143 fits

// Waves per SIMD the launch bounds ask for.  The table route's casts wait on two dependent
// lookups and gain from occupancy, as k_render_pq<.., CT>'s: 6 waves (80 VGPRs) is the most
// the kernel holds without spilling (71-80 used; 8 waves spill 5-75 VGPRs to scratch), 5 for
// the CPU rule's four-word masks (89).  The scan and the BVH are bound by their own loops.
__host__ __device__ constexpr int probe_waves(int route, int rule, int nw) {
    return route != kRouteTable ? 4 : (rule == 0 && nw == 4 ? 5 : 6);
}

struct ProbeLaunch {
    DeviceScene scene;
    const float* pos;     // [n][3]
    const int32_t* tri;   // [n]
    const uint32_t* ids;  // [n]
    int n;
    uint32_t first_sample;
    int spp, split, per_chunk, max_bounces;
    uint32_t seed_lo, seed_hi;
    float t_scale, env_light;
    int use_filter;            // the scene's filter records hold at this t_scale (origins checked per cast)
    float* csum;               // [n * 144 * split][6]: the chunk sums of L and of L * cos
    unsigned long long* work;  // the queue's counter (zeroed by the launcher)
    float* out_rad;            // [n][144][3]
    float* out_irr;            // [n][144][3] or null
    float* out_dir;            // [n][144][3] or null
    unsigned long long* casts;  // accumulated into, or null
};

template <int SAMPLER, int RULE, int ROUTE, int NW>
__global__ __launch_bounds__(256, probe_waves(ROUTE, RULE, NW)) void k_probe(const ProbeLaunch a) {
    __shared__ __attribute__((aligned(16))) float s_mfw[ROUTE == kRouteTable ? 4 * kMfWaveFloats : 1];
    __shared__ int s_stk[ROUTE == kRouteBvh ? kBvhMaxDepth * 256 : 1];
    float* const wl = s_mfw + (ROUTE == kRouteTable ? ((int)threadIdx.x >> 6) * kMfWaveFloats : 0);
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const long long per_point = (long long)kProbeSectors * a.split;
    const long long total = (long long)a.n * per_point;
    long long qb = 0, qe = 0;  // wave-uniform: the wave's claimed, not yet handed out items
    bool exhausted = false;     // wave-uniform: the launch's queue is empty
    bool have = false;          // the lane holds a chunk
    long long item = 0;
    int point = 0, tri0 = 0, sector = 0;
    uint32_t pix = 0, s = 0;
    int left = 0;    // samples of the chunk still to finish, the current one included
    int depth = 1;   // the probed point stands for the path's first surface
    int surf = -1;   // the surface the ray leaves
    float cosn = 0.0f;  // dot(N, d) of the sample's first direction
    f3 o = make3(0.0f, 0.0f, 0.0f), d = make3(0.0f, 0.0f, 1.0f), tp = make3(1.0f, 1.0f, 1.0f);
    f3 acc = make3(0.0f, 0.0f, 0.0f), acci = make3(0.0f, 0.0f, 0.0f);
    unsigned n_casts = 0;
    // the first ray of sample s: the sampler's jittered direction inside the sector
    auto begin = [&](bool first) {
        const float4 N4 = shade[tri0 * kShadeF4 + 0];
        const float4 T4 = shade[tri0 * kShadeF4 + 1];
        const float4 B4 = shade[tri0 * kShadeF4 + 2];
        const f3 N = make3(N4.x, N4.y, N4.z);
        const f3 pos = make3(a.pos[(size_t)point * 3 + 0], a.pos[(size_t)point * 3 + 1], a.pos[(size_t)point * 3 + 2]);
        const f3 dir = sector_first_ray(pix, s, sector, N, make3(T4.x, T4.y, T4.z), make3(B4.x, B4.y, B4.z), pos,
                                        a.seed_lo, a.seed_hi, &o, &d);
        if (first && a.out_dir != nullptr)
            store_rgb(a.out_dir + ((size_t)point * kProbeSectors + sector) * 3, dir.x, dir.y, dir.z);
        cosn = dot(N, d);
        tp = make3(1.0f, 1.0f, 1.0f);
        depth = 1;
        surf = tri0;
    };
    auto finish = [&]() {
        store_rgb(a.csum + (size_t)item * 6, acc.x, acc.y, acc.z);
        store_rgb(a.csum + (size_t)item * 6 + 3, acci.x, acci.y, acci.z);
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
                        const long long p = j / per_point;
                        const int r = (int)(j - p * per_point);
                        sector = r / a.split;
                        const int c = r - sector * a.split;
                        point = (int)p;
                        tri0 = a.tri[p];
                        const uint32_t id = a.ids[p];
                        acc = make3(0.0f, 0.0f, 0.0f);
                        acci = make3(0.0f, 0.0f, 0.0f);
                        // (the host entry refuses such points; a device list's give zeros)
                        const bool ok = tri0 >= 0 && tri0 < n_surf && id < kProbeMaxId;
                        have = true;
                        if (ok) {
                            pix = id * (uint32_t)kProbeSectors + (uint32_t)sector;
                            s = a.first_sample + (uint32_t)(c * a.per_chunk);
                            left = a.per_chunk;
                            begin(c == 0);
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
            acci.x = acci.x + L.x * cosn;
            acci.y = acci.y + L.y * cosn;
            acci.z = acci.z + L.z * cosn;
            ++s;
            if (--left > 0)
                begin(false);
            else
                finish();
        }
    }
    if (a.casts != nullptr) {
        const unsigned tot = wave_sum(n_casts);
        if (lane == 0 && tot != 0u) atomicAdd(a.casts, (unsigned long long)tot);
    }
}

// the sectors of k_probe's launch: chunk sums in chunk order, / spp (k_render's fold)
__global__ __launch_bounds__(256) void k_probe_fold(const ProbeLaunch a) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // point * 144 + sector
    if (q >= (long long)a.n * kProbeSectors) return;
    const float* c = a.csum + (size_t)q * a.split * 6;
    f3 rad = make3(c[0], c[1], c[2]), irr = make3(c[3], c[4], c[5]);
    for (int k = 1; k < a.split; ++k) {
        rad.x = rad.x + c[6 * k + 0];
        rad.y = rad.y + c[6 * k + 1];
        rad.z = rad.z + c[6 * k + 2];
        irr.x = irr.x + c[6 * k + 3];
        irr.y = irr.y + c[6 * k + 4];
        irr.z = irr.z + c[6 * k + 5];
    }
    const float fs = (float)a.spp;
    store_rgb(a.out_rad + (size_t)q * 3, rad.x / fs, rad.y / fs, rad.z / fs);
    if (a.out_irr != nullptr) store_rgb(a.out_irr + (size_t)q * 3, irr.x / fs, irr.y / fs, irr.z / fs);
}

template <int SAMPLER, int RULE>
void launch_probe_t(const ProbeLaunch& a, int route, hipStream_t stream) {
    const long long items = (long long)a.n * kProbeSectors * a.split;
    const long long wanted = (items + 255) / 256;
    const int waves = probe_waves(route, RULE, a.scene.n_tri <= 64 ? 1 : 4);
    const unsigned wgs = (unsigned)std::min<long long>(wanted, (long long)waves * device_cu_count());
    (void)hipMemsetAsync(a.work, 0, sizeof(unsigned long long), stream);
    {
        KernelTimer kt(KT_PROBE, stream);
        if (route == kRouteTable && a.scene.n_tri <= 64)
            hipLaunchKernelGGL((k_probe<SAMPLER, RULE, kRouteTable, 1>), dim3(wgs), dim3(256), 0, stream, a);
        else if (route == kRouteTable)
            hipLaunchKernelGGL((k_probe<SAMPLER, RULE, kRouteTable, 4>), dim3(wgs), dim3(256), 0, stream, a);
        else if (route == kRouteBvh)
            hipLaunchKernelGGL((k_probe<SAMPLER, RULE, kRouteBvh, 1>), dim3(wgs), dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((k_probe<SAMPLER, RULE, kRouteSel, 1>), dim3(wgs), dim3(256), 0, stream, a);
    }
    const long long sectors = (long long)a.n * kProbeSectors;
    hipLaunchKernelGGL(k_probe_fold, dim3((unsigned)((sectors + 255) / 256)), dim3(256), 0, stream, a);
}

hipError_t launch_probe(const ProbeLaunch& a, int sampler, int rule, int route, hipStream_t stream) {
    switch (sampler * 2 + rule) {
        case 0: launch_probe_t<0, 0>(a, route, stream); break;
        case 1: launch_probe_t<0, 1>(a, route, stream); break;
        case 2: launch_probe_t<1, 0>(a, route, stream); break;
        case 3: launch_probe_t<1, 1>(a, route, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The chunk sums and the queue counter of a context's probes, grown on demand and kept
// (one host thread per context: launches of one context share it, in stream order or not
// at all)
struct ProbeWorkspace {
    float* csum = nullptr;
    size_t cap = 0;  // floats
    unsigned long long* work = nullptr;
    ~ProbeWorkspace() {
        if (csum) (void)hipFree(csum);
        if (work) (void)hipFree(work);
    }
};
std::mutex g_ws_mu;
std::map<const rt_ctx*, std::unique_ptr<ProbeWorkspace>> g_ws;
ProbeWorkspace* workspace_for(const rt_ctx* ctx) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto& w = g_ws[ctx];
    if (!w) w.reset(new ProbeWorkspace());
    return w.get();
}

// what both entries check before they look at the point list
int check_probe(const rt_ctx* ctx, const rt_scene* scene, const rt_params* p, int n) {
    const int rc = check_leaving_args(ctx, scene, p, n);
    if (rc != RT_OK) return rc;
    const int split = p->spp_split <= 0 ? 1 : p->spp_split;
    if (p->spp % split != 0) return errorf(RT_E_INVALID, "spp_split %d does not divide spp %d", split, p->spp);
    if (p->max_bounces < 1) return errorf(RT_E_INVALID, "max_bounces must be >= 1 (got %d)", p->max_bounces);
    if (p->sampler != RT_SAMPLER_UNIFORM && p->sampler != RT_SAMPLER_COSINE)
        return errorf(RT_E_INVALID, "bad sampler %d", p->sampler);
    return RT_OK;
}

int probe_device(rt_ctx* ctx, const rt_scene* scene, const rt_params* p, const float* d_pos, const int32_t* d_tri,
                 const uint32_t* d_ids, int n, uint32_t first_sample, float* d_rad, float* d_irr, float* d_dir,
                 uint64_t* d_casts, hipStream_t stream) {
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    ProbeLaunch a;
    const int route = leaving_route(scene, p, &a.scene);
    if (route < 0) return route;
    a.pos = d_pos;
    a.tri = d_tri;
    a.ids = d_ids;
    a.n = n;
    a.first_sample = first_sample;
    a.spp = p->spp;
    a.split = p->spp_split <= 0 ? 1 : p->spp_split;
    a.per_chunk = a.spp / a.split;
    a.max_bounces = p->max_bounces;
    a.seed_lo = (uint32_t)p->seed;
    a.seed_hi = (uint32_t)(p->seed >> 32);
    a.t_scale = p->t_scale;
    a.env_light = p->env_light;
    a.use_filter = filter_usable(a.scene, 0.0f, 0.0f, 0.0f, p->t_scale);
    a.out_rad = d_rad;
    a.out_irr = d_irr;
    a.out_dir = d_dir;
    a.casts = reinterpret_cast<unsigned long long*>(d_casts);
    ProbeWorkspace* ws = workspace_for(ctx);
    const size_t floats = (size_t)n * kProbeSectors * (size_t)a.split * 6;
    if (floats > ws->cap) {
        if (ws->csum) (void)hipFree(ws->csum);  // (waits for the launches that use it)
        ws->csum = nullptr;
        ws->cap = 0;
        e = hipMalloc(&ws->csum, sizeof(float) * floats);
        if (e != hipSuccess) return errorf(RT_E_NOMEM, "rt_probe_radiance: %zu bytes of chunk sums: %s", sizeof(float) * floats, hipGetErrorString(e));
        ws->cap = floats;
    }
    if (!ws->work) {
        e = hipMalloc(&ws->work, sizeof(unsigned long long));
        if (e != hipSuccess) return errorf(RT_E_NOMEM, "rt_probe_radiance: %s", hipGetErrorString(e));
    }
    a.csum = ws->csum;
    a.work = ws->work;
    e = launch_probe(a, p->sampler, p->hit_rule, route, stream);
    if (e != hipSuccess) return errorf(RT_E_HIP, "rt_probe_radiance: %s", hipGetErrorString(e));
    return RT_OK;
}

}  // namespace

void release_probe_workspace(const rt_ctx* ctx) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws.erase(ctx);
}

}  // namespace rt

extern "C" {

int rt_probe_radiance_device(rt_ctx* ctx, const rt_scene* scene, const rt_params* params, const float* d_pos,
                             const int32_t* d_tri, const uint32_t* d_ids, int n, uint32_t first_sample,
                             float* d_rad, float* d_irr, float* d_dir, uint64_t* d_casts, void* stream) {
    const int rc = rt::check_probe(ctx, scene, params, n);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    if (!d_pos) return rt::errorf(RT_E_INVALID, "pos is NULL");
    if (!d_tri) return rt::errorf(RT_E_INVALID, "tri is NULL");
    if (!d_ids) return rt::errorf(RT_E_INVALID, "ids is NULL");
    if (!d_rad) return rt::errorf(RT_E_INVALID, "out_rad is NULL");
    return rt::probe_device(ctx, scene, params, d_pos, d_tri, d_ids, n, first_sample, d_rad, d_irr, d_dir, d_casts,
                            (hipStream_t)stream);
}

int rt_probe_radiance(rt_ctx* ctx, const rt_scene* scene, const rt_params* params, const float* pos,
                      const int32_t* tri, const uint32_t* ids, int n, uint32_t first_sample, float* out_rad,
                      float* out_irr, float* out_dir, uint64_t* out_casts) {
    int rc = rt::check_probe(ctx, scene, params, n);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    if (!pos) return rt::errorf(RT_E_INVALID, "pos is NULL");
    if (!tri) return rt::errorf(RT_E_INVALID, "tri is NULL");
    if (!ids) return rt::errorf(RT_E_INVALID, "ids is NULL");
    if (!out_rad) return rt::errorf(RT_E_INVALID, "out_rad is NULL");
    const int n_surf = rt::scene_launch_view(scene).n_surf;
    for (int p = 0; p < n; ++p) {
        if (tri[p] < 0 || tri[p] >= n_surf)
            return rt::errorf(RT_E_INVALID, "tri[%d] = %d outside [0, %d)", p, tri[p], n_surf);
        if (ids[p] >= rt::kProbeMaxId)
            return rt::errorf(RT_E_INVALID, "ids[%d] = %u: ids * %d must fit 32 bits (ids < %u)", p, ids[p],
                            rt::kProbeSectors, rt::kProbeMaxId);
    }
    hipError_t e = hipSetDevice(rt::ctx_device(ctx));
    if (e != hipSuccess) return rt::errorf(RT_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    float *d_pos = nullptr, *d_rad = nullptr, *d_irr = nullptr, *d_dir = nullptr;
    int32_t* d_tri = nullptr;
    uint32_t* d_ids = nullptr;
    unsigned long long* d_casts = nullptr;
    const size_t b3 = sizeof(float) * 3 * (size_t)n, bo = b3 * rt::kProbeSectors;
    e = hipMalloc(&d_pos, b3);
    if (e == hipSuccess) e = hipMalloc(&d_tri, sizeof(int32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&d_ids, sizeof(uint32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&d_rad, bo);
    if (e == hipSuccess && out_irr) e = hipMalloc(&d_irr, bo);
    if (e == hipSuccess && out_dir) e = hipMalloc(&d_dir, bo);
    if (e == hipSuccess) e = hipMalloc(&d_casts, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_casts, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(d_pos, pos, b3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_tri, tri, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_ids, ids, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice);
    rc = RT_OK;
    if (e == hipSuccess)
        rc = rt::probe_device(ctx, scene, params, d_pos, d_tri, d_ids, n, first_sample, d_rad, d_irr, d_dir,
                              reinterpret_cast<uint64_t*>(d_casts), 0);
    if (rc == RT_OK && e == hipSuccess) e = hipDeviceSynchronize();
    if (rc == RT_OK && e == hipSuccess) e = hipMemcpy(out_rad, d_rad, bo, hipMemcpyDeviceToHost);
    if (rc == RT_OK && e == hipSuccess && out_irr) e = hipMemcpy(out_irr, d_irr, bo, hipMemcpyDeviceToHost);
    if (rc == RT_OK && e == hipSuccess && out_dir) e = hipMemcpy(out_dir, d_dir, bo, hipMemcpyDeviceToHost);
    unsigned long long casts = 0;
    if (rc == RT_OK && e == hipSuccess) e = hipMemcpy(&casts, d_casts, sizeof(casts), hipMemcpyDeviceToHost);
    (void)hipFree(d_pos);
    (void)hipFree(d_tri);
    (void)hipFree(d_ids);
    (void)hipFree(d_rad);
    (void)hipFree(d_irr);
    (void)hipFree(d_dir);
    (void)hipFree(d_casts);
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return rt::errorf(RT_E_HIP, "rt_probe_radiance: %s", hipGetErrorString(e));
    if (out_casts) *out_casts = casts;
    return RT_OK;
}

}  // extern "C"
