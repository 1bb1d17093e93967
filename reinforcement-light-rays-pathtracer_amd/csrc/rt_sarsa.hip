// rt_sarsa.hip — Expected-SARSA radiance-volume path tracer (BASELINE config 3).
//
// Reference: GPU/path_tracing/reinforcement_path_tracing.cu:6-120 (render
// kernel, per-frame distribution update), GPU/radiance_volumes/radiance_map.cu
// (:90-146 sampling + TD update dispatch, :149-203 nearest volume),
// GPU/radiance_volumes/radiance_volume.cu (:93-112 expected_sarsa_irradiance,
// :148-188 update_radiance_distribution, :191-244 CDF sampling,
// :282-307 temporal_difference_update, irradiance estimate).
//
// Determinism: the reference updates the Q-table racily while
// it renders (non-atomic read-modify-write + atomicExch).  Here a frame reads
// the Q-table, irradiance and CDFs of the previous frame, and every TD target
// is added to a per-(volume, sector) fixed-point sum (2^-32 units, integer
// atomics: order-independent) with a visit count; k_sarsa_apply then folds
// the frame's targets into Q in closed form — the running mean that
// alpha = 1/(1 + visits) produces — and rebuilds the CDFs.  Same frames, same
// seed: bit-identical Q-table and image on any GPU count, and against oracle/.
#include <float.h>

#include "rt_trace.hpp"
// the nearest-volume search (sarsa_nearest*, sarsa_resolve_walks), shared with
// rt_views.hip (the read-only views and queries of the map) and rt_sweep.hip
#include "rt_sarsa_search.hpp"

#ifndef RT_SARSA_PROF
#define RT_SARSA_PROF 0  // 1: k_sarsa_render_pq sums per-phase s_memtime cycles into SarsaMap::prof (timing builds)
#endif

namespace rt {

namespace {

constexpr float kGridRhoS = 1.0f / ((float)kGridRes * (float)kGridRes);             // GRID_RHO
constexpr float kRadianceThreshold = (1.f / ((float)kGridRes * (float)kGridRes)) * 0.8f;  // RADIANCE_THRESHOLD
constexpr float kThroughputThreshold = 0.0001f;  // THROUGHPUT_THRESHOLD (constants/monte_carlo_settings.h:11)

// The sampling volume's per-frame data, loaded as soon as the volume is known (sarsa_step):
// its CDF row ends (one 64-B line) and its frame (N, T, B with the position)
struct VolPre {
    float4 t0, t1, t2, t3;
    float4 N4, T4, B4;
};
__device__ __forceinline__ VolPre vol_load(const SarsaMap& m, int rv) {
    VolPre v;
    const float4* tp = m.cdf_top + (size_t)rv * 4;
    v.t0 = tp[0];
    v.t1 = tp[1];
    v.t2 = tp[2];
    v.t3 = tp[3];
    v.N4 = m.vol_frame[rv * 3 + 0];
    v.T4 = m.vol_frame[rv * 3 + 1];
    v.B4 = m.vol_frame[rv * 3 + 2];
    return v;
}

// sample_direction_from_radiance_distribution (radiance_volume.cu:191-244); vp: vol_load(m, rv)
__device__ bool sarsa_sample(const SarsaMap& m, int rv, const VolPre& vp, float r, float rx, float ry, int* sector,
                             f3* dir, float* pdf) {
    const float* __restrict__ cdf = m.cdf + (size_t)rv * kSarsaSectors;
    int found = -1;
    float mv = 0.0f, pv = 0.0f;
    // The CDF is non-decreasing, so the reference's binary search returns i0, the first
    // sector with cdf > r, unless one of its probes meets cdf[k] == r (it then turns
    // left of i0 and fails), which requires cdf[i0 - 1] == r.  i0 from two rounds of
    // independent loads (the 12 row ends, then one 12-sector row) instead of 8
    // dependent probes; the rare equal / NaN cases run the search itself.
    bool exact = false;
    const float4 t0 = vp.t0, t1 = vp.t1, t2 = vp.t2, t3 = vp.t3;  // one 64-B line: cdf[0] and the row ends
    const float c0 = t0.x;
    if (r <= c0) {
        found = 0;
        mv = c0;
    } else {
        const float top[kGridRes] = {t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, t3.x};
        int row = 0;
        bool nan = false;
#pragma unroll
        for (int x = 0; x < kGridRes; ++x) {
            row += (top[x] <= r) ? 1 : 0;
            nan |= (top[x] != top[x]);
        }
        if (row < kGridRes && !nan) {
            const float4* rp = reinterpret_cast<const float4*>(cdf + row * kGridRes);
            const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2];
            const float v[kGridRes] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            int j = 0;
            float prev = (row > 0) ? top[row - 1] : 0.0f;
#pragma unroll
            for (int k = 0; k < kGridRes; ++k) {
                const bool le = v[k] <= r;
                j += le ? 1 : 0;
                prev = le ? v[k] : prev;
                nan |= (v[k] != v[k]);
            }
            // j < 12: the row's last value is top[row] > r
            if (nan || prev == r) {
                exact = true;
            } else {
                found = row * kGridRes + j;
                mv = v[j < kGridRes ? j : kGridRes - 1];
                pv = prev;
            }
        } else {
            exact = nan;  // row == 12: no sector has cdf > r, the search fails
        }
    }
    if (exact) {
        int start = 0, end = kSarsaSectors - 1;
        while (start <= end) {
            const int mid = (end + start) / 2;
            const float mval = cdf[mid];
            const float pval = (mid > 0) ? cdf[mid - 1] : 0.0f;
            if (r < mval && pval <= r) {
                found = mid;
                mv = mval;
                pv = pval;
                break;
            } else if (mval < r) {
                start = mid + 1;
            } else {
                end = mid - 1;
            }
        }
    }
    if (found < 0) return false;
    const int sx = found / kGridRes;
    const int sy = found - sx * kGridRes;
    *sector = found;
    *pdf = kRho * ((found == 0 ? mv : (mv - pv)) / kGridRhoS);
    const float4 N4 = vp.N4, T4 = vp.T4, B4 = vp.B4;
    *dir = grid_direction((float)sx + rx, (float)sy + ry, make3(N4.x, N4.y, N4.z), make3(T4.x, T4.y, T4.z),
                          make3(B4.x, B4.y, B4.z), make3(N4.w, T4.w, B4.w));
    return true;
}

// a live value of the in-frame TD mode's shared state (Q, irradiance): read at device scope,
// past this CU's L1, so a lane sees the other lanes' (and its own earlier) atomicExch writes
__device__ __forceinline__ float live_load(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sample_max_direction_from_radiance_distribution (radiance_volume.cu:246-278): the first
// sector of largest Q, uniform within it; the pdf is the CDF step of that sector, 0 for
// sector 0 (the reference's last_pdf is cdf[0] there, :274).  Frame-synchronous TD: Q is
// fixed within the frame, so its argmax (qmax) is kept by k_sarsa_apply; in-frame TD
// (TD = 1): the reference's scan of the live radiance grid at every sample (:251-257), the
// CDF still the frame's (update_radiance_volume_distributions runs between frames).
template <int TD>
__device__ void sarsa_sample_max(const SarsaMap& m, int rv, const VolPre& vp, float rx, float ry, int* sector, f3* dir,
                                 float* pdf) {
    const float* __restrict__ cdf = m.cdf + (size_t)rv * kSarsaSectors;
    int mi;
    if constexpr (TD == 1) {
        const float* q = m.Q + (size_t)rv * kSarsaSectors;
        mi = 0;
        float mq = live_load(q);
        // the reference's scan (radiance_volume.cu:251-257) starts at i = 0 with grid[0] already
        // loaded; its plain (non-volatile) loads let the compiler read grid[0] once, so the
        // k = 0 step (mq < q[0] with mq = q[0]) is skipped: 144 device-scope loads, not 145
        for (int k = 1; k < kSarsaSectors; ++k) {
            const float v = live_load(q + k);
            if (mq < v) {
                mq = v;
                mi = k;
            }
        }
    } else {
        mi = m.qmax[rv];
    }
    const float mv = cdf[mi];
    const float last = cdf[mi > 0 ? mi - 1 : 0];
    const int sx = mi / kGridRes;
    const int sy = mi - sx * kGridRes;
    *sector = mi;
    *pdf = kRho * ((mv - last) / kGridRhoS);
    const float4 N4 = vp.N4, T4 = vp.T4, B4 = vp.B4;
    *dir = grid_direction((float)sx + rx, (float)sy + ry, make3(N4.x, N4.y, N4.z), make3(T4.x, T4.y, T4.z),
                          make3(B4.x, B4.y, B4.z), make3(N4.w, T4.w, B4.w));
}

// temporal_difference_update + expected_sarsa_irradiance as the reference runs them
// (radiance_volume.cu:282-301, :93-112): read-modify-write of the sector's Q and the
// volume's irradiance while other lanes do the same -- a lost update is the reference's own
// race.  The visit count comes from the atomic's return (the reference reads it first).
__device__ __forceinline__ void td_event_inframe(const SarsaMap& m, int rv, int sector, float target) {
    const size_t k = (size_t)rv * kSarsaSectors + sector;
    const uint32_t vs = atomicAdd(&m.visits[k], 1u);
    const float alpha = 1.f / (1.f + (float)vs);
    const float q_old = live_load(&m.Q[k]);
    float upd = ((1.f - alpha) * q_old) + (alpha * target);
    upd = upd > kRadianceThreshold ? upd : kRadianceThreshold;
    const float cc = m.cos_corner[k];
    const float brdf = m.vol_brdf[rv];
    const float acc = live_load(&m.accum[rv]);
    const float acc_new = (acc - ((q_old * cc) * brdf)) + ((upd * cc) * brdf);
    atomicExch(&m.Q[k], upd);
    atomicExch(&m.accum[rv], acc_new);
}

template <int TD>
__device__ __forceinline__ void td_event(const SarsaMap& m, int rv, int sector, float target) {
    if constexpr (TD == 2) return;  // RT_SARSA_TD_OFF: the map is read-only
    if constexpr (TD == 1) {
        td_event_inframe(m, rv, sector, target);
        return;
    }
    const long long v = __float2ll_rn(target * 4294967296.0f);
    const size_t k = (size_t)rv * kSarsaSectors + sector;
    atomicAdd(&m.acc_sum[k], (unsigned long long)v);
    atomicAdd(&m.acc_cnt[k], 1u);
}

// The path's state between casts (k_sarsa_render_pq)
struct SarsaPath {
    f3 o, d, tp;
    int depth, cur_rv, cur_sector;
    float cur_brdf;
    bool null_ray;  // set by sarsa_step: the path ended by tracing the zero direction
};

// One cast of path_trace_reinforcement_iterative after its closest hit h and the volume
// rv at a surface hit: the TD event of the previous step, then light / miss / the next
// direction from the volume's distribution.  Returns true when the path ends, with its
// value in *L (n_casts counts the reference's extra cast of a zero direction).
template <int TD>
__device__ __forceinline__ bool sarsa_step(const RenderLaunch& a, const SarsaMap& m, const Hit& h, bool is_surf,
                                           f3 pos, f3 nrm, int rv, bool td, uint32_t pix, int s, SarsaPath& P,
                                           unsigned& n_casts, f3* L_out) {
    const float4* __restrict__ shade = a.scene.shade;
    // the volume this hit samples from, and its data loaded now: in flight with the TD
    // target's irradiance load, the TD atomics and the Philox block
    const int sv = (td || (P.depth == 0 && is_surf)) ? rv : P.cur_rv;
    VolPre vp;
    if (is_surf && sv >= 0) vp = vol_load(m, sv);
    if (td) {
        // TD = 2 (RT_SARSA_TD_OFF, a frozen map): no target, no irradiance load, no atomics; the
        // path's state moves on exactly as in the learning modes
        if constexpr (TD != 2) {
            float target;
            if (h.tri < 0) {
                target = P.cur_brdf * a.env_light;
            } else if (!is_surf) {
                target = P.cur_brdf * m.tri_lum[h.tri];
            } else {
                target = ((TD == 1 ? live_load(&m.accum[rv]) : m.accum[rv]) * kIrrScale) * P.cur_brdf;
            }
            td_event<TD>(m, P.cur_rv, P.cur_sector, target);
        }
        P.cur_rv = rv;
        P.cur_sector = -1;
    } else if (P.depth == 0 && is_surf) {
        P.cur_rv = rv;
    }
    bool terminal = false;
    f3 L = make3(0.f, 0.f, 0.f);
    if (h.tri < 0) {
        terminal = true;
        L = make3(P.tp.x * a.env_light, P.tp.y * a.env_light, P.tp.z * a.env_light);
    } else if (!is_surf) {
        terminal = true;
        const float4 e = shade[h.tri * kShadeF4 + 3];
        L = make3(P.tp.x * e.x, P.tp.y * e.y, P.tp.z * e.z);
    } else {
        uint32_t rn[4];
        philox4x32_10(pix, a.sample_base + (uint32_t)s, 1u + (uint32_t)P.depth, 0u, a.seed_lo, a.seed_hi, rn);
        f3 sd;
        float pdf;
        bool ok = true;
        if (P.cur_rv < 0) {  // no volume: uniform hemisphere, pdf = RHO
            const float4 T4 = shade[h.tri * kShadeF4 + 1], B4 = shade[h.tri * kShadeF4 + 2];
            const float c = u01(rn[0]);
            const float st = sqrtf(1.0f - c * c);
            float sphi, cphi;
            sincos_turn(u01(rn[1]), &sphi, &cphi);
            const float sx = st * cphi, sz = st * sphi;
            sd = make3((sx * B4.x + c * nrm.x) + sz * T4.x, (sx * B4.y + c * nrm.y) + sz * T4.y,
                       (sx * B4.z + c * nrm.z) + sz * T4.z);
            pdf = kRho;
        } else if (m.sample_max) {
            sarsa_sample_max<TD>(m, P.cur_rv, vp, u01_oc(rn[1]), u01_oc(rn[2]), &P.cur_sector, &sd, &pdf);
        } else {
            ok = sarsa_sample(m, P.cur_rv, vp, u01_oc(rn[0]), u01_oc(rn[1]), u01_oc(rn[2]), &P.cur_sector, &sd, &pdf);
        }
        if (!ok) {
            // no sector: the reference traces the zero direction it returns, which
            // hits nothing (one more cast; its radiance there is NaN, here the miss value)
            terminal = true;
            if (P.depth + 1 < a.max_bounces) {
                ++n_casts;
                L = make3(P.tp.x * a.env_light, P.tp.y * a.env_light, P.tp.z * a.env_light);
                // the reference's throughput is (BRDF * 0) / pdf 0 = NaN here: its radiance is
                // NaN, which its zero-contribution test (NaN < threshold) does not count
                P.null_ray = true;
            }
        } else {
            const float4 brdf = shade[h.tri * kShadeF4 + 3];
            const float cos_theta = dot(nrm, sd);
            P.cur_brdf = m.tri_lum[h.tri] / kPi;
            P.tp.x = P.tp.x * ((brdf.x * cos_theta) / pdf);
            P.tp.y = P.tp.y * ((brdf.y * cos_theta) / pdf);
            P.tp.z = P.tp.z * ((brdf.z * cos_theta) / pdf);
            P.o = make3(pos.x + sd.x * kEps, pos.y + sd.y * kEps, pos.z + sd.z * kEps);
            P.d = normalize(sd);
            ++P.depth;
            if (P.depth == a.max_bounces) terminal = true;
        }
    }
    *L_out = L;
    return terminal;
}

// path_trace_reinforcement_iterative (reinforcement_path_tracing.cu:50-120), GPU preset, on a
// persistent grid over a launch-wide (pixel, chunk) queue, as k_render_pq does for the GPU
// preset (rt_kernels.hip): a lane claims a chunk (the samples [c m, (c + 1) m) of pixel p),
// traces them one after another (per cast: the closest hit, the volume search at a surface
// hit, sarsa_step), sums their values in sample order, stores the chunk's value sum and ray
// casts, and claims the next, so lanes idle only at the end of the frame instead of at
// each wave's longest path (frame 0: 41 casts per path on door_room, up to 80).
// k_sarsa_fold adds each pixel's chunks in chunk order and takes its path-length statistic.
// The volume search still runs with every lane of the wave (the walks of the grid's
// undecided queries, sarsa_resolve_walks).  csum: float4 per chunk {r, g, b, casts (bits)}.
#ifndef RT_SARSA_WAVES
#define RT_SARSA_WAVES 5  // waves per SIMD of the persistent render (its grid: that many workgroups per CU)
#endif
// BVH: scenes with the exact BVH (large models, rt_scene_set_accel): the casts through
// closest_hit_bvh, its stack in the lane's k-d stack column (free until the volume search)
template <int RULE, int TD, bool BVH = false>
#ifndef RT_SARSA_BVH_WAVES
#define RT_SARSA_BVH_WAVES 4  // the BVH variant's traversal state: 128 VGPRs, no spills (96 at 5 waves spilled)
#endif
__global__ __launch_bounds__(256, BVH ? RT_SARSA_BVH_WAVES : RT_SARSA_WAVES) void k_sarsa_render_pq(const RenderLaunch a,
                                                                                        const SarsaMap m) {
    __shared__ __attribute__((aligned(16))) int kd_stack[kKdStack * 256];
    int* const st = kd_stack_of(kd_stack);
    int* const blk_ws = kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64);  // the wave's block
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const long long total = (long long)a.n_blocks * 256 * a.split;
    const f3 cam = make3(a.cam_x, a.cam_y, a.cam_z);
    long long qb = 0, qe = 0;  // wave-uniform: the wave's claimed, not yet handed out items
    bool exhausted = false;
    bool have = false;
    long long item = 0;
    int s = 0, s_end = 0, px = 0, py = 0;
    uint32_t pix = 0;
    SarsaPath P{cam, make3(0.f, 0.f, 1.f), make3(1.f, 1.f, 1.f), 0, -1, -1, 0.0f, false};
    f3 acc = make3(0.f, 0.f, 0.f);
    unsigned n_casts = 0, n_zero = 0, casts0 = 0;
#if RT_SARSA_PROF
    uint64_t pr[6] = {0, 0, 0, 0, 0, 0};  // trace, grid search, walks, step (TD + sampling), trips, active lanes
#endif
    auto camera = [&]() {
        float r1, r2;
        draw2(pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
        camera_ray<1>(a, px, py, r1, r2, &P.d);
        P.o = cam;
        P.tp = make3(1.f, 1.f, 1.f);
        P.depth = 0;
        P.cur_rv = -1;
        P.cur_sector = -1;
        P.null_ray = false;
    };
    for (;;) {
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
                        const long long p = j >> a.split_log2;
                        const int c = (int)(j & (a.split - 1));
                        const BlockDesc blk = a.blocks[p >> 8];
                        const int q = (int)(p & 255);
                        px = blk.px0 + (q & 15);
                        py = blk.py0 + (q >> 4);
                        if (px < a.clip_x1 && py < a.clip_y1) {
                            pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
                            s = c * a.per_chunk;
                            s_end = s + a.per_chunk;
                            acc = make3(0.f, 0.f, 0.f);
                            casts0 = n_casts;
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
            continue;
        }
#if RT_SARSA_PROF
        const uint64_t pt0 = __builtin_amdgcn_s_memtime();
        pr[5] += (uint64_t)__builtin_popcountll(__ballot(active));
#endif
        Hit h;
        h.t = 0.0f;
        h.tri = -1;
        if constexpr (BVH) {
            static_assert(kKdStack >= kBvhMaxDepth, "the BVH stack fits the k-d stack column");
            if (active) h = closest_hit_bvh<RULE, 64>(a.scene, P.o, P.d, a.t_scale, st);
        } else if (active) {
            h = closest_hit_sel<RULE>(a.scene, a.use_filter, P.o, P.d, a.t_scale);
        }
#if RT_SARSA_PROF
        const uint64_t pt1 = __builtin_amdgcn_s_memtime();
#endif
        if (active) ++n_casts;
        const bool is_surf = active && (h.tri >= 0) && (h.tri < n_surf);
        f3 pos = P.o;
        f3 nrm = make3(0.f, 0.f, 0.f);
        if (is_surf) {
            const float Dx = P.d.x * a.t_scale, Dy = P.d.y * a.t_scale, Dz = P.d.z * a.t_scale;
            pos = make3(P.o.x + h.t * Dx, P.o.y + h.t * Dy, P.o.z + h.t * Dz);
            const float4 N4 = shade[h.tri * kShadeF4 + 0];
            nrm = make3(N4.x, N4.y, N4.z);
        }
        const bool td = active && P.depth > 0 && P.cur_rv >= 0 && P.cur_sector >= 0;
        int rv = -1;
        if (is_surf && (P.depth == 0 || td))
            rv = m.use_grid ? sarsa_nearest_grid_tri(m, h.tri, pos, nrm) : kNeedWalk;
#if RT_SARSA_PROF
        const uint64_t pt2 = __builtin_amdgcn_s_memtime();
#endif
        if (m.use_grid)
            sarsa_resolve_walks(m, pos, nrm, &rv, blk_ws, st, lane);
        else if (rv == kNeedWalk)
            rv = sarsa_nearest(m, pos, nrm, st);
#if RT_SARSA_PROF
        const uint64_t pt3 = __builtin_amdgcn_s_memtime();
        f3 L;
        const bool term = active && sarsa_step<TD>(a, m, h, is_surf, pos, nrm, rv, td, pix, s, P, n_casts, &L);
        const uint64_t pt4 = __builtin_amdgcn_s_memtime();
        pr[0] += pt1 - pt0;
        pr[1] += pt2 - pt1;
        pr[2] += pt3 - pt2;
        pr[3] += pt4 - pt3;
        pr[4] += 1;
        if (!active) continue;
        if (term) {
#else
        if (!active) continue;
        f3 L;
        const bool term = sarsa_step<TD>(a, m, h, is_surf, pos, nrm, rv, td, pix, s, P, n_casts, &L);
        if (term) {
#endif
            acc.x = acc.x + L.x;
            acc.y = acc.y + L.y;
            acc.z = acc.z + L.z;
            n_zero += (!P.null_ray && (L.x + L.y + L.z) / 3.f < kThroughputThreshold) ? 1u : 0u;
            ++s;
            if (s < s_end) {
                camera();
            } else {
                reinterpret_cast<float4*>(a.csum)[item] = make_float4(acc.x, acc.y, acc.z, __uint_as_float(n_casts - casts0));
                have = false;
            }
        }
    }
    if (m.stats != nullptr) {
        const unsigned sz = wave_sum(n_zero);
        if (lane == 0) atomicAdd(&m.stats[1], (unsigned long long)sz);
    }
    if (a.casts != nullptr) {
        const unsigned tot = wave_sum(n_casts);
        if (lane == 0) atomicAdd(a.casts, (unsigned long long)tot);
    }
#if RT_SARSA_PROF
    if (m.prof != nullptr && lane == 0)
        for (int i = 0; i < 6; ++i) atomicAdd(m.prof + i, (unsigned long long)pr[i]);
#endif
}

// the pixels of k_sarsa_render_pq's launch: the chunk sums in chunk order / spp, and the
// per-pixel statistic int(path lengths / SAMPLES_PER_PIXEL) (main.cu:321-339)
__global__ __launch_bounds__(256) void k_sarsa_fold(const RenderLaunch a, const SarsaMap m) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const BlockDesc blk = a.blocks[blockIdx.x];
    const int q = threadIdx.x, lx = q & 15, ly = q >> 4;
    const bool valid = (blk.px0 + lx < a.clip_x1) && (blk.py0 + ly < a.clip_y1);
    unsigned pf = 0;
    if (valid) {
        const float4* c = reinterpret_cast<const float4*>(a.csum) + (size_t)p * a.split;
        float4 v = c[0];
        f3 tot = make3(v.x, v.y, v.z);
        unsigned pix_casts = __float_as_uint(v.w);
        for (int k = 1; k < a.split; ++k) {
            v = c[k];
            tot.x = tot.x + v.x;
            tot.y = tot.y + v.y;
            tot.z = tot.z + v.z;
            pix_casts += __float_as_uint(v.w);
        }
        pf = pix_casts / (unsigned)a.spp;
        const float fs = (float)a.spp;
        float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
        store_rgb(dst, tot.x / fs, tot.y / fs, tot.z / fs);
    }
    if (m.stats != nullptr) {
        const unsigned sp = wave_sum(pf);
        if ((threadIdx.x & 63) == 0) atomicAdd(&m.stats[0], (unsigned long long)sp);
    }
}

// update_radiance_distribution (radiance_volume.cu:148-188) of volume v, its row ends, and
// the first sector of largest Q (the max-direction sampler's scan, radiance_volume.cu:251-257)
__device__ void rebuild_volume(const SarsaMap& m, int v) {
    const size_t b = (size_t)v * kSarsaSectors;
    float total = 0.0000000001f;
    for (int k = 0; k < kSarsaSectors; ++k) {
        float t = m.Q[b + k] * m.cos_center[b + k];
        t = t > 0.0f ? t : 0.0f;
        total += t;
    }
    float prev = 0.0f;
    float* top = reinterpret_cast<float*>(m.cdf_top + (size_t)v * 4);
    for (int k = 0; k < kSarsaSectors; ++k) {
        float t = m.Q[b + k] * m.cos_center[b + k];
        t = t > 0.0f ? t : 0.0f;
        const float rad = t / total + prev;
        m.cdf[b + k] = rad;
        if (k == 0) top[0] = rad;
        if (k % kGridRes == kGridRes - 1) top[1 + k / kGridRes] = rad;
        prev = rad;
    }
    int mi = 0;
    float mq = m.Q[b];
    for (int k = 0; k < kSarsaSectors; ++k) {
        const float q = m.Q[b + k];
        if (mq < q) {
            mq = q;
            mi = k;
        }
    }
    m.qmax[v] = mi;
}

// End of frame, one lane per volume: fold the frame's TD targets (the running
// mean of alpha = 1/(1+visits), clamped at RADIANCE_THRESHOLD), update the
// irradiance with expected_sarsa_irradiance's increments (cell corners), and
// rebuild the CDF from Q*cos(cell centre) (update_radiance_distribution).
__global__ __launch_bounds__(256) void k_sarsa_apply(const SarsaMap m) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.n_vol) return;
    const size_t b = (size_t)v * kSarsaSectors;
    const float brdf = m.vol_brdf[v];
    float accum = m.accum[v];
    for (int k = 0; k < kSarsaSectors; ++k) {
        const uint32_t n = m.acc_cnt[b + k];
        if (n == 0u) continue;
        const long long S = (long long)m.acc_sum[b + k];
        const float sum = (float)((double)S * 2.3283064365386962890625e-10);
        const uint32_t vis = m.visits[b + k];
        const float q_old = m.Q[b + k];
        float q_new = (q_old * (float)vis + sum) / (float)(vis + n);
        q_new = q_new > kRadianceThreshold ? q_new : kRadianceThreshold;
        const float cc = m.cos_corner[b + k];
        accum = (accum - ((q_old * cc) * brdf)) + ((q_new * cc) * brdf);
        m.Q[b + k] = q_new;
        m.visits[b + k] = vis + n;
        m.acc_cnt[b + k] = 0u;
        m.acc_sum[b + k] = 0ull;
    }
    m.accum[v] = accum;
    rebuild_volume(m, v);
}

// CDF and argmax of Q after a load (rt_sarsa_load_q)
__global__ __launch_bounds__(256) void k_sarsa_rebuild(const SarsaMap m) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.n_vol) return;
    rebuild_volume(m, v);
}

// the same for the volumes [v0, v0 + n) alone (rt_sarsa_write, rt_sarsa_bake)
__global__ __launch_bounds__(256) void k_sarsa_rebuild_range(const SarsaMap m, int v0, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rebuild_volume(m, v0 + i);
}

}  // namespace

namespace {

// the render launch of one TD rule (TD: k_sarsa_render_pq's template argument, so the default
// frame-synchronous kernel carries no in-frame branch)
template <int TD>
hipError_t launch_sarsa_render_t(const RenderLaunch& a, const SarsaMap& m, hipStream_t stream) {
    if (a.csum == nullptr || a.work == nullptr) return hipErrorInvalidValue;
    (void)hipMemsetAsync(a.work, 0, sizeof(unsigned long long), stream);
    // as many workgroups as fit: RT_SARSA_WAVES per CU (registers and the k-d stack's LDS)
    const int per_cu = a.scene.bvh_nodes != nullptr ? RT_SARSA_BVH_WAVES : RT_SARSA_WAVES;
    int wgs = min(a.n_blocks * a.split, per_cu * device_cu_count());
    if (m.max_wgs > 0) wgs = min(wgs, m.max_wgs);  // rt_sarsa_set_inframe_lanes
    const dim3 grid((unsigned)wgs);
    if (a.scene.bvh_nodes != nullptr) {  // the exact BVH (large scenes)
        if (a.hit_rule == 0)
            hipLaunchKernelGGL((k_sarsa_render_pq<0, TD, true>), grid, dim3(256), 0, stream, a, m);
        else
            hipLaunchKernelGGL((k_sarsa_render_pq<1, TD, true>), grid, dim3(256), 0, stream, a, m);
    } else {
        if (a.hit_rule == 0)
            hipLaunchKernelGGL((k_sarsa_render_pq<0, TD>), grid, dim3(256), 0, stream, a, m);
        else
            hipLaunchKernelGGL((k_sarsa_render_pq<1, TD>), grid, dim3(256), 0, stream, a, m);
    }
    hipLaunchKernelGGL(k_sarsa_fold, dim3((unsigned)a.n_blocks), dim3(256), 0, stream, a, m);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sarsa_render(const RenderLaunch& a, const SarsaMap& m, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    KernelTimer kt(KT_SARSA_RENDER, stream);
    if (m.td_off) return launch_sarsa_render_t<2>(a, m, stream);
    return m.td_inframe ? launch_sarsa_render_t<1>(a, m, stream) : launch_sarsa_render_t<0>(a, m, stream);
}

hipError_t launch_sarsa_rebuild(const SarsaMap& m, hipStream_t stream) {
    if (m.n_vol <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sarsa_rebuild, dim3((unsigned)((m.n_vol + 255) / 256)), dim3(256), 0, stream, m);
    return hipGetLastError();
}

hipError_t launch_sarsa_rebuild_range(const SarsaMap& m, int v0, int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (v0 < 0 || n > m.n_vol - v0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sarsa_rebuild_range, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, v0, n);
    return hipGetLastError();
}

bool sarsa_prof_compiled() { return RT_SARSA_PROF != 0; }

hipError_t launch_sarsa_apply(const SarsaMap& m, hipStream_t stream) {
    if (m.n_vol <= 0) return hipSuccess;
    KernelTimer kt(KT_SARSA_APPLY, stream);
    hipLaunchKernelGGL(k_sarsa_apply, dim3((unsigned)((m.n_vol + 255) / 256)), dim3(256), 0, stream, m);
    return hipGetLastError();
}

}  // namespace rt
