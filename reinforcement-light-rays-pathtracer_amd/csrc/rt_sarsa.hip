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
// the nearest-volume search (sarsa_nearest*, sarsa_resolve_walks) and its A/B knobs, shared with
// rt_sweep.hip
#include "rt_sarsa_search.hpp"

// A/B knobs (timing builds only): RT_SARSA_NO_TD drops the TD atomics
#ifndef RT_SARSA_NO_TD
#define RT_SARSA_NO_TD 0
#endif
#ifndef RT_SARSA_PROF
#define RT_SARSA_PROF 0  // 1: k_sarsa_render_pq sums per-phase s_memtime cycles into SarsaMap::prof (timing builds)
#endif

namespace rt {

namespace {

constexpr float kGridRhoS = 1.0f / ((float)kGridRes * (float)kGridRes);             // GRID_RHO
constexpr float kRadianceThreshold = (1.f / ((float)kGridRes * (float)kGridRes)) * 0.8f;  // RADIANCE_THRESHOLD
constexpr float kIrrScale = (2.f * kPi) / ((float)(kGridRes * kGridRes));          // get_irradiance_estimate
constexpr float kThroughputThreshold = 0.0001f;  // THROUGHPUT_THRESHOLD (constants/monte_carlo_settings.h:11)

// normal class of a query normal (queries without a surface index)
__device__ int sarsa_class_of(const SarsaMap& m, f3 nrm) {
    for (int c = 0; c < m.n_class; ++c) {
        const float4 n4 = m.class_nrm[c];
        if (nrm.x == n4.x && nrm.y == n4.y && nrm.z == n4.z) return c;
    }
    return -1;
}

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
    if (RT_SARSA_NO_TD) return;
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

// The path's state between casts (k_sarsa_render, k_sarsa_render_pq)
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

// path_trace_reinforcement_iterative (reinforcement_path_tracing.cu:50-120), GPU preset
// MF > 0: every cast on the matrix-core filter (closest_hit_mf, wave-level; the launcher
// picks it as launch_render_t does for k_render: image present, camera inside its bound)
// MF: the exact phase's LDS is the wave's own block of the k-d stack (free between searches;
// wave_lds_sync orders the two uses), so the workgroup needs the stack's 32 KB only; scenes
// of <= 64 triangles held to 4 waves per SIMD (<= 128 VGPRs without spills; the 4-block
// variant would spill there and keeps the compiler's 3 waves).
#ifndef RT_MF_SARSA_WAVES
#define RT_MF_SARSA_WAVES 4
#endif
template <int RULE, int MF, int TD>
__global__ __launch_bounds__(256, MF == 1 ? RT_MF_SARSA_WAVES : 1) void k_sarsa_render(const RenderLaunch a,
                                                                                     const SarsaMap m) {
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    const int part = blockIdx.x & (a.split - 1);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int chunk = threadIdx.x & (a.split - 1);
    const int lane = threadIdx.x & 63;
    const int lx = q & 15, ly = q >> 4;
    const int px = blk.px0 + lx, py = blk.py0 + ly;
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    const uint32_t pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const int s_end = (chunk + 1) * a.per_chunk;
    __shared__ int kd_stack[kKdStack * 256];
    int* const st = kd_stack_of(kd_stack);
    static_assert(kKdStack * 64 >= kMfWaveFloats, "the exact phase's LDS fits a wave's stack block");
    float* const wl = reinterpret_cast<float*>(kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64));

    int s = valid ? chunk * a.per_chunk : s_end;
    int depth = 0;
    int cur_rv = -1, cur_sector = -1;
    float cur_brdf = 0.0f;
    f3 o = make3(a.cam_x, a.cam_y, a.cam_z), d = make3(0.f, 0.f, 1.f);
    f3 tp = make3(1.f, 1.f, 1.f), acc = make3(0.f, 0.f, 0.f);
    unsigned n_casts = 0, n_zero = 0;
    if (s < s_end) {
        float r1, r2;
        draw2(pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
        camera_ray<1>(a, px, py, r1, r2, &d);
    }
    for (;;) {
        const bool active = s < s_end;
        if (__ballot(active) == 0ull) break;
        Hit h;
        h.t = 0.0f;
        h.tri = -1;
        if constexpr (MF > 0) {
            wave_lds_sync();  // the previous search's stack accesses stay before the exact phase
            h = closest_hit_mf<RULE, false, MF>(a.scene, o, d, a.t_scale, active, wl);
            wave_lds_sync();  // and its LDS traffic before the next search
        } else if (active) {
            h = closest_hit_sel<RULE>(a.scene, a.use_filter, o, d, a.t_scale);
        }
        // (inactive lanes go on to the volume search, which the whole wave runs, with no query)
        if (active) ++n_casts;
        const bool is_surf = active && (h.tri >= 0) && (h.tri < n_surf);
        f3 pos = o;
        f3 nrm = make3(0.f, 0.f, 0.f);
        if (is_surf) {
            const float Dx = d.x * a.t_scale, Dy = d.y * a.t_scale, Dz = d.z * a.t_scale;
            pos = make3(o.x + h.t * Dx, o.y + h.t * Dy, o.z + h.t * Dz);
            const float4 N4 = shade[h.tri * kShadeF4 + 0];
            nrm = make3(N4.x, N4.y, N4.z);
        }
        // temporal_difference_update_radiance_volume_sector at every bounce after a
        // sampled sector; the volume at a surface hit serves both the TD target and
        // the next sampling step (one search call site: the search is divergent)
        const bool td = active && depth > 0 && cur_rv >= 0 && cur_sector >= 0;
        int rv = -1;
        if (is_surf && (depth == 0 || td))
            rv = m.use_grid ? sarsa_nearest_grid_tri(m, h.tri, pos, nrm) : kNeedWalk;
        if (m.use_grid)  // the grid's few undecided queries: walked by the whole wave
            sarsa_resolve_walks(m, pos, nrm, &rv, kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64), st, lane);
        else if (rv == kNeedWalk)
            rv = sarsa_nearest(m, pos, nrm, st);
        if (!active) continue;
        SarsaPath P{o, d, tp, depth, cur_rv, cur_sector, cur_brdf, false};
        f3 L;
        const bool terminal = sarsa_step<TD>(a, m, h, is_surf, pos, nrm, rv, td, pix, s, P, n_casts, &L);
        o = P.o;
        d = P.d;
        tp = P.tp;
        depth = P.depth;
        cur_rv = P.cur_rv;
        cur_sector = P.cur_sector;
        cur_brdf = P.cur_brdf;
        if (terminal) {
            acc.x = acc.x + L.x;
            acc.y = acc.y + L.y;
            acc.z = acc.z + L.z;
            // a zero-contribution light path (reinforcement_path_tracing.cu:36-40)
            n_zero += (!P.null_ray && (L.x + L.y + L.z) / 3.f < kThroughputThreshold) ? 1u : 0u;
            ++s;
            depth = 0;
            cur_rv = -1;
            cur_sector = -1;
            tp = make3(1.f, 1.f, 1.f);
            o = make3(a.cam_x, a.cam_y, a.cam_z);
            if (s < s_end) {
                float r1, r2;
                draw2(pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
                camera_ray<1>(a, px, py, r1, r2, &d);
            }
        }
    }
    const int base = lane & ~(a.split - 1);
    f3 tot = acc;
    unsigned pix_casts = n_casts;  // a sample's path length is its ray casts
    for (int k = 1; k < a.split; ++k) {
        const float vx = __shfl(acc.x, base + k, 64);
        const float vy = __shfl(acc.y, base + k, 64);
        const float vz = __shfl(acc.z, base + k, 64);
        pix_casts += (unsigned)__shfl((int)n_casts, base + k, 64);
        tot.x = tot.x + vx;
        tot.y = tot.y + vy;
        tot.z = tot.z + vz;
    }
    if (m.stats != nullptr) {
        // main.cu:321-339 statistics: int(total_path_lengths / SAMPLES_PER_PIXEL) per pixel
        const unsigned pf = (valid && chunk == 0) ? pix_casts / (unsigned)a.spp : 0u;
        const unsigned sp = wave_sum(pf), sz = wave_sum(n_zero);
        if (lane == 0) {
            atomicAdd(&m.stats[0], (unsigned long long)sp);
            atomicAdd(&m.stats[1], (unsigned long long)sz);
        }
    }
    if (valid && chunk == 0) {
        const float fs = (float)a.spp;
        float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
        store_rgb(dst, tot.x / fs, tot.y / fs, tot.z / fs);
    }
    if (a.casts != nullptr) {
        const unsigned total = wave_sum(n_casts);
        if (lane == 0) atomicAdd(a.casts, (unsigned long long)total);
    }
}

// k_sarsa_render on a persistent grid over a launch-wide (pixel, chunk) queue, as
// k_render_pq does for the GPU preset (rt_kernels.hip): a lane claims a chunk (the samples
// [c m, (c + 1) m) of pixel p), traces them one after another with k_sarsa_render's
// per-cast work (sarsa_step) and its fixed-chunk sum, stores the chunk's value sum and ray
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
// CT > 0: the casts take their candidates from tables (CT mask words; k_render_pq's CT route:
// a camera ray the cull of its pixel's 16x4 rectangle in a.cull, a bounce ray the candidate
// table of the surface it leaves) and closest_hit_cand tests them in index order
template <int RULE, int MF, int TD, bool BVH = false, int CT = 0>
#ifndef RT_SARSA_BVH_WAVES
#define RT_SARSA_BVH_WAVES 4  // the BVH variant's traversal state: 128 VGPRs, no spills (96 at 5 waves spilled)
#endif
__global__ __launch_bounds__(256, BVH ? RT_SARSA_BVH_WAVES : (MF == 1 ? RT_MF_SARSA_WAVES : RT_SARSA_WAVES)) void k_sarsa_render_pq(const RenderLaunch a,
                                                                                        const SarsaMap m) {
    __shared__ __attribute__((aligned(16))) int kd_stack[kKdStack * 256];
    static_assert(kKdStack * 64 >= kMfWaveFloats, "the exact phase's LDS fits a wave's stack block");
    int* const st = kd_stack_of(kd_stack);
    int* const blk_ws = kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64);  // the wave's block
    float* const wl = reinterpret_cast<float*>(blk_ws);
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
    int surf = -1, cidx = 0;  // CT: the surface the ray leaves; the pixel's rectangle in a.cull
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
                            cidx = (int)(p >> 8) * 4 + (q >> 6);
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
        } else if constexpr (CT > 0) {
            uint64_t F[CT];
#pragma unroll
            for (int k = 0; k < CT; ++k) F[k] = 0ull;
            if (active && P.depth == 0) {
#pragma unroll
                for (int k = 0; k < CT; ++k)
                    F[k] = (k < kRenderCullWords) ? a.cull[(size_t)cidx * kRenderCullWords + k] : 0ull;
            } else if (active) {
                ctab_candidates<CT>(a.scene.ctab[RULE], a.scene.n_tri, n_surf, surf, P.o, P.d, F);
            }
            wave_lds_sync();
            h = closest_hit_cand<RULE, CT>(a.scene, F, P.o, P.d, a.t_scale, wl);
            wave_lds_sync();
        } else if constexpr (MF > 0) {
            wave_lds_sync();
            h = closest_hit_mf<RULE, false, MF>(a.scene, P.o, P.d, a.t_scale, active, wl);
            wave_lds_sync();
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
        surf = h.tri;
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
        surf = h.tri;  // (a continuing path leaves the surface it hit)
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
    if (m.use_grid) {  // as k_sarsa_render searches
        if (in) v = RT_SARSA_NO_KD ? 0 : sarsa_nearest_grid(m, sarsa_class_of(m, nr), p, nr);
        sarsa_resolve_walks(m, p, nr, &v, kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64), kd_stack_of(kd_stack),
                            threadIdx.x & 63);
    } else if (in) {
        v = sarsa_nearest(m, p, nr, kd_stack_of(kd_stack));
    }
    if (in) out[i] = v;
}

// The radiance-map view (the reference's PATH_TRACING_METHOD 2: GPU/path_tracing/
// voronoi_trace.cu:6-41, RadianceMap::get_voronoi_colour, radiance_map.cu:218-225): per
// sample the camera ray of k_sarsa_render (sample index a.sample_base + s), its closest hit,
// the nearest volume of a surface hit as the render searches it, and that volume's entry of
// the colour table; (1, 1, 1) for a light or a miss.  One lane per (pixel, chunk) in
// k_sarsa_render's layout -- a wave covers 16 x 4 pixels at split 1 -- and its chunk fold.
// Every lane of a wave that has a pixel runs all per_chunk trips: a lane outside the image
// or the tile casts nothing and searches nothing, but stays for the cull's ballots, the
// shared k-d walks (sarsa_resolve_walks) and the fold's shuffles.  Reads the map only
// (grid_fallbacks counts its undecided queries as in the render).
// cull: the camera rays take the cull of the wave's pixel rectangle (launch_sarsa_view).
// out_tri / out_vol / out_pos (each may be null): triangle (-1: miss), volume (-1: no
// surface) and hit point (zeros: no surface) of sample a.sample_base, by output pixel.
template <int RULE>
__global__ __launch_bounds__(256) void k_sarsa_view(const RenderLaunch a, const SarsaMap m,
                                                    const float4* __restrict__ colours, int cull,
                                                    int32_t* __restrict__ out_tri, int32_t* __restrict__ out_vol,
                                                    float* __restrict__ out_pos) {
    __shared__ int kd_stack[kKdStack * 256];
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    const int part = blockIdx.x & (a.split - 1);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int chunk = threadIdx.x & (a.split - 1);
    const int lane = threadIdx.x & 63;
    const int lx = q & 15, ly = q >> 4;
    const int px = blk.px0 + lx, py = blk.py0 + ly;
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    if (__ballot(valid) == 0ull) return;  // (whole waves outside the image)
    const uint32_t pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    int* const st = kd_stack_of(kd_stack);
    int* const blk_ws = kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64);
    const f3 o = make3(a.cam_x, a.cam_y, a.cam_z);
    uint64_t cm[kRenderCullWords] = {0ull, 0ull, 0ull, 0ull};
    if (cull) wave_candidates<RULE>(a, valid, px, py, lane, cm);
    f3 acc = make3(0.f, 0.f, 0.f);
    for (int k = 0; k < a.per_chunk; ++k) {
        const int s = chunk * a.per_chunk + k;
        Hit h;
        h.t = 0.0f;
        h.tri = -1;
        f3 d = make3(0.f, 0.f, 1.f);
        if (valid) {
            float r1, r2;
            draw2(pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
            camera_ray<1>(a, px, py, r1, r2, &d);
            h = cull ? view_hit_culled<RULE>(a.scene, cm, o, d, a.t_scale)
                     : closest_hit<RULE>(a.scene.isect, a.scene.n_tri, o, d, a.t_scale);
        }
        const bool is_surf = valid && (h.tri >= 0) && (h.tri < n_surf);
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
        float4 c = make_float4(1.f, 1.f, 1.f, 0.f);
        if (rv >= 0) c = colours[rv];
        acc.x = acc.x + c.x;
        acc.y = acc.y + c.y;
        acc.z = acc.z + c.z;
        if (k == 0 && chunk == 0 && valid) {
            const size_t op = (size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx);
            if (out_tri != nullptr) out_tri[op] = h.tri;
            if (out_vol != nullptr) out_vol[op] = rv;
            if (out_pos != nullptr) {
                out_pos[3 * op + 0] = is_surf ? pos.x : 0.0f;
                out_pos[3 * op + 1] = is_surf ? pos.y : 0.0f;
                out_pos[3 * op + 2] = is_surf ? pos.z : 0.0f;
            }
        }
    }
    const int base = lane & ~(a.split - 1);
    f3 tot = acc;
    for (int k = 1; k < a.split; ++k) {
        const float vx = __shfl(acc.x, base + k, 64);
        const float vy = __shfl(acc.y, base + k, 64);
        const float vz = __shfl(acc.z, base + k, 64);
        tot.x = tot.x + vx;
        tot.y = tot.y + vy;
        tot.z = tot.z + vz;
    }
    if (valid && chunk == 0) {
        const float fs = (float)a.spp;
        float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
        store_rgb(dst, tot.x / fs, tot.y / fs, tot.z / fs);
    }
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
// closest hit of k_sarsa_view, and at a surface hit the map's interpolated estimate
// (irr_estimate) of the hit point under the surface's stored normal -- grey, or (tint) times
// the surface's albedo over its luminance; a light gives its emission, a miss env_light.
// k_sarsa_view's lane layout, cull and chunk fold; no k-d walk, so no LDS.  Reads the map only.
// out_tri / out_pos as k_sarsa_view's; out_vol / out_dist [pixel][k]: the volumes found for
// sample a.sample_base and their distances (-1 / +inf: none, or no surface hit).
template <int RULE>
__global__ __launch_bounds__(256) void k_sarsa_irr(const RenderLaunch a, const SarsaMap m, const IrrOpts o, int cull,
                                                   int32_t* __restrict__ out_tri, float* __restrict__ out_pos,
                                                   int32_t* __restrict__ out_vol, float* __restrict__ out_dist) {
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    const int part = blockIdx.x & (a.split - 1);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int chunk = threadIdx.x & (a.split - 1);
    const int lane = threadIdx.x & 63;
    const int lx = q & 15, ly = q >> 4;
    const int px = blk.px0 + lx, py = blk.py0 + ly;
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    if (__ballot(valid) == 0ull) return;  // (whole waves outside the image)
    const uint32_t pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const f3 o3 = make3(a.cam_x, a.cam_y, a.cam_z);
    uint64_t cm[kRenderCullWords] = {0ull, 0ull, 0ull, 0ull};
    if (cull) wave_candidates<RULE>(a, valid, px, py, lane, cm);
    f3 acc = make3(0.f, 0.f, 0.f);
    for (int t = 0; t < a.per_chunk; ++t) {
        const int s = chunk * a.per_chunk + t;
        Hit h;
        h.t = 0.0f;
        h.tri = -1;
        f3 d = make3(0.f, 0.f, 1.f);
        if (valid) {
            float r1, r2;
            draw2(pix, a.sample_base + (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
            camera_ray<1>(a, px, py, r1, r2, &d);
            h = cull ? view_hit_culled<RULE>(a.scene, cm, o3, d, a.t_scale)
                     : closest_hit<RULE>(a.scene.isect, a.scene.n_tri, o3, d, a.t_scale);
        }
        const bool is_surf = valid && (h.tri >= 0) && (h.tri < n_surf);
        f3 pos = o3;
        KnnSet ks;
        knn_clear(ks);
        f3 c = make3(a.env_light, a.env_light, a.env_light);  // a miss
        if (is_surf) {
            const float Dx = d.x * a.t_scale, Dy = d.y * a.t_scale, Dz = d.z * a.t_scale;
            pos = make3(o3.x + h.t * Dx, o3.y + h.t * Dy, o3.z + h.t * Dz);
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
        if (t == 0 && chunk == 0 && valid) {
            const size_t op = (size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx);
            if (out_tri != nullptr) out_tri[op] = h.tri;
            if (out_pos != nullptr) {
                out_pos[3 * op + 0] = is_surf ? pos.x : 0.0f;
                out_pos[3 * op + 1] = is_surf ? pos.y : 0.0f;
                out_pos[3 * op + 2] = is_surf ? pos.z : 0.0f;
            }
#define KNN_X(u)                                                          \
    if (u < o.k) {                                                        \
        if (out_vol != nullptr) out_vol[op * o.k + u] = ks.v##u;      \
        if (out_dist != nullptr) out_dist[op * o.k + u] = ks.d##u; \
    }
            KNN_SLOTS(KNN_X)
#undef KNN_X
        }
    }
    const int base = lane & ~(a.split - 1);
    f3 tot = acc;
    for (int j = 1; j < a.split; ++j) {
        const float vx = __shfl(acc.x, base + j, 64);
        const float vy = __shfl(acc.y, base + j, 64);
        const float vz = __shfl(acc.z, base + j, 64);
        tot.x = tot.x + vx;
        tot.y = tot.y + vy;
        tot.z = tot.z + vz;
    }
    if (valid && chunk == 0) {
        const float fs = (float)a.spp;
        float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
        store_rgb(dst, tot.x / fs, tot.y / fs, tot.z / fs);
    }
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

// the rectangle cull where launch_sarsa_view takes it
hipError_t launch_sarsa_irr(const RenderLaunch& a, const SarsaMap& m, int k, float radius, int cone, int tint,
                            int32_t* out_tri, float* out_pos, int32_t* out_vol, float* out_dist, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    if (a.out == nullptr || m.grid_leaf == nullptr || k < 1 || k > kKnnMax || !(radius > 0.0f && radius <= m.grid_h))
        return hipErrorInvalidValue;
    if (a.split < 1 || a.split > 64 || (1 << a.split_log2) != a.split || a.per_chunk * a.split != a.spp)
        return hipErrorInvalidValue;
    const int cull = (a.use_filter && a.scene.filt != nullptr && a.scene.n_tri <= 64 * kRenderCullWords &&
                      a.cos_x == 1.0f && a.sin_x == 0.0f) ? 1 : 0;
    const IrrOpts o{k, radius, cone, tint};
    const dim3 grid((unsigned)(a.n_blocks * a.split));
    if (a.hit_rule == 0)
        hipLaunchKernelGGL((k_sarsa_irr<0>), grid, dim3(256), 0, stream, a, m, o, cull, out_tri, out_pos, out_vol, out_dist);
    else
        hipLaunchKernelGGL((k_sarsa_irr<1>), grid, dim3(256), 0, stream, a, m, o, cull, out_tri, out_pos, out_vol, out_dist);
    return hipGetLastError();
}

// the camera rays take the rectangle cull where k_render_ps takes it (filter records valid
// for this camera and t_scale, at most 256 triangles) and the GPU preset's ray is the cull's
// camera model: pitch 0 (camera_ray's second rotation is then the identity, exactly)
hipError_t launch_sarsa_view(const RenderLaunch& a, const SarsaMap& m, const float4* colours, int32_t* out_tri,
                             int32_t* out_vol, float* out_pos, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    if (colours == nullptr || a.out == nullptr) return hipErrorInvalidValue;
    if (a.split < 1 || a.split > 64 || (1 << a.split_log2) != a.split || a.per_chunk * a.split != a.spp)
        return hipErrorInvalidValue;
    const int cull = (a.use_filter && a.scene.filt != nullptr && a.scene.n_tri <= 64 * kRenderCullWords &&
                      a.cos_x == 1.0f && a.sin_x == 0.0f) ? 1 : 0;
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

#ifndef RT_MF_SARSA
#define RT_MF_SARSA 0  // 1: the casts on the matrix-core filter (measured slower: DESIGN.md §4)
#endif

#ifndef RT_SARSA_CTAB
#define RT_SARSA_CTAB 0  // 1: k_sarsa_render_pq's casts from the candidate tables (door_room 512^2 x 256: 110.3 vs 92.1 ms per frame)
#endif

#ifndef RT_SARSA_PQ
#define RT_SARSA_PQ 1  // 0: the per-pixel k_sarsa_render (A/B builds)
#endif

namespace {

// the render launch of one TD rule (TD: k_sarsa_render's template argument, so the default
// frame-synchronous kernel carries no in-frame branch)
template <int TD>
hipError_t launch_sarsa_render_t(const RenderLaunch& a, const SarsaMap& m, hipStream_t stream) {
    const float cb = a.scene.mf_bound;
    const bool mf = RT_MF_SARSA && a.scene.bvh_nodes == nullptr && a.use_filter && a.scene.mf_frag != nullptr && a.t_scale > 0.0f &&
                    a.t_scale <= kFiltMaxTScale && fabsf(a.cam_x) <= cb && fabsf(a.cam_y) <= cb &&
                    fabsf(a.cam_z) <= cb;
    const bool one = a.scene.n_tri <= 64;
    // the table route (k_sarsa_render_pq CT): as k_render_pq's -- the scene's candidate table for
    // this hit rule and t_scale, the camera rays' rectangle cull (pitch 0, filter records valid
    // for the camera)
    const CtabDev& T = a.scene.ctab[a.hit_rule == 0 ? 0 : 1];
    const bool ct = !mf && RT_SARSA_CTAB && a.scene.bvh_nodes == nullptr && a.cull != nullptr && a.use_filter &&
                    a.cos_x == 1.0f && a.sin_x == 0.0f && a.scene.n_tri <= 64 * kRenderCullWords &&
                    T.masks != nullptr && T.bins == kCtabBins && T.graze_n == kCtabGraze && a.t_scale >= T.ts_min &&
                    T.words <= (one ? 1 : 4);
    if constexpr (RT_SARSA_PQ) {
        if (a.csum == nullptr || a.work == nullptr) return hipErrorInvalidValue;
        (void)hipMemsetAsync(a.work, 0, sizeof(unsigned long long), stream);
        // as many workgroups as fit: RT_SARSA_WAVES per CU (registers and the k-d stack's LDS)
        const int per_cu = a.scene.bvh_nodes != nullptr ? RT_SARSA_BVH_WAVES : (mf ? RT_MF_SARSA_WAVES : RT_SARSA_WAVES);
        int wgs = min(a.n_blocks * a.split, per_cu * device_cu_count());
        if (m.max_wgs > 0) wgs = min(wgs, m.max_wgs);  // rt_sarsa_set_inframe_lanes
        const dim3 grid((unsigned)wgs);
        if constexpr (RT_MF_SARSA) {
            if (mf) {
                if (a.hit_rule == 0 && one)
                    hipLaunchKernelGGL((k_sarsa_render_pq<0, 1, TD>), grid, dim3(256), 0, stream, a, m);
                else if (a.hit_rule == 0)
                    hipLaunchKernelGGL((k_sarsa_render_pq<0, 4, TD>), grid, dim3(256), 0, stream, a, m);
                else if (one)
                    hipLaunchKernelGGL((k_sarsa_render_pq<1, 1, TD>), grid, dim3(256), 0, stream, a, m);
                else
                    hipLaunchKernelGGL((k_sarsa_render_pq<1, 4, TD>), grid, dim3(256), 0, stream, a, m);
            }
        }
        if (a.scene.bvh_nodes != nullptr) {  // the exact BVH (large scenes)
            if (a.hit_rule == 0)
                hipLaunchKernelGGL((k_sarsa_render_pq<0, 0, TD, true>), grid, dim3(256), 0, stream, a, m);
            else
                hipLaunchKernelGGL((k_sarsa_render_pq<1, 0, TD, true>), grid, dim3(256), 0, stream, a, m);
        } else if (ct) {
            RenderLaunch c = a;  // one workgroup per 16x16 block: the masks of its four 16x4 rectangles
            c.split = 1;
            c.split_log2 = 0;
            (void)launch_cull(c, stream);
            if (a.hit_rule == 0) {
                if (one)
                    hipLaunchKernelGGL((k_sarsa_render_pq<0, 0, TD, false, 1>), grid, dim3(256), 0, stream, a, m);
                else
                    hipLaunchKernelGGL((k_sarsa_render_pq<0, 0, TD, false, 4>), grid, dim3(256), 0, stream, a, m);
            } else {
                if (one)
                    hipLaunchKernelGGL((k_sarsa_render_pq<1, 0, TD, false, 1>), grid, dim3(256), 0, stream, a, m);
                else
                    hipLaunchKernelGGL((k_sarsa_render_pq<1, 0, TD, false, 4>), grid, dim3(256), 0, stream, a, m);
            }
        } else if (!mf) {
            if (a.hit_rule == 0)
                hipLaunchKernelGGL((k_sarsa_render_pq<0, 0, TD>), grid, dim3(256), 0, stream, a, m);
            else
                hipLaunchKernelGGL((k_sarsa_render_pq<1, 0, TD>), grid, dim3(256), 0, stream, a, m);
        }
        hipLaunchKernelGGL(k_sarsa_fold, dim3((unsigned)a.n_blocks), dim3(256), 0, stream, a, m);
        return hipGetLastError();
    } else {
        const dim3 grid((unsigned)(a.n_blocks * a.split));
        if constexpr (RT_MF_SARSA) {
            if (mf) {
                if (a.hit_rule == 0 && one)
                    hipLaunchKernelGGL((k_sarsa_render<0, 1, TD>), grid, dim3(256), 0, stream, a, m);
                else if (a.hit_rule == 0)
                    hipLaunchKernelGGL((k_sarsa_render<0, 4, TD>), grid, dim3(256), 0, stream, a, m);
                else if (one)
                    hipLaunchKernelGGL((k_sarsa_render<1, 1, TD>), grid, dim3(256), 0, stream, a, m);
                else
                    hipLaunchKernelGGL((k_sarsa_render<1, 4, TD>), grid, dim3(256), 0, stream, a, m);
            }
        }
        if (!mf) {
            if (a.hit_rule == 0)
                hipLaunchKernelGGL((k_sarsa_render<0, 0, TD>), grid, dim3(256), 0, stream, a, m);
            else
                hipLaunchKernelGGL((k_sarsa_render<1, 0, TD>), grid, dim3(256), 0, stream, a, m);
        }
        return hipGetLastError();
    }
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
bool sarsa_ctab_compiled() { return RT_SARSA_CTAB != 0; }

hipError_t launch_sarsa_apply(const SarsaMap& m, hipStream_t stream) {
    if (m.n_vol <= 0) return hipSuccess;
    KernelTimer kt(KT_SARSA_APPLY, stream);
    hipLaunchKernelGGL(k_sarsa_apply, dim3((unsigned)((m.n_vol + 255) / 256)), dim3(256), 0, stream, m);
    return hipGetLastError();
}

}  // namespace rt
