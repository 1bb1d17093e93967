// rt_sarsa_search.hpp — the nearest-volume search of a radiance map, as device code: the
// reference's k-d walk (sarsa_nearest), its exact shortcut through the per-normal grid
// (sarsa_nearest_grid*) and the wave-cooperative walk of the queries the grid leaves open
// (sarsa_nearest_wave, sarsa_resolve_walks).  Included by the kernels that search as the
// render does: rt_sarsa.hip (the learning render), rt_views.hip (views, queries) and rt_sweep.hip
// (k_sweep).
#pragma once

#include <float.h>

#include "rt_trace.hpp"

namespace rt {

namespace {

// get_irradiance_estimate: a volume's irradiance estimate is accum * kIrrScale (the render's TD
// target, the sweep's, the irradiance render)
constexpr float kIrrScale = (2.f * kPi) / ((float)(kGridRes * kGridRes));

__device__ __forceinline__ float len3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// find_closest_radiance_volume_iterative (radiance_map.cu:149-203): explicit-stack
// KD descent; a far child is visited when delta^2 < MAX_DIST; leaves need an
// identical normal; the search starts from volume 0 at the distance of element 0's
// position (the origin for an internal root).  The stack lives in LDS, one column per
// lane of the wave's own block (st[k * 64], kd_stack_of); its depth is bounded by the
// tree depth (host-checked).
// the k-d stack column of this lane: each wave owns a contiguous kKdStack x 64 block (the
// wave-cooperative walk's frontier reuses it between searches: sarsa_nearest_wave)
__device__ __forceinline__ int* kd_stack_of(int* kd_stack) {
    return kd_stack + ((int)threadIdx.x >> 6) * (kKdStack * 64) + ((int)threadIdx.x & 63);
}

__device__ int sarsa_nearest(const SarsaMap& m, f3 pos, f3 nrm, int* st) {
    const uint4* __restrict__ kd = m.kd4;
    int best = 0;
    float best_d = len3(pos.x - m.root_x, pos.y - m.root_y, pos.z - m.root_z);
    st[0] = 0;
    int sp = 1;
    while (sp > 0) {
        --sp;
        const uint4 nd = kd[st[sp * 64]];
        if (nd.w != 0xFFFFFFFFu) {  // leaf
            const float d = len3(__uint_as_float(nd.x) - pos.x, __uint_as_float(nd.y) - pos.y,
                                 __uint_as_float(nd.z) - pos.z);
            if (d < best_d) {
                const float4 n4 = m.vol_frame[nd.w * 3];
                if (nrm.x == n4.x && nrm.y == n4.y && nrm.z == n4.z) {
                    best = (int)nd.w;
                    best_d = d;
                }
            }
        } else {
            const float pc = (nd.z == 0u) ? pos.x : ((nd.z == 1u) ? pos.y : pos.z);
            const float delta = pc - __uint_as_float(nd.x);
            const bool near_split = (delta * delta) < m.max_dist;
            const int left = (int)nd.y;
            const int nearc = delta < 0.0f ? left : left + 1;
            if (near_split) st[(sp++) * 64] = (left + left + 1) - nearc;
            st[(sp++) * 64] = nearc;
        }
    }
    return best;
}

// The same volume as sarsa_nearest, from the per-normal grid when that is provably
// equal (rt_sarsa_host.cpp NearestGrid): the nearest same-normal volume among the
// 3x3x3 cells around pos, if its distance is below grid_h (so the KD walk visits it)
// and no other candidate has the same float distance (the KD walk's order would
// break the tie).  cls: normal class of the hit surface (-1: no volume has its
// normal, the KD walk keeps volume 0).  Otherwise kNeedWalk: the KD walk decides
// (sarsa_resolve_walks).
constexpr int kNeedWalk = -2;  // sarsa_nearest_grid: only the KD walk decides this query

// G, D: the class grid's origin (w: first cell, bits) and cells per axis
__device__ int sarsa_nearest_grid_gd(const SarsaMap& m, float4 G, int4 D, f3 pos) {
    {
        const float ic = m.grid_inv_cs;
        // padded cell of the query (rt_sarsa_host.cpp grid_cell): its list holds every
        // class volume of the 3x3x3 neighbourhood
        const int ix = (int)floorf(fminf(fmaxf((pos.x - G.x) * ic, 0.0f), (float)(D.x - 1)));
        const int iy = (int)floorf(fminf(fmaxf((pos.y - G.y) * ic, 0.0f), (float)(D.y - 1)));
        const int iz = (int)floorf(fminf(fmaxf((pos.z - G.z) * ic, 0.0f), (float)(D.z - 1)));
        const uint32_t c = __float_as_uint(G.w) + (uint32_t)((iz * D.y + iy) * D.x + ix);
        uint32_t k0, e;
        // the cell's range and first three candidates as one 64-B record
        const float4* hp = m.cell_head + (size_t)c * 4;
        const float4 h0 = hp[0];
        const float4 H[3] = {hp[1], hp[2], hp[3]};
        k0 = __float_as_uint(h0.x);
        e = __float_as_uint(h0.y);
        // The list is sorted by distance to the cell centre C: d(q, L) >= d(C, L) - d(q, C),
        // so once d(C, L) exceeds best + d(q, C) (with a 2^-12 margin: such a candidate's
        // float distance is strictly above the best, no tie either) no later one can win.
        const float cx = G.x + ((float)ix + 0.5f) * m.grid_cs;
        const float cy = G.y + ((float)iy + 0.5f) * m.grid_cs;
        const float cz = G.z + ((float)iz + 0.5f) * m.grid_cs;
        const float qx = pos.x - cx, qy = pos.y - cy, qz = pos.z - cz;
        const float dq = __builtin_sqrtf((qx * qx + qy * qy) + qz * qz);
        float b1 = INFINITY, b2 = INFINITY;
        int bv = -1;
        uint32_t kb = k0;
        // the cell record's own first three candidates (no break test before the first
        // candidates: the limit is infinite there); the scan goes on from the fourth.  Where
        // the scan's batches start does not change its answer: the break only skips
        // candidates that can neither win nor tie.
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const float dx = H[u].x - pos.x, dy = H[u].y - pos.y, dz = H[u].z - pos.z;
            const float s = (dx * dx + dy * dy) + dz * dz;  // len3's sum
            if (k0 + (uint32_t)u < e) {
                if (s < b1) {
                    b2 = b1;
                    b1 = s;
                    bv = __float_as_int(H[u].w);
                } else if (s < b2) {
                    b2 = s;
                }
            }
        }
        kb = k0 + 3;
        for (uint32_t k = kb; k < e; k += 4) {  // 4 candidate loads in flight
            float4 L[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) L[u] = m.grid_leaf[min(k + (uint32_t)u, e - 1u)];
            {
                const float lim = (__builtin_sqrtf(b1) + dq) * (1.0f + 0x1p-12f) + 1e-6f;
                const float ex = L[0].x - cx, ey = L[0].y - cy, ez = L[0].z - cz;
                if ((ex * ex + ey * ey) + ez * ez > lim * lim) break;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float dx = L[u].x - pos.x, dy = L[u].y - pos.y, dz = L[u].z - pos.z;
                const float s = (dx * dx + dy * dy) + dz * dz;  // len3's sum
                if (k + (uint32_t)u < e) {
                    if (s < b1) {
                        b2 = b1;
                        b1 = s;
                        bv = __float_as_int(L[u].w);
                    } else if (s < b2) {
                        b2 = s;
                    }
                }
            }
        }
        const float d = sqrtf(b1);
        if (bv >= 0 && d < m.grid_h && sqrtf(b2) != d) {
            const float d0 = len3(pos.x - m.root_x, pos.y - m.root_y, pos.z - m.root_z);
            return d < d0 ? bv : 0;
        }
        if (m.grid_fallbacks != nullptr) atomicAdd(m.grid_fallbacks, 1ull);
    }
    return kNeedWalk;
}

// cls: normal class of the query (-1: no volume has its normal -- the KD walk keeps volume 0)
__device__ int sarsa_nearest_grid(const SarsaMap& m, int cls, f3 pos, f3 nrm) {
    (void)nrm;
    if (cls < 0) return 0;
    return sarsa_nearest_grid_gd(m, m.class_org[cls], m.class_dim[cls], pos);
}

// the same for a hit on surface tri: its class's grid descriptor in one per-surface record
// (two independent loads instead of the class, then its descriptor)
__device__ int sarsa_nearest_grid_tri(const SarsaMap& m, int tri, f3 pos, f3 nrm) {
    const float4 G = m.tri_grid[2 * tri];
    const float4 Df = m.tri_grid[2 * tri + 1];
    const int4 D = make_int4(__float_as_int(Df.x), __float_as_int(Df.y), __float_as_int(Df.z), __float_as_int(Df.w));
    if (D.w < 0) return 0;
    return sarsa_nearest_grid_gd(m, G, D, pos);
}

constexpr int kKdFront = kKdStack * 32;  // frontier entries per buffer: two fill a wave's stack block

// sarsa_nearest for ONE query (pos, nrm: wave-uniform values) walked by the whole wave.
// The walk of sarsa_nearest visits a node iff every ancestor's split lets it through
// ((q_k - split)^2 < MAX_DIST for the far child), which does not depend on the best found
// so far: the visited leaves are a fixed set.  Here the wave expands that set level by
// level (breadth first, one node per lane and step, the frontier in the wave's LDS block)
// instead of one dependent load per visited node on one lane.  The walk's answer is the
// first leaf in its visit order with the smallest distance (same len3) and the query's
// normal, if that distance is below the start distance d0, else volume 0: equal here
// unless two visited leaves share the smallest distance (then the order decides) -- *ok is
// false then, on a frontier overflow and for a non-finite query, and the caller walks.
// All lanes of the wave take part; blk = the wave's kKdStack x 64 block.
__device__ int sarsa_nearest_wave(const SarsaMap& m, f3 pos, f3 nrm, int* blk, int lane, bool* ok) {
    const uint4* __restrict__ kd = m.kd4;
    *ok = false;
    if (!(__builtin_isfinite(pos.x) && __builtin_isfinite(pos.y) && __builtin_isfinite(pos.z))) return 0;
    int* cur = blk;
    int* nxt = blk + kKdFront;
    wave_lds_sync();  // the block's previous use (stack, exact phase) is done
    if (lane == 0) cur[0] = 0;
    wave_lds_sync();
    int n = 1;
    float best_d = INFINITY;
    int best = -1;
    bool tie = false;
    while (n > 0) {
        int m_next = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int c0 = -1, c1 = -1;
            if (i < n) {
                const uint4 nd = kd[cur[i]];
                if (nd.w != 0xFFFFFFFFu) {  // leaf
                    const float d = len3(__uint_as_float(nd.x) - pos.x, __uint_as_float(nd.y) - pos.y,
                                         __uint_as_float(nd.z) - pos.z);
                    if (d <= best_d) {
                        const float4 n4 = m.vol_frame[nd.w * 3];
                        if (nrm.x == n4.x && nrm.y == n4.y && nrm.z == n4.z) {
                            tie = (d == best_d);
                            if (d < best_d) {
                                best_d = d;
                                best = (int)nd.w;
                            }
                        }
                    }
                } else {
                    const float pc = (nd.z == 0u) ? pos.x : ((nd.z == 1u) ? pos.y : pos.z);
                    const float delta = pc - __uint_as_float(nd.x);
                    const int left = (int)nd.y;
                    c0 = delta < 0.0f ? left : left + 1;
                    if ((delta * delta) < m.max_dist) c1 = (left + left + 1) - c0;
                }
            }
            // append the children: exclusive prefix of the lanes' counts (0..2) by ballots
            const int cnt = (c0 >= 0 ? 1 : 0) + (c1 >= 0 ? 1 : 0);
            const uint64_t b0 = __ballot(cnt & 1), b1 = __ballot(cnt >> 1);
            const int excl = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                             2 * (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
            const int tot = __builtin_popcountll(b0) + 2 * __builtin_popcountll(b1);
            if (m_next + tot > kKdFront) return 0;  // (wave-uniform) overflow: the caller walks
            if (c0 >= 0) nxt[m_next + excl] = c0;
            if (c1 >= 0) nxt[m_next + excl + 1] = c1;
            m_next += tot;
        }
        wave_lds_sync();  // the next level is written before any lane reads it
        int* t = cur;
        cur = nxt;
        nxt = t;
        n = m_next;
    }
    // the smallest distance over the wave, and whether it is unique
    float g = best_d;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) g = fminf(g, __shfl_xor(g, off, 64));
    const bool at_min = best >= 0 && best_d == g;
    const uint64_t holders = __ballot(at_min), ties = __ballot(at_min && tie);
    wave_lds_sync();  // the frontier reads are done before the block's next use
    if (holders == 0ull) {  // no visited leaf has the normal: the start volume
        *ok = true;
        return 0;
    }
    if (__builtin_popcountll(holders) > 1 || ties != 0ull) return 0;  // the visit order decides
    const int src = __builtin_ctzll(holders);
    const int v = __shfl(best, src, 64);
    const float d0 = len3(pos.x - m.root_x, pos.y - m.root_y, pos.z - m.root_z);
    *ok = true;
    return g < d0 ? v : 0;
}

// every lane with *rv == kNeedWalk gets sarsa_nearest's volume: the wave walks the queries
// one after another (sarsa_nearest_wave), a lane whose query it cannot settle walks alone.
// All lanes take part.
__device__ void sarsa_resolve_walks(const SarsaMap& m, f3 pos, f3 nrm, int* rv, int* blk, int* st, int lane) {
    uint64_t need = __ballot(*rv == kNeedWalk);
    while (need != 0ull) {
        const int L = __builtin_ctzll(need);
        need &= need - 1ull;
        const f3 q = make3(__shfl(pos.x, L, 64), __shfl(pos.y, L, 64), __shfl(pos.z, L, 64));
        const f3 qn = make3(__shfl(nrm.x, L, 64), __shfl(nrm.y, L, 64), __shfl(nrm.z, L, 64));
        bool ok;
        const int v = sarsa_nearest_wave(m, q, qn, blk, lane, &ok);
        if (lane == L && ok) *rv = v;
    }
    if (*rv == kNeedWalk) *rv = sarsa_nearest(m, pos, nrm, st);
}

}  // namespace

}  // namespace rt
