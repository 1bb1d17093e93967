// rt_kernels.hip — gfx950 kernels of the path tracer's hot path.
//
//  k_intersect : Ray::closest_intersection over a batch of rays (one lane per
//                ray) — the reference's innermost loop (CPU/rays/ray.cpp:14-28,
//                GPU/rays/ray.cu:16-141) as a standalone kernel.
//  k_render    : the per-pixel trace loop (pixel -> SPP -> bounce) as one
//                megakernel: camera ray, closest hit, uniform-hemisphere
//                sampling, Lambertian estimator, SPP mean
//                (CPU/path_tracing/default_path_tracing.cpp:5-101,
//                GPU/path_tracing/default_path_tracing.cu:7-88).
//
// CDNA4 mapping:
//  * one lane = one (pixel, sample chunk); a pixel's `split` chunks sit in
//    adjacent lanes and are folded with wave shuffles in a fixed order; a
//    16x16 pixel block is `split` workgroups of 256 threads.  A lane runs its
//    chunk's samples in order and
//    regenerates a camera ray the moment its path ends, so every lane casts a
//    ray on every loop trip until its pixel is done (no idle lanes waiting
//    for the longest path of the wave); the loop exit is a wave ballot.
//  * the triangle loop index is wave-uniform: the triangle records are
//    fetched with scalar loads (s_load_dwordx4) into SGPRs and broadcast as
//    VALU operands — no LDS round trip and no per-lane address math.
//  * per-pixel sums are kept in registers in sample order, so the image is
//    bit-identical to the CPU restatement (oracle/) and to any tiling.
//
// Numerics: built with -ffp-contract=off and hipcc's default correctly
// rounded fp32 division / sqrt; no fast-math (see rt_math.hpp).

#include <float.h>

#include <type_traits>

#include "rt_paths.hpp"

namespace rt {

namespace {

template <int RULE>
__global__ __launch_bounds__(256) void k_intersect(const DeviceScene s, int use_filter,
                                                   const int32_t* __restrict__ code,
                                                   const float* __restrict__ orig,
                                                   const float* __restrict__ dir, int n,
                                                   float t_scale, float* __restrict__ out_t,
                                                   int32_t* __restrict__ out_hit) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const f3 o = make3(orig[3 * r + 0], orig[3 * r + 1], orig[3 * r + 2]);
    const f3 d = make3(dir[3 * r + 0], dir[3 * r + 1], dir[3 * r + 2]);
    const Hit h = closest_hit_sel<RULE>(s, use_filter, o, d, t_scale);
    out_t[r] = (h.tri >= 0) ? h.t : __builtin_inff();
    out_hit[r] = (h.tri >= 0) ? code[h.tri] : -1;
}

// The matrix-core filter on caller rays (rt_intersect_method): every lane of a wave
// takes part, lanes past n cast a dummy ray with no candidates.  cand (optional): the
// candidates of each ray that reached the exact test.
template <int RULE>
__global__ __launch_bounds__(256) void k_intersect_mf(const DeviceScene s, const int32_t* __restrict__ code,
                                                      const float* __restrict__ orig,
                                                      const float* __restrict__ dir, int n, float t_scale,
                                                      float* __restrict__ out_t, int32_t* __restrict__ out_hit,
                                                      int32_t* __restrict__ cand) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    const f3 o = in ? make3(orig[3 * r + 0], orig[3 * r + 1], orig[3 * r + 2]) : make3(0.0f, 0.0f, 0.0f);
    const f3 d = in ? make3(dir[3 * r + 0], dir[3 * r + 1], dir[3 * r + 2]) : make3(0.0f, 0.0f, 1.0f);
    __shared__ float wls[4][kMfWaveFloats];
    int nc = 0;
    const Hit h = closest_hit_mf<RULE, true>(s, o, d, t_scale, in, wls[threadIdx.x >> 6], &nc);
    if (!in) return;
    out_t[r] = (h.tri >= 0) ? h.t : __builtin_inff();
    out_hit[r] = (h.tri >= 0) ? code[h.tri] : -1;
    if (cand != nullptr) cand[r] = nc;
}

// The candidate route on caller rays (rt_intersect_cand): every lane of a wave takes part,
// lanes past n hold no candidates (F = 0).  surf != nullptr: the candidates from the scene's
// table as a bounce ray leaving surf[r] gets them (closest_hit_ctab; out_masks, optional:
// what the lookup gave, `words` per ray); else the caller's masks_in (closest_hit_cand, as
// k_render_pq<.., CT> feeds it the rectangle cull's masks).  Each wave's LDS block is exactly
// mf_wave_floats(CAP, RULE) floats and the four are adjacent, as in the render kernels of
// the same instantiation: a write past a block lands in the next wave's rays.
template <int RULE, int NW, int CAP>
__global__ __launch_bounds__(256) void k_intersect_cand(const DeviceScene s, const int32_t* __restrict__ code,
                                                        const float* __restrict__ orig,
                                                        const float* __restrict__ dir, int n, float t_scale,
                                                        const int32_t* __restrict__ surf,
                                                        const unsigned long long* __restrict__ masks_in, int words,
                                                        float* __restrict__ out_t, int32_t* __restrict__ out_hit,
                                                        unsigned long long* __restrict__ out_masks) {
    constexpr int wf = mf_wave_floats(CAP, RULE);
    static_assert(wf % 2 == 0, "the blocks' 64-bit keys and masks stay aligned");
    __shared__ __attribute__((aligned(16))) float wls[4 * wf];
    float* wl = wls + (threadIdx.x >> 6) * wf;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    const f3 o = in ? make3(orig[3 * r + 0], orig[3 * r + 1], orig[3 * r + 2]) : make3(0.0f, 0.0f, 0.0f);
    const f3 d = in ? make3(dir[3 * r + 0], dir[3 * r + 1], dir[3 * r + 2]) : make3(0.0f, 0.0f, 1.0f);
    Hit h;
    if (surf != nullptr) {  // (wave-uniform)
        const CtabDev& T = s.ctab[RULE];
        const int sf = in ? surf[r] : -1;
        if (in && out_masks != nullptr) {
            uint64_t F[NW];
            ctab_candidates<NW>(T, s.n_tri, s.n_surf, sf, o, d, F);
#pragma unroll
            for (int k = 0; k < NW; ++k)
                if (k < words) out_masks[(size_t)r * words + k] = F[k];
        }
        h = closest_hit_ctab<RULE, NW, CAP>(s, T, sf, o, d, t_scale, in, wl);
    } else {
        uint64_t F[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) F[k] = (in && k < words) ? masks_in[(size_t)r * words + k] : 0ull;
        h = closest_hit_cand<RULE, NW, CAP>(s, F, o, d, t_scale, wl);
    }
    if (!in) return;
    out_t[r] = (h.tri >= 0) ? h.t : __builtin_inff();
    out_hit[r] = (h.tri >= 0) ? code[h.tri] : -1;
}

// The exact BVH path on caller rays (large scenes).
template <int RULE>
__global__ __launch_bounds__(256) void k_intersect_bvh(const DeviceScene s, const int32_t* __restrict__ code,
                                                       const float* __restrict__ orig, const float* __restrict__ dir,
                                                       int n, float t_scale, float* __restrict__ out_t,
                                                       int32_t* __restrict__ out_hit) {
    __shared__ int stk[kBvhMaxDepth * 256];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const f3 o = make3(orig[3 * r + 0], orig[3 * r + 1], orig[3 * r + 2]);
    const f3 d = make3(dir[3 * r + 0], dir[3 * r + 1], dir[3 * r + 2]);
    const Hit h = closest_hit_bvh<RULE>(s, o, d, t_scale, stk + threadIdx.x);
    out_t[r] = (h.tri >= 0) ? h.t : __builtin_inff();
    out_hit[r] = (h.tri >= 0) ? code[h.tri] : -1;
}




// PRESET 0: CPU engine recursion (a path's value is folded from the light
// back to the camera: L_k = ((L_{k+1} * brdf_k) * cos_k) / rho), cap <= 2.
// PRESET 1: GPU engine iterative throughput.
//
// STEAL: the lanes of a pixel share its samples instead of owning fixed chunks: a lane
// whose path ends claims the pixel's next unclaimed sample (ballot + mbcnt rank), so
// no lane idles while another finishes a long chunk (with fixed chunks the wave runs
// for the longest chunk: ~90% lane use at 4 samples per lane).  Each sample's value
// goes to LDS; at the end lane c sums samples [c m, (c + 1) m) in order, exactly the
// chunk sum of the fixed assignment, so the image is bit-identical.
//
// BVH: large scenes cast through closest_hit_bvh (the exact BVH path: same hits as the
// scan).
//
// MF (> 0: 64-triangle blocks per super-block): every cast on the matrix-core filter
// (closest_hit_mf, wave-level: lanes without a live sample take part with no
// candidates), as the bounce casts of k_render_ps; the launcher picks it when the camera
// lies inside the image's origin bound (else every camera ray would keep every triangle).
template <int PRESET, int SAMPLER, int RULE, bool STEAL, bool BVH, int MF = 0>
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 1
#endif
#ifndef RT_MF_RENDER_WAVES
#define RT_MF_RENDER_WAVES 4  // occupancy floor of the MF variants (<= 128 VGPRs; 1: the compiler's 142-150)
#endif
__global__ __launch_bounds__(256, MF > 0 ? RT_MF_RENDER_WAVES : RT_MIN_WAVES) void k_render(const RenderLaunch a) {
    extern __shared__ float s_val[];  // STEAL: [pixel of the workgroup][spp][3]
    __shared__ int s_stk[BVH ? kBvhMaxDepth * 256 : 1];
    __shared__ float s_mfw[MF > 0 ? 4 * kMfWaveFloats : 1];  // MF: the waves' exact-phase LDS
    // workgroup -> (16x16 block, part); lane -> (pixel of the block, sample chunk)
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    const int part = blockIdx.x & (a.split - 1);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int chunk = threadIdx.x & (a.split - 1);
    const int lane = threadIdx.x & 63;
    const int lx = q & 15;
    const int ly = q >> 4;
    const int px = blk.px0 + lx;
    const int py = blk.py0 + ly;
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    const uint32_t pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const int s_end = STEAL ? a.spp : (chunk + 1) * a.per_chunk;
    float* const pvals = STEAL ? s_val + (size_t)((int)threadIdx.x >> lg) * a.spp * 3 : nullptr;
    const int gbase = lane & ~(a.split - 1);  // first lane of this pixel's group
    const unsigned long long gmask = (a.split == 64) ? ~0ull : ((1ull << a.split) - 1ull);
    int next = a.split;                       // STEAL: the pixel's next unclaimed sample

    int s = valid ? (STEAL ? chunk : chunk * a.per_chunk) : s_end;  // current sample
    int depth = 0;              // surface bounces so far on this path
    f3 o = make3(a.cam_x, a.cam_y, a.cam_z);
    f3 d = make3(0.0f, 0.0f, 1.0f);
    f3 acc = make3(0.0f, 0.0f, 0.0f);
    f3 tp = make3(1.0f, 1.0f, 1.0f);     // PRESET 1 throughput
    int f_tri0 = 0, f_tri1 = 0;          // PRESET 0 factors (cap <= 2)
    float f_cos0 = 0.0f, f_cos1 = 0.0f;
    unsigned n_casts = 0;

    if (s < s_end) {
        float r1, r2;
        draw2(pix, (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
        camera_ray<PRESET>(a, px, py, r1, r2, &d);
    }
    // MF with the camera outside the image's bound: camera rays take the wave's cull
    uint64_t cm[kRenderCullWords] = {0ull, 0ull, 0ull, 0ull};
    if (MF > 0 && a.cam_cull && __ballot(valid) != 0ull) wave_candidates<RULE>(a, valid, px, py, lane, cm);

    for (;;) {
        const bool active = s < s_end;
        if (__ballot(active) == 0ull) break;
        Hit h;
        if constexpr (MF > 0) {
            h = closest_hit_mf<RULE, false, MF>(a.scene, o, d, a.t_scale, active,
                                                s_mfw + ((int)threadIdx.x >> 6) * kMfWaveFloats, nullptr, nullptr,
                                                a.cam_cull ? cm : nullptr, depth == 0);
            if (!active) continue;
        } else {
            if (!active) continue;
            h = BVH ? closest_hit_bvh<RULE>(a.scene, o, d, a.t_scale, s_stk + threadIdx.x)
                    : closest_hit_sel<RULE>(a.scene, a.use_filter, o, d, a.t_scale);
        }
        ++n_casts;

        bool terminal = false;
        f3 L = make3(0.0f, 0.0f, 0.0f);
        if (h.tri < 0) {
            terminal = true;
            if (PRESET == 1) L = make3(tp.x * a.env_light, tp.y * a.env_light, tp.z * a.env_light);
        } else if (h.tri >= n_surf) {
            terminal = true;
            const float4 e = shade[h.tri * kShadeF4 + 3];
            if (PRESET == 0) {
                L = make3(e.x, e.y, e.z);
                if (depth >= 2) {
                    const float4 c = shade[f_tri1 * kShadeF4 + (SAMPLER == 0 ? 3 : 4)];
                    if (SAMPLER == 0) {
                        L.x = div_rho((L.x * c.x) * f_cos1);
                        L.y = div_rho((L.y * c.y) * f_cos1);
                        L.z = div_rho((L.z * c.z) * f_cos1);
                    } else {
                        L = make3(L.x * c.x, L.y * c.y, L.z * c.z);
                    }
                }
                if (depth >= 1) {
                    const float4 c = shade[f_tri0 * kShadeF4 + (SAMPLER == 0 ? 3 : 4)];
                    if (SAMPLER == 0) {
                        L.x = div_rho((L.x * c.x) * f_cos0);
                        L.y = div_rho((L.y * c.y) * f_cos0);
                        L.z = div_rho((L.z * c.z) * f_cos0);
                    } else {
                        L = make3(L.x * c.x, L.y * c.y, L.z * c.z);
                    }
                }
            } else {
                L = make3(tp.x * e.x, tp.y * e.y, tp.z * e.z);
            }
        } else if (PRESET == 0 && depth == a.max_bounces) {
            terminal = true;  // bounces == MAX_RAY_BOUNCES -> vec3(0)
        } else {
            // surface: position, sample a direction, update the estimator
            f3 pos, sd;
            const float cos_theta = bounce_direction<SAMPLER>(h, o, d, a.t_scale, shade, pix, (uint32_t)s, depth, a.seed_lo,
                                                              a.seed_hi, &pos, &sd);
            if (PRESET == 0) {
                if (depth == 0) {
                    f_tri0 = h.tri;
                    f_cos0 = cos_theta;
                } else {
                    f_tri1 = h.tri;
                    f_cos1 = cos_theta;
                }
            } else {
                tp = bounce_throughput<SAMPLER>(tp, shade, h.tri, cos_theta);
            }
            o = make3(pos.x + kEps * sd.x, pos.y + kEps * sd.y, pos.z + kEps * sd.z);
            d = normalize(sd);
            ++depth;
            if (PRESET == 1 && depth == a.max_bounces) terminal = true;  // loop exhausted -> 0
        }

        if (STEAL) {
            const unsigned long long m = (__ballot(terminal) >> gbase) & gmask;
            if (terminal) {
                pvals[s * 3 + 0] = L.x;
                pvals[s * 3 + 1] = L.y;
                pvals[s * 3 + 2] = L.z;
                s = next + __popcll(m & ((1ull << chunk) - 1ull));
            }
            next += __popcll(m);
        }
        if (terminal) {
            if (!STEAL) {
                acc.x = acc.x + L.x;
                acc.y = acc.y + L.y;
                acc.z = acc.z + L.z;
                ++s;
            }
            depth = 0;
            tp = make3(1.0f, 1.0f, 1.0f);
            o = make3(a.cam_x, a.cam_y, a.cam_z);
            if (s < s_end) {
                float r1, r2;
                draw2(pix, (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
                camera_ray<PRESET>(a, px, py, r1, r2, &d);
            }
        }
    }

    if (STEAL) {
        // every sample of the pixel was computed by a lane of this wave
        __syncthreads();
        if (valid) {
            for (int k = chunk * a.per_chunk; k < (chunk + 1) * a.per_chunk; ++k) {
                acc.x = acc.x + pvals[k * 3 + 0];
                acc.y = acc.y + pvals[k * 3 + 1];
                acc.z = acc.z + pvals[k * 3 + 2];
            }
        }
    }
    // fold the chunk sums of a pixel in chunk order: ((P0 + P1) + P2) + ...
    const int base = gbase;
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
    if (a.casts != nullptr) {
        const unsigned total = wave_sum(n_casts);
        if (lane == 0) atomicAdd(a.casts, (unsigned long long)total);
    }
}

// ---- GPU preset: a persistent grid over a queue of (pixel, chunk) work items ----
// k_render gives each wave a fixed set of pixels: once their samples are out, the wave's
// lanes idle until its longest path (up to 80 casts) ends -- 3.21 MFMAs per cast against
// the 2.63 of full waves on complex_light_room, and sample stealing within the wave does
// not help.  Here a lane claims a chunk (pixel p, chunk c: samples
// [c m, (c + 1) m), m = spp / split) from a launch-wide queue, traces its samples one after
// another summing their values in sample order (k_render's fixed-chunk sum, bit for bit),
// stores the chunk sum and claims the next; lanes idle only at the end of the whole launch.
// k_fold_chunks then adds each pixel's chunk sums in chunk order (((P0 + P1) + P2) + ...)
// and divides by spp, as k_render's fold does.  The wave takes items 64 at a time from the
// global counter (one atomic per 64 chunks) and hands them to its lanes by ballot rank.
// Camera inside the matrix-core image's bound, MF > 0.
// CT: the casts take their candidates from tables instead of the matrix-core filter -- a
// camera ray the cull of its pixel's 16x4 rectangle (rect_cull, k_cull_ps over the launch's
// blocks, a.cull), a bounce ray the candidate table of the surface it leaves (ctab_candidates,
// rt_ctab.cpp) -- and closest_hit_cand tests them in index order: the same hit.
#ifndef RT_PQ_CT_WAVES
#define RT_PQ_CT_WAVES 8  // waves per SIMD of the table route's persistent grid (complex_light_room 2048^2 x 64: 4 / 6 / 8 -> 640 / 536 / 517 ms: its lookups' latency)
#endif
template <int SAMPLER, int RULE, int MF, bool CT = false>
__global__ __launch_bounds__(256, CT ? RT_PQ_CT_WAVES : RT_MF_RENDER_WAVES) void k_render_pq(const RenderLaunch a) {
    __shared__ __attribute__((aligned(16))) float s_mfw[4 * kMfWaveFloats];
    float* const wl = s_mfw + ((int)threadIdx.x >> 6) * kMfWaveFloats;
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    const long long total = (long long)a.n_blocks * 256 * a.split;
    const f3 cam = make3(a.cam_x, a.cam_y, a.cam_z);
    long long qb = 0, qe = 0;  // wave-uniform: the wave's claimed, not yet handed out items
    bool exhausted = false;     // wave-uniform: the launch's queue is empty
    bool have = false;          // the lane holds a chunk
    long long item = 0;
    int s = 0, s_end = 0, px = 0, py = 0;
    uint32_t pix = 0;
    int depth = 0;
    int surf = -1, cidx = 0;  // CT: the surface the ray leaves; the pixel's rectangle in a.cull
    f3 o = cam, d = make3(0.0f, 0.0f, 1.0f), tp = make3(1.0f, 1.0f, 1.0f), acc = make3(0.0f, 0.0f, 0.0f);
    unsigned n_casts = 0;
    auto camera = [&]() {
        float r1, r2;
        draw2(pix, (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
        camera_ray<1>(a, px, py, r1, r2, &d);
        o = cam;
        tp = make3(1.0f, 1.0f, 1.0f);
        depth = 0;
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
                        const long long p = j >> a.split_log2;
                        const int c = (int)(j & (a.split - 1));
                        const BlockDesc blk = a.blocks[p >> 8];
                        const int q = (int)(p & 255);
                        px = blk.px0 + (q & 15);
                        py = blk.py0 + (q >> 4);
                        if (px < a.clip_x1 && py < a.clip_y1) {  // (a clipped pixel's chunks: nothing)
                            pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
                            cidx = (int)(p >> 8) * 4 + (q >> 6);
                            s = c * a.per_chunk;
                            s_end = s + a.per_chunk;
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
        Hit h;
        if constexpr (CT) {
            constexpr int NW = MF;
            uint64_t F[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) F[k] = 0ull;
            if (active && depth == 0) {
#pragma unroll
                for (int k = 0; k < NW; ++k)
                    F[k] = (k < kRenderCullWords) ? a.cull[(size_t)cidx * kRenderCullWords + k] : 0ull;
            } else if (active) {
                ctab_candidates<NW>(a.scene.ctab[RULE], a.scene.n_tri, n_surf, surf, o, d, F);
            }
            h = closest_hit_cand<RULE, NW>(a.scene, F, o, d, a.t_scale, wl);
        } else {
            h = closest_hit_mf<RULE, false, MF>(a.scene, o, d, a.t_scale, active, wl);
        }
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
            surf = surface_step<SAMPLER>(h, o, d, tp, a.t_scale, shade, pix, (uint32_t)s, depth, a.seed_lo, a.seed_hi);
            ++depth;
            if (depth == a.max_bounces) terminal = true;  // loop exhausted -> 0
        }
        if (terminal) {
            acc.x = acc.x + L.x;
            acc.y = acc.y + L.y;
            acc.z = acc.z + L.z;
            ++s;
            if (s < s_end) {
                camera();
            } else {
                store_rgb(a.csum + (size_t)item * 3, acc.x, acc.y, acc.z);
                have = false;
            }
        }
    }
    if (a.casts != nullptr) {
        const unsigned tot = wave_sum(n_casts);
        if (lane == 0) atomicAdd(a.casts, (unsigned long long)tot);
    }
}

// the pixels of k_render_pq's launch: chunk sums in chunk order, / spp (k_render's fold)
__global__ __launch_bounds__(256) void k_fold_chunks(const RenderLaunch a) {
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

// k_render_ps: the CPU-engine preset (PRESET 0) in two phases per wave.
//
// Primary rays are a known family: the camera position and the pixel rectangle of the
// wave bound every direction, so a triangle whose filter certainly rejects all of them
// (rect_cull, rt_trace.hpp) cannot be hit by any of them.  Phase P traces every sample's
// primary ray of the lane against the few remaining candidates only (exact test, index
// order: the reference's hit bit for bit) and parks the result in LDS: the direction and
// hit of a path that continues, or the value of one that ends at its first cast.  Phase S
// is the bounce loop of k_render without camera rays: when a path ends, the lane takes
// its next sample's primary hit from LDS (adding the values of samples that ended at the
// first cast on the way, in sample order) and shades it, so every trip casts a secondary
// ray on every live lane.  The image, the ray casts and the sum order are those of
// k_render<0, ...> (oracle/ parity); PRESET 0 paths are 1-3 casts, so about 37% of the
// casts of the frame move from the full-scene scan to a few exact tests.
//
// LDS: per wave and sample slot k, three 64-lane float rows (lane-contiguous: conflict-free)
// and one int16 row of hit codes:
//   continuing: the hit point x, y, z, triangle;  ended: L.x, L.y, L.z, -1.
// (int16 codes: 13 KB of slots per 256-lane workgroup at 4 samples per lane instead of 16 KB --
// with the table route's pair list that is 25.6 KB per workgroup, six per CU; the table-route
// variant's codes are bytes, ps_wave_floats)
constexpr int kPsFields = 3;     // float rows per sample slot
constexpr int kPsPrimBatch = 4;  // samples per candidate pass of phase P
constexpr int kPsSplitLights = 8;  // the light pre-test runs when the scene has at most this many light triangles
// floats of LDS per wave: the sample slots' float rows, their int16 codes, then the wave's
// queue of continuing samples, one u16 (k << 6 | lane) per slot.
// narrow (the table-route variant up to kPsNarrowChunk samples per lane: its codes are triangles
// below 64 or -1, its entries k << 6 | lane below 256): a byte per code and per entry, the block
// rounded up to 256 bytes (ps_finish reads the wave's first rows 16 bytes at a time).  The
// layout is a constant of the kernel's template (NARROW), chosen by the launcher: picked at run
// time inside one kernel, the two queue paths cost the bench frame 2 % (DESIGN.md section 7,
// round 12).
constexpr int kPsNarrowChunk = 4;
__host__ __device__ constexpr bool ps_narrow(bool ct, int pc) { return ct && pc <= kPsNarrowChunk; }
// one pixel per wave (k_render_ps's ONEPX instances, of the narrow layout): the 64 lanes of a wave
// are the 64 chunks of one pixel
__host__ __device__ constexpr bool ps_onepx(bool narrow, int split) { return narrow && split == 64; }
__host__ __device__ constexpr int ps_wave_floats(int pc, bool narrow) {
    return narrow ? (pc * kPsFields * 64 + pc * 16 + pc * 16 + 63) & ~63 : pc * kPsFields * 64 + pc * 32 + pc * 32;
}
// The table-route variant's shading records in LDS, kPsFrameF4 rows per triangle:
// [N.xyz, F.x] [T.xyz, F.y] [B.xyz, F.z] -- the frame, and in the w lanes the one colour a fold
// reads there: a surface's fold row for the kernel's sampler, a light's emission
constexpr int kPsFrameF4 = 3;
#ifndef RT_PS_PASS_MIN
// pending samples at which a trip of the table-route variant's pipelined loop runs a pre-test
// pass (ps_body; 1: in every trip that has any)
#define RT_PS_PASS_MIN 64
#endif
constexpr int kPsPassMin = RT_PS_PASS_MIN;
// (a trip adds at most 64 samples to fewer than kPsPassMin left pending: under 128, two registers)
static_assert(kPsPassMin >= 1 && kPsPassMin <= 64, "the pending list holds what a trip can leave pending");
static_assert(ps_wave_floats(4, true) == 896, "the narrow wave block at 4 samples per lane");
static_assert(ps_wave_floats(3, true) % 64 == 0 && ps_wave_floats(1, true) % 64 == 0, "wave blocks are 256-byte multiples");


// The rectangle-independent half of the primary-ray cull (cull_forms, rt_cull.hpp), one thread
// per triangle: row k of triangle i to forms[k * kCullFormStride + i].  Threads past the scene
// zero their column, so every lane of a cull wave reads initialised rows.
__global__ __launch_bounds__(kCullFormStride) void k_cull_forms(const float4* __restrict__ filt, int n_tri,
                                                               const CamConst k, float4* __restrict__ forms) {
    const int i = threadIdx.x;
    float4 r[kCullFormRows];
    if (i < n_tri) {
        cull_forms_rows(cull_forms(filt + (size_t)i * kFiltF4, k), r);
    } else {
        for (int j = 0; j < kCullFormRows; ++j) r[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    for (int j = 0; j < kCullFormRows; ++j) forms[j * kCullFormStride + i] = r[j];
}

// Candidate masks of the primary-ray phase: wave w of workgroup b writes
// cull[(b * 4 + w) * kRenderCullWords + g], bit j = triangle 64 g + j may be the hit of a
// camera ray through the wave's pixel rectangle (rect_cull, rt_trace.hpp).  Same grid
// and lane -> pixel mapping as k_render_ps.
// Candidate masks of the wave's pixel rectangle (the valid lanes' pixels): bit j of
// cm[g] = triangle 64 g + j may be the hit of a camera ray through the rectangle
// (rect_cull); never a bit past the scene.  All lanes of the wave take part.
// The masks alone, as k_render_ps computes them, into a.cull (wave w of workgroup b at
// words (b * 4 + w) * kRenderCullWords ..): the diagnostic rt_cull_masks_device.
// cf.forms (k_cull_forms' rows for this launch's camera): the split cull of k_render_ps; without,
// wave_candidates.
template <int RULE>
__global__ __launch_bounds__(256) void k_cull_ps(const RenderLaunch a, const CullLaunch cf) {
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    const int part = blockIdx.x & (a.split - 1);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int lane = threadIdx.x & 63;
    const int px = blk.px0 + (q & 15);
    const int py = blk.py0 + (q >> 4);
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    uint64_t cm[kRenderCullWords];
    if (__ballot(valid) == 0ull) {
        for (int g = 0; g < kRenderCullWords; ++g) cm[g] = 0ull;
    } else if (cf.forms != nullptr) {
        wave_candidates_forms<RULE>(a, cf, blk, q, lane, cm);
    } else {
        wave_candidates<RULE>(a, valid, px, py, lane, cm);
    }
    unsigned long long* w = a.cull + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kRenderCullWords;
    if (lane < kRenderCullWords) {
        uint64_t v = cm[0];
#pragma unroll
        for (int g = 1; g < kRenderCullWords; ++g) v = (lane == g) ? cm[g] : v;
        w[lane] = v;
    }
}

// The table-route kernel does not keep a light pre-test pass in its lane for the wave's next
// trip: the wave settles the pass on the spot (ps_body's pipelined loop).  Whether
// k_render_ps<.., MF, CT> is that variant (the name is from the pooled trip of the workgroup that
// traced the passes before, DESIGN.md section 7, rounds 7 and 10): a constant of the template, never
// chosen at run time
__host__ __device__ constexpr bool ps_pooled(int mf, bool ct) { return ct && mf == 1; }
// lane l's value of v (l wave-uniform)
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// the next direction from the surface hit (pos, hit_tri) at bounce depth dep of sample cur of
// pixel lpix: cos theta and the ray (o = pos + eps sd, d = normalize(sd)), sampled with the
// path's Philox draw
// (ps_shade_dir: with the surface's shading frame N, T, B in hand -- a caller that loads the
// records ahead of time, the pipelined loop)
// lpx: the Philox words of the sample's pixel (philox_pix).  The square roots and the normalize
// are the forms without range guards (sqrt_rn_pos, normalize_unit: rt_math.hpp), the same bits
// on the ranges the sampling has.
template <int SAMPLER>
__device__ __forceinline__ void ps_shade_dir(const RenderLaunch& a, const float4& N, const float4& T, const float4& B,
                                             const PhiloxPix& lpx, int cur, int dep, const f3& pos, float* cos_out,
                                             f3* o_out, f3* d_out) {
    float r1, r2;
    draw2_px(lpx, (uint32_t)cur, 1u + (uint32_t)dep, a.seed_lo, a.seed_hi, &r1, &r2);
    // r1 = k 2^-24, k < 2^24: r1 r1 <= 1 - 2^-23, so 1 - r1 r1 lies in [2^-23, 1]; r1 is +0 or in
    // [2^-24, 1), 1 - r1 in [2^-24, 1]
    float cos_theta, sin_theta;
    if (SAMPLER == 0) {
        cos_theta = r1;
        sin_theta = sqrt_rn_pos(1.0f - r1 * r1);
    } else {
        cos_theta = sqrt_rn_pos(r1);
        sin_theta = sqrt_rn_pos(1.0f - r1);
    }
    float sphi, cphi;
    sincos_turn(r2, &sphi, &cphi);
    const float sx = sin_theta * cphi, sz = sin_theta * sphi;
    const f3 sd = make3((sx * B.x + cos_theta * N.x) + sz * T.x,
                        (sx * B.y + cos_theta * N.y) + sz * T.y,
                        (sx * B.z + cos_theta * N.z) + sz * T.z);
    *cos_out = cos_theta;
    *o_out = make3(pos.x + kEps * sd.x, pos.y + kEps * sd.y, pos.z + kEps * sd.z);
    // sd = (sin cphi) B + cos N + (sin sphi) T on an orthonormal frame with sin^2 + cos^2 and
    // sphi^2 + cphi^2 within a few ulp of 1: dot(sd, sd) is 1 +- a few ulp
    *d_out = normalize_unit(sd);
}
// (LF: shade is the table-route variant's LDS copy, kPsFrameF4 rows per triangle)
template <int SAMPLER, bool LF = false>
__device__ __forceinline__ void ps_shade_hit(const RenderLaunch& a, const float4* __restrict__ shade,
                                             const PhiloxPix& lpx, int cur, int dep, const f3& pos, int hit_tri,
                                             float* cos_out, f3* o_out, f3* d_out) {
    constexpr int rows = LF ? kPsFrameF4 : kShadeF4;
    const float4 N = shade[hit_tri * rows + 0];
    const float4 T = shade[hit_tri * rows + 1];
    const float4 B = shade[hit_tri * rows + 2];
    ps_shade_dir<SAMPLER>(a, N, T, B, lpx, cur, dep, pos, cos_out, o_out, d_out);
}
// the colour in the w lanes of triangle tri's rows of the LDS copy (kPsFrameF4)
__device__ __forceinline__ float4 ps_frame_colour(const float4* __restrict__ frames, int tri) {
    return make_float4(frames[tri * kPsFrameF4 + 0].w, frames[tri * kPsFrameF4 + 1].w, frames[tri * kPsFrameF4 + 2].w,
                       0.0f);
}
// the emission of light triangle tri
template <bool LF = false>
__device__ __forceinline__ float4 ps_emission(const float4* __restrict__ shade, int tri) {
    if constexpr (LF)
        return ps_frame_colour(shade, tri);
    else
        return shade[tri * kShadeF4 + 3];
}
// folds the light L back through the bounce at surface tri whose direction had cos theta = c
template <int SAMPLER, bool LF = false>
__device__ __forceinline__ void ps_fold(const float4* __restrict__ shade, f3& L, int tri, float cosv) {
    float4 c;
    if constexpr (LF)
        c = ps_frame_colour(shade, tri);
    else
        c = shade[tri * kShadeF4 + (SAMPLER == 0 ? 3 : 4)];
    if (SAMPLER == 0) {
        L.x = div_rho((L.x * c.x) * cosv);
        L.y = div_rho((L.y * c.y) * cosv);
        L.z = div_rho((L.z * c.z) * cosv);
    } else {
        L = make3(L.x * c.x, L.y * c.y, L.z * c.z);
    }
}

// The keys of the sample behind queue entry e (k << 6 | lane) of a wave whose lane 0 holds
// pixel wq0 of the block: its pixel (the RNG key) and its sample index
struct PsKeys {
    uint32_t pix;
    int cur;
};
__device__ __forceinline__ PsKeys ps_owner_keys(const RenderLaunch& a, const BlockDesc& blk, int wq0, int e) {
    const int ol = e & 63, kk = e >> 6;
    const int oq = wq0 + (ol >> a.split_log2);  // the owner lane's pixel
    PsKeys key;
    key.pix = (uint32_t)(blk.py0 + (oq >> 4)) * (uint32_t)a.width + (uint32_t)(blk.px0 + (oq & 15));
    key.cur = (ol & (a.split - 1)) * a.per_chunk + kk;
    return key;
}
// the light pre-test of the ray (lo, ld): whether a light triangle passes the exact test without
// its t window (ps_body says what follows from it)
template <int RULE>
__device__ __forceinline__ bool ps_light_pass(const RenderLaunch& a, const DeviceScene& ms, const f3& lo, const f3& ld) {
    const float nDx = -(ld.x * a.t_scale), nDy = -(ld.y * a.t_scale), nDz = -(ld.z * a.t_scale);
    bool pass = false;
    for (int j = a.scene.n_surf; j < a.scene.n_tri; ++j)
        pass |= exact_tv<RULE>(ms.isect, j, lo, nDx, nDy, nDz) != __builtin_inff();
    return pass;
}

// the end of k_render_ps for one wave with at least one pixel: every lane sums its own slots
// in sample order onto acc (ended samples hold their value in fields 0..2), the
// chunk sums of a pixel fold in chunk order and the pixel is stored
// (wslots: the wave's block of ps_wave_floats floats)
__device__ __forceinline__ void ps_finish(const RenderLaunch& a, const BlockDesc& blk, float* wslots, int chunk, int lane,
                                          int lx, int ly, bool valid, f3 acc) {
    const int pc = a.per_chunk;
    const float* const slots = wslots + lane;
    for (int kk = 0; kk < pc; ++kk) {
        const float* sl = slots + kk * kPsFields * 64;
        acc.x = acc.x + sl[0 * 64];
        acc.y = acc.y + sl[1 * 64];
        acc.z = acc.z + sl[2 * 64];
    }
    // fold the chunk sums of a pixel in chunk order: ((P0 + P1) + P2) + ...
    const int base = lane & ~(a.split - 1);
    // From four chunks on, through LDS: the lanes park their sums in the wave's slot region
    // (row c of slot 0, position lane: the lane's own, already summed above) and the pixel's
    // lanes of chunk 0, 1 and 2 each walk one channel in chunk order -- the same additions on
    // the same operands as the shuffle fold below, which keeps all 64 lanes busy for
    // split - 1 dependent rounds of three cross-lane reads each.
    if (a.split >= 4) {
        float* const parkf = wslots;
        parkf[0 * 64 + lane] = acc.x;
        parkf[1 * 64 + lane] = acc.y;
        parkf[2 * 64 + lane] = acc.z;
        wave_lds_sync();
        if (valid && chunk < 3) {
            // four chunk sums per LDS read (the pixel's piece of the row starts on a multiple of
            // split >= 4 floats of a 256-byte-aligned row), added in the same order
            const float4* src = reinterpret_cast<const float4*>(parkf + chunk * 64 + base);
            float4 v = src[0];
            float t = ((v.x + v.y) + v.z) + v.w;
            for (int k4 = 1; k4 < (a.split >> 2); ++k4) {
                v = src[k4];
                t = ((t + v.x) + v.y) + v.z;
                t = t + v.w;
            }
            float* dst = a.out + ((size_t)(blk.oy0 + ly) * (size_t)a.out_pitch + (size_t)(blk.ox0 + lx)) * 3;
            dst[chunk] = t / (float)a.spp;
        }
        return;
    }
    f3 tot = acc;
    for (int kk = 1; kk < a.split; ++kk) {
        const float vx = __shfl(acc.x, base + kk, 64);
        const float vy = __shfl(acc.y, base + kk, 64);
        const float vz = __shfl(acc.z, base + kk, 64);
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

// the work of k_render_ps for one wave with at least one pixel; returns the lane's casts.
// CT: the bounce casts from the scene's candidate table (the launcher checked it serves this
// launch) -- the matrix-core path is not compiled in, so the kernel's registers allow more waves.
// NARROW: the launch's wave blocks are the narrow ones (ps_wave_floats; the launcher: ps_narrow).
// ONEPX: every lane of a wave holds the same pixel (split 64; the launcher: ps_onepx), so the pixel's
// Philox words are wave-uniform and the scalar unit computes them, once per wave.
template <int SAMPLER, int RULE, int MF, bool CT = false, bool NARROW = false, bool ONEPX = false>
__device__ __forceinline__ unsigned ps_body(const RenderLaunch& a, const CullLaunch& cf, const DeviceScene& ms,
                                            float* wl, const BlockDesc& blk, int q, int chunk, int lane, int lx, int ly, int px,
                                            int py, bool valid) {
    extern __shared__ float s_ps[];
    const uint32_t pix = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
    const float4* __restrict__ shade = ms.shade;  // (the workgroup's LDS copy, when the kernel staged one)
    const int n_surf = a.scene.n_surf;
    const int pc = a.per_chunk;
    // the table-route variant: shade is the kernel's LDS copy of the frames (kPsFrameF4), its slot
    // codes are bytes, and so are its queue's entries in the narrow layout (ps_wave_floats)
    constexpr bool LF = ps_pooled(MF, CT);
    static_assert(LF || !NARROW, "only the table-route variant has the narrow layout");
    static_assert(NARROW || !ONEPX, "one pixel per wave is an instance of the narrow layout only");
    constexpr bool narrow = NARROW;
    float* const wslots = s_ps + (size_t)(threadIdx.x >> 6) * ps_wave_floats(pc, narrow);
    float* const slots = wslots + lane;
    // a slot's hit code: the triangle a continuing path's primary hit is on, or -1 (ended)
    using code_t = std::conditional_t<LF, int8_t, int16_t>;
    code_t* const wcodes = reinterpret_cast<code_t*>(wslots + pc * kPsFields * 64);
    auto code_at = [&](int kk, int ln) -> int { return (int)wcodes[kk * 64 + ln]; };
    auto set_code_at = [&](int kk, int ln, int c) { wcodes[kk * 64 + ln] = (code_t)c; };
    const f3 cam = make3(a.cam_x, a.cam_y, a.cam_z);
    // The Philox words of the lane's pixel (philox_pix: the two products of a block that see only
    // the pixel and the key), the same for all its samples.  ONEPX: the wave's pixel -- every lane
    // of a wave that gets here is valid and holds it -- so the words are scalars.
    PhiloxPix ppx;
    if constexpr (ONEPX) {
        ppx = philox_pix((uint32_t)__builtin_amdgcn_readfirstlane((int)pix), a.seed_lo, a.seed_hi);
    } else {
        ppx = philox_pix(pix, a.seed_lo, a.seed_hi);
    }
    // the words of pixel p, the owner of a queued sample (ONEPX: the wave's)
    auto px_of = [&](uint32_t p) -> PhiloxPix {
        if constexpr (ONEPX)
            return ppx;
        else
            return philox_pix(p, a.seed_lo, a.seed_hi);
    };

    // ---- candidate triangles of the wave's pixel rectangle (rect_cull, rt_cull.hpp) ----
    // (from the launch's precomputed forms; a launch without them runs the whole cull here)
    uint64_t cm[kRenderCullWords];
    if (cf.forms != nullptr)
        wave_candidates_forms<RULE>(a, cf, blk, q, lane, cm);
    else
        wave_candidates<RULE>(a, valid, px, py, lane, cm);

    // ---- phase P: primary rays of the lane's samples ----
    unsigned n_casts = 0;
#if RT_PROF
    // P, shade, filter masks, exact, post, loops, light pre-test passes, loops with < 16 live lanes
    uint64_t pt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ExactProf xprof = {0u, 0u, 0u, 0u, 0u, 0u};  // the bounce trips' shared exact phase
    uint64_t t0 = __builtin_amdgcn_s_memtime();
#endif
    const float nts = a.t_scale;
    cfloat4* __restrict__ isect = as_const(a.scene.isect);
    // parks sample k's primary result (the shading's pos = cam + t D, or the final value)
    auto park = [&](int k, const f3& d, const Hit& h) {
        n_casts += valid ? 1u : 0u;
        // a continuing path parks its hit point (the same operations the bounce loop's
        // shading used to apply to (cam, t, d): D = d t_scale, pos = cam + t D)
        float v0 = cam.x + h.t * (d.x * a.t_scale), v1 = cam.y + h.t * (d.y * a.t_scale),
              v2 = cam.z + h.t * (d.z * a.t_scale);
        int code = h.tri;
        if (h.tri < 0) {
            v0 = v1 = v2 = 0.0f;  // PRESET 0: a miss contributes 0
            code = -1;
        } else if (h.tri >= n_surf) {
            const float4 e = ps_emission<LF>(shade, h.tri);
            v0 = e.x; v1 = e.y; v2 = e.z;  // the light's emission, no surface bounce to fold
            code = -1;
        } else if (a.max_bounces == 0) {
            v0 = v1 = v2 = 0.0f;
            code = -1;
        }
        float* sl = slots + k * kPsFields * 64;
        sl[0 * 64] = v0;
        sl[1 * 64] = v1;
        sl[2 * 64] = v2;
        set_code_at(k, lane, code);
    };
    // The primary rays all start at the camera, so the cofactors of the exact test that
    // involve only b = cam - v0 and the edges (s3, s4, s6, det_t) are the same for every
    // sample of the wave: computed once per candidate for a batch of samples, each sample
    // then runs the direction-dependent rest (exact_one's operations on the same
    // operands in the same order: the same bits).  Samples of a batch fold the candidates
    // in index order each.
    constexpr int PB = kPsPrimBatch;
    for (int k0 = 0; k0 < pc; k0 += PB) {
        f3 dd[PB];
        float nx[PB], ny[PB], nz[PB];
        Hit hh[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int s = chunk * pc + min(k0 + j, pc - 1);
            float r1, r2;
            draw2_px(ppx, (uint32_t)s, 0u, a.seed_lo, a.seed_hi, &r1, &r2);
            camera_ray<0, true>(a, px, py, r1, r2, &dd[j]);
            nx[j] = -(dd[j].x * nts);
            ny[j] = -(dd[j].y * nts);
            nz[j] = -(dd[j].z * nts);
            hh[j].t = (RULE == 0) ? FLT_MAX : 999999.0f;
            hh[j].tri = -1;
        }
#pragma unroll
        for (int g = 0; g < kRenderCullWords; ++g) {
            uint64_t m = cm[g];
            while (m != 0ull) {
                const int b = __builtin_ctzll(m);
                m &= m - 1ull;
                const int i = g * 64 + b;
                const float4 A = ldc(isect + i * kIsectF4 + 0);
                const float4 E1 = ldc(isect + i * kIsectF4 + 1);
                const float4 E2 = ldc(isect + i * kIsectF4 + 2);
                const float bx = cam.x - A.x, by = cam.y - A.y, bz = cam.z - A.z;
                const float s3 = by * E2.z - E2.y * bz;
                const float s4 = by * E1.z - E1.y * bz;
                const float det_t = (bx * A.w - E1.x * s3) + E2.x * s4;
                const float s6 = E1.y * bz - by * E1.z;
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    const float s1 = ny[j] * E2.z - E2.y * nz[j];
                    const float s2 = ny[j] * E1.z - E1.y * nz[j];
                    const float detA = (nx[j] * A.w - E1.x * s1) + E2.x * s2;
                    const float s5 = ny[j] * bz - by * nz[j];
                    const float det_u = (nx[j] * s3 - bx * s1) + E2.x * s5;
                    const float det_v = (nx[j] * s6 - E1.x * s5) + bx * s2;
                    exact_test<RULE>(detA, det_t, det_u, det_v, i, hh[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PB; ++j)
            if (k0 + j < pc) park(k0 + j, dd[j], hh[j]);
    }

    // ---- phase S: bounces ----
#if RT_PROF
    const uint64_t t_s = __builtin_amdgcn_s_memtime();
    pt[0] += t_s - t0;
#endif
    f3 acc = make3(0.0f, 0.0f, 0.0f);
    int cur = 0;       // sample of the live path
    int depth = 0;      // surface bounces of the live path so far
    f3 o = cam, d = make3(0.0f, 0.0f, 1.0f);
    f3 pos = cam;       // the live path's surface hit to shade next, and its triangle
    int hit_tri = 0;
    int f_tri0 = 0;
    float f_cos0 = 0.0f;
    // The wave's continuing samples form one queue (slot-major: k, then lane), so a lane
    // whose path ends takes the next queued sample of any lane of the wave instead of
    // only its own: the wave runs ceil(casts / 64) trips instead of its busiest lane's.
    // A finished sample's value goes back into its slot; every lane then sums its own
    // slots in sample order (the fixed-chunk sum: the image is unchanged).
    // (after the codes: pc * 64 of them, int16 or bytes)
    uint16_t* const queue = reinterpret_cast<uint16_t*>(wcodes + pc * 64);
    uint8_t* const queue8 = reinterpret_cast<uint8_t*>(queue);  // the narrow layout's
    auto queue_at = [&](int j) -> uint32_t { return narrow ? (uint32_t)queue8[j] : (uint32_t)queue[j]; };
    auto set_queue_at = [&](int j, int e) {
        if (narrow)
            queue8[j] = (uint8_t)e;
        else
            queue[j] = (uint16_t)e;
    };
    int q_total = 0;
    for (int kk = 0; kk < pc; ++kk) {
        const bool cont = valid && code_at(kk, lane) >= 0;
        const uint64_t m = __ballot(cont);
        if (cont) set_queue_at(q_total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)), (kk << 6) | lane);
        q_total += __builtin_popcountll(m);
    }
    int q_next = 0;       // wave-uniform: next queue entry
    int own_e = lane;     // queue entry (k << 6 | lane) of the live path's sample (any lane's)
    uint32_t lpix = pix;  // its pixel (RNG key)
    bool live = false;
    // the slot of the live path's sample
    auto own_slot = [&]() -> float* { return wslots + (own_e >> 6) * kPsFields * 64 + (own_e & 63); };
    auto claim = [&]() {  // wave-level: lanes without a path take the next queued samples
        const uint64_t need = __ballot(!live);
        if (need == 0ull || q_next >= q_total) return;
        const int j = q_next + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        if (!live && j < q_total) {
            const uint32_t e = queue_at(j);
            const int ol = (int)(e & 63u), kk = (int)(e >> 6);
            own_e = (int)e;
            const float* own = wslots + kk * kPsFields * 64 + ol;
            pos = make3(own[0 * 64], own[1 * 64], own[2 * 64]);
            hit_tri = code_at(kk, ol);
            depth = 0;
            const PsKeys key = ps_owner_keys(a, blk, q - (lane >> a.split_log2), (int)e);
            lpix = key.pix;
            cur = key.cur;
            live = true;
        }
        q_next = min(q_total, q_next + __builtin_popcountll(need));
    };
    // the bounce casts on the matrix cores when the scene has the image (wave-uniform)
    const bool use_mf = MF > 0;  // the launcher: MF = 64-triangle blocks of the scene (image present), else 0
    // scenes of at most 64 triangles: the candidates from the scene's table (rt_ctab.cpp) instead
    // of the image's masks (wave-uniform)
    constexpr bool use_ctab = CT && MF == 1;
    // the next direction from the surface hit (pos, hit_tri) at bounce depth dep: cos theta
    // and the ray (o = pos + eps sd, d = normalize(sd)), sampled with the path's Philox draw
    auto shade_hit = [&](int dep, float* cos_out, f3* o_out, f3* d_out) {
        ps_shade_hit<SAMPLER, LF>(a, shade, px_of(lpix), cur, dep, pos, hit_tri, cos_out, o_out, d_out);
    };
    // Light pre-test.  The terminal cast of a path (the one at depth
    // max_bounces) adds light only if its closest hit is a light triangle; a surface or a miss
    // there gives 0.  If no light triangle passes the exact test without its t window
    // (exact_tv: the full test's own operations), the closest hit cannot be a light, and the
    // cast's value is 0 whatever the surfaces are.  So when a cast leaves a path whose next
    // cast is terminal, the lane samples that next ray at once and tests only the light
    // triangles: no pass -> the path ends with 0 (the terminal cast counted); a pass (a few
    // percent of rays) -> the path stays live and the next trip traces the same ray (same
    // Philox draw) in full.  Terminal casts thus stop taking slots of the matrix-core trips:
    // the image and the ray casts are k_render's bit for bit.
    // In the table-route variant (ps_pooled) a pass does not stay in its lane either: those
    // retraces arrive after the wave's queue has drained, so most waves ran one more trip with a
    // handful of live lanes at the cost of a full one.  The wave settles the pass where the
    // pre-test finds it (pretest_pending, below).
    const bool split = use_mf && a.max_bounces >= 1 &&
                       (a.scene.n_tri - n_surf) <= kPsSplitLights;
#if RT_PROF
    unsigned n_pass = 0;  // the lane's light pre-test passes
    unsigned max_settle = 0;  // wave-uniform: the most lanes settled in one pre-test pass
#endif
    // the pre-test of the terminal ray from (pos, hit_tri) at depth dep = max_bounces - 1
    auto light_pass = [&](int dep) -> bool {
        float c;
        f3 lo, ld;
        shade_hit(dep, &c, &lo, &ld);
        return ps_light_pass<RULE>(a, ms, lo, ld);
    };
#if RT_PROF
    uint64_t t_pre = 0;  // wave cycles inside the light pre-test
    // wave-uniform: the pipelined loop's pre-test passes run inside the loop and after it, and the
    // pending lanes over those passes
    unsigned pp_loop = 0, pp_drain = 0, pp_lanes = 0;
    bool pp_in_loop = true;
#endif
    bool piped = false;  // the pipelined loop has done the bounces: the loop after it does not run
    // The pipelined loop (the table-route variant with the pre-test on: every live lane ends its
    // path in the trip that claimed it, so every trip starts with all lanes free and the paths at
    // depth 0; launch_render refuses the CPU preset above two bounces).  In this variant the loop
    // after it runs only with the pre-test off.  The cast's table lookup opens with two dependent
    // global loads that nothing in the lane's own chain covers, and the pre-test that follows a
    // surface hit shares no data with the lane's next sample.  So a sample whose cast hit a surface does not run its pre-test on
    // the spot: the lane parks it as pending and goes free.  The hit point goes into the sample's
    // own slot (its three floats are dead between the claim and the final value), and the sample
    // (its entry packed with the two triangles) joins the wave's pending list at a position from
    // one ballot, as the queue is built.  The list lives in two registers of the wave, entry j of
    // its up to 127 in lane j % 64 of list_a (j < 64) or list_b: one cross-lane permute appends a
    // trip's samples, a pass takes list_a as it stands, lane l entry l, and list_b moves down.  (In
    // LDS the list would need 128 bytes per wave beside the queue's dead prefix, which the bench
    // launch does not have below six workgroups per CU.)
    // A pre-test pass costs the wave the same whatever the number of pending lanes, so it runs
    // only on a full wave of them: a trip claims, shades the new
    // samples, issues their lookups (closest_hit_ctab_begin), then, with kPsPassMin samples
    // pending, runs a pass on the oldest -- keys re-derived from the entry as claim() derives
    // them -- settles what passes, stores the values, and only then uses the lookup's words
    // (closest_hit_ctab_finish).  Loads return in the order of their
    // issue, so a wait inside the pre-test for a global load would wait for the lookup's words as
    // well: the pre-test issues none.  Its sample, its surface's shading frame, the hit-test
    // records and the rows a settled ray that ends on a light folds with all come from LDS.
    // Every sample runs
    // the same float operations on the same operands as in the loop below, and the casts are
    // counted at the same events, in whichever lane: the image and the ray casts are unchanged.
    // When the queue has drained, passes run after the loop until the list is empty, the last one
    // partial.  Nothing but the list and wave-uniform counters is carried from trip to trip.
    if constexpr (ps_pooled(MF, CT)) piped = split;
    if constexpr (ps_pooled(MF, CT)) {
        if (piped) {
            const CtabDev& tab = ms.ctab[RULE];
            int list_a = 0, list_b = 0;  // an entry: the sample's queue entry << 12 | f_tri0 << 6 | hit_tri
            int l_cnt = 0;               // wave-uniform: pending samples
            // one pre-test pass over the (up to 64) oldest pending samples, what passes settled on
            // the spot (wave-level)
            auto pretest_pending = [&]() {
                const bool pend = lane < l_cnt;
                const int p_pack = list_a;
                list_a = list_b;
                l_cnt = max(0, l_cnt - 64);
#if RT_PROF
                const uint64_t tp = __builtin_amdgcn_s_memtime();
                pp_loop += pp_in_loop ? 1u : 0u;
                pp_drain += pp_in_loop ? 0u : 1u;
                pp_lanes += (unsigned)__builtin_popcountll(__ballot(pend));
#endif
                const int e = p_pack >> 12, p_tri = p_pack & 63;  // the sample's entry, the triangle its cast hit
                bool pass = false;
                PsKeys key;
                key.pix = 0u;
                key.cur = 0;
                float c = 0.0f;
                f3 lo = cam, ld = make3(0.0f, 0.0f, 1.0f);
                if (pend) {
                    const float* own = wslots + (e >> 6) * kPsFields * 64 + (e & 63);
                    const f3 p_pos = make3(own[0 * 64], own[1 * 64], own[2 * 64]);
                    key = ps_owner_keys(a, blk, q - (lane >> a.split_log2), e);
                    // (a sample is pending only at max_bounces 2, launch_render's limit for this
                    // preset: its pre-test's depth is 1, the event a constant)
                    ps_shade_hit<SAMPLER, LF>(a, shade, px_of(key.pix), key.cur, 1, p_pos, p_tri, &c, &lo, &ld);
                    pass = ps_light_pass<RULE>(a, ms, lo, ld);
                }
                // The passes are settled here, one ray at a time by the whole wave: lane j tests
                // triangle j against the passing lane's ray (exact_tv on the LDS records, the
                // function the cast's own-lane tests and shared phase call), and the scan's window
                // runs in index order over the triangles that pass.  A triangle outside the
                // table's candidate mask fails the test for this ray and a failing one is +inf,
                // which no window accepts: `tri` is the cast's hit.
                int tri = -1;
                uint64_t pm = __ballot(pass);
                if (pm != 0ull) {
#if RT_PROF
                    n_pass += pass ? 1u : 0u;
                    max_settle = max(max_settle, (unsigned)__builtin_popcountll(pm));
#endif
                    const float nDx = -(ld.x * a.t_scale), nDy = -(ld.y * a.t_scale), nDz = -(ld.z * a.t_scale);
                    do {
                        const int pl = __builtin_ctzll(pm);
                        pm &= pm - 1ull;
                        const f3 ro = make3(readlane_f(lo.x, pl), readlane_f(lo.y, pl), readlane_f(lo.z, pl));
                        const float rx = readlane_f(nDx, pl), ry = readlane_f(nDy, pl), rz = readlane_f(nDz, pl);
                        float tj = __builtin_inff();
                        if (lane < a.scene.n_tri) tj = exact_tv<RULE>(ms.isect, lane, ro, rx, ry, rz);
                        uint64_t hits = __ballot(tj != __builtin_inff());
                        float best = (RULE == 0) ? FLT_MAX : 999999.0f;
                        int bt = -1;
                        while (hits != 0ull) {
                            const int b = __builtin_ctzll(hits);
                            hits &= hits - 1ull;
                            const float t = readlane_f(tj, b);
                            if ((RULE == 0) ? (t < best + kEps) : (t < best)) {
                                best = t;
                                bt = b;
                            }
                        }
                        tri = (lane == pl) ? bt : tri;
                    } while (pm != 0ull);
                }
                if (pend) {
                    ++n_casts;  // the terminal cast: settled above, or no light triangle can be its hit
                    f3 v = make3(0.0f, 0.0f, 0.0f);
                    if (tri >= n_surf) {
                        // a light: its emission folded back through both bounces, as the general
                        // loop folds it (the pre-test's own cos at this surface, then the path's
                        // first surface with the cos its shading at depth 0 drew)
                        const int dep = a.max_bounces - 1;
                        const float4 em = ps_emission<LF>(shade, tri);
                        v = make3(em.x, em.y, em.z);
                        if (dep >= 1) ps_fold<SAMPLER, LF>(shade, v, p_tri, c);
                        float f_c0 = c;
                        if (SAMPLER == 0 && dep >= 1) {
                            float r1, r2;
                            draw2_px(px_of(key.pix), (uint32_t)key.cur, 1u, a.seed_lo, a.seed_hi, &r1, &r2);
                            f_c0 = r1;
                        }
                        ps_fold<SAMPLER, LF>(shade, v, (p_pack >> 6) & 63, f_c0);
                    }
                    float* own = wslots + (e >> 6) * kPsFields * 64 + (e & 63);
                    own[0 * 64] = v.x;
                    own[1 * 64] = v.y;
                    own[2 * 64] = v.z;
                }
#if RT_PROF
                t_pre += __builtin_amdgcn_s_memtime() - tp;
#endif
            };
            while (q_next < q_total) {
#if RT_PROF
                const uint64_t ta = __builtin_amdgcn_s_memtime();
                pt[5] += 1;
                pt[7] += q_total - q_next < 16 ? 1 : 0;
#endif
                // claim(): every lane is free, lane l takes entry q_next + l
                const int qj = q_next + lane;
                const bool has = qj < q_total;
                q_next = min(q_total, q_next + 64);
                int s_tri = 0, s_e = 0;
                float s_cos = 0.0f;
                f3 so = cam, sd = make3(0.0f, 0.0f, 1.0f);  // (a lane without a sample: a finite ray, no candidates)
                CtabLook<1> look = ctab_no_look<1>();
                if (has) {
                    s_e = (int)queue_at(qj);
                    const int ol = s_e & 63, kk = s_e >> 6;
                    const float* own = wslots + kk * kPsFields * 64 + ol;
                    const f3 spos = make3(own[0 * 64], own[1 * 64], own[2 * 64]);
                    s_tri = code_at(kk, ol);
                    // the new sample's one global load, its patch frame (the lookup's first link),
                    // ahead of the Philox block; its shading frame is in LDS
                    const CtabFrame R = ctab_frame(tab, s_tri);
                    const PsKeys key = ps_owner_keys(a, blk, q - (lane >> a.split_log2), s_e);  // the owner's
                    ps_shade_hit<SAMPLER, LF>(a, shade, px_of(key.pix), key.cur, 0, spos, s_tri, &s_cos, &so, &sd);
                    look = closest_hit_ctab_begin<1>(tab, R, so, sd, true);
                }
#if RT_PROF
                const uint64_t tb = __builtin_amdgcn_s_memtime();
                const uint64_t tp0 = t_pre;
#endif
                if (l_cnt >= kPsPassMin) pretest_pending();
#if RT_PROF
                const Hit h = closest_hit_ctab_finish<RULE, 1, kCtPairCap>(ms, tab, s_tri, look, so, sd, a.t_scale, has,
                                                                           wl, &xprof);
#else
                const Hit h = closest_hit_ctab_finish<RULE, 1, kCtPairCap>(ms, tab, s_tri, look, so, sd, a.t_scale, has,
                                                                           wl);
#endif
#if RT_PROF
                pt[1] += tb - ta;  // (with the claim and the lookup's begin half)
                pt[3] += (__builtin_amdgcn_s_memtime() - tb) - (t_pre - tp0);
#endif
                n_casts += has ? 1u : 0u;
                // a surface with one bounce left: pending
                const bool park_it = has && h.tri >= 0 && h.tri < n_surf && 1 < a.max_bounces;
                f3 L = make3(0.0f, 0.0f, 0.0f);  // a miss, or a surface at max_bounces
                if (park_it) {
                    L = make3(so.x + h.t * (sd.x * a.t_scale), so.y + h.t * (sd.y * a.t_scale),
                              so.z + h.t * (sd.z * a.t_scale));
                } else if (h.tri >= n_surf) {
                    const float4 e = ps_emission<LF>(shade, h.tri);
                    L = make3(e.x, e.y, e.z);
                    ps_fold<SAMPLER, LF>(shade, L, s_tri, s_cos);  // (depth 1: the path's first bounce)
                }
                // The list grows by this trip's n pending samples (wave-level): the k-th of them, in
                // lane order, becomes entry l_cnt + k.  One permute of the whole wave carries it to
                // that entry's lane; the other lanes send to the lanes past those, so that no two
                // lanes send to the same one.
                {
                    const uint64_t pm = __ballot(park_it);
                    const int n = __builtin_popcountll(pm);
                    const uint64_t om = ~pm;
                    // (the counts start from the wave-uniform offsets: l_cnt + k, and l_cnt + n + the
                    // lane's rank among the others)
                    const int kp = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)pm, (uint32_t)l_cnt));
                    const int ko = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)om, (uint32_t)(l_cnt + n)));
                    const int to = (park_it ? kp : ko) & 63;
                    // (h.tri of a pending sample is a surface, below 64; what the other lanes send is never read)
                    const int got = __builtin_amdgcn_ds_permute(to << 2, (s_e << 12) | (s_tri << 6) | h.tri);
                    const int k = (lane - l_cnt) & 63;  // this lane holds entry l_cnt + k, new if k < n
                    if (k < n) {
                        if (l_cnt + k < 64)
                            list_a = got;
                        else
                            list_b = got;
                    }
                    l_cnt += n;
                }
                if (has) {  // the hit point of a pending sample, or the sample's value
                    float* own = wslots + (s_e >> 6) * kPsFields * 64 + (s_e & 63);
                    own[0 * 64] = L.x;
                    own[1 * 64] = L.y;
                    own[2 * 64] = L.z;
                }
            }
#if RT_PROF
            pp_in_loop = false;
#endif
            while (l_cnt > 0) pretest_pending();
        }
    }
    for (; !piped;) {
        claim();
        if (__ballot(live) == 0ull) break;
        if (!use_mf && !live) continue;
#if RT_PROF
        const uint64_t ta = __builtin_amdgcn_s_memtime();
        pt[5] += 1;
        pt[7] += __builtin_popcountll(__ballot(live)) < 16 ? 1 : 0;
#endif
        int s_tri = 0;
        float s_cos = 0.0f;
        if (live) {
            // shade the live path's surface hit (depth < max_bounces by construction)
            s_tri = hit_tri;
            shade_hit(depth, &s_cos, &o, &d);
            if (depth == 0) {
                f_tri0 = s_tri;
                f_cos0 = s_cos;
            }
            ++depth;
        }
        // every lane of the wave takes part in the matrix-core filter; a lane without a
        // live path casts its stale (finite) ray with no candidates
#if RT_PROF
        const uint64_t tb = __builtin_amdgcn_s_memtime();
        uint64_t tm = tb;
#endif
        Hit h;
        if constexpr (use_ctab)
            h = closest_hit_ctab<RULE, 1, kCtPairCap>(ms, ms.ctab[RULE], s_tri, o, d, a.t_scale, live, wl);
        else if (use_mf)
#if RT_PROF
            h = closest_hit_mf<RULE, false, (MF > 0 ? MF : 1)>(ms, o, d, a.t_scale, live, wl, nullptr, &tm);
#else
            h = closest_hit_mf<RULE, false, (MF > 0 ? MF : 1)>(ms, o, d, a.t_scale, live, wl);
#endif
        else
            h = closest_hit_sel<RULE>(a.scene, 1, o, d, a.t_scale);
#if RT_PROF
        const uint64_t tc = __builtin_amdgcn_s_memtime();
        pt[1] += tb - ta;
        pt[2] += tm - tb;
        pt[3] += tc - tm;
#endif
        if (!live) continue;
        ++n_casts;

        bool terminal = true;
        f3 L = make3(0.0f, 0.0f, 0.0f);
        if (h.tri < 0) {
            // miss: 0
        } else if (h.tri >= n_surf) {
            const float4 e = ps_emission<LF>(shade, h.tri);
            L = make3(e.x, e.y, e.z);
            // fold back through the surface bounces: depth 2 (this shading), then depth 1
            if (depth >= 2) ps_fold<SAMPLER, LF>(shade, L, s_tri, s_cos);
            ps_fold<SAMPLER, LF>(shade, L, f_tri0, f_cos0);
        } else if (depth == a.max_bounces) {
            // bounces == MAX_RAY_BOUNCES -> vec3(0)
        } else {
            terminal = false;  // shade the hit on the next trip
            pos = make3(o.x + h.t * (d.x * a.t_scale), o.y + h.t * (d.y * a.t_scale), o.z + h.t * (d.z * a.t_scale));
            hit_tri = h.tri;
            if (split && depth + 1 == a.max_bounces) {
#if RT_PROF
                const uint64_t tp = __builtin_amdgcn_s_memtime();
                const bool lp = light_pass(depth);
                t_pre += __builtin_amdgcn_s_memtime() - tp;
                if (!lp) {
#else
                if (!light_pass(depth)) {
#endif
                    ++n_casts;  // the terminal cast: no light triangle can be its hit
                    terminal = true;
                } else {
#if RT_PROF
                    ++n_pass;
#endif
                }
            }
        }
        if (terminal) {
            float* own = own_slot();
            own[0 * 64] = L.x;
            own[1 * 64] = L.y;
            own[2 * 64] = L.z;
            live = false;
        }
    }
#if RT_PROF
    pt[4] = __builtin_amdgcn_s_memtime() - t_s;  // the whole bounce phase
    pt[6] = wave_sum(n_pass);
    if (a.prof != nullptr && lane == 0) {
        for (int i = 0; i < 8; ++i) atomicAdd(a.prof + i, (unsigned long long)pt[i]);
        atomicAdd(a.prof + 9, (unsigned long long)t_pre);
        atomicMax(a.prof + 8, (unsigned long long)max_settle);
        // the passes a wave would run on 64 pending samples each, and the waves that would run fewer
        const unsigned pp_dense = (pp_lanes + 63u) >> 6;
        atomicAdd(a.prof + 10, (unsigned long long)pp_loop);
        atomicAdd(a.prof + 11, (unsigned long long)pp_drain);
        atomicAdd(a.prof + 12, (unsigned long long)pp_lanes);
        atomicAdd(a.prof + 13, (unsigned long long)pp_dense);
        atomicAdd(a.prof + 14, (unsigned long long)(pp_dense < pp_loop + pp_drain ? 1u : 0u));
        atomicAdd(a.prof + 15, 1ull);
        atomicAdd(a.prof + 16, (unsigned long long)xprof.list_iters);
        atomicAdd(a.prof + 17, (unsigned long long)xprof.fold_iters);
        atomicAdd(a.prof + 18, (unsigned long long)xprof.pairs);
        atomicAdd(a.prof + 19, (unsigned long long)xprof.rounds);
        atomicAdd(a.prof + 20, (unsigned long long)xprof.passes);
        atomicAdd(a.prof + 21, (unsigned long long)xprof.max_pass);
    }
#endif
    ps_finish(a, blk, wslots, chunk, lane, lx, ly, valid, acc);
    return n_casts;
}

#ifndef RT_PS_MIN_WAVES
#define RT_PS_MIN_WAVES 4  // the matrix-core filter's operands: ~99 VGPRs
#endif
#ifndef RT_PS_CT_WAVES
// occupancy floor of the table-route variant: 6 (80 VGPRs, 3 spilled) -- with the narrow wave
// blocks its workgroup takes 26.4 KB of LDS, shading frames included, and six fit a CU (Cornell
// 512^2 x 256 at the int16 codes' 26.7 KB: 2.39 -> 2.24 ms, profiles/r6v/; at the 28.7-KB layout
// LDS held it to five and 6 only added spills)
#define RT_PS_CT_WAVES 6
#endif
// NARROW: the wave blocks of this launch are the narrow ones (ps_wave_floats); the table-route
// variant only, chosen by the launcher (ps_narrow)
// ONEPX: this launch has one pixel per wave (split 64: ps_onepx); an instance of the narrow layout
template <int SAMPLER, int RULE, int MF, bool CT = false, bool NARROW = false, bool ONEPX = false>
__global__ __launch_bounds__(256, CT ? RT_PS_CT_WAVES : RT_PS_MIN_WAVES) void k_render_ps(const RenderLaunch a,
                                                                                                const CullLaunch cf) {
    const int lg = a.split_log2;
    const BlockDesc blk = a.blocks[blockIdx.x >> lg];
    // XCD-aware parts: workgroups go to the 8 XCDs round-robin by blockIdx, so the
    // workgroups of one XCD take consecutive parts (whole pixel rows of the block) and a
    // row's output lines are written through one XCD's L2 instead of eight
    int part = blockIdx.x & (a.split - 1);
    if (a.split >= 8) part = ((part & 7) << (lg - 3)) | (part >> 3);
    const int q = (part << (8 - lg)) + ((int)threadIdx.x >> lg);
    const int chunk = threadIdx.x & (a.split - 1);
    const int lane = threadIdx.x & 63;
    const int lx = q & 15;
    const int ly = q >> 4;
    const int px = blk.px0 + lx;
    const int py = blk.py0 + ly;
    const bool valid = (px < a.clip_x1) && (py < a.clip_y1);
    const uint64_t vmask = __ballot(valid);
    // ray casts: one atomic per workgroup (a wave's count through LDS, one barrier at the
    // end; every wave reaches it, a wave without pixels contributes 0): one atomic per
    // wave put 16 MB per launch of atomic write traffic on a 3 MB frame
    __shared__ unsigned wg_casts[4];
    // LDS after the sample slots (launch_render_t sizes it): the waves' exact-phase
    // regions, then the scene's hit-test records and its shading records (the table-route
    // variant: the frames and one colour per triangle, kPsFrameF4)
    DeviceScene ms = a.scene;
    float* wl = nullptr;
    if (MF > 0) {
        extern __shared__ float s_ps[];
        float* const mf_base = s_ps + (size_t)4 * ps_wave_floats(a.per_chunk, NARROW);
        // (the table route's wave blocks hold a shorter pair list: mf_wave_floats)
        constexpr int wf = CT ? mf_wave_floats(kCtPairCap, RULE) : kMfWaveFloats;
        wl = mf_base + (size_t)(threadIdx.x >> 6) * wf;
        // hit-test and shading records of the scene (divergent per-lane reads: LDS latency
        // instead of L1/L2).  The table-route kernel stages what ps_body reads of a shading
        // record, 48 of its 80 bytes: rows N, T, B, and in their w lanes the surface's fold row
        // for this sampler or the light's emission.  The byte codes and queue of its wave blocks
        // pay for them: the bench launch stays below the 26.7 KB that six workgroups per CU had
        // (launch_render_t's static_assert).
        const int n = a.scene.n_tri;
        float4* li = reinterpret_cast<float4*>(mf_base + 4 * wf);
        float4* ls = li + (size_t)n * kIsectF4;
        if constexpr (ps_pooled(MF, CT)) {
            // waves 0 and 1 move the hit-test records, waves 2 and 3 the frames, every load of a
            // thread issued ahead of its first wait (a workgroup lives a few trips: a second
            // round trip in front of the barrier shows in the frame)
            if (threadIdx.x < 128) {
                for (int i = threadIdx.x; i < n * kIsectF4; i += 128) li[i] = a.scene.isect[i];
            } else {
                for (int i = threadIdx.x - 128; i < n * kPsFrameF4; i += 128) {
                    const int tri = i / kPsFrameF4, r = i - tri * kPsFrameF4;
                    const float4 row = a.scene.shade[tri * kShadeF4 + r];
                    const float4* col = a.scene.shade + tri * kShadeF4 + ((SAMPLER == 0 || tri >= a.scene.n_surf) ? 3 : 4);
                    ls[i] = make_float4(row.x, row.y, row.z, reinterpret_cast<const float*>(col)[r]);
                }
            }
            ms.shade = ls;
        } else {
            for (int i = threadIdx.x; i < n * kIsectF4; i += 256) li[i] = a.scene.isect[i];
            if (!CT) {
                for (int i = threadIdx.x; i < n * kShadeF4; i += 256) ls[i] = a.scene.shade[i];
                ms.shade = ls;
            }
        }
        ms.isect = li;
        __syncthreads();
    }
    // (a wave without pixels does nothing until the casts barrier below, the kernel's only one
    // after the staging)
    unsigned n_casts = 0;
    if (vmask != 0ull) n_casts = ps_body<SAMPLER, RULE, MF, CT, NARROW, ONEPX>(a, cf, ms, wl, blk, q, chunk, lane, lx, ly, px, py, valid);
    if (a.casts != nullptr) {
        // the wave's sum bit-sliced through ballots (a lane's count is at most 3 per_chunk: a few
        // bits), no cross-lane permutes
        unsigned total = 0;
        for (int b = 0; __ballot((n_casts >> b) != 0u) != 0ull; ++b)
            total += (unsigned)__builtin_popcountll(__ballot((n_casts >> b) & 1u)) << b;
        if (lane == 0) wg_casts[threadIdx.x >> 6] = total;
        __syncthreads();
        if (threadIdx.x == 0)
            atomicAdd(a.casts, (unsigned long long)((wg_casts[0] + wg_casts[1]) + (wg_casts[2] + wg_casts[3])));
    }
}

// Exhaustive check of rcp_rn against IEEE division: thread g covers the
// 4096 bit patterns [g*4096, (g+1)*4096).  Counts mismatches (ignoring NaN
// payloads) and keeps the smallest mismatching pattern.
// WHICH = RT_SELFTEST_RCP: rcp_rn(x) vs IEEE 1.0f / x over all 2^32 floats;
// RT_SELFTEST_DIV12: div12(x) vs x / 12.0f over its domain (+0, |x| in [2^-100, 2^100]);
// RT_SELFTEST_DIVRHO: div_rho(x) vs x / RHO over all 2^32 floats (its fallback included).
// RT_SELFTEST_SQRT_POS: sqrt_rn_pos(x) vs sqrtf(x) over its domain (+0, x in [2^-96, FLT_MAX]);
// RT_SELFTEST_RCP_IN: rcp_rn_in(x) vs IEEE 1.0f / x over its domain (|x| in [2^-125, 2^125]).
// NaNs compare equal to NaNs.
constexpr int kSelfRcp = 1, kSelfDiv12 = 2, kSelfDivRho = 3;  // RT_SELFTEST_* (rtmi.h)
constexpr int kSelfSqrtPos = 4, kSelfRcpIn = 5, kSelfPhiloxPx = 6;

template <int WHICH>
__global__ __launch_bounds__(256) void k_selftest(unsigned long long* mism, unsigned* first) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned bad = 0;
    for (uint32_t k = 0; k < 4096u; ++k) {
        const uint32_t bits = (uint32_t)(g * 4096u + k);
        const float x = __uint_as_float(bits);
        float a, b;
        if constexpr (WHICH == kSelfRcp) {
            a = rcp_rn(x);
            b = 1.0f / x;
        } else if constexpr (WHICH == kSelfDiv12) {
            const float ax = fabsf(x);
            if (!(bits == 0u || (ax >= 0x1p-100f && ax <= 0x1p100f))) continue;
            a = div12(x);
            b = x / 12.0f;
        } else if constexpr (WHICH == kSelfSqrtPos) {
            if (!(bits == 0u || (x >= 0x1p-96f && x <= FLT_MAX))) continue;
            a = sqrt_rn_pos(x);
            b = sqrtf(x);
        } else if constexpr (WHICH == kSelfRcpIn) {
            const float ax = fabsf(x);
            if (!(ax >= 0x1p-125f && ax <= 0x1p125f)) continue;
            a = rcp_rn_in(x);
            b = 1.0f / x;
        } else {
            constexpr float rho = 1.0f / (2.0f * 3.14159265358979323846f);
            a = div_rho(x);
            b = x / rho;
        }
        const bool same = (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b);
        if (!same) {
            ++bad;
            atomicMin(first, bits);
        }
    }
    if (bad) atomicAdd(mism, (unsigned long long)bad);
}

// RT_SELFTEST_PHILOX_PX: the split block (philox_pix, philox_ev, philox_finish) against
// philox4x32_10, all four words, over 2^24 counters (pixel, sample, event, 0) per key and form:
// 4096 pixels (0, 1, 2^16 - 1, 2^16, 2^31, 2^32 - 1 and a hashed spread) x samples 0..1023 x events
// 0..3, for the key (1984, 0) and one with a high word.  Form 0: the pixel is the workgroup's, its
// words go through readfirstlane (the scalar unit's products, ps_body's ONEPX); form 1: a pixel
// per lane (thread t of block b takes pixel index (b + t) mod 4096, so every pair is met once).
// Same grid as k_selftest.  first: the lowest form << 25 | key << 24 | pixel index << 12 |
// sample << 2 | event that mismatched.
__device__ __forceinline__ uint32_t selftest_pixel(uint32_t i) {
    const uint32_t special[6] = {0u, 1u, 0xFFFFu, 0x10000u, 0x80000000u, 0xFFFFFFFFu};
    return i < 6u ? special[i] : i * 0x9E3779B1u + 0x7F4A7C15u;
}
__global__ __launch_bounds__(256) void k_selftest_philox(unsigned long long* mism, unsigned* first) {
    unsigned bad = 0;
    for (uint32_t form = 0; form < 2u; ++form) {
        const uint32_t pi = form == 0u ? blockIdx.x : ((blockIdx.x + threadIdx.x) & 4095u);
        const uint32_t pixel = selftest_pixel(pi);
        for (uint32_t key = 0; key < 2u; ++key) {
            const uint32_t k0 = key == 0u ? 1984u : 0x89ABCDEFu, k1 = key == 0u ? 0u : 0x01234567u;
            PhiloxPix px;
            if (form == 0u)
                px = philox_pix((uint32_t)__builtin_amdgcn_readfirstlane((int)pixel), k0, k1);
            else
                px = philox_pix(pixel, k0, k1);
            for (uint32_t smp = threadIdx.x; smp < 1024u; smp += 256u) {
                for (uint32_t ev = 0; ev < 4u; ++ev) {
                    uint32_t want[4], got[4];
                    philox4x32_10(pixel, smp, ev, 0u, k0, k1, want);
                    philox_finish(px, philox_ev(ev), smp, k0, k1, got);
                    if (want[0] != got[0] || want[1] != got[1] || want[2] != got[2] || want[3] != got[3]) {
                        ++bad;
                        atomicMin(first, form << 25 | key << 24 | pi << 12 | smp << 2 | ev);
                    }
                }
            }
        }
    }
    if (bad) atomicAdd(mism, (unsigned long long)bad);
}

}  // namespace

hipError_t launch_selftest(int which, unsigned long long* mism, unsigned* first, hipStream_t stream) {
    if (which == kSelfRcp)
        hipLaunchKernelGGL(k_selftest<kSelfRcp>, dim3(4096), dim3(256), 0, stream, mism, first);
    else if (which == kSelfDiv12)
        hipLaunchKernelGGL(k_selftest<kSelfDiv12>, dim3(4096), dim3(256), 0, stream, mism, first);
    else if (which == kSelfDivRho)
        hipLaunchKernelGGL(k_selftest<kSelfDivRho>, dim3(4096), dim3(256), 0, stream, mism, first);
    else if (which == kSelfSqrtPos)
        hipLaunchKernelGGL(k_selftest<kSelfSqrtPos>, dim3(4096), dim3(256), 0, stream, mism, first);
    else if (which == kSelfRcpIn)
        hipLaunchKernelGGL(k_selftest<kSelfRcpIn>, dim3(4096), dim3(256), 0, stream, mism, first);
    else if (which == kSelfPhiloxPx)
        hipLaunchKernelGGL(k_selftest_philox, dim3(4096), dim3(256), 0, stream, mism, first);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_intersect(const DeviceScene& s, const float* orig, const float* dir, int n,
                            float t_scale, int hit_rule, int use_filter, float* out_t,
                            int32_t* out_hit, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 block(256);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (hit_rule == 0) {
        hipLaunchKernelGGL(k_intersect<0>, grid, block, 0, stream, s, use_filter, s.code_cpu, orig, dir,
                           n, t_scale, out_t, out_hit);
    } else {
        hipLaunchKernelGGL(k_intersect<1>, grid, block, 0, stream, s, use_filter, s.code_gpu, orig, dir,
                           n, t_scale, out_t, out_hit);
    }
    return hipGetLastError();
}

hipError_t launch_intersect_bvh(const DeviceScene& s, const float* orig, const float* dir, int n, float t_scale,
                                int hit_rule, float* out_t, int32_t* out_hit, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (s.bvh_nodes == nullptr) return hipErrorInvalidValue;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    if (hit_rule == 0)
        hipLaunchKernelGGL(k_intersect_bvh<0>, grid, block, 0, stream, s, s.code_cpu, orig, dir, n, t_scale, out_t,
                           out_hit);
    else
        hipLaunchKernelGGL(k_intersect_bvh<1>, grid, block, 0, stream, s, s.code_gpu, orig, dir, n, t_scale, out_t,
                           out_hit);
    return hipGetLastError();
}

hipError_t launch_intersect_mf(const DeviceScene& s, const float* orig, const float* dir, int n, float t_scale,
                               int hit_rule, float* out_t, int32_t* out_hit, int32_t* cand, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (s.mf_frag == nullptr || !(t_scale > 0.0f && t_scale <= kFiltMaxTScale))
        return hipErrorInvalidValue;
    const dim3 block(256);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (hit_rule == 0)
        hipLaunchKernelGGL(k_intersect_mf<0>, grid, block, 0, stream, s, s.code_cpu, orig, dir, n, t_scale, out_t,
                           out_hit, cand);
    else
        hipLaunchKernelGGL(k_intersect_mf<1>, grid, block, 0, stream, s, s.code_gpu, orig, dir, n, t_scale, out_t,
                           out_hit, cand);
    return hipGetLastError();
}

// The instantiations of the candidate route the render kernels use: one mask word (scenes of
// at most 64 triangles) with either pair cap, four words with kMfPairCap.  surf: the table
// route (s.ctab[hit_rule] must serve t_scale), else masks_in.
bool cand_pair_cap_served(int n_tri, int pair_cap) {
    return n_tri > 0 && n_tri <= 256 && (pair_cap == kMfPairCap || (pair_cap == kCtPairCap && n_tri <= 64));
}
hipError_t launch_intersect_cand(const DeviceScene& s, const float* orig, const float* dir, int n, float t_scale,
                                 int hit_rule, const int32_t* surf, const unsigned long long* masks_in, int pair_cap,
                                 float* out_t, int32_t* out_hit, unsigned long long* out_masks, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int words = (s.n_tri + 63) / 64;
    const int nw = s.n_tri <= 64 ? 1 : 4;
    if (s.n_tri <= 0 || words > nw || (surf == nullptr) == (masks_in == nullptr)) return hipErrorInvalidValue;
    if (!cand_pair_cap_served(s.n_tri, pair_cap)) return hipErrorInvalidValue;
    if (surf != nullptr && (s.ctab[hit_rule].masks == nullptr || s.ctab[hit_rule].words != words ||
                            s.ctab[hit_rule].bins != kCtabBins || s.ctab[hit_rule].graze_n != kCtabGraze ||
                            !(t_scale >= s.ctab[hit_rule].ts_min)))
        return hipErrorInvalidValue;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    const int32_t* code = hit_rule == 0 ? s.code_cpu : s.code_gpu;
#define RT_LAUNCH_CAND(RULE, NW, CAP)                                                                            \
    hipLaunchKernelGGL((k_intersect_cand<RULE, NW, CAP>), grid, block, 0, stream, s, code, orig, dir, n, t_scale, \
                       surf, masks_in, words, out_t, out_hit, out_masks)
    if (hit_rule == 0) {
        if (nw == 4)
            RT_LAUNCH_CAND(0, 4, kMfPairCap);
        else if (pair_cap == kMfPairCap)
            RT_LAUNCH_CAND(0, 1, kMfPairCap);
        else
            RT_LAUNCH_CAND(0, 1, kCtPairCap);
    } else {
        if (nw == 4)
            RT_LAUNCH_CAND(1, 4, kMfPairCap);
        else if (pair_cap == kMfPairCap)
            RT_LAUNCH_CAND(1, 1, kMfPairCap);
        else
            RT_LAUNCH_CAND(1, 1, kCtPairCap);
    }
#undef RT_LAUNCH_CAND
    return hipGetLastError();
}

// Sample stealing pays where path lengths vary (GPU preset, up to 80 casts: Cornell
// +24%, complex_light_room +32%); with the CPU preset's cap of 3 casts the lanes stay
// in step and it costs 1%, so that preset keeps the fixed chunks.
#ifndef RT_STEAL_MAX_LDS
#define RT_STEAL_MAX_LDS (64 * 1024)  // sample stealing when its LDS fits (0: never)
#endif
#ifndef RT_PS_MAX_LDS
#define RT_PS_MAX_LDS (40 * 1024)  // per workgroup: 8 samples per lane
#endif

template <int PRESET, int SAMPLER, int RULE>
static void launch_render_t(const RenderLaunch& a, hipStream_t stream, const CullLaunch& cf) {
    if (PRESET == 0 && a.use_filter && a.scene.n_tri <= 64 * kRenderCullWords &&
        a.scene.bvh_nodes == nullptr) {
        // (the routing predicate is on the wide layout, whichever the launch then takes)
        size_t ps_lds = (size_t)4 * ps_wave_floats(a.per_chunk, false) * sizeof(float);
        if (ps_lds <= (size_t)RT_PS_MAX_LDS) {
            // the bounce casts from the scene's candidate table (rt_ctab.cpp) when it serves this
            // launch: one mask word, this build's bins, t_scale >= its ts_min
            const CtabDev& T = a.scene.ctab[RULE];
            const bool ct = a.scene.mf_frag != nullptr && a.scene.n_tri <= 64 && T.masks != nullptr &&
                            T.bins == kCtabBins && T.graze_n == kCtabGraze && a.t_scale >= T.ts_min && T.words == 1;
            // The kernel's dynamic LDS, in its order: ps_lds, the four waves' slots, codes and
            // queue (ps_wave_floats); then, with the matrix-core image, the four waves' exact-phase
            // blocks (the table route's hold the shorter pair list), the scene's isect records and
            // its shading records (the table route's: kPsFrameF4 rows, and its wave blocks are
            // the narrow ones up to kPsNarrowChunk samples per lane)
            size_t mf_lds = 0;
            if (a.scene.mf_frag != nullptr) {
                mf_lds = (size_t)4 * (ct ? mf_wave_floats(kCtPairCap, RULE) : kMfWaveFloats) * sizeof(float);
                mf_lds += (size_t)a.scene.n_tri * (kIsectF4 + (ct ? kPsFrameF4 : kShadeF4)) * sizeof(float4);
            }
            const bool narrow = ps_narrow(ct, a.per_chunk);
            if (narrow) ps_lds = (size_t)4 * ps_wave_floats(a.per_chunk, true) * sizeof(float);
            // the bench launch (4 samples per lane, Cornell's 38 triangles): no more than the
            // 26,656 B of the int16 layout without the frames, six workgroups per CU
            static_assert((4 * ps_wave_floats(4, true) + 4 * mf_wave_floats(kCtPairCap, 0)) * sizeof(float) +
                                  38 * (kIsectF4 + kPsFrameF4) * sizeof(float4) <= 26656,
                          "the table route's bench launch outgrew its LDS");
            const dim3 grid((unsigned)(a.n_blocks * a.split));
            KernelTimer kt(KT_RENDER_PS, stream);
            if (ps_onepx(narrow, a.split))
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 1, true, true, true>), grid, dim3(256), ps_lds + mf_lds,
                                   stream, a, cf);
            else if (narrow)
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 1, true, true>), grid, dim3(256), ps_lds + mf_lds, stream, a,
                                   cf);
            else if (ct)
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 1, true>), grid, dim3(256), ps_lds + mf_lds, stream, a, cf);
            else if (mf_lds > 0 && a.scene.n_tri <= 64)
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 1>), grid, dim3(256), ps_lds + mf_lds, stream, a, cf);
            else if (mf_lds > 0)
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 4>), grid, dim3(256), ps_lds + mf_lds, stream, a, cf);
            else
                hipLaunchKernelGGL((k_render_ps<SAMPLER, RULE, 0>), grid, dim3(256), ps_lds, stream, a, cf);
            return;
        }
    }
    const size_t lds = (size_t)(256 / a.split) * (size_t)a.spp * 3 * sizeof(float);
    const dim3 grid((unsigned)(a.n_blocks * a.split));
    const bool steal = PRESET == 1 && lds <= (size_t)RT_STEAL_MAX_LDS;
    KernelTimer kt(KT_RENDER, stream);
    // the GPU preset's casts on the matrix-core filter: when the scene has the image and
    // the camera is inside its origin bound (camera rays then get real masks)
    const float cb = a.scene.mf_bound;
    const bool mf_base = PRESET == 1 && a.use_filter && a.scene.mf_frag != nullptr &&
                         a.scene.bvh_nodes == nullptr && a.t_scale > 0.0f && a.t_scale <= kFiltMaxTScale;
    const bool cam_in = fabsf(a.cam_x) <= cb && fabsf(a.cam_y) <= cb && fabsf(a.cam_z) <= cb;
    // a camera outside the bound: its rays take the wave's primary-ray cull (rt_cull.hpp),
    // which models the CPU preset's camera -- the GPU preset's is the same ray when the
    // pitch is 0 (camera_ray: the second rotation is the identity, exactly)
    const bool cam_cull = !cam_in && a.scene.n_tri <= 64 * kRenderCullWords &&
                          a.cos_x == 1.0f && a.sin_x == 0.0f;
    const bool mf = mf_base && (cam_in || cam_cull);
    if (mf) {
        if (PRESET == 1) {  // (the CPU preset runs k_render_ps)
            RenderLaunch b = a;
            b.cam_cull = cam_in ? 0 : 1;
            const bool one = a.scene.n_tri <= 64;
            if (cam_in && a.csum != nullptr && a.work != nullptr) {
                (void)hipMemsetAsync(a.work, 0, sizeof(unsigned long long), stream);
                // a persistent grid: as many workgroups as the device holds at 4 waves per SIMD
                const unsigned wgs = (unsigned)min(a.n_blocks * a.split, RT_MF_RENDER_WAVES * device_cu_count());
                // the table route (k_render_pq CT): the scene's candidate table for this hit rule and
                // t_scale, and the camera rays' rectangle cull -- CPU-preset camera geometry, i.e.
                // pitch 0 (camera_ray: the second rotation is then the identity, exactly)
                const CtabDev& T = a.scene.ctab[RULE];
                const bool ct = a.cull != nullptr && a.cos_x == 1.0f && a.sin_x == 0.0f &&
                                a.scene.n_tri <= 64 * kRenderCullWords && T.masks != nullptr && T.bins == kCtabBins &&
                                T.graze_n == kCtabGraze && a.t_scale >= T.ts_min && T.words <= (one ? 1 : 4);
                if (ct) {
                    RenderLaunch c = b;  // one workgroup per 16x16 block: the masks of its four 16x4 rectangles
                    c.split = 1;
                    c.split_log2 = 0;
                    hipLaunchKernelGGL((k_cull_ps<RULE>), dim3((unsigned)a.n_blocks), dim3(256), 0, stream, c, CullLaunch{});
                    const unsigned wct = (unsigned)min(a.n_blocks * a.split, RT_PQ_CT_WAVES * device_cu_count());
                    if (one)
                        hipLaunchKernelGGL((k_render_pq<SAMPLER, RULE, 1, true>), dim3(wct), dim3(256), 0, stream, b);
                    else
                        hipLaunchKernelGGL((k_render_pq<SAMPLER, RULE, 4, true>), dim3(wct), dim3(256), 0, stream, b);
                } else if (one)
                    hipLaunchKernelGGL((k_render_pq<SAMPLER, RULE, 1>), dim3(wgs), dim3(256), 0, stream, b);
                else
                    hipLaunchKernelGGL((k_render_pq<SAMPLER, RULE, 4>), dim3(wgs), dim3(256), 0, stream, b);
                hipLaunchKernelGGL(k_fold_chunks, dim3((unsigned)a.n_blocks), dim3(256), 0, stream, b);
                return;
            }
            if (steal && one)
                hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, true, false, 1>), grid, dim3(256), lds, stream, b);
            else if (steal)
                hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, true, false, 4>), grid, dim3(256), lds, stream, b);
            else if (one)
                hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, false, false, 1>), grid, dim3(256), 0, stream, b);
            else
                hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, false, false, 4>), grid, dim3(256), 0, stream, b);
        }
        return;
    }
    if (a.scene.bvh_nodes != nullptr) {
        if (steal)
            hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, true, true>), grid, dim3(256), lds, stream, a);
        else
            hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, false, true>), grid, dim3(256), 0, stream, a);
    } else if (steal) {
        hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, true, false>), grid, dim3(256), lds, stream, a);
    } else {
        hipLaunchKernelGGL((k_render<PRESET, SAMPLER, RULE, false, false>), grid, dim3(256), 0, stream, a);
    }
}

hipError_t launch_cull_forms(const float4* filt, int n_tri, const CamConst& k, float4* forms, hipStream_t stream) {
    if (filt == nullptr || forms == nullptr || n_tri <= 0 || n_tri > kCullFormStride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cull_forms, dim3(1), dim3(kCullFormStride), 0, stream, filt, n_tri, k, forms);
    return hipGetLastError();
}

hipError_t launch_cull(const RenderLaunch& a, hipStream_t stream, const CullLaunch* cfp) {
    if (a.n_blocks <= 0 || a.cull == nullptr || a.scene.filt == nullptr) return hipErrorInvalidValue;
    const CullLaunch cf = cfp != nullptr ? *cfp : CullLaunch{};
    if (a.hit_rule == 0)
        hipLaunchKernelGGL((k_cull_ps<0>), dim3((unsigned)(a.n_blocks * a.split)), dim3(256), 0, stream, a, cf);
    else
        hipLaunchKernelGGL((k_cull_ps<1>), dim3((unsigned)(a.n_blocks * a.split)), dim3(256), 0, stream, a, cf);
    return hipGetLastError();
}

hipError_t launch_render(const RenderLaunch& a, hipStream_t stream, const CullLaunch* cfp) {
    if (a.n_blocks <= 0) return hipSuccess;
    const CullLaunch cf = cfp != nullptr ? *cfp : CullLaunch{};
    if (a.preset == 0 && a.max_bounces > 2) return hipErrorInvalidValue;
    if (a.split < 1 || a.split > 64 || (a.split & (a.split - 1)) != 0 || (1 << a.split_log2) != a.split ||
        a.per_chunk * a.split != a.spp)
        return hipErrorInvalidValue;
    const int key = a.preset * 4 + a.sampler * 2 + a.hit_rule;
    switch (key) {
        case 0: launch_render_t<0, 0, 0>(a, stream, cf); break;
        case 1: launch_render_t<0, 0, 1>(a, stream, cf); break;
        case 2: launch_render_t<0, 1, 0>(a, stream, cf); break;
        case 3: launch_render_t<0, 1, 1>(a, stream, cf); break;
        case 4: launch_render_t<1, 0, 0>(a, stream, cf); break;
        case 5: launch_render_t<1, 0, 1>(a, stream, cf); break;
        case 6: launch_render_t<1, 1, 0>(a, stream, cf); break;
        case 7: launch_render_t<1, 1, 1>(a, stream, cf); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rt
