// rt_trace.hpp — device-side building blocks shared by the path-trace
// megakernel (rt_kernels.hip) and the DQN wavefront kernels (rt_dqn.hip):
// the closest-hit loop with the reference's two hit predicates, the
// correctly-rounded reciprocal, and the Philox draws.
#pragma once

#include <float.h>

#include "rt_cull.hpp"
#include "rt_internal.hpp"

namespace rt {

// One pixel's RGB as a single 12-B store (global_store_dwordx3): three dword stores of a
// lone lane are three partial-line writes in the memory system's count
typedef float rgb3 __attribute__((ext_vector_type(3), aligned(4)));
__device__ __forceinline__ void store_rgb(float* dst, float r, float g, float b) {
    rgb3 v;
    v.x = r;
    v.y = g;
    v.z = b;
    *reinterpret_cast<rgb3*>(dst) = v;
}

constexpr float kRho = 1.0f / (2.0f * kPi);  // RHO: GPU/constants/image_settings.h:14

// Triangle records are read-only for a launch: loads through the constant address
// space are selected as scalar loads (SGPR broadcast) whenever the address is
// wave-uniform, even in kernels with global stores or atomics in the loop (the
// compiler otherwise falls back to per-lane vector loads of the same address there).
typedef float __attribute__((ext_vector_type(4))) f32x4_t;
typedef __attribute__((address_space(4))) const f32x4_t cfloat4;
__device__ __forceinline__ cfloat4* as_const(const float4* p) { return (cfloat4*)p; }
__device__ __forceinline__ float4 ldc(cfloat4* p) {
    const f32x4_t v = *p;
    return make_float4(v.x, v.y, v.z, v.w);
}

struct Hit {
    float t;
    int tri;
};

// Closest hit over the triangle soup.  D = dir * t_scale, A = [-D | e1 | e2],
// x = (t,u,v) by Cramer's rule with GLM's determinant order
// (glm/glm/detail/func_matrix.inl:214-217):
//   det(c0,c1,c2) = (c0.x*(c1.y*c2.z - c2.y*c1.z) - c1.x*(c0.y*c2.z - c2.y*c0.z))
//                   + c2.x*(c0.y*c1.z - c1.y*c0.z)
// The minors shared between detA, det_t, det_u and det_v are evaluated once
// (same operands, same order, so the same bits).
// RULE 0 = CPU triangle.cpp.o predicate (inv = 1/detA; accept t>=0, u>=0, v>=0,
//          u+v<=1, t < best+1e-5, t > 1e-5; best starts at FLT_MAX)
// RULE 1 = GPU/rays/ray.cu:63-64 (true divisions; t < best; best starts 999999)
// The scan rejects conservatively first (v_rcp_f32) and runs the exact IEEE test only for
// lanes it cannot reject: 7% faster than the exact test behind a branch on the t test on
// Cornell 512^2/256 spp, same image (profiles/r1_ab3.json).  1/detA is rcp_rn (v_rcp_f32 +
// Newton, exhaustively verified; rcp_rn / rcp_rn_from: rt_math.hpp).

// Exact hit test of one triangle (the reference's arithmetic, see above).
template <int RULE>
__device__ __forceinline__ void exact_test_inv(float detA, float inv, float det_t, float det_u,
                                               float det_v, int i, Hit& h) {
    // RULE 0 with inv = RN(1/detA) already computed
    const float t = det_t * inv;
    const float u = det_u * inv;
    const float v = det_v * inv;
    if ((detA != 0.0f) && (t >= 0.0f) && (u >= 0.0f) && (v >= 0.0f) && ((u + v) <= 1.0f) &&
        (t < h.t + kEps) && (t > kEps)) {
        h.t = t;
        h.tri = i;
    }
}

template <int RULE>
__device__ __forceinline__ void exact_test(float detA, float det_t, float det_u, float det_v, int i,
                                           Hit& h) {
    if (RULE == 0) {
        const float inv = rcp_rn(detA);
        const float t = det_t * inv;
        const float u = det_u * inv;
        const float v = det_v * inv;
        if ((detA != 0.0f) && (t >= 0.0f) && (u >= 0.0f) && (v >= 0.0f) && ((u + v) <= 1.0f) &&
            (t < h.t + kEps) && (t > kEps)) {
            h.t = t;
            h.tri = i;
        }
    } else {
        const float t = det_t / detA;
        const float u = det_u / detA;
        const float v = det_v / detA;
        if ((detA != 0.0f) && (t >= 0.0f) && (u >= 0.0f) && (v >= 0.0f) && ((u + v) <= 1.0f) &&
            (t < h.t)) {
            h.t = t;
            h.tri = i;
        }
    }
}

template <int RULE>
__device__ __forceinline__ Hit closest_hit(const float4* __restrict__ tri_g, int n_tri, f3 o, f3 d,
                                           float t_scale) {
    cfloat4* __restrict__ tri = as_const(tri_g);
    const float nDx = -(d.x * t_scale);
    const float nDy = -(d.y * t_scale);
    const float nDz = -(d.z * t_scale);
    Hit h;
    h.t = (RULE == 0) ? FLT_MAX : 999999.0f;
    h.tri = -1;
    // upper bound of the t window, widened by 2^-18 (RULE 0: best + eps)
    float hi = ((RULE == 0) ? (h.t + kEps) : h.t) * (1.0f + 0x1p-18f);
#pragma unroll 1
    for (int i = 0; i < n_tri; ++i) {
        const float4 A = ldc(tri + i * kIsectF4 + 0);
        const float4 E1 = ldc(tri + i * kIsectF4 + 1);
        const float4 E2 = ldc(tri + i * kIsectF4 + 2);
        const float bx = o.x - A.x, by = o.y - A.y, bz = o.z - A.z;
        // detA = det(-D, e1, e2)
        const float s1 = nDy * E2.z - E2.y * nDz;
        const float s2 = nDy * E1.z - E1.y * nDz;
        const float detA = (nDx * A.w - E1.x * s1) + E2.x * s2;
        // det_t = det(b, e1, e2)
        const float s3 = by * E2.z - E2.y * bz;
        const float s4 = by * E1.z - E1.y * bz;
        const float det_t = (bx * A.w - E1.x * s3) + E2.x * s4;
        // det_u = det(-D, b, e2), det_v = det(-D, e1, b)
        const float s5 = nDy * bz - by * nDz;
        const float s6 = E1.y * bz - by * E1.z;
        const float det_u = (nDx * s3 - bx * s1) + E2.x * s5;
        const float det_v = (nDx * s6 - E1.x * s5) + bx * s2;
        // Conservative rejection: with |detA| in [2^-100, 2^100], v_rcp_f32 is
        // within 1 ulp, so ta/ua/va differ from the exact t/u/v by < 2^-21
        // relative.  A lane is rejected only if the exact test must fail:
        //   ta < eps(1-2^-18) (RULE 0) or ta < -2^-90 (RULE 1)  =>  t fails
        //   ta > hi = (best [+eps]) (1+2^-18)                   =>  t fails
        //   ua or va < -2^-90 (no underflow to -0 possible)     =>  u/v fail
        //   ua + va > 1 + 2^-18 (with ua, va >= -2^-90)         =>  u+v > 1
        // NaN/inf or out-of-range detA never rejects.
        const float r = __builtin_amdgcn_rcpf(detA);
        const float ta = det_t * r, ua = det_u * r, va = det_v * r;
        const float ad = fabsf(detA);
        const float lo = (RULE == 0) ? kEps * (1.0f - 0x1p-18f) : -0x1p-90f;
        const bool sure_miss = (ad >= 0x1p-100f) && (ad <= 0x1p100f) &&
                               ((ta < lo) || (ta > hi) || (ua < -0x1p-90f) || (va < -0x1p-90f) ||
                                ((ua + va) > 1.0f + 0x1p-18f));
        if (!sure_miss) {
            if (RULE == 0)
                exact_test_inv<RULE>(detA, rcp_rn_from(detA, r), det_t, det_u, det_v, i, h);
            else
                exact_test<RULE>(detA, det_t, det_u, det_v, i, h);
            hi = ((RULE == 0) ? (h.t + kEps) : h.t) * (1.0f + 0x1p-18f);
        }
    }
    return h;
}

// Exact test of triangle i, record loaded by this lane: the operations of
// closest_hit (same operands, same order), so the same bits.
template <int RULE>
__device__ __forceinline__ void exact_one(const float4* __restrict__ tri, int i, f3 o, float nDx,
                                          float nDy, float nDz, Hit& h) {
    const float4 A = tri[i * kIsectF4 + 0];
    const float4 E1 = tri[i * kIsectF4 + 1];
    const float4 E2 = tri[i * kIsectF4 + 2];
    const float bx = o.x - A.x, by = o.y - A.y, bz = o.z - A.z;
    const float s1 = nDy * E2.z - E2.y * nDz;
    const float s2 = nDy * E1.z - E1.y * nDz;
    const float detA = (nDx * A.w - E1.x * s1) + E2.x * s2;
    const float s3 = by * E2.z - E2.y * bz;
    const float s4 = by * E1.z - E1.y * bz;
    const float det_t = (bx * A.w - E1.x * s3) + E2.x * s4;
    const float s5 = nDy * bz - by * nDz;
    const float s6 = E1.y * bz - by * E1.z;
    const float det_u = (nDx * s3 - bx * s1) + E2.x * s5;
    const float det_v = (nDx * s6 - E1.x * s5) + bx * s2;
    exact_test<RULE>(detA, det_t, det_u, det_v, i, h);
}

// exact_one with a wave-uniform triangle index: the record arrives by scalar loads
// (same operands, same order, so the same bits).
template <int RULE>
__device__ __forceinline__ void exact_one_c(cfloat4* __restrict__ tri, int i, f3 o, float nDx,
                                            float nDy, float nDz, Hit& h) {
    const float4 A = ldc(tri + i * kIsectF4 + 0);
    const float4 E1 = ldc(tri + i * kIsectF4 + 1);
    const float4 E2 = ldc(tri + i * kIsectF4 + 2);
    const float bx = o.x - A.x, by = o.y - A.y, bz = o.z - A.z;
    const float s1 = nDy * E2.z - E2.y * nDz;
    const float s2 = nDy * E1.z - E1.y * nDz;
    const float detA = (nDx * A.w - E1.x * s1) + E2.x * s2;
    const float s3 = by * E2.z - E2.y * bz;
    const float s4 = by * E1.z - E1.y * bz;
    const float det_t = (bx * A.w - E1.x * s3) + E2.x * s4;
    const float s5 = nDy * bz - by * nDz;
    const float s6 = E1.y * bz - by * E1.z;
    const float det_u = (nDx * s3 - bx * s1) + E2.x * s5;
    const float det_v = (nDx * s6 - E1.x * s5) + bx * s2;
    exact_test<RULE>(detA, det_t, det_u, det_v, i, h);
}

// ---- Primary-ray culling (k_render_ps) ----
// A camera ray through pixel (px, py) with jitter (r1, r2) in [0, 1)^2 has direction
// d = Rf p / |p| (+ rounding), p = (px + r1 - W/2, py + r2 - H/2, H), Rf the camera's float
// rotation (camera_ray).  Over a pixel rectangle every filter quantity of
// closest_hit_filtered is a linear form a.d (or a constant): Ad = N.d, U = (o x e2 - G2).d,
// V = (-(o x e1) + G1).d, T = w0 - o.N, with o the camera position.  A triangle is culled
// for the rectangle when, for every such d, the filter's rejection holds with twice its
// margins -- the filter's float evaluation differs from these real values by at most
// 18u S (record and evaluation rounding), below the margins' c S = 256u S, so the filter
// would reject every one of these rays, and the filter rejects only pairs whose exact
// test fails (build_filter, rt_capi.cpp).  So a culled triangle cannot be the hit of any
// primary ray of the rectangle, and testing the others in index order gives the
// reference's hit bit for bit.
// CamRect, rect_cull: rt_cull.hpp (shared with the host for tests)

// Two-phase closest hit: the same Hit as closest_hit, bit for bit.
//
// The reference's predicate is the exact float Cramer test of every triangle in
// index order, each accepted hit narrowing the t window of the next.  Its result
// depends only on the triangles that pass the geometric part of the test
// (detA != 0, u >= 0, v >= 0, u + v <= 1, t > eps [RULE 0] / t >= 0 [RULE 1]),
// taken in index order.  Phase 1 (wave-uniform loop, records in SGPRs) evaluates
// the same quantities with 18 FMAs instead of 43 unfused operations, scaled by
// 1/t_scale and with the sign of the determinant folded in:
//   Ad = d.N,  T = w0 - o.N,  U = e2.R - d.G2,  V = -e1.R + d.G1   (R = d x o)
//   u = U/Ad,  v = V/Ad,  t = T/(t_scale Ad)
// and rejects a pair only when it is farther from the decision boundary than the
// combined rounding error of both evaluations (the per-triangle bounds eA, EW, ET
// of build_filter, rt_capi.cpp); the survivors set a bit of the lane's candidate
// mask.  Phase 2 runs the exact test (exact_one) on the candidates in index order.
// NaN/inf inputs never reject (the comparisons fail), and a zero direction leaves
// |Ad| <= eA, which never rejects either.
// Phase-1 quantities of one (ray, triangle) pair against filter record `f`,
// returned as three floats whose sign bits say "certain to fail":
//   x1 = eA - |Ad|        < 0  <=>  |Ad| > eA   (the sign of Ad is certain)
//   x2 = min(u,v,w) + EW  < 0  <=>  a barycentric test certainly fails
//   x3 = tm + ET          < 0  <=>  the t test certainly fails
// The exact test certainly fails iff x1 < 0 and (x2 < 0 or x3 < 0).  The sums are
// exact in sign (a nonzero exact sum never rounds to zero under gradual underflow,
// and an exact zero is +0), so each sign bit equals the comparison it stands for.
// Finite inputs only (the caller keeps every triangle of a non-finite ray).
template <int RULE>
__device__ __forceinline__ void filter_eval(cfloat4* __restrict__ f, f3 o, f3 d, float Rx,
                                            float Ry, float Rz, float ets, float* x1, float* x2,
                                            float* x3) {
    const float4 F0 = ldc(f + 0), F1 = ldc(f + 1), F2 = ldc(f + 2), F3 = ldc(f + 3), F4 = ldc(f + 4);
    const float ad = fmaf(d.x, F0.x, fmaf(d.y, F0.y, d.z * F0.z));
    const float tt = fmaf(-o.x, F0.x, fmaf(-o.y, F0.y, fmaf(-o.z, F0.z, F0.w)));
    const float uu = fmaf(F1.x, Rx, fmaf(F1.y, Ry, fmaf(F1.z, Rz,
                     fmaf(d.x, F2.x, fmaf(d.y, F2.y, d.z * F2.z)))));
    const float vv = fmaf(F3.x, Rx, fmaf(F3.y, Ry, fmaf(F3.z, Rz,
                     fmaf(d.x, F4.x, fmaf(d.y, F4.y, d.z * F4.z)))));
    const uint32_t sg = __float_as_uint(ad) & 0x80000000u;
    const float su = __uint_as_float(__float_as_uint(uu) ^ sg);
    const float sv = __uint_as_float(__float_as_uint(vv) ^ sg);
    const float st = __uint_as_float(__float_as_uint(tt) ^ sg);
    const float aa = fabsf(ad);
    const float w = (aa - su) - sv;
    const float m = fminf(fminf(su, sv), w);
    const float tm = (RULE == 0) ? fmaf(-ets, aa, st) : st;
    *x1 = F1.w - aa;
    *x2 = m + F2.w;
    *x3 = tm + F3.w;
}

// keep bit (bit 31) of one pair: NOT (x1 & (x2 | x3)) on the sign bits
__device__ __forceinline__ uint32_t keep_bit(float x1, float x2, float x3) {
    return ~(__float_as_uint(x1) & (__float_as_uint(x2) | __float_as_uint(x3)));
}

// Phase 1 over triangles [0, cnt) of one 32-triangle block `f`, in pairs (records
// padded to an even count), branch-free and all-VALU: each keep bit is shifted in
// at bit 0 (v_alignbit), so triangle j ends at bit cnt-1-j (the pad falls off the
// bottom).  `finite`: false for a ray with a non-finite component (keep all).
template <int RULE>
__device__ __forceinline__ uint32_t filter_block(cfloat4* __restrict__ f, int cnt, bool finite,
                                                 f3 o, f3 d, float Rx, float Ry, float Rz,
                                                 float ets) {
    uint32_t mask = 0u;
    const int cnt2 = (cnt + 1) & ~1;
#pragma clang loop vectorize(disable) unroll(disable)
    for (int j = 0; j < cnt2; j += 2) {
        float a1, a2, a3, b1, b2, b3;
        filter_eval<RULE>(f + j * kFiltF4, o, d, Rx, Ry, Rz, ets, &a1, &a2, &a3);
        filter_eval<RULE>(f + (j + 1) * kFiltF4, o, d, Rx, Ry, Rz, ets, &b1, &b2, &b3);
        mask = __builtin_amdgcn_alignbit(mask, keep_bit(a1, a2, a3), 31);
        mask = __builtin_amdgcn_alignbit(mask, keep_bit(b1, b2, b3), 31);
    }
    mask >>= (cnt2 - cnt);
    const uint32_t all = (cnt >= 32) ? 0xffffffffu : ((1u << cnt) - 1u);
    return finite ? mask : all;
}

template <int RULE>
__device__ __forceinline__ Hit closest_hit_filtered(const float4* __restrict__ filt,
                                                    const float4* __restrict__ tri, int n_tri, f3 o,
                                                    f3 d, float t_scale) {
    const float nDx = -(d.x * t_scale);
    const float nDy = -(d.y * t_scale);
    const float nDz = -(d.z * t_scale);
    const float Rx = fmaf(d.y, o.z, -(d.z * o.y));
    const float Ry = fmaf(d.z, o.x, -(d.x * o.z));
    const float Rz = fmaf(d.x, o.y, -(d.y * o.x));
    const float ets = kEps * t_scale;
    const bool finite = __builtin_isfinite(o.x) & __builtin_isfinite(o.y) & __builtin_isfinite(o.z) &
                        __builtin_isfinite(d.x) & __builtin_isfinite(d.y) & __builtin_isfinite(d.z);
    Hit h;
    h.t = (RULE == 0) ? FLT_MAX : 999999.0f;
    h.tri = -1;
    // 64 triangles per round: both masks first, then ONE divergent phase-2 loop over a
    // lane's candidates of the round in index order (the wave iterates the max over
    // lanes of the round's total instead of the sum of two per-block maxima; rounds of
    // 128 with a two-word mask measured slower).  Triangle base + i sits at bit
    // (c0 + c1 - 1 - i) of (m0 << c1 | m1).
    for (int base = 0; base < n_tri; base += 64) {
        const int c0 = min(32, n_tri - base);
        const int c1 = min(32, n_tri - base - 32);
        const uint32_t m0 =
            filter_block<RULE>(as_const(filt) + (size_t)base * kFiltF4, c0, finite, o, d, Rx, Ry, Rz, ets);
        uint32_t m1 = 0u;
        if (c1 > 0)
            m1 = filter_block<RULE>(as_const(filt) + (size_t)(base + 32) * kFiltF4, c1, finite, o, d, Rx, Ry,
                                    Rz, ets);
        uint64_t mm = ((uint64_t)m0 << (c1 > 0 ? c1 : 0)) | (uint64_t)m1;
        const int top = base + c0 + (c1 > 0 ? c1 : 0) - 1;
        while (mm != 0ull) {
            const int b = 63 - __builtin_clzll(mm);
            mm ^= 1ull << b;
            exact_one<RULE>(tri, top - b, o, nDx, nDy, nDz, h);
        }
    }
    return h;
}

// ---- The filter on the matrix cores (rays from surface points) ----
// closest_hit_filtered spends 31 VALU instructions per (ray, triangle) pair, 18 of them
// the four dot products A, T, U, V.  closest_hit_mf evaluates those on
// v_mfma_f32_16x16x32_bf16 (features and rows split into bf16 hi + lo, three products
// per term: rt_internal.hpp, kMfRound) and keeps 10 VALU instructions per pair for
// the tests, at margins 16x wider (c = 2^-12) than the fp32 filter's, folded into the
// rows' scale (build_mf_rows in rt_capi.cpp): no per-triangle margin loads.  Wave-level: every lane of the wave calls it
// (`active` false: a lane whose result is not used; it gets no candidates).
typedef __bf16 mf_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mf_bf16x2 __attribute__((ext_vector_type(2)));
typedef float mf_f32x4 __attribute__((ext_vector_type(4)));
typedef float mf_f32x2 __attribute__((ext_vector_type(2)));

// x, y -> bf16x2 hi (RNE) and bf16x2 lo = RNE(x - hi) (x - hi is exact)
__device__ __forceinline__ void mf_split2(float x, float y, uint32_t* hi, uint32_t* lo) {
    const mf_f32x2 v = {x, y};
    const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, mf_bf16x2));
    const mf_f32x2 r = {x - __uint_as_float(hb << 16), y - __uint_as_float(hb & 0xffff0000u)};
    *hi = hb;
    *lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, mf_bf16x2));
}

// 4x4 transpose of the 16-lane rows: in, x_p at row r = M[r][p]; out, x_c at row r = M[c][r]
__device__ __forceinline__ void mf_transpose(uint32_t& x0, uint32_t& x1, uint32_t& x2, uint32_t& x3) {
    auto a = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);  // rows 2,3 of x0 <-> rows 0,1 of x2
    auto b = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
    auto c = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);  // odd rows of x0 <-> even rows of x1
    auto d = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    x0 = c[0];
    x1 = c[1];
    x2 = d[0];
    x3 = d[1];
}

typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));

// A 16-B global load the compiler cannot move or merge (closest_hit_mf's prefetch), and
// the waits that make its result usable: vmcnt(1) = every load but the newest landed
// (the other fragment may still be in flight; extra loads of the compiler's only make it
// stricter), vmcnt(0) = all landed.  The fragments pass through the waits' asm as
// in/out operands, so no use of them can be scheduled above the wait.  No memory clobber:
// the image is read-only, and the compiler's own loads need no ordering against these
// (its waits count only its loads, so ours can only make them wait longer).
__device__ __forceinline__ mf_u32x4 mf_load(const uint4* p) {
    mf_u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p));
    return v;
}
__device__ __forceinline__ void mf_wait1(mf_u32x4& v) { asm volatile("s_waitcnt vmcnt(1)" : "+v"(v)); }
__device__ __forceinline__ void mf_wait0(mf_u32x4& a, mf_u32x4& b) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b));
}

__device__ __forceinline__ mf_bf16x8 mf_frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {a, b, c, d};
    return __builtin_bit_cast(mf_bf16x8, v);
}

// drop bit (bit 31) of one pair from the scaled row values A, T', U, V (build_mf_rows:
// margins 1, sign-test threshold rho): set iff the exact test must fail, i.e. |A| > rho and
// one of s U, s V, s W (W = A - U - V), s T' is below -1, s = sign A.  s X + 1 < 0 is tested
// as the sign of fma(X, A, |A|) = |A| (s X + 1), which one rounding cannot flip (an exact
// 0 gives +0: keep); W's two subtractions round as the fp32 filter's (aa - su) - sv do.
__device__ __forceinline__ uint32_t mf_drop(mf_f32x4 q, float rho) {
    const float A = q[0], aa = fabsf(q[0]);
    const float w = (A - q[2]) - q[3];
    const float xu = fmaf(q[2], A, aa), xv = fmaf(q[3], A, aa);
    const float xw = fmaf(w, A, aa), xt = fmaf(q[1], A, aa);
    const float mn = fminf(fminf(xu, xv), fminf(xw, xt));
    return __float_as_uint(rho - aa) & __float_as_uint(mn);
}

// groups of the image that hold triangles (all rounds but the last are full)
__host__ __device__ inline int mf_groups(int n_tri) {
    if (n_tri <= 0) return 0;
    const int rounds = (n_tri + kMfRound - 1) / kMfRound;
    const int last = n_tri - (rounds - 1) * kMfRound;
    return (rounds - 1) * kMfGroupsPerRound + (last + 3) / 4;
}

// The exact test of triangle i without the t window: t if the triangle passes
// (detA != 0, t >= 0, u, v >= 0, u + v <= 1, t > eps for RULE 0), else +inf; the
// operations of exact_one (same operands, same order, so the same bits).  Accepting t
// when t < best + eps (RULE 0) / t < best (RULE 1), in index order, is exact_one's
// result (+inf, like a NaN, never passes either window).
template <int RULE>
__device__ __forceinline__ float exact_tv(const float4* __restrict__ tri, int i, f3 o, float nDx, float nDy,
                                          float nDz) {
    const float4 A = tri[i * kIsectF4 + 0];
    const float4 E1 = tri[i * kIsectF4 + 1];
    const float4 E2 = tri[i * kIsectF4 + 2];
    const float bx = o.x - A.x, by = o.y - A.y, bz = o.z - A.z;
    const float s1 = nDy * E2.z - E2.y * nDz;
    const float s2 = nDy * E1.z - E1.y * nDz;
    const float detA = (nDx * A.w - E1.x * s1) + E2.x * s2;
    const float s3 = by * E2.z - E2.y * bz;
    const float s4 = by * E1.z - E1.y * bz;
    const float det_t = (bx * A.w - E1.x * s3) + E2.x * s4;
    const float s5 = nDy * bz - by * nDz;
    const float s6 = E1.y * bz - by * E1.z;
    const float det_u = (nDx * s3 - bx * s1) + E2.x * s5;
    const float det_v = (nDx * s6 - E1.x * s5) + bx * s2;
    float t, u, v;
    if (RULE == 0) {
        const float inv = rcp_rn(detA);
        t = det_t * inv;
        u = det_u * inv;
        v = det_v * inv;
    } else {
        t = det_t / detA;
        u = det_u / detA;
        v = det_v / detA;
    }
    const bool ok = (detA != 0.0f) && (t >= 0.0f) && (u >= 0.0f) && (v >= 0.0f) && ((u + v) <= 1.0f) &&
                    (RULE != 0 || t > kEps);
    return ok ? t : __builtin_inff();
}

#ifndef RT_PROF
#define RT_PROF 0  // 1: k_render_ps sums per-phase s_memtime cycles into RenderLaunch::prof
#endif

// LDS of one wave for the shared exact phase: rays [6][64] (o, -D), pairs [cap] u16
// (lane << 6 | triangle of the block), then the tests' t values [cap] (read back from LDS:
// by cross-lane reads instead, Cornell 512^2 x 256 took 4.19 vs 3.96 ms)
#ifndef RT_MF_PAIR_CAP
#define RT_MF_PAIR_CAP 256
#endif
constexpr int kMfPairCap = RT_MF_PAIR_CAP;
constexpr int kMfWaveFloats = 6 * 64 + kMfPairCap / 2 + kMfPairCap;
static_assert(kMfWaveFloats >= 11 * 64, "cand_exact_min's LDS (rays, first, mask, key) fits a wave's block");
// The table-route kernel k_render_ps<.., CT> (RULE 0): about 3 candidates per ray of which the
// lane tests its first RT_CTAB_OWN itself, so the shared phase lists a few dozen pairs per wave;
// a smaller list block (with the shading records left in L1/L2) lets one more workgroup fit a
// CU's LDS
#ifndef RT_PS_CT_PAIR_CAP
#define RT_PS_CT_PAIR_CAP 96  // (64 / 96 / 128 / 256: 2.37 / 2.33 / 2.34 / 2.63 ms with the shading records in L1/L2)
#endif
constexpr int kCtPairCap = RT_PS_CT_PAIR_CAP;
__host__ __device__ constexpr int mf_wave_floats(int cap, int rule) {
    return (rule == 1 && 6 * 64 + cap / 2 + cap < 11 * 64) ? 11 * 64 : 6 * 64 + cap / 2 + cap;
}

#if RT_PROF
// counters of the shared exact phase, per wave (RT_PROF builds; k_render_ps sums them into
// RenderLaunch::prof): iterations of the listing walk and of the fold loop, pairs listed, test
// rounds of 64, pairs that pass exact_tv, and the sum over trips of the most passing pairs one
// lane owned
struct ExactProf {
    unsigned list_iters, fold_iters, pairs, rounds, passes, max_pass;
};
#else
struct ExactProf;
#endif

__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The exact phase of one 64-triangle block (triangles tri0 + bit of F) shared by the
// wave: the lanes' candidate pairs are listed in LDS in (lane, index) order and tested
// 64 at a time by all lanes, then each lane folds its own results in index order.  The
// trip count is (candidates of the wave) / 64 instead of the largest per-lane count.
template <int RULE, int CAP = kMfPairCap>
__device__ __forceinline__ void mf_exact_wave(const float4* __restrict__ isect, int tri0, uint64_t F, f3 o,
                                              float nDx, float nDy, float nDz, float* wl, int lane, Hit& h,
                                              ExactProf* xp = nullptr) {
    const int cnt = __builtin_popcountll(F);  // 0..64: 7 bits
    // exclusive prefix sum over the lanes, bit-sliced through ballots (no LDS round trips,
    // unlike a shuffle scan: the cross-lane permutes were a dependent chain of 6)
    int excl = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const uint64_t bm = __ballot((cnt >> b) & 1);
        excl += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u)) << b;
        total += __builtin_popcountll(bm) << b;
    }
    if (total == 0) return;
    const float* ray = wl;  // (o, -D) of every lane: written by closest_hit_mf before its masks
    uint16_t* pr = reinterpret_cast<uint16_t*>(wl + 6 * 64);
#if RT_PROF
    unsigned my_pass = 0, walk = 0;
    if (xp) {
        for (int c = 64; c >= 1; --c)
            if (walk == 0 && __ballot(cnt >= c) != 0ull) walk = (unsigned)c;  // the busiest lane's count
        xp->pairs += total;
    }
#endif
    for (int cb = 0; cb < total; cb += CAP) {
#if RT_PROF
        if (xp) {
            xp->list_iters += walk;
            xp->fold_iters += walk;
        }
#endif
        {
            uint64_t G = F;
            int p = excl - cb;
            while (G != 0ull) {
                const int b = __builtin_ctzll(G);
                G &= G - 1ull;
                if (p >= 0 && p < CAP) pr[p] = (uint16_t)((lane << 6) | b);
                ++p;
            }
        }
        wave_lds_sync();
        const int nb = min(CAP, total - cb);
        float* tv = wl + 6 * 64 + CAP / 2;
        for (int k = lane; k < nb; k += 64) {
            const uint32_t q = pr[k];
            const int rl = (int)(q >> 6);
            const f3 ro = make3(ray[0 * 64 + rl], ray[1 * 64 + rl], ray[2 * 64 + rl]);
            tv[k] = exact_tv<RULE>(isect, tri0 + (int)(q & 63u), ro, ray[3 * 64 + rl], ray[4 * 64 + rl],
                                   ray[5 * 64 + rl]);
#if RT_PROF
            if (xp) {
                xp->rounds += 1;
                xp->passes += __builtin_popcountll(__ballot(tv[k] < __builtin_inff()));
            }
#endif
        }
        wave_lds_sync();
        {
            uint64_t G = F;
            int p = excl - cb;
            while (G != 0ull) {
                const int b = __builtin_ctzll(G);
                G &= G - 1ull;
                if (p >= 0 && p < CAP) {
                    const float t = tv[p];
#if RT_PROF
                    my_pass += t < __builtin_inff() ? 1u : 0u;
#endif
                    if ((RULE == 0) ? (t < h.t + kEps) : (t < h.t)) {
                        h.t = t;
                        h.tri = tri0 + b;
                    }
                }
                ++p;
            }
        }
        wave_lds_sync();  // the pair list is read before the next window overwrites it
    }
#if RT_PROF
    if (xp) {
        for (int c = 61; c >= 1; --c)
            if (__ballot(my_pass >= (unsigned)c) != 0ull) {
                xp->max_pass += (unsigned)c;
                break;
            }
    }
#endif
}

// s.mf_frag may point to a workgroup's LDS copy of the image (k_render_ps);
// wl: the wave's LDS for the shared exact phase (kMfWaveFloats floats)
// NB: 64-triangle blocks per super-block (1: scenes of <= 64 triangles, fewer registers)
// ovr (wave-uniform, kRenderCullWords 64-triangle masks) with use_ovr: the lane's candidates
// are ovr's instead of the filter's (k_render's camera rays: the wave's primary-ray cull,
// rt_cull.hpp, when the camera lies outside mf_bound); they join the shared exact phase.
template <int RULE, bool COUNT = false, int NB = 4>
__device__ __forceinline__ Hit closest_hit_mf(const DeviceScene& s, f3 o, f3 d, float t_scale, bool active,
                                              float* wl, int* n_cand = nullptr, uint64_t* t_mask_end = nullptr,
                                              const uint64_t* ovr = nullptr, bool use_ovr = false) {
    const float nDx = -(d.x * t_scale);
    const float nDy = -(d.y * t_scale);
    const float nDz = -(d.z * t_scale);
    const bool finite = __builtin_isfinite(o.x) & __builtin_isfinite(o.y) & __builtin_isfinite(o.z) &
                        __builtin_isfinite(d.x) & __builtin_isfinite(d.y) & __builtin_isfinite(d.z);
    const float om = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const float dm = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    const bool keep_all = !(finite && om <= s.mf_bound && dm <= kMfDirBound);
    const int lane = threadIdx.x & 63;
    // the lane's ray for the shared exact phase, parked in LDS now: o and -D are not held in
    // registers through the masks (the caller may read them back: wl rows 0-5)
    wl[0 * 64 + lane] = o.x;
    wl[1 * 64 + lane] = o.y;
    wl[2 * 64 + lane] = o.z;
    wl[3 * 64 + lane] = nDx;
    wl[4 * 64 + lane] = nDy;
    wl[5 * 64 + lane] = nDz;
    const uint4* __restrict__ frag = s.mf_frag;
    const mf_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    Hit h;
    h.t = (RULE == 0) ? FLT_MAX : 999999.0f;
    h.tri = -1;
    const int n_tri = s.n_tri;
    // super-blocks of 256 triangles: the masks of all 8 rounds first (the ray operands
    // die there), then the exact phase of each 64-triangle block
    for (int sb = 0; sb < n_tri; sb += 2 * NB * kMfRound) {
        uint64_t F0 = 0ull, F1 = 0ull, F2 = 0ull, F3 = 0ull;
        {
            const float Rx = fmaf(d.y, o.z, -(d.z * o.y));
            const float Ry = fmaf(d.z, o.x, -(d.x * o.z));
            const float Rz = fmaf(d.x, o.y, -(d.y * o.x));
            const float ets = (RULE == 0) ? kEps * t_scale : 0.0f;
            const float px = fmaf(-ets, d.x, -o.x), py = fmaf(-ets, d.y, -o.y), pz = fmaf(-ets, d.z, -o.z);
            // features f = (d, o', R, 1) as bf16 pairs: h_k = (fh_2k, fh_2k+1), l_k likewise
            uint32_t h0, h1, h2, h3, h4, l0, l1, l2, l3, l4;
            mf_split2(d.x, d.y, &h0, &l0);
            mf_split2(d.z, px, &h1, &l1);
            mf_split2(py, pz, &h2, &l2);
            mf_split2(Rx, Ry, &h3, &l3);
            mf_split2(Rz, 1.0f, &h4, &l4);
            // the four K parts of the lane's ray, then across the rows: B operand of ray block c
            uint32_t b00 = h0, b01 = h1, b02 = h2, b03 = h3;  // k  0.. 7
            uint32_t b10 = h4, b11 = l0, b12 = l1, b13 = l2;  // k  8..15
            uint32_t b20 = l3, b21 = l4, b22 = h0, b23 = h1;  // k 16..23
            uint32_t b30 = h2, b31 = h3, b32 = h4, b33 = 0u;  // k 24..31
            mf_transpose(b00, b10, b20, b30);
            mf_transpose(b01, b11, b21, b31);
            mf_transpose(b02, b12, b22, b32);
            mf_transpose(b03, b13, b23, b33);
            const mf_bf16x8 B0 = mf_frag(b00, b01, b02, b03), B1 = mf_frag(b10, b11, b12, b13);
            const mf_bf16x8 B2 = mf_frag(b20, b21, b22, b23), B3 = mf_frag(b30, b31, b32, b33);
            const int n_rounds = min(2 * NB, (n_tri - sb + kMfRound - 1) / kMfRound);
#pragma clang loop unroll(disable)
            for (int rr = 0; rr < n_rounds; ++rr) {
                const int r = sb / kMfRound + rr;
                const int cnt = min(kMfRound, n_tri - r * kMfRound);
                const int G = (cnt + 3) >> 2;
                uint32_t m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u;
                const int gi0 = r * kMfGroupsPerRound;
                // one 4-triangle group: 4 MFMAs (ray blocks 0..3), drop bits shifted in
                auto group = [&](const mf_u32x4 af) {
                    // the slots' sign-test thresholds, stored in the fragment's unused K entries
                    // (build_mf_image: lane 48 + 4 s, dword 3): the group's largest, lane 49 (one scalar
                    // per group, a looser test for its smaller triangles; measured faster than
                    // per-slot thresholds and than the bound 1/2 for all, profiles/r3i)
                    const float rho = __int_as_float(__builtin_amdgcn_readlane((int)af[3], 49));
                    const mf_bf16x8 A = __builtin_bit_cast(mf_bf16x8, af);
                    const mf_f32x4 q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B0, zero, 0, 0, 0);
                    const mf_f32x4 q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B1, zero, 0, 0, 0);
                    const mf_f32x4 q2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B2, zero, 0, 0, 0);
                    const mf_f32x4 q3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B3, zero, 0, 0, 0);
                    m0 = __builtin_amdgcn_alignbit(m0, mf_drop(q0, rho), 31);
                    m1 = __builtin_amdgcn_alignbit(m1, mf_drop(q1, rho), 31);
                    m2 = __builtin_amdgcn_alignbit(m2, mf_drop(q2, rho), 31);
                    m3 = __builtin_amdgcn_alignbit(m3, mf_drop(q3, rho), 31);
                };
                // two operand sets in flight: group g + 2's fragment is loaded right after
                // group g's MFMAs have read theirs, a whole group of work before its use.
                // The loads are inline asm with explicit waits: written as plain loads, the
                // optimizer proves the prefetched value equals a load at the top of the
                // next trip and moves it there, waiting on it at once.  mf_wait1 returns
                // the fragment (tied through the asm), so its MFMAs cannot move above it.
                // An odd G starts with a pad group (index G < 8: zero rows, so its drop bit
                // is 0 and lands at bit G of the slot mask, where the next slot's bit 0 is
                // or-ed in).  The prefetches past the end reload group G - 1 (in range).
                const uint4* __restrict__ fr = frag + (size_t)gi0 * 64 + lane;
                const int gs = -(G & 1);
                mf_u32x4 fa = mf_load(fr + (gs < 0 ? G : 0) * 64);
                mf_u32x4 fb = mf_load(fr + (gs + 1) * 64);
                for (int g = gs; g < G; g += 2) {
                    const int n2 = min(g + 2, G - 1), n3 = min(g + 3, G - 1);
                    mf_wait1(fa);
                    group(fa);
                    fa = mf_load(fr + n2 * 64);
                    mf_wait1(fb);
                    group(fb);
                    fb = mf_load(fr + n3 * 64);
                }
                mf_wait0(fa, fb);  // the last (unused) loads land before their registers are reused
                // lane (slot s, ray q) holds m_c for ray 16 c + q; after the transpose lane
                // (c, q) holds the masks of slots 0..3 of its own ray: bit j of slot s's mask
                // is triangle s G + j of the round
                mf_transpose(m0, m1, m2, m3);
                const uint32_t Dr = m0 | (m1 << G) | (m2 << (2 * G)) | (m3 << (3 * G));  // drop bits
                const uint32_t all = (cnt >= 32) ? 0xffffffffu : ((1u << cnt) - 1u);
                const uint32_t Fr = keep_all ? all : (~Dr & all);
                const uint64_t Fs = (uint64_t)Fr << (32 * (rr & 1));  // wave-uniform word select
                const int w = rr >> 1;
                F0 |= (w == 0) ? Fs : 0ull;
                if (NB > 1) {
                    F1 |= (w == 1) ? Fs : 0ull;
                    F2 |= (w == 2) ? Fs : 0ull;
                    F3 |= (w == 3) ? Fs : 0ull;
                }
            }
        }
#if RT_PROF
        if (t_mask_end) *t_mask_end = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
        for (int w = 0; w < NB; ++w) {
            const int tri0 = sb + 64 * w;
            if (tri0 >= n_tri) break;
            uint64_t Fw = active ? (w == 0 ? F0 : w == 1 ? F1 : w == 2 ? F2 : F3) : 0ull;
            if (ovr != nullptr) {
                const int g = (sb >> 6) + w;
                Fw = use_ovr ? ((active && g < 4) ? ovr[g < 4 ? g : 0] : 0ull) : Fw;
            }
            if (COUNT) *n_cand += __builtin_popcountll(Fw);
            // With one 64-triangle block the lane's first candidate on its own lane (its own ray,
            // no pair list: every live lane has one, usually its hit), then the rest (≈ 0.3 per
            // ray) shared by the wave (Cornell 512^2 x 256: 3.92 vs 4.00 ms; on
            // complex_light_room's four blocks it measured 314 vs 310 ms, so wider scenes share
            // every pair: profiles/r3q/)
            if (NB == 1 && Fw != 0ull) {
                const int b = __builtin_ctzll(Fw);
                const float t = exact_tv<RULE>(s.isect, tri0 + b, o, nDx, nDy, nDz);
                if ((RULE == 0) ? (t < h.t + kEps) : (t < h.t)) {
                    h.t = t;
                    h.tri = tri0 + b;
                }
                Fw &= Fw - 1ull;
            }
            mf_exact_wave<RULE>(s.isect, tri0, Fw, o, nDx, nDy, nDz, wl, lane, h);
        }
    }
    return h;
}

// The candidates of a bounce ray leaving surface `surf` (rt_ctab.cpp) from the table T of the
// launch's hit rule: the mask of its (origin patch, direction bin) OR that of its grazing bin
// OR, for a direction within T.cop_th of the surface's plane (always, under rule 1), the
// triangles coplanar with it -- every other triangle fails the exact test for this ray -- or
// every triangle where the table does not apply (origin off the surface's plane or grid, a
// direction off its hemisphere, non-unit or non-finite).  F: NW >= T.words mask words (the
// rest 0).  rt_ctab.cpp ctab_lookup is the same lookup on the host.
//
// The lookup in two halves, for a caller with independent work to put between them
// (k_render_ps's pipelined bounce loop): ctab_begin runs the address arithmetic and issues the
// loads of the entry's mask words -- the end of a chain of two dependent global loads (the
// surface's patch frame, then the entry) -- and ctab_finish, the first use of those words,
// folds them into F.  ctab_candidates is the two back to back.
template <int NW>
struct CtabLook {
    uint64_t m[NW];  // the entry's mask words as loaded (0 where the table does not apply)
    int gi;          // the direction's grazing bin
    bool in, cp;     // the table applies; the coplanar triangles join
};
struct CtabFrame {  // a surface's patch frame (CtabDev::tri), the first link of the chain
    float4 R0, R1, R2, R3;
};
__device__ __forceinline__ CtabFrame ctab_frame(const CtabDev& T, int surf) {
    return CtabFrame{T.tri[surf * 4 + 0], T.tri[surf * 4 + 1], T.tri[surf * 4 + 2], T.tri[surf * 4 + 3]};
}
template <int NW>
__device__ __forceinline__ CtabLook<NW> ctab_no_look() {
    CtabLook<NW> L;
#pragma unroll
    for (int k = 0; k < NW; ++k) L.m[k] = 0ull;
    L.gi = 0;
    L.in = false;
    L.cp = false;
    return L;
}
// (with the frame of the surface, 0 <= surf < n_surf, in hand)
template <int NW>
__device__ __forceinline__ CtabLook<NW> ctab_begin(const CtabDev& T, const CtabFrame& R, f3 o, f3 d) {
    CtabLook<NW> L = ctab_no_look<NW>();
    const int W = T.words;
    const float4 R0 = R.R0, R1 = R.R1, R2 = R.R2, R3 = R.R3;
    const float bx = o.x - R0.x, by = o.y - R0.y, bz = o.z - R0.z;
    const float w = (bx * R3.x + by * R3.y) + bz * R3.z;
    const float pu = ((bx * R1.x + by * R1.y) + bz * R1.z) * R0.w;
    const float pv = ((bx * R2.x + by * R2.y) + bz * R2.z) * R0.w;
    const int nu = __float_as_int(R1.w), nv = __float_as_int(R2.w), base = __float_as_int(R3.w);
    const float len2 = fmaf(d.x, d.x, fmaf(d.y, d.y, d.z * d.z));
    const float cn = (d.x * R3.x + d.y * R3.y) + d.z * R3.z;  // R3: the surface's shading normal
    const bool in = (fabsf(w) <= T.h) & (pu >= 0.0f) & (pu < (float)nu) & (pv >= 0.0f) & (pv < (float)nv) &
                    (len2 >= 1.0f - 0x1p-20f) & (len2 <= 1.0f + 0x1p-20f) & (cn >= -kCtabHemi);
    if (!in) return L;
    // cube-map face: the axis of the largest |d_i| (x before y before z on ties), u, v the next two
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const bool fx = (ax >= ay) & (ax >= az), fy = !fx & (ay >= az);
    const float dm = fx ? d.x : (fy ? d.y : d.z);
    const float da = fx ? d.y : (fy ? d.z : d.x);
    const float db = fx ? d.z : (fy ? d.x : d.y);
    const int f = (fx ? 0 : (fy ? 2 : 4)) + (dm < 0.0f ? 1 : 0);
    const float r = __builtin_amdgcn_rcpf(fabsf(dm));
    const float u1 = da * r + 1.0f, v1 = db * r + 1.0f;  // (the build contracts nothing: two roundings)
    const int iu = min(kCtabBins - 1, max(0, (int)(u1 * (0.5f * kCtabBins))));
    const int iv = min(kCtabBins - 1, max(0, (int)(v1 * (0.5f * kCtabBins))));
    const int gu = min(kCtabGraze - 1, max(0, (int)(u1 * (0.5f * kCtabGraze))));
    const int gv = min(kCtabGraze - 1, max(0, (int)(v1 * (0.5f * kCtabGraze))));
    const int patch = base + (int)pu * nv + (int)pv;
    const unsigned long long* mm = T.masks + ((size_t)patch * (6 * kCtabBins * kCtabBins) + (f * kCtabBins + iu) * kCtabBins + iv) * W;
    L.gi = (f * kCtabGraze + gu) * kCtabGraze + gv;
    // the triangles coplanar with the surface join near its plane's great circle (rule 0) or always (rule 1)
    L.cp = fabsf(cn) < T.cop_th;
    L.in = true;
#pragma unroll
    for (int k = 0; k < NW; ++k) L.m[k] = (k < W) ? mm[k] : 0ull;
    return L;
}
template <int NW>
__device__ __forceinline__ CtabLook<NW> ctab_begin(const CtabDev& T, int n_surf, int surf, f3 o, f3 d) {
    if (surf < 0 || surf >= n_surf) return ctab_no_look<NW>();
    return ctab_begin<NW>(T, ctab_frame(T, surf), o, d);
}
template <int NW>
__device__ __forceinline__ void ctab_finish(const CtabDev& T, int n_tri, int surf, const CtabLook<NW>& L,
                                            uint64_t (&F)[NW]) {
    const int W = T.words;
#pragma unroll
    for (int w = 0; w < NW; ++w) F[w] = (w < W) ? ((n_tri - 64 * w >= 64) ? ~0ull : ((1ull << (n_tri - 64 * w)) - 1ull)) : 0ull;
    if (!L.in) return;
    const uint64_t (&m)[NW] = L.m;
    const int gi = L.gi;
    const bool cp = L.cp;
    if (T.gflag) {
        // the grazing fold (rt_ctab.cpp): the entry holds its bin's grazing mask unless bit 63 of
        // its last word asks for the lookup -- one dependent access for most rays, not three
        uint64_t last = 0ull;
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (k == W - 1) last = m[k];
        const bool look = (last & kCtabGflagBit) != 0ull;
        const unsigned long long* gg = look ? T.gdict + (size_t)T.gid[gi] * W : nullptr;
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (k < W)
                F[k] = (m[k] & (k == W - 1 ? ~kCtabGflagBit : ~0ull)) | (look ? gg[k] : 0ull) |
                       (cp ? T.cop[surf * W + k] : 0ull);
        return;
    }
    const unsigned long long* gg = T.gdict + (size_t)T.gid[gi] * W;
#pragma unroll
    for (int k = 0; k < NW; ++k)
        if (k < W) F[k] = m[k] | gg[k] | (cp ? T.cop[surf * W + k] : 0ull);
}
template <int NW>
__device__ __forceinline__ void ctab_candidates(const CtabDev& T, int n_tri, int n_surf, int surf, f3 o, f3 d,
                                                uint64_t (&F)[NW]) {
    const CtabLook<NW> L = ctab_begin<NW>(T, n_surf, surf, o, d);
    ctab_finish<NW>(T, n_tri, surf, L, F);
}

#ifndef RT_CTAB_OWN
#define RT_CTAB_OWN 3  // candidates each lane tests on its own lane before the shared exact phase (Cornell
                       // 512^2 x 256: 1 / 3 / 5 -> 3.04 / 2.90 / 2.96 ms with 8x8 bins, profiles/r5t)
#endif
// the table usable for a launch: built with this build's dimensions, for its t_scale
__device__ __forceinline__ bool ctab_usable(const CtabDev& T, float t_scale) {
    return T.masks != nullptr && T.bins == kCtabBins && T.graze_n == kCtabGraze && t_scale >= T.ts_min;
}
// closest_hit_mf's result for a ray whose candidates are given, F (NW mask words): every other
// triangle fails the exact test for the lane's ray, so testing F in index order gives the scan's
// hit.  The lane's first RT_CTAB_OWN candidates on its own lane, the rest shared by the wave
// (mf_exact_wave, per 64-triangle block).  Wave-level like closest_hit_mf (a lane without a ray:
// F = 0).  closest_hit_ctab: F from the table T for a bounce ray leaving surface `surf`.
// RULE 1's shared exact phase folds by minimum (cand_exact_min) instead of per-lane list walks.
#ifndef RT_CAND_DENSE
#define RT_CAND_DENSE 1  // 0: the one-word table route's shared phase by mf_exact_wave's list walks, as every
                         // other route (the A/B of profiles/r15_*)
#endif
#ifndef RT_CAND_OWN_MIN
#define RT_CAND_OWN_MIN 0  // RT_CTAB_OWN of the min-fold phase (complex_light_room 512^2 x 64: 0 / 1 -> 50.9 / 66.8 ms)
#endif

// RULE 1's window (accept t < best, in index order, from best = 999999, tri -1) picks the
// lexicographic minimum of (t, index) over the passing candidates and the start: a 64-bit key,
// |t|'s bits above the index + 1 (0: the start, which wins a tie at its t) and t's sign bit
// (a pass can be -0: ordered as +0, returned as it was)
__device__ __forceinline__ uint64_t min_key(float t, int tri) {
    const uint32_t b = __float_as_uint(t);
    return ((uint64_t)(b & 0x7fffffffu) << 32) | ((uint64_t)(uint32_t)(tri + 1) << 1) | (uint64_t)(b >> 31);
}
__device__ __forceinline__ void min_unkey(uint64_t k, Hit& h) {
    const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
    h.t = __uint_as_float(hi | (lo << 31));
    h.tri = (int)(lo >> 1) - 1;
}
// position of the j-th (from 0) set bit of x (j < popcount(x))
__device__ __forceinline__ int select_bit(uint64_t x, int j) {
    uint32_t w = (uint32_t)x;
    int pos = 0, c = __builtin_popcount(w);
    if (j >= c) {
        j -= c;
        w = (uint32_t)(x >> 32);
        pos = 32;
    }
#pragma unroll
    for (int sh = 16; sh >= 1; sh >>= 1) {
        c = __builtin_popcount(w & ((1u << sh) - 1u));
        if (j >= c) {
            j -= c;
            w >>= sh;
            pos += sh;
        }
    }
    return pos;
}
// The shared exact phase of one 64-triangle block under RULE 1, folded by minimum: the wave's
// (lane, candidate) pairs are numbered lane-major, and lane k of each round of 64 finds pair
// cb + k's lane (binary search over the lanes' first pair numbers) and triangle (the j-th set
// bit of that lane's mask), tests it and folds its t into that lane's key with an LDS atomic
// minimum.  No lane walks its own list: a round costs the same whatever the lanes' counts.
// LDS (wl, after the rays' 6 x 64 floats): first[64] int, mask[64] u64, key[64] u64.
__device__ __forceinline__ void cand_exact_min(const float4* __restrict__ isect, int tri0, uint64_t F, float* wl,
                                               int lane, unsigned long long* key) {
    const int cnt = __builtin_popcountll(F);
    int excl = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const uint64_t bm = __ballot((cnt >> b) & 1);
        excl += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u)) << b;
        total += __builtin_popcountll(bm) << b;
    }
    if (total == 0) return;
    int* first = reinterpret_cast<int*>(wl + 6 * 64);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(wl + 7 * 64);
    first[lane] = excl;
    mask[lane] = F;
    wave_lds_sync();
    const float* ray = wl;
    for (int cb = 0; cb < total; cb += 64) {
        const int k = cb + lane;
        if (k < total) {
            int r = 0;
#pragma unroll
            for (int st = 32; st >= 1; st >>= 1)
                if (first[r + st] <= k) r += st;
            const int i = tri0 + select_bit(mask[r], k - first[r]);
            const f3 ro = make3(ray[0 * 64 + r], ray[1 * 64 + r], ray[2 * 64 + r]);
            const float t = exact_tv<1>(isect, i, ro, ray[3 * 64 + r], ray[4 * 64 + r], ray[5 * 64 + r]);
            if (t < 999999.0f) atomicMin(key + r, (unsigned long long)min_key(t, i));
        }
    }
    wave_lds_sync();
}

// inclusive maximum scan of v >= 0 over the wave's lanes: shifts within the rows of 16, then each
// row's last value broadcast to the rows after it (DPP: no LDS round trip; a lane without a
// source keeps 0)
__device__ __forceinline__ int wave_max_scan(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1, 3
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2, 3
    return v;
}

// The shared exact phase of the one-word table route under RULE 0, at a cost per round of 64
// pairs that does not depend on the lanes' counts.  The wave's (lane, candidate) pairs are
// numbered lane-major as in mf_exact_wave; lane k of a round tests pair cb + k.
//   listing: an owner with candidates writes lane + 1 at byte `excl - cb` of a zeroed row of 64
//     (positions are distinct: owners' excl strictly increase).  The inclusive maximum scan of
//     the row, with the previous round's last value carried in, gives every pair its owner; the
//     owner's mask and first pair number come by ds_bpermute and the triangle is the
//     (k - excl_owner)-th set bit of that mask.  No lane walks its list.
//   fold: one ballot of the passes (t finite: +inf never passes the window); an owner cuts its
//     range [excl, excl + cnt) of the round out of it and fetches t and the triangle of its set
//     bits only, in ascending position = ascending triangle index, under the window
//     t < best + eps.  A failing pair never changed mf_exact_wave's best either, so the hit is
//     the same bit for bit; a range that straddles rounds carries best over in h.
// LDS (wl): the rays' 6 x 64 floats as closest_hit_cand parks them, then the row's 64 bytes.
__device__ __forceinline__ void cand_exact_dense(const float4* __restrict__ isect, uint64_t F, float* wl, int lane,
                                                 Hit& h, ExactProf* xp = nullptr) {
    const int cnt = __builtin_popcountll(F);
    int excl = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const uint64_t bm = __ballot((cnt >> b) & 1);
        excl += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u)) << b;
        total += __builtin_popcountll(bm) << b;
    }
    if (total == 0) return;
    const float* ray = wl;
    uint8_t* row = reinterpret_cast<uint8_t*>(wl + 6 * 64);
    const int f_lo = (int)(uint32_t)F, f_hi = (int)(uint32_t)(F >> 32);
    int carry = 0;  // lane + 1 of the owner of the previous round's last pair
#if RT_PROF
    unsigned my_pass = 0;
#endif
    for (int cb = 0; cb < total; cb += 64) {
        const int lo = excl - cb;  // the lane's pairs in this round: positions [lo, lo + cnt) of [0, 64)
        row[lane] = 0;
        if (cnt != 0 && lo >= 0 && lo < 64) row[lo] = (uint8_t)(lane + 1);
        wave_lds_sync();
        const int own = max(wave_max_scan((int)row[lane]), carry);
        carry = __builtin_amdgcn_readlane(own, 63);
        const int k = cb + lane;
        const bool valid = k < total;
        // (every lane takes part in the permutes: a lane reads its owner's registers)
        const int ra = (valid ? (own - 1) & 63 : lane) << 2;
        const uint32_t o_lo = (uint32_t)__builtin_amdgcn_ds_bpermute(ra, f_lo);
        const uint32_t o_hi = (uint32_t)__builtin_amdgcn_ds_bpermute(ra, f_hi);
        const int o_ex = __builtin_amdgcn_ds_bpermute(ra, excl);
        float t = __builtin_inff();
        int tri = 0;
        if (valid) {
            const int rl = ra >> 2;
            tri = select_bit(((uint64_t)o_hi << 32) | o_lo, k - o_ex);
            const f3 ro = make3(ray[0 * 64 + rl], ray[1 * 64 + rl], ray[2 * 64 + rl]);
            t = exact_tv<0>(isect, tri, ro, ray[3 * 64 + rl], ray[4 * 64 + rl], ray[5 * 64 + rl]);
        }
        const uint64_t pass = __ballot(t < __builtin_inff());
        // the lane's part [ra0, rb0) of the round (shift counts taken mod 64 where it is empty)
        const int ra0 = max(lo, 0), rb0 = min(lo + cnt, 64);
        uint64_t m = ra0 < rb0 ? pass & (~0ull << (ra0 & 63)) & (~0ull >> ((64 - rb0) & 63)) : 0ull;
#if RT_PROF
        if (xp) {
            xp->rounds += 1;
            xp->passes += __builtin_popcountll(pass);
            my_pass += __builtin_popcountll(m);
        }
#endif
        while (__ballot(m != 0ull) != 0ull) {
            const bool mine = m != 0ull;
            const int ja = (mine ? __builtin_ctzll(m) : lane) << 2;
            const float tj = __int_as_float(__builtin_amdgcn_ds_bpermute(ja, __float_as_int(t)));
            const int bj = __builtin_amdgcn_ds_bpermute(ja, tri);
            if (mine && tj < h.t + kEps) {
                h.t = tj;
                h.tri = bj;
            }
            m &= m - 1ull;
#if RT_PROF
            if (xp) xp->fold_iters += 1;
#endif
        }
    }
#if RT_PROF
    if (xp) {
        xp->pairs += total;
        xp->max_pass += __builtin_amdgcn_readlane(wave_max_scan((int)my_pass), 63);
    }
#endif
}

template <int RULE, int NW, int CAP = kMfPairCap>
__device__ __forceinline__ Hit closest_hit_cand(const DeviceScene& s, uint64_t (&F)[NW], f3 o, f3 d, float t_scale,
                                                float* wl, ExactProf* xp = nullptr) {
    const float nDx = -(d.x * t_scale);
    const float nDy = -(d.y * t_scale);
    const float nDz = -(d.z * t_scale);
    const int lane = threadIdx.x & 63;
    // the lane's ray for the shared exact phase (rows 0-5 of wl, as closest_hit_mf parks it)
    wl[0 * 64 + lane] = o.x;
    wl[1 * 64 + lane] = o.y;
    wl[2 * 64 + lane] = o.z;
    wl[3 * 64 + lane] = nDx;
    wl[4 * 64 + lane] = nDy;
    wl[5 * 64 + lane] = nDz;
    Hit h;
    h.t = (RULE == 0) ? FLT_MAX : 999999.0f;
    h.tri = -1;
    constexpr bool kMin = RULE == 1;
    // the lane's first candidates (in index order) on its own lane
#pragma unroll
    for (int k = 0; k < (kMin ? RT_CAND_OWN_MIN : RT_CTAB_OWN); ++k) {
        int wsel = -1;
#pragma unroll
        for (int w = NW - 1; w >= 0; --w)
            if (F[w] != 0ull) wsel = w;
        if (wsel >= 0) {
            uint64_t fw = 0ull;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (w == wsel) fw = F[w];
            const int b = 64 * wsel + __builtin_ctzll(fw);
            const float t = exact_tv<RULE>(s.isect, b, o, nDx, nDy, nDz);
            if ((RULE == 0) ? (t < h.t + kEps) : (t < h.t)) {
                h.t = t;
                h.tri = b;
            }
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (w == wsel) F[w] &= F[w] - 1ull;
        }
    }
    if constexpr (kMin) {
        unsigned long long* key = reinterpret_cast<unsigned long long*>(wl + 9 * 64);
        key[lane] = min_key(h.t, h.tri);
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if (64 * w < s.n_tri) cand_exact_min(s.isect, 64 * w, F[w], wl, lane, key);
        wave_lds_sync();
        min_unkey(key[lane], h);
    } else {
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if (64 * w < s.n_tri) {
                if constexpr (RT_CAND_DENSE && RULE == 0 && NW == 1 && CAP == kCtPairCap)
                    cand_exact_dense(s.isect, F[w], wl, lane, h, xp);
                else
                    mf_exact_wave<RULE, CAP>(s.isect, 64 * w, F[w], o, nDx, nDy, nDz, wl, lane, h, xp);
            }
    }
    return h;
}
template <int RULE, int NW, int CAP = kMfPairCap>
__device__ __forceinline__ Hit closest_hit_ctab(const DeviceScene& s, const CtabDev& T, int surf, f3 o, f3 d,
                                                float t_scale, bool active, float* wl) {
    uint64_t F[NW];
    if (active) {
        ctab_candidates<NW>(T, s.n_tri, s.n_surf, surf, o, d, F);
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) F[k] = 0ull;
    }
    return closest_hit_cand<RULE, NW, CAP>(s, F, o, d, t_scale, wl);
}
// closest_hit_ctab in two halves (ctab_begin / ctab_finish): what the caller runs between them
// covers the latency of the entry's loads.  Same hit as the unsplit cast.
// (an active lane's surface frame loaded by the caller, ctab_frame; an inactive lane loads nothing)
template <int NW>
__device__ __forceinline__ CtabLook<NW> closest_hit_ctab_begin(const CtabDev& T, const CtabFrame& R, f3 o, f3 d,
                                                               bool active) {
    if (!active) return ctab_no_look<NW>();
    return ctab_begin<NW>(T, R, o, d);
}
template <int RULE, int NW, int CAP = kMfPairCap>
__device__ __forceinline__ Hit closest_hit_ctab_finish(const DeviceScene& s, const CtabDev& T, int surf,
                                                       const CtabLook<NW>& L, f3 o, f3 d, float t_scale, bool active,
                                                       float* wl, ExactProf* xp = nullptr) {
    uint64_t F[NW];
    if (active) {
        ctab_finish<NW>(T, s.n_tri, surf, L, F);
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) F[k] = 0ull;
    }
    return closest_hit_cand<RULE, NW, CAP>(s, F, o, d, t_scale, wl, xp);
}

template <int RULE>
__device__ __forceinline__ Hit closest_hit_sel(const DeviceScene& s, int use_filter, f3 o, f3 d,
                                               float t_scale) {
    if (use_filter) return closest_hit_filtered<RULE>(s.filt, s.isect, s.n_tri, o, d, t_scale);
    return closest_hit<RULE>(s.isect, s.n_tri, o, d, t_scale);
}

// ---- Exact BVH path (large scenes; rt_bvh.cpp has the proof obligations) ----
// Rule-1 result: the smallest t below 999999, ties to the smallest index (the scan's
// strict t < best in index order).  Rule 0 (t < best + eps, ties to the later index)
// depends on the order, but only through the triangles with t below tmin + 2 eps: the
// first triangle with t = tmin resets the scan's best to tmin, and after it a triangle
// is accepted only below best + eps.  Those few are kept (index, t), sorted by index
// and folded as the scan folds them; if the fold's best could reach the cut, or more
// than kBvhCand arrive, the ray takes the exact scan.
struct BvhCand {
    float tmin, cut;               // rule 0: smallest t, fl(fl(tmin + eps) + eps)
    float ct[kBvhCand];
    int ci[kBvhCand];
    int nc;
    bool overflow;
    float bt;                      // rule 1: best t, index
    int bi;
};

template <int RULE>
__device__ __forceinline__ void bvh_insert(BvhCand& c, float t, int idx) {
    if (RULE == 1) {
        if (t < c.bt || (t == c.bt && idx < c.bi)) {
            c.bt = t;
            c.bi = idx;
        }
        return;
    }
    if (!(t < c.cut)) return;
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k)
        if (k < c.nc && c.ci[k] == idx) return;  // listed already (BVH leaf and grazing list)
    if (c.nc == kBvhCand) {
        c.overflow = true;
        return;
    }
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k)
        if (k == c.nc) {
            c.ct[k] = t;
            c.ci[k] = idx;
        }
    ++c.nc;
    if (t < c.tmin) {
        c.tmin = t;
        c.cut = (t + kEps) + kEps;
    }
}

// the window of the traversal in ray-parameter units (lambda = t * t_scale): a regular
// pair passing the exact test with t below the cut has lambda <= (cut ts + a) / (1 - b)
template <int RULE>
__device__ __forceinline__ float bvh_lam_hi(const BvhCand& c, const DeviceScene& s, float t_scale) {
    const float cut = (RULE == 0) ? c.cut : c.bt;
    return ((cut * t_scale + s.bvh_sig_a) / (1.0f - s.bvh_sig_b)) * 1.0000002f;
}

// stk: the lane's LDS stack (kBvhMaxDepth entries), STRIDE ints apart.
template <int RULE, int STRIDE = 256>
__device__ Hit closest_hit_bvh(const DeviceScene& s, f3 o, f3 d, float t_scale, int* stk) {
    const float nDx = -(d.x * t_scale), nDy = -(d.y * t_scale), nDz = -(d.z * t_scale);
    const float om = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const float dm = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    // outside the bounds the records were built for (non-finite included): the scan
    if (!(om <= s.origin_bound && dm <= kMfDirBound && t_scale > 0.0f && t_scale <= kFiltMaxTScale))
        return closest_hit<RULE>(s.isect, s.n_tri, o, d, t_scale);
    BvhCand c;
    c.tmin = FLT_MAX;
    c.cut = FLT_MAX;
    c.nc = 0;
    c.overflow = false;
    c.bt = 999999.0f;
    c.bi = -1;
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k) {
        c.ct[k] = 0.0f;
        c.ci[k] = 0;
    }
    // slab test: directions clamped away from 0 by 2^-100 (the node padding covers it)
    auto safe = [](float x) { return (fabsf(x) < 7.8886091e-31f) ? copysignf(7.8886091e-31f, x) : x; };
    const float ix = 1.0f / safe(d.x), iy = 1.0f / safe(d.y), iz = 1.0f / safe(d.z);
    const float lam_lo = -2.0f * s.bvh_sig_a - 1e-6f;
    const float4* __restrict__ nodes = s.bvh_nodes;
    const float4* __restrict__ tris = s.bvh_tris;
    auto slab = [&](int n, float lam_hi, float* entry) -> bool {
        const float4 lo = nodes[2 * n], hi = nodes[2 * n + 1];
        const float x0 = (lo.x - o.x) * ix, x1 = (hi.x - o.x) * ix;
        const float y0 = (lo.y - o.y) * iy, y1 = (hi.y - o.y) * iy;
        const float z0 = (lo.z - o.z) * iz, z1 = (hi.z - o.z) * iz;
        const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), lam_lo));
        const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), lam_hi));
        *entry = tn;
        return tn <= tf;
    };
    int sp = 0;
    int node = 0;
    for (;;) {
        const float4 hi = nodes[2 * node + 1];
        const int cnt = __float_as_int(hi.w);
        const int link = __float_as_int(nodes[2 * node].w);
        if (cnt > 0) {
            for (int j = link; j < link + cnt; ++j) {
                const float t = exact_tv<RULE>(tris, j, o, nDx, nDy, nDz);
                if (t <= FLT_MAX) bvh_insert<RULE>(c, t, __float_as_int(tris[j * kIsectF4 + 1].w));
            }
        } else {
            const float lh = bvh_lam_hi<RULE>(c, s, t_scale);
            float e0, e1;
            const bool h0 = slab(link, lh, &e0);
            const bool h1 = slab(link + 1, lh, &e1);
            if (h0 && h1) {
                const bool first0 = e0 <= e1;
                stk[(sp++) * STRIDE] = first0 ? link + 1 : link;
                node = first0 ? link : link + 1;
                continue;
            }
            if (h0 || h1) {
                node = h0 ? link : link + 1;
                continue;
            }
        }
        if (sp == 0) break;
        node = stk[(--sp) * STRIDE];
    }
    // grazing pairs (rt_bvh.cpp): the list of the ray's cube-map cell of directions, each
    // triangle tested for |d.N~| <= alpha B + beta and, with a window lambda, for its plane
    // within PA B + PB + (alpha B + beta) lambda of the origin (N units)
    {
        const float cut = (RULE == 0) ? c.cut : c.bt;
        const float lam_cut = cut * t_scale * 1.0000002f;
        const bool bounded = lam_cut <= 3.0e38f;
        const float B = om * 1.000001f;
        // the cube-map cell of d (the host lists hold for any direction of the cell, plus
        // the rounding of this choice)
        const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
        int f;
        float u, v, m;
        if (ax >= ay && ax >= az) {
            f = d.x >= 0.0f ? 0 : 1; m = ax; u = d.y; v = d.z;
        } else if (ay >= az) {
            f = d.y >= 0.0f ? 2 : 3; m = ay; u = d.z; v = d.x;
        } else {
            f = d.z >= 0.0f ? 4 : 5; m = az; u = d.x; v = d.y;
        }
        const float G = (float)kBvhDirGrid;
        const int iu = min(kBvhDirGrid - 1, max(0, (int)((u / m + 1.0f) * 0.5f * G)));
        const int iv = min(kBvhDirGrid - 1, max(0, (int)((v / m + 1.0f) * 0.5f * G)));
        const int cell = (f * kBvhDirGrid + iu) * kBvhDirGrid + iv;
        const bool cam = !(B <= s.bvh_B_lists);
        const int32_t* st = s.bvh_dstart + (cam ? 6 * kBvhDirGrid * kBvhDirGrid + 1 : 0);
        const int32_t* __restrict__ dl = cam ? s.bvh_dlist_cam : s.bvh_dlist;
        const float4* __restrict__ gr = s.bvh_grec;
        const int j0 = st[cell], j1 = st[cell + 1];
        for (int j = j0; j < j1; ++j) {
            const int i = dl[j];
            const float4 g = gr[2 * i];
            const float a = fmaf(d.z, g.z, fmaf(d.y, g.y, d.x * g.x));
            const float4 q = gr[2 * i + 1];
            const float thr = fmaf(g.w, B, q.x) * 1.000001f;
            bool cand = fabsf(a) <= thr;
            if (cand && bounded) {
                const float w = fmaf(o.z, g.z, fmaf(o.y, g.y, o.x * g.x)) - q.y;
                cand = fabsf(w) <= fmaf(thr, lam_cut, fmaf(q.z, B, q.w)) * 1.00001f;
            }
            if (cand) {
                const float t = exact_tv<RULE>(s.isect, i, o, nDx, nDy, nDz);
                if (t <= FLT_MAX) bvh_insert<RULE>(c, t, i);
            }
        }
    }
    Hit h;
    if (RULE == 1) {
        h.t = c.bt;
        h.tri = c.bi;
        return h;
    }
    if (c.overflow) return closest_hit<RULE>(s.isect, s.n_tri, o, d, t_scale);
    // the listed triangles below the final cut, in index order (insertion sort)
    float ft[kBvhCand];
    int fi[kBvhCand];
    int m = 0;
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k) {
        ft[k] = 0.0f;
        fi[k] = 0x7fffffff;
    }
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k) {
        if (k < c.nc && c.ct[k] < c.cut) {
            float t = c.ct[k];
            int i = c.ci[k];
#pragma unroll
            for (int j = 0; j < kBvhCand; ++j) {  // keep fi ascending: swap the larger one on
                if (j <= m && i < fi[j]) {
                    const float tt = ft[j];
                    const int ii = fi[j];
                    ft[j] = t;
                    fi[j] = i;
                    t = tt;
                    i = ii;
                }
            }
            ++m;
        }
    }
    h.t = FLT_MAX;
    h.tri = -1;
    bool seen = false;
    float bmax = 0.0f;
#pragma unroll
    for (int k = 0; k < kBvhCand; ++k) {
        if (k < m) {
            if (ft[k] < h.t + kEps) {
                h.t = ft[k];
                h.tri = fi[k];
            }
            if (ft[k] == c.tmin) seen = true;
            if (seen) bmax = fmaxf(bmax, h.t);
        }
    }
    if (m > 0 && !(bmax + kEps <= c.cut)) return closest_hit<RULE>(s.isect, s.n_tri, o, d, t_scale);
    return h;
}

// two uniforms of event `ev` of sample `smp` of pixel `pix`
__device__ __forceinline__ void draw2(uint32_t pix, uint32_t smp, uint32_t ev, uint32_t k0,
                                      uint32_t k1, float* a, float* b) {
#ifdef RT_TIMING_CHEAP_RNG
    // timing-only build (wrong images): what the Philox rounds cost
    const uint32_t h = (pix * 0x9E3779B9u) ^ (smp * 0x85EBCA6Bu) ^ (ev * 0xC2B2AE35u) ^ k0;
    *a = u01(h * 0x27D4EB2Fu);
    *b = u01((h ^ (h >> 15)) * 0x165667B1u);
    return;
#endif
    uint32_t o[4];
    philox4x32_10(pix, smp, ev, 0u, k0, k1, o);
    *a = u01(o[0]);
    *b = u01(o[1]);
}

// draw2 with the pixel's Philox words in hand (philox_pix of the pixel and the key: the same for
// every sample and event of the pixel, and wave-uniform when the wave holds one pixel); the same
// two uniforms as draw2(pix, smp, ev, k0, k1)
__device__ __forceinline__ void draw2_px(const PhiloxPix& px, uint32_t smp, uint32_t ev, uint32_t k0, uint32_t k1,
                                         float* a, float* b) {
#ifdef RT_TIMING_CHEAP_RNG
    // timing-only build (wrong images), as draw2's: px.lo0 stands for the pixel
    const uint32_t h = px.lo0 ^ (smp * 0x85EBCA6Bu) ^ (ev * 0xC2B2AE35u) ^ k0;
    *a = u01(h * 0x27D4EB2Fu);
    *b = u01((h ^ (h >> 15)) * 0x165667B1u);
    return;
#endif
    uint32_t o[4];
    philox_finish(px, philox_ev(ev), smp, k0, k1, o);
    *a = u01(o[0]);
    *b = u01(o[1]);
}

// Camera ray through (px+r1, py+r2): default_path_tracing.cpp:25-34, Ray::Ray
// (ray.cpp:7-11), rotate_ray (ray.cpp:47-52; GPU/rays/ray.cu:161-172), with
// glm's mat4*vec4 order (m0*v0 + m1*v1) + (m2*v2 + m3*v3).
// UNIT: the normalize without its range guards (normalize_unit, rt_math.hpp; ps_body alone
// selects it).  dot(dir, dir) >= height^2 >= 1, and with |x|, |y| < 2^24 it is below 2^50.
template <int PRESET, bool UNIT = false>
__device__ __forceinline__ void camera_ray(const RenderLaunch& a, int px, int py, float r1, float r2,
                                           f3* d_out) {
    const float x = (float)px + r1;
    const float y = (float)py + r2;
    f3 dir = make3(x - (float)a.width / 2.0f, y - (float)a.height / 2.0f, (float)a.height);
    dir = UNIT ? normalize_unit(dir) : normalize(dir);
    const float w = 1.0f;
    f3 r;
    r.x = (a.cos_y * dir.x + 0.0f * dir.y) + (-a.sin_y * dir.z + 0.0f * w);
    r.y = (0.0f * dir.x + 1.0f * dir.y) + (0.0f * dir.z + 0.0f * w);
    r.z = (a.sin_y * dir.x + 0.0f * dir.y) + (a.cos_y * dir.z + 0.0f * w);
    if (PRESET == 1) {
        const float rw = (0.0f * dir.x + 0.0f * dir.y) + (0.0f * dir.z + 1.0f * w);
        f3 q;
        q.x = (1.0f * r.x + 0.0f * r.y) + (0.0f * r.z + 0.0f * rw);
        q.y = (0.0f * r.x + a.cos_x * r.y) + (a.sin_x * r.z + 0.0f * rw);
        q.z = (0.0f * r.x + -a.sin_x * r.y) + (a.cos_x * r.z + 0.0f * rw);
        r = q;
    }
    *d_out = r;
}

// the bits of 64-triangle group g that are triangles of an n-triangle scene
__device__ __forceinline__ uint64_t tri_mask(int n, int g) {
    const int k = n - 64 * g;
    return k >= 64 ? ~0ull : (k <= 0 ? 0ull : ((1ull << k) - 1ull));
}

// The candidate triangles of the wave's camera rays: bit i of cm[i / 64] = triangle i may
// be the hit of a camera ray through one of the wave's pixels (the pixel rectangle's cull,
// rect_cull in rt_cull.hpp; wave-uniform).  k_render_ps phase P, k_render<MF> camera rays.
template <int RULE>
__device__ __forceinline__ void wave_candidates(const RenderLaunch& a, bool valid, int px, int py, int lane,
                                                uint64_t* cm) {
    int x0 = valid ? px : 0x7fffffff, x1 = valid ? px : -1;
    int y0 = valid ? py : 0x7fffffff, y1 = valid ? py : -1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64));
        y0 = min(y0, __shfl_xor(y0, off, 64));
        y1 = max(y1, __shfl_xor(y1, off, 64));
    }
    const CamRect c = make_cam_rect(a.cam_x, a.cam_y, a.cam_z, a.cos_y, a.sin_y, a.width, a.height, a.t_scale,
                                    __builtin_amdgcn_readfirstlane(x0), __builtin_amdgcn_readfirstlane(x1),
                                    __builtin_amdgcn_readfirstlane(y0), __builtin_amdgcn_readfirstlane(y1));
    const int n_tri = a.scene.n_tri;
#pragma unroll
    for (int g = 0; g < kRenderCullWords; ++g) {
        if (g * 64 >= n_tri) {  // (wave-uniform) no triangle in this word
            cm[g] = 0ull;
            continue;
        }
        const int i = g * 64 + lane;
        const bool in_range = i < n_tri;
#ifdef RT_TIMING_NO_CULL
        const bool keep = in_range;
#else
        // every lane tests a real record (triangle 0 past the end), the range masks after
        const bool cull = rect_cull<RULE>(a.scene.filt + (size_t)(in_range ? i : 0) * kFiltF4, c);
        const bool keep = in_range && !cull;
#endif
        cm[g] = __ballot(keep) & tri_mask(n_tri, g);
    }
}

// closest_hit's answer from the wave's camera-ray candidates (wave_candidates: the triangles
// the cull of the wave's pixel rectangle keeps; cm is wave-uniform): the exact test on the
// kept triangles in index order, their records by scalar loads.  No wave-level operation:
// lanes without a ray skip it.  The view kernels' camera cast (k_sarsa_view, k_sarsa_irr,
// k_glyph_view).
template <int RULE>
__device__ __forceinline__ Hit view_hit_culled(const DeviceScene& sc, const uint64_t* cm, f3 o, f3 d, float t_scale) {
    cfloat4* __restrict__ tri = as_const(sc.isect);
    const float nDx = -(d.x * t_scale);
    const float nDy = -(d.y * t_scale);
    const float nDz = -(d.z * t_scale);
    Hit h;
    h.t = (RULE == 0) ? FLT_MAX : 999999.0f;
    h.tri = -1;
#pragma unroll
    for (int g = 0; g < kRenderCullWords; ++g) {
        uint64_t w = cm[g];
        while (w != 0ull) {
            const int i = 64 * g + __builtin_ctzll(w);
            w &= w - 1ull;
            exact_one_c<RULE>(tri, i, o, nDx, nDy, nDz, h);
        }
    }
    return h;
}

// wave_candidates from the launch's precomputed forms (k_cull_forms; rt_cull.hpp's two halves),
// for k_render_ps and k_cull_ps: a wave with at least one valid pixel whose lane 0 holds pixel
// q (index in the 16x16 block, wave-uniform) and whose lanes hold 64 >> split_log2 consecutive
// pixels from there.  Those are whole rows of the block or an aligned piece of one row, and the
// valid ones are its intersection with the clip, so the rectangle wave_candidates reduces out
// of the lanes is this closed form; the masks are wave_candidates' bit for bit.
template <int RULE>
__device__ __forceinline__ void wave_candidates_forms(const RenderLaunch& a, const CullLaunch& cf,
                                                      const BlockDesc& blk, int q, int lane, uint64_t* cm) {
    const int q0 = __builtin_amdgcn_readfirstlane(q);
    const int q1 = q0 + (64 >> a.split_log2) - 1;
    const int x0 = blk.px0 + (q0 & 15), y0 = blk.py0 + (q0 >> 4);
    const int x1 = min(blk.px0 + (q1 & 15), a.clip_x1 - 1), y1 = min(blk.py0 + (q1 >> 4), a.clip_y1 - 1);
    const CamRect c = cam_rect_of(cf.cam, x0, x1, y0, y1);
    const int n_tri = a.scene.n_tri;
    cfloat4* __restrict__ forms = as_const(cf.forms);
#pragma unroll
    for (int g = 0; g < kRenderCullWords; ++g) {
        if (g * 64 >= n_tri) {  // (wave-uniform) no triangle in this word
            cm[g] = 0ull;
            continue;
        }
        const int i = g * 64 + lane;
        const bool in_range = i < n_tri;
        // (rows past the scene's triangles are zero-filled: every lane reads a record)
        float4 r[kCullFormRows];
#pragma unroll
        for (int k = 0; k < kCullFormRows; ++k) r[k] = ldc(forms + k * kCullFormStride + i);
        const bool keep = in_range && !rect_cull_forms<RULE>(cull_forms_of_rows(r), c);
        cm[g] = __ballot(keep) & tri_mask(n_tri, g);
    }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace rt
