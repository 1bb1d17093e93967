/*
 * rt_oracle.c — CPU restatement of the reference's hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  This file is the parity checker for the
 * MI355X path tracer in reinforcement-light-rays-pathtracer_amd/.  Only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * it; the product never links, includes or calls anything under oracle/.
 *
 * It is a clean-room restatement (plain C, written from reading the
 * reference as text) of:
 *   - the Cornell scene builders
 *       CPU preset: Old_CPU_Rendering_Engine/Source/scenes/cornell_box_scene.cpp:3-205
 *       GPU preset: GPU_Rendering_Engine/Source/scenes/cornell_box_scene.cu:4-... (emission 14*0.9, :81)
 *   - triangle normal  normalize(cross(e2,e1))   CPU/objects/triangle.cpp:73-82
 *   - ray construction / normalisation           CPU/rays/ray.cpp:7-11
 *   - camera ray through a pixel + yaw rotation  CPU/path_tracing/default_path_tracing.cpp:25-34,
 *                                                CPU/rays/ray.cpp:47-52, GPU/rays/ray.cu:143-172
 *   - closest hit, surfaces then light planes    CPU/rays/ray.cpp:14-28, CPU/lights/area_light_plane.cpp:25-33
 *   - the hit predicate:
 *       rule 0 = the CPU engine's prebuilt object
 *         Old_CPU_Rendering_Engine/CMakeFiles/Monte_Carlo_Raytracer.dir/Source/objects/triangle.cpp.o
 *         (Triangle::intersects @0x460, disassembled):
 *         inv = 1/detA; t,u,v = det_(t,u,v) * inv; accept iff t>=0,u>=0,v>=0,u+v<=1,
 *         t < dist+1e-5, t > 1e-5
 *       rule 1 = GPU/rays/ray.cu:38-141: t,u,v = det_(t,u,v) / detA; accept iff
 *         t>=0,u>=0,v>=0,u+v<=1, t < dist (dist starts at 999999)
 *     3x3 determinants in GLM's operation order
 *     (glm/glm/detail/func_matrix.inl:210-220; confirmed in the .o's
 *     compute_determinant<3,3,float> body)
 *   - uniform hemisphere sampling + tangent frame CPU/utils/hemisphere_helpers.cpp:4-39,60-83
 *   - Lambertian estimator, recursive (CPU)      CPU/path_tracing/default_path_tracing.cpp:46-101
 *   - iterative throughput (GPU preset)          GPU/path_tracing/default_path_tracing.cu:36-88
 *   - SPP mean                                   CPU/path_tracing/default_path_tracing.cpp:20-41
 *   - ARGB pack                                  CPU/sdl/sdl_screen.cpp:100-112
 *
 * Random numbers: the reference draws from rand() (CPU) / cuRAND XORWOW
 * (GPU); neither stream is reproducible on another machine or under
 * OpenMP.  Both this oracle and the HIP kernels draw from a counter-based
 * Philox4x32-10 keyed on (seed, global pixel, sample, event) — the spec in
 * DESIGN.md §3.  sin/cos of 2*pi*r use the spec's own quarter-turn
 * polynomial so host and device agree bit for bit.  orc_render_sequential
 * restates the reference's own stream (glibc rand(), one thread, its loop
 * order and libm trig) as the statistical bridge of SURVEY.md §8(c) gate 3.
 *
 * PARITY PINNING: the reference ships no tests and no golden outputs for
 * this path; its code could not be compiled or run here (SURVEY.md §8(c),
 * recorded denial).  The oracle is pinned by (1) the hit-predicate constants
 * and operation order read from the prebuilt triangle.cpp.o, (2) the
 * Random123 Philox known-answer vectors, (3) analytic intersection KATs,
 * (4) the archway loader golden Radiance_Map_Data/vertices.txt, and
 * (5) statistical agreement with the reference's committed Cornell renders
 * (the PNGs under Images/cornell/).  See tests/.
 *
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -fopenmp -shared -fPIC
 * (no FMA contraction: every float op is rounded exactly as written).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <float.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ORC_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------ */
/* Philox4x32-10 (Salmon et al., SC'11; Random123 reference constants) */
/* ------------------------------------------------------------------ */
static void philox_round(uint32_t c[4], const uint32_t k[2]) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c[1] ^ k[0];
    uint32_t n2 = hi0 ^ c[3] ^ k[1];
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

ORC_API void orc_philox4x32_10(const uint32_t ctr_in[4], const uint32_t key_in[2], uint32_t out[4]) {
    uint32_t c[4] = {ctr_in[0], ctr_in[1], ctr_in[2], ctr_in[3]};
    uint32_t k[2] = {key_in[0], key_in[1]};
    for (int r = 0; r < 10; r++) {
        philox_round(c, k);
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    memcpy(out, c, sizeof(c));
}

/* uniform float in [0,1): top 24 bits */
static float u01(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }
/* (0, 1], curand_uniform's range: the SARSA sector draws (r = 0 would pick sector 0 of a
 * zero-mass CDF prefix, which the reference's curand cannot) */
static float u01_oc(uint32_t x) { return (float)((x >> 8) + 1u) * 0x1p-24f; }
/* the two 16-bit uniforms of one word (the DQN sampler's cell jitters, rt_math.hpp u16lo/hi) */
static float u16lo(uint32_t x) { return (float)(x & 0xffffu) * 0x1p-16f; }
static float u16hi(uint32_t x) { return (float)(x >> 16) * 0x1p-16f; }

/* two uniforms for (pixel, sample, event) */
static void draw2(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t event, float *a, float *b) {
    uint32_t ctr[4] = {pixel, sample, event, 0u};
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t o[4];
    orc_philox4x32_10(ctr, key, o);
    *a = u01(o[0]);
    *b = u01(o[1]);
}

/* ------------------------------------------------------------------ */
/* sin/cos of a turn fraction (spec)                     */
/* ------------------------------------------------------------------ */
/* Taylor coefficients of sin(pi/2 f) and cos(pi/2 f) on f in [-1/2,1/2],
 * rounded to float.  Horner, no contraction. */
static const float S1 = 1.57079632679489662f;
static const float S3 = -0.645964097506246254f;
static const float S5 = 0.0796926262461670451f;
static const float S7 = -0.00468175413531868810f;
static const float S9 = 0.000160441184757112456f;
static const float C2 = -1.23370055013616983f;
static const float C4 = 0.253669507901048014f;
static const float C6 = -0.0208634807633529609f;
static const float C8 = 0.000919260274839426046f;
static const float C10 = -0.0000252020423730606054f;

ORC_API void orc_sincos_turn(float r, float *s_out, float *c_out) {
    float x = r * 4.0f;                 /* exact */
    float q = rintf(x);                 /* nearest quadrant (ties-to-even) */
    float f = x - q;                    /* exact, in [-0.5, 0.5] */
    int qi = ((int)q) & 3;
    float f2 = f * f;
    float sp = S9;
    sp = sp * f2; sp = sp + S7;
    sp = sp * f2; sp = sp + S5;
    sp = sp * f2; sp = sp + S3;
    sp = sp * f2; sp = sp + S1;
    sp = sp * f;
    float cp = C10;
    cp = cp * f2; cp = cp + C8;
    cp = cp * f2; cp = cp + C6;
    cp = cp * f2; cp = cp + C4;
    cp = cp * f2; cp = cp + C2;
    cp = cp * f2; cp = cp + 1.0f;
    float s, c;
    switch (qi) {
        case 0: s = sp; c = cp; break;
        case 1: s = cp; c = -sp; break;
        case 2: s = -sp; c = -cp; break;
        default: s = -cp; c = sp; break;
    }
    *s_out = s; *c_out = c;
}

/* ------------------------------------------------------------------ */
/* GLM-order vector helpers                                            */
/* ------------------------------------------------------------------ */
typedef struct { float x, y, z; } v3;

static v3 mk(float x, float y, float z) { v3 r = {x, y, z}; return r; }
/* glm compute_dot<vec3>: tmp = a*b; (tmp.x + tmp.y) + tmp.z */
static float dot3(v3 a, v3 b) { float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z; return (tx + ty) + tz; }
/* glm normalize: v * inversesqrt(dot(v,v)), inversesqrt = 1/sqrt */
static v3 normalize3(v3 v) {
    float inv = 1.0f / sqrtf(dot3(v, v));
    return mk(v.x * inv, v.y * inv, v.z * inv);
}
/* glm compute_cross */
static v3 cross3(v3 x, v3 y) {
    return mk(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}

/* glm compute_determinant<3,3>: columns c0,c1,c2 (m[i][j] = column i, row j) */
static float det3(v3 c0, v3 c1, v3 c2) {
    float a = c0.x * (c1.y * c2.z - c2.y * c1.z);
    float b = c1.x * (c0.y * c2.z - c2.y * c0.z);
    float c = c2.x * (c0.y * c1.z - c1.y * c0.z);
    return (a - b) + c;
}

/* ------------------------------------------------------------------ */
/* scene                                                               */
/* ------------------------------------------------------------------ */
typedef struct {
    int n_surf, n_light;
    const float *tri;      /* (n_surf+n_light) x 9: v0,v1,v2 (surfaces first) */
    const float *albedo;   /* n_surf x 3 */
    const float *emission; /* n_light x 3 */
    const int32_t *light_group; /* n_light: plane index (CPU light hit index) */
    float *normal;         /* (n_surf+n_light) x 3, computed */
} orc_scene;

static v3 vtx(const float *tri, int i, int k) {
    const float *p = tri + (size_t)i * 9 + k * 3;
    return mk(p[0], p[1], p[2]);
}

/* CPU/objects/triangle.cpp:73-82 */
ORC_API void orc_triangle_normals(const float *tri, int n, float *normal_out) {
    for (int i = 0; i < n; i++) {
        v3 v0 = vtx(tri, i, 0), v1 = vtx(tri, i, 1), v2 = vtx(tri, i, 2);
        v3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z);
        v3 e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
        v3 n3 = normalize3(cross3(e2, e1));
        normal_out[i * 3 + 0] = n3.x; normal_out[i * 3 + 1] = n3.y; normal_out[i * 3 + 2] = n3.z;
    }
}

/* ------------------------------------------------------------------ */
/* Cornell box builders                                                */
/* ------------------------------------------------------------------ */
typedef struct { float x, y, z; } p3;

static void put_tri(float *dst, p3 a, p3 b, p3 c) {
    dst[0] = a.x; dst[1] = a.y; dst[2] = a.z;
    dst[3] = b.x; dst[4] = b.y; dst[5] = b.z;
    dst[6] = c.x; dst[7] = c.y; dst[8] = c.z;
}

/* CPU/scenes/cornell_box_scene.cpp:161-199: v*(2/l) - 1, negate x and y. */
static p3 cornell_xform(p3 v, float l) {
    float s = 2.0f / l;
    p3 r;
    r.x = v.x * s; r.y = v.y * s; r.z = v.z * s;
    r.x = r.x - 1.0f; r.y = r.y - 1.0f; r.z = r.z - 1.0f;
    r.x = r.x * -1.0f; r.y = r.y * -1.0f;
    return r;
}

/*
 * variant 0 = CPU engine (one light plane K,I,J,L fanned into (K,I,J),(K,J,L),
 *             emission 1*(1,1,0.9), light hit index = plane 0)
 * variant 1 = GPU engine (two AreaLights (K,I,J),(K,J,L), emission 14*(0.9,0.9,0.9))
 * Surfaces, in reference order: floor 2, left 2, right 2, ceiling 8, back 2,
 * short block 10, tall block 10 = 36.
 * Returns n_surf*9 + ... into caller arrays sized for 36 surfaces, 2 lights.
 */
ORC_API int orc_cornell(int variant, float *tri /*38x9*/, float *albedo /*36x3*/,
                        float *emission /*2x3*/, int32_t *light_group /*2*/,
                        int *n_surf, int *n_light) {
    const float l = 555.0f;
    p3 A = {l, 0, 0}, B = {0, 0, 0}, C = {l, 0, l}, D = {0, 0, l};
    p3 E = {l, l, 0}, F = {0, l, 0}, G = {l, l, l}, H = {0, l, l};
    p3 I = {l / 3.0f, l, (2.0f * l) / 3.0f}, J = {(2.0f * l) / 3.0f, l, (2.0f * l) / 3.0f};
    p3 K = {l / 3.0f, l, l / 3.0f}, L = {(2.0f * l) / 3.0f, l, l / 3.0f};
    const float blue[3] = {0.15f, 0.15f, 0.75f}, white[3] = {0.75f, 0.75f, 0.75f};
    const float red[3] = {0.75f, 0.15f, 0.15f}, green[3] = {0.15f, 0.75f, 0.15f};
    const float yellow[3] = {0.75f, 0.75f, 0.15f}, cyan[3] = {0.15f, 0.75f, 0.75f};
    p3 raw[36][3];
    const float *mat[36];
    int k = 0;
#define ADD(a, b, c, m) do { raw[k][0] = a; raw[k][1] = b; raw[k][2] = c; mat[k] = m; k++; } while (0)
    ADD(C, B, A, green); ADD(C, D, B, green);
    ADD(A, E, C, white); ADD(C, E, G, white);
    ADD(F, B, D, white); ADD(H, F, D, white);
    ADD(F, H, I, cyan); ADD(F, I, K, cyan); ADD(F, K, E, cyan); ADD(K, L, E, cyan);
    ADD(L, G, E, cyan); ADD(L, J, G, cyan); ADD(I, G, J, cyan); ADD(H, G, I, cyan);
    ADD(G, D, C, yellow); ADD(G, H, D, yellow);
    {
        p3 a = {240, 0, 234}, b = {80, 0, 185}, c = {190, 0, 392}, d = {32, 0, 345};
        p3 e = {240, 165, 234}, f = {80, 165, 185}, g = {190, 165, 392}, h = {32, 165, 345};
        ADD(e, b, a, blue); ADD(e, f, b, blue); ADD(f, d, b, blue); ADD(f, h, d, blue);
        ADD(h, c, d, blue); ADD(h, g, c, blue); ADD(g, e, c, blue); ADD(e, a, c, blue);
        ADD(g, f, e, blue); ADD(g, h, f, blue);
    }
    {
        p3 a = {443, 0, 247}, b = {285, 0, 296}, c = {492, 0, 406}, d = {334, 0, 456};
        p3 e = {443, 330, 247}, f = {285, 330, 296}, g = {492, 330, 406}, h = {334, 330, 456};
        ADD(e, b, a, red); ADD(e, f, b, red); ADD(f, d, b, red); ADD(f, h, d, red);
        ADD(h, c, d, red); ADD(h, g, c, red); ADD(g, e, c, red); ADD(e, a, c, red);
        ADD(g, f, e, red); ADD(g, h, f, red);
    }
#undef ADD
    for (int i = 0; i < 36; i++) {
        put_tri(tri + i * 9, cornell_xform(raw[i][0], l), cornell_xform(raw[i][1], l), cornell_xform(raw[i][2], l));
        albedo[i * 3 + 0] = mat[i][0]; albedo[i * 3 + 1] = mat[i][1]; albedo[i * 3 + 2] = mat[i][2];
    }
    p3 k2 = cornell_xform(K, l), i2 = cornell_xform(I, l), j2 = cornell_xform(J, l), l2 = cornell_xform(L, l);
    put_tri(tri + 36 * 9, k2, i2, j2);
    put_tri(tri + 37 * 9, k2, j2, l2);
    if (variant == 0) {
        /* vec3 diffuse_p = 1.f * vec3(1, 1, 0.9) */
        for (int j = 0; j < 2; j++) {
            emission[j * 3 + 0] = 1.0f * 1.0f; emission[j * 3 + 1] = 1.0f * 1.0f; emission[j * 3 + 2] = 1.0f * 0.9f;
            light_group[j] = 0;
        }
    } else {
        /* vec3 diffuse_p = 14.f * vec3(0.9, 0.9, 0.9) */
        for (int j = 0; j < 2; j++) {
            emission[j * 3 + 0] = 14.0f * 0.9f; emission[j * 3 + 1] = 14.0f * 0.9f; emission[j * 3 + 2] = 14.0f * 0.9f;
            light_group[j] = j;
        }
    }
    *n_surf = 36; *n_light = 2;
    return 0;
}

/* ------------------------------------------------------------------ */
/* intersection                                                        */
/* ------------------------------------------------------------------ */
typedef struct {
    float t;       /* distance in t_scale units */
    int tri;       /* unified triangle index, -1 none */
} hit_t;

/* The test of triangle i without the closest-hit window: 1 and *t_out if it passes the rule's
 * detA, t, u, v conditions (rule 0: through inv = 1 / detA, and t > 1e-5; rule 1: divided
 * directly), else 0.  nD = -(d * t_scale). */
static inline int tri_pass_t(const float *tri, int i, v3 o, v3 nD, int hit_rule, float *t_out) {
    v3 v0 = vtx(tri, i, 0), v1 = vtx(tri, i, 1), v2 = vtx(tri, i, 2);
    v3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z);
    v3 e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
    v3 b = mk(o.x - v0.x, o.y - v0.y, o.z - v0.z);
    float detA = det3(nD, e1, e2);
    if (!(detA != 0.0f)) return 0;
    float t, u, v;
    if (hit_rule == 0) {
        float inv = 1.0f / detA;
        t = det3(b, e1, e2) * inv;
        u = det3(nD, b, e2) * inv;
        v = det3(nD, e1, b) * inv;
        if (!(t >= 0.0f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f && t > 1e-5f)) return 0;
    } else {
        t = det3(b, e1, e2) / detA;
        u = det3(nD, b, e2) / detA;
        v = det3(nD, e1, b) / detA;
        if (!(t >= 0.0f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f)) return 0;
    }
    *t_out = t;
    return 1;
}

/* mask (NULL: every triangle): only the triangles whose bit is set are tested, in index order */
static hit_t closest_hit_masked(const orc_scene *sc, v3 o, v3 d, float t_scale, int hit_rule,
                                const uint64_t *mask) {
    hit_t h;
    h.tri = -1;
    h.t = (hit_rule == 0) ? FLT_MAX : 999999.0f;
    v3 D = mk(d.x * t_scale, d.y * t_scale, d.z * t_scale);
    v3 nD = mk(-D.x, -D.y, -D.z);
    int n = sc->n_surf + sc->n_light;
    for (int i = 0; i < n; i++) {
        if (mask && !((mask[i / 64] >> (i % 64)) & 1u)) continue;
        float t;
        if (!tri_pass_t(sc->tri, i, o, nD, hit_rule, &t)) continue;
        if (hit_rule == 0 ? (t < h.t + 1e-5f) : (t < h.t)) {
            h.t = t; h.tri = i;
        }
    }
    return h;
}

static hit_t closest_hit(const orc_scene *sc, v3 o, v3 d, float t_scale, int hit_rule) {
    return closest_hit_masked(sc, o, d, t_scale, hit_rule, NULL);
}

static int32_t pack_hit(const orc_scene *sc, int tri, int hit_rule) {
    if (tri < 0) return -1;
    if (tri < sc->n_surf) return (int32_t)((2u << 30) | (uint32_t)tri);
    int j = tri - sc->n_surf;
    int idx = (hit_rule == 0) ? sc->light_group[j] : j;
    return (int32_t)((1u << 30) | (uint32_t)idx);
}

static void scene_init(orc_scene *sc, const float *tri, const float *albedo, int n_surf,
                       const float *emission, const int32_t *light_group, int n_light) {
    sc->n_surf = n_surf; sc->n_light = n_light;
    sc->tri = tri; sc->albedo = albedo; sc->emission = emission; sc->light_group = light_group;
    sc->normal = (float *)malloc(sizeof(float) * 3 * (size_t)(n_surf + n_light + 1));
    orc_triangle_normals(tri, n_surf + n_light, sc->normal);
}

/* Ray-cast a batch: the standalone north-star kernel's contract.
 * dir is normalised by the caller (as Ray::Ray does); t_scale = SCREEN_HEIGHT. */
ORC_API void orc_intersect(const float *tri, int n_surf, int n_light, const int32_t *light_group,
                           const float *orig, const float *dir, int n, float t_scale, int hit_rule,
                           float *out_t, int32_t *out_hit) {
    orc_scene sc;
    scene_init(&sc, tri, NULL, n_surf, NULL, light_group, n_light);
    #pragma omp parallel for schedule(static)
    for (int r = 0; r < n; r++) {
        v3 o = mk(orig[r * 3], orig[r * 3 + 1], orig[r * 3 + 2]);
        v3 d = mk(dir[r * 3], dir[r * 3 + 1], dir[r * 3 + 2]);
        hit_t h = closest_hit(&sc, o, d, t_scale, hit_rule);
        out_t[r] = h.tri >= 0 ? h.t : INFINITY;
        out_hit[r] = pack_hit(&sc, h.tri, hit_rule);
    }
    free(sc.normal);
}

/* orc_intersect restricted to each ray's candidates: bit i % 64 of masks[r * words + i / 64]
 * (words = ceil((n_surf + n_light) / 64)) = triangle i is tested for ray r.  The triangles
 * of the mask in index order through the rule's own window -- rule 0's t < best + 1e-5, which
 * depends on that order, rule 1's t < best from 999999 -- so the expected (t, hit) of the
 * kernels' candidate route for any mask, one that omits the scan's hit included. */
ORC_API void orc_intersect_masked(const float *tri, int n_surf, int n_light, const int32_t *light_group,
                                  const float *orig, const float *dir, const uint64_t *masks, int n,
                                  float t_scale, int hit_rule, float *out_t, int32_t *out_hit) {
    orc_scene sc;
    scene_init(&sc, tri, NULL, n_surf, NULL, light_group, n_light);
    const int words = (n_surf + n_light + 63) / 64;
    #pragma omp parallel for schedule(static)
    for (int r = 0; r < n; r++) {
        v3 o = mk(orig[r * 3], orig[r * 3 + 1], orig[r * 3 + 2]);
        v3 d = mk(dir[r * 3], dir[r * 3 + 1], dir[r * 3 + 2]);
        hit_t h = closest_hit_masked(&sc, o, d, t_scale, hit_rule, masks + (size_t)r * words);
        out_t[r] = h.tri >= 0 ? h.t : INFINITY;
        out_hit[r] = pack_hit(&sc, h.tri, hit_rule);
    }
    free(sc.normal);
}

/* The pass set of the geometric test per triangle, without the closest-hit window: bit i
 * of masks[r * words + i / 64] = triangle i passes Triangle::intersects' test for ray r
 * (the detA, t, u, v conditions of closest_hit above, CPU/rays/ray.cpp:14-28 and Appendix A
 * of SURVEY.md for rule 0; GPU/rays/ray.cu:63-64 for rule 1).  A candidate filter must keep
 * every such triangle (tests of the kernels' culls and candidate tables). */
ORC_API void orc_pass_masks(const float *tri, int n_tri, const float *orig, const float *dir, int n,
                            float t_scale, int hit_rule, uint64_t *masks) {
    const int words = (n_tri + 63) / 64;
    #pragma omp parallel for schedule(static)
    for (int r = 0; r < n; r++) {
        v3 o = mk(orig[r * 3], orig[r * 3 + 1], orig[r * 3 + 2]);
        v3 d = mk(dir[r * 3], dir[r * 3 + 1], dir[r * 3 + 2]);
        v3 nD = mk(-(d.x * t_scale), -(d.y * t_scale), -(d.z * t_scale));
        uint64_t *m = masks + (size_t)r * words;
        for (int w = 0; w < words; w++) m[w] = 0;
        for (int i = 0; i < n_tri; i++) {
            v3 v0 = vtx(tri, i, 0), v1 = vtx(tri, i, 1), v2 = vtx(tri, i, 2);
            v3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z);
            v3 e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
            v3 b = mk(o.x - v0.x, o.y - v0.y, o.z - v0.z);
            float detA = det3(nD, e1, e2);
            if (!(detA != 0.0f)) continue;
            float t, u, v;
            if (hit_rule == 0) {
                float inv = 1.0f / detA;
                t = det3(b, e1, e2) * inv;
                u = det3(nD, b, e2) * inv;
                v = det3(nD, e1, b) * inv;
            } else {
                t = det3(b, e1, e2) / detA;
                u = det3(nD, b, e2) / detA;
                v = det3(nD, e1, b) / detA;
            }
            if (t >= 0.0f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f && (hit_rule != 0 || t > 1e-5f))
                m[i / 64] |= 1ull << (i % 64);
        }
    }
}

/* out[r * n_tri + i] = the t of triangle i's test for ray r under the rule's arithmetic and
 * pass conditions (closest_hit_masked's per-triangle code, no closest-hit window), +inf if
 * it does not pass: what a test needs to count the triangles below a ray's rule-0 cut or at
 * bit-equal t without restating the arithmetic. */
ORC_API void orc_pass_t(const float *tri, int n_tri, const float *orig, const float *dir, int n,
                        float t_scale, int hit_rule, float *out) {
    #pragma omp parallel for schedule(static)
    for (int r = 0; r < n; r++) {
        v3 o = mk(orig[r * 3], orig[r * 3 + 1], orig[r * 3 + 2]);
        v3 d = mk(dir[r * 3], dir[r * 3 + 1], dir[r * 3 + 2]);
        v3 D = mk(d.x * t_scale, d.y * t_scale, d.z * t_scale);
        v3 nD = mk(-D.x, -D.y, -D.z);
        float *row = out + (size_t)r * n_tri;
        for (int i = 0; i < n_tri; i++) {
            float t;
            row[i] = tri_pass_t(tri, i, o, nD, hit_rule, &t) ? t : INFINITY;
        }
    }
}

/* ------------------------------------------------------------------ */
/* sampling                                                            */
/* ------------------------------------------------------------------ */
/* CPU/utils/hemisphere_helpers.cpp:26-39 */
static void normal_frame(v3 n, v3 *T, v3 *Bv) {
    if (fabsf(n.x) > fabsf(n.y)) *T = normalize3(mk(n.z, 0.0f, -n.x));
    else *T = normalize3(mk(0.0f, -n.z, n.y));
    *Bv = cross3(n, *T);
}

/* reference_sequential mode (parity gate 3): the CPU engine's own
 * random stream — glibc rand() (never seeded by the reference: seed 1), drawn as
 * (float)rand() / RAND_MAX (CPU/path_tracing/default_path_tracing.cpp:26-27,
 * CPU/utils/hemisphere_helpers.cpp:69-70) in the order of one thread running the
 * x-outer / y-inner pixel loop (default_path_tracing.cpp:9-17) — and its libm trig
 * (phi = 2 * M_PI * r2 in double, then cosf/sinf, hemisphere_helpers.cpp:14-20).
 * Set only inside orc_render_sequential, which runs on one thread. */
static int g_seq = 0;

static float rand01(void) { return (float)rand() / (float)RAND_MAX; }

/* CPU/utils/hemisphere_helpers.cpp:4-21 (sampler 0) + cosine variant (sampler 1);
 * world = (s.x*B + s.y*N) + s.z*T, :73-77 */
static v3 sample_dir(v3 n, float r1, float r2, int sampler, float *cos_theta) {
    v3 T, Bv;
    normal_frame(n, &T, &Bv);
    float y, sin_theta;
    if (sampler == 0) {
        y = r1;
        sin_theta = sqrtf(1.0f - r1 * r1);
    } else {
        y = sqrtf(r1);
        sin_theta = sqrtf(1.0f - r1);
    }
    float sphi, cphi;
    if (g_seq) {
        const float phi = (float)(2 * 3.14159265358979323846 * (double)r2); /* M_PI */
        sphi = sinf(phi);
        cphi = cosf(phi);
    } else {
        orc_sincos_turn(r2, &sphi, &cphi);
    }
    float sx = sin_theta * cphi, sz = sin_theta * sphi;
    *cos_theta = y;
    return mk((sx * Bv.x + y * n.x) + sz * T.x,
              (sx * Bv.y + y * n.y) + sz * T.y,
              (sx * Bv.z + y * n.z) + sz * T.z);
}

/* ------------------------------------------------------------------ */
/* render                                                              */
/* ------------------------------------------------------------------ */
typedef struct {
    int32_t width, height, spp, max_bounces, sampler, preset, hit_rule, spp_split;
    uint64_t seed;
    float env_light, t_scale;
} orc_params;

typedef struct { float pos[4]; float yaw_y, yaw_x; } orc_camera;

static const float PI_F = 3.14159265358979323846f;  /* (float)M_PI */

/* camera ray: CPU/path_tracing/default_path_tracing.cpp:25-34 + Ray::Ray + rotate_ray
 * (glm mat4*vec4: (m0*v0 + m1*v1) + (m2*v2 + m3*v3), type_mat4x4.inl:561-570) */
static void camera_ray(const orc_camera *cam, const orc_params *p, float cy, float sy, float cx, float sx,
                       int px, int py, float r1, float r2, v3 *o, v3 *d) {
    float x = (float)px + r1;
    float y = (float)py + r2;
    v3 dir = mk(x - (float)p->width / 2.0f, y - (float)p->height / 2.0f, (float)p->height);
    dir = normalize3(dir);
    /* yaw about y: R[0]=(c,0,s,0) R[1]=(0,1,0,0) R[2]=(-s,0,c,0) R[3]=(0,0,0,1), w=1 */
    float w = 1.0f;
    v3 r;
    r.x = (cy * dir.x + 0.0f * dir.y) + (-sy * dir.z + 0.0f * w);
    r.y = (0.0f * dir.x + 1.0f * dir.y) + (0.0f * dir.z + 0.0f * w);
    r.z = (sy * dir.x + 0.0f * dir.y) + (cy * dir.z + 0.0f * w);
    float rw = (0.0f * dir.x + 0.0f * dir.y) + (0.0f * dir.z + 1.0f * w);
    if (p->preset == 1) {
        /* GPU/rays/ray.cu:168-171: R[1]=(0,c,-s,0) R[2]=(0,s,c,0) about x */
        v3 q;
        q.x = (1.0f * r.x + 0.0f * r.y) + (0.0f * r.z + 0.0f * rw);
        q.y = (0.0f * r.x + cx * r.y) + (sx * r.z + 0.0f * rw);
        q.z = (0.0f * r.x + -sx * r.y) + (cx * r.z + 0.0f * rw);
        r = q;
    }
    *o = mk(cam->pos[0], cam->pos[1], cam->pos[2]);
    *d = r;
}

/* CPU-engine recursion: path_trace_recursive / indirect_irradiance */
static v3 trace_recursive(const orc_scene *sc, const orc_params *p, uint32_t pix, uint32_t smp,
                          v3 o, v3 d, int bounces, uint64_t *casts) {
    hit_t h = closest_hit(sc, o, d, p->t_scale, p->hit_rule);
    (*casts)++;
    if (h.tri < 0) return mk(0.0f, 0.0f, 0.0f);
    if (h.tri >= sc->n_surf) {
        const float *e = sc->emission + (size_t)(h.tri - sc->n_surf) * 3;
        return mk(e[0], e[1], e[2]);
    }
    if (bounces == p->max_bounces) return mk(0.0f, 0.0f, 0.0f);
    /* position = o + t*D  (D = d*t_scale) */
    v3 D = mk(d.x * p->t_scale, d.y * p->t_scale, d.z * p->t_scale);
    v3 pos = mk(o.x + h.t * D.x, o.y + h.t * D.y, o.z + h.t * D.z);
    const float *nn = sc->normal + (size_t)h.tri * 3;
    float r1, r2;
    if (g_seq) {
        r1 = rand01();
        r2 = rand01();
    } else {
        draw2(p->seed, pix, smp, 1u + (uint32_t)bounces, &r1, &r2);
    }
    float cos_theta;
    v3 s = sample_dir(mk(nn[0], nn[1], nn[2]), r1, r2, p->sampler, &cos_theta);
    v3 start = mk(pos.x + 1e-5f * s.x, pos.y + 1e-5f * s.y, pos.z + 1e-5f * s.z);
    v3 nd = normalize3(s);
    v3 rad = trace_recursive(sc, p, pix, smp, start, nd, bounces + 1, casts);
    const float *al = sc->albedo + (size_t)h.tri * 3;
    v3 out;
    if (p->sampler == 0) {
        v3 brdf = mk(al[0] / PI_F, al[1] / PI_F, al[2] / PI_F);
        float rho = 1.0f / (2.0f * PI_F);
        out.x = ((rad.x * brdf.x) * cos_theta) / rho;
        out.y = ((rad.y * brdf.y) * cos_theta) / rho;
        out.z = ((rad.z * brdf.z) * cos_theta) / rho;
    } else {
        out = mk(rad.x * al[0], rad.y * al[1], rad.z * al[2]);
    }
    return out;
}

/* GPU-engine iteration: path_trace_iterative */
static v3 trace_iterative(const orc_scene *sc, const orc_params *p, uint32_t pix, uint32_t smp,
                          v3 o, v3 d, uint64_t *casts) {
    v3 tp = mk(1.0f, 1.0f, 1.0f);
    const float RHO = 1.0f / (2.0f * 3.1415926535f);
    for (int i = 0; i < p->max_bounces; i++) {
        hit_t h = closest_hit(sc, o, d, p->t_scale, p->hit_rule);
        (*casts)++;
        if (h.tri < 0) return mk(tp.x * p->env_light, tp.y * p->env_light, tp.z * p->env_light);
        if (h.tri >= sc->n_surf) {
            const float *e = sc->emission + (size_t)(h.tri - sc->n_surf) * 3;
            return mk(tp.x * e[0], tp.y * e[1], tp.z * e[2]);
        }
        v3 D = mk(d.x * p->t_scale, d.y * p->t_scale, d.z * p->t_scale);
        v3 pos = mk(o.x + h.t * D.x, o.y + h.t * D.y, o.z + h.t * D.z);
        const float *nn = sc->normal + (size_t)h.tri * 3;
        float r1, r2;
        draw2(p->seed, pix, smp, 1u + (uint32_t)i, &r1, &r2);
        float cos_theta;
        v3 s = sample_dir(mk(nn[0], nn[1], nn[2]), r1, r2, p->sampler, &cos_theta);
        const float *al = sc->albedo + (size_t)h.tri * 3;
        if (p->sampler == 0) {
            v3 brdf = mk(al[0] / PI_F, al[1] / PI_F, al[2] / PI_F);
            tp.x = ((tp.x * brdf.x) * cos_theta) / RHO;
            tp.y = ((tp.y * brdf.y) * cos_theta) / RHO;
            tp.z = ((tp.z * brdf.z) * cos_theta) / RHO;
        } else {
            tp = mk(tp.x * al[0], tp.y * al[1], tp.z * al[2]);
        }
        o = mk(pos.x + 1e-5f * s.x, pos.y + 1e-5f * s.y, pos.z + 1e-5f * s.z);
        d = normalize3(s);
    }
    return mk(0.0f, 0.0f, 0.0f);
}

/*
 * Render the rectangle [x0,x0+w) x [y0,y0+h) of a width x height image.
 * out_rgb: w*h*3 floats, row-major (row = y - y0).  out_casts: total ray casts.
 * Threads: OpenMP over rows (deterministic: the RNG is keyed per pixel).
 */
ORC_API int orc_render(const float *tri, const float *albedo, int n_surf,
                       const float *emission, const int32_t *light_group, int n_light,
                       const orc_camera *cam, const orc_params *p,
                       int x0, int y0, int w, int h, float *out_rgb, uint64_t *out_casts) {
    orc_scene sc;
    scene_init(&sc, tri, albedo, n_surf, emission, light_group, n_light);
    /* Camera trig evaluated once on the host in double, rounded to float
     * (Ray::rotate_ray's cos(yaw)/sin(yaw)). */
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    uint64_t total = 0;
    #pragma omp parallel for schedule(dynamic, 1) reduction(+:total)
    for (int yy = 0; yy < h; yy++) {
        for (int xx = 0; xx < w; xx++) {
            int px = x0 + xx, py = y0 + yy;
            uint32_t pix = (uint32_t)py * (uint32_t)p->width + (uint32_t)px;
            /* spp_split S: chunk c sums samples [c*m, (c+1)*m) in order (m = spp/S);
             * the pixel sum is ((P0 + P1) + P2) + ...  (rtmi.h, rt_params.spp_split) */
            int S = p->spp_split <= 0 ? 1 : p->spp_split;
            int m = p->spp / S;
            v3 acc = mk(0.0f, 0.0f, 0.0f);
            uint64_t casts = 0;
            for (int c = 0; c < S; c++) {
                v3 part = mk(0.0f, 0.0f, 0.0f);
                for (int s = c * m; s < (c + 1) * m; s++) {
                    float r1, r2;
                    draw2(p->seed, pix, (uint32_t)s, 0u, &r1, &r2);
                    v3 o, d;
                    camera_ray(cam, p, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
                    v3 L = (p->preset == 0) ? trace_recursive(&sc, p, pix, (uint32_t)s, o, d, 0, &casts)
                                            : trace_iterative(&sc, p, pix, (uint32_t)s, o, d, &casts);
                    part.x = part.x + L.x; part.y = part.y + L.y; part.z = part.z + L.z;
                }
                if (c == 0) acc = part;
                else { acc.x = acc.x + part.x; acc.y = acc.y + part.y; acc.z = acc.z + part.z; }
            }
            float fs = (float)p->spp;
            float *dst = out_rgb + ((size_t)yy * w + xx) * 3;
            dst[0] = acc.x / fs; dst[1] = acc.y / fs; dst[2] = acc.z / fs;
            total += casts;
        }
    }
    free(sc.normal);
    if (out_casts) *out_casts = total;
    return 0;
}

/*
 * Primary-ray hits of the rectangle [x0,x0+w) x [y0,y0+h), samples [s0, s1) of every
 * pixel: the triangle index (surfaces then light triangles; -1 = miss) of each camera
 * ray, in (row, column, sample) order.  The check of the kernels' primary-ray cull
 * (rt_rect_candidates): every triangle hit here must be a candidate of the rectangle.
 */
ORC_API void orc_primary_hits(const float *tri, int n_surf, int n_light, const orc_camera *cam,
                              const orc_params *p, int x0, int y0, int w, int h, int s0, int s1,
                              int32_t *out_tri) {
    orc_scene sc;
    scene_init(&sc, tri, NULL, n_surf, NULL, NULL, n_light);
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    const int ns = s1 - s0;
    #pragma omp parallel for schedule(static)
    for (int yy = 0; yy < h; yy++) {
        for (int xx = 0; xx < w; xx++) {
            int px = x0 + xx, py = y0 + yy;
            uint32_t pix = (uint32_t)py * (uint32_t)p->width + (uint32_t)px;
            for (int s = s0; s < s1; s++) {
                float r1, r2;
                draw2(p->seed, pix, (uint32_t)s, 0u, &r1, &r2);
                v3 o, d;
                camera_ray(cam, p, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
                hit_t ht = closest_hit(&sc, o, d, p->t_scale, p->hit_rule);
                out_tri[((size_t)yy * w + xx) * ns + (s - s0)] = ht.tri;
            }
        }
    }
    free(sc.normal);
}

/*
 * The whole frame in the reference's own sampling order and random stream
 * (g_seq above): CPU preset, uniform sampler, CPU hit rule only.  out_rgb: W*H*3,
 * row-major.  srand(seed) first (seed 1 = the reference's unseeded stream).  Its
 * images match the Philox renders only statistically (gate 3, tests/).
 */
ORC_API int orc_render_sequential(const float *tri, const float *albedo, int n_surf,
                                  const float *emission, const int32_t *light_group, int n_light,
                                  const orc_camera *cam, const orc_params *p, float *out_rgb,
                                  uint64_t *out_casts) {
    if (p->preset != 0 || p->sampler != 0 || p->hit_rule != 0) return -1;
    orc_scene sc;
    scene_init(&sc, tri, albedo, n_surf, emission, light_group, n_light);
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    uint64_t casts = 0;
    srand((unsigned)p->seed);
    g_seq = 1;
    for (int px = 0; px < p->width; px++) {
        for (int py = 0; py < p->height; py++) {
            v3 acc = mk(0.0f, 0.0f, 0.0f);
            for (int s = 0; s < p->spp; s++) {
                const float r1 = rand01();
                const float r2 = rand01();
                v3 o, d;
                camera_ray(cam, p, cy, sy, 1.0f, 0.0f, px, py, r1, r2, &o, &d);
                v3 L = trace_recursive(&sc, p, 0u, 0u, o, d, 0, &casts);
                acc.x = acc.x + L.x; acc.y = acc.y + L.y; acc.z = acc.z + L.z;
            }
            const float fs = (float)p->spp;
            float *dst = out_rgb + ((size_t)py * p->width + px) * 3;
            dst[0] = acc.x / fs; dst[1] = acc.y / fs; dst[2] = acc.z / fs;
        }
    }
    g_seq = 0;
    free(sc.normal);
    if (out_casts) *out_casts = casts;
    return 0;
}

/* the first n values of glibc rand() after srand(seed) (pins the stream above) */
ORC_API void orc_glibc_rand(unsigned seed, int n, int32_t *out) {
    srand(seed);
    for (int i = 0; i < n; i++) out[i] = (int32_t)rand();
}

/* CPU/sdl/sdl_screen.cpp:100-112: uint32(clamp(255*c, 0, 255)), (128<<24)+(r<<16)+(g<<8)+b */
static uint32_t chan8(float c) {
    float v = 255.0f * c;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);   /* glm::clamp = min(max(x,lo),hi) */
    return (uint32_t)v;
}

ORC_API void orc_pack_argb(const float *rgb, int n, uint32_t *out) {
    for (int i = 0; i < n; i++) {
        out[i] = (128u << 24) + (chan8(rgb[i * 3]) << 16) + (chan8(rgb[i * 3 + 1]) << 8) + chan8(rgb[i * 3 + 2]);
    }
}

ORC_API int orc_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

ORC_API void orc_set_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

/* ================================================================== */
/* DQN path (BASELINE config 4)                                        */
/* ================================================================== */
/*
 * Restates:
 *   DQNetwork::network_inference  NN_Builders/dq_network.cu:36-49 and
 *   FCLayer::run_inference        NN_Builders/fc_layer.cu:40-72: h = ReLU(W h + b) x 4
 *   NN input                      GPU/deep_learning/nn_rendering_helpers.cu:280-298: v - x
 *   importance_sample_direction   nn_rendering_helpers.cu:391-489
 *   sample_ray_for_grid_index     nn_rendering_helpers.cu:38-57
 *   convert_grid_pos_to_direction_random + map (Chiu)  GPU/utils/hemisphere_helpers.cu:95-226,
 *     restated in turns: cos(theta) = 1 - xx^2, sin(theta) = xx*sqrt(2 - xx^2),
 *     phi = offset + (yy/xx)/8 turns (identical mathematically)
 *   render_frame / initialise_ray / trace_ray  GPU/deep_learning/pre_trained_pathtracer.cu:188-491
 * RNG: event 1+b of bounce b >= 1: Philox counter word 3 = 0 gives rv,
 * = 1 + a/2 the jitter of cells a (pairs), = 73 the final jitter.
 * The forward pass accumulates in double (bf16 = 0: the reference's fp32 network,
 * DyNet) or follows the kernel's arithmetic (bf16 = 1): layer 0 folded to the affine
 * map h1 = ReLU(c0 - fma(S2, z, fma(S1, y, S0 x))) of the ray position (c0 = W1 v + b1,
 * S = W1's column sums per coordinate, both summed in double in index order and
 * rounded to float, as rt_dqn_create does), bf16-rounded; layers 1-3 with bf16
 * operands and activations, double accumulation.
 */
typedef struct {
    int n_in, h1, h2, h3, n_out;
    const float *W[4], *b[4]; /* row-major [out][in] */
    const float *verts;       /* n_in: Scene::vertices */
    /* bf16 arithmetic, computed once per network by dqn_prepare (the same values the
     * per-call evaluation gives): the folded layer 0 {c0, S0, S1, S2} per output and the
     * bf16-rounded weights of layers 1-3 */
    float *fold;
    float *Wb[4];
} orc_dqn;

static float bf16_round(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) { u |= 0x400000u; u &= 0xffff0000u; }
    else { u += 0x7fffu + ((u >> 16) & 1u); u &= 0xffff0000u; }
    float r;
    memcpy(&r, &u, 4);
    return r;
}

/* the bf16 path's per-network constants (orc_dqn.fold, .Wb) */
static void dqn_prepare(orc_dqn *net) {
    net->fold = (float *)malloc(sizeof(float) * 4 * (size_t)net->h1);
    for (int o = 0; o < net->h1; o++) {
        const float *w = net->W[0] + (size_t)o * net->n_in;
        double c0 = (double)net->b[0][o], S[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < net->n_in; i++) {
            c0 += (double)w[i] * (double)net->verts[i];
            S[i % 3] += (double)w[i];
        }
        net->fold[4 * o + 0] = (float)c0;
        net->fold[4 * o + 1] = (float)S[0];
        net->fold[4 * o + 2] = (float)S[1];
        net->fold[4 * o + 3] = (float)S[2];
    }
    int dims[5] = {net->n_in, net->h1, net->h2, net->h3, net->n_out};
    net->Wb[0] = NULL;
    for (int l = 1; l < 4; l++) {
        size_t n = (size_t)dims[l] * dims[l + 1];
        float *w = (float *)malloc(sizeof(float) * n);
        for (size_t i = 0; i < n; i++) w[i] = bf16_round(net->W[l][i]);
        net->Wb[l] = w;
    }
}

static void dqn_release(orc_dqn *net) {
    free(net->fold);
    for (int l = 1; l < 4; l++) free(net->Wb[l]);
}

static void dqn_forward_one(const orc_dqn *net, const float *loc, int bf16, float *q_out, float *scratch) {
    int dims[5] = {net->n_in, net->h1, net->h2, net->h3, net->n_out};
    float *in = scratch, *out = scratch + 1024;
    int l0 = 0;
    if (bf16) {
        for (int o = 0; o < net->h1; o++) {
            const float cf = net->fold[4 * o], s0 = net->fold[4 * o + 1], s1 = net->fold[4 * o + 2],
                        s2 = net->fold[4 * o + 3];
            float h = cf - fmaf(s2, loc[2], fmaf(s1, loc[1], s0 * loc[0]));
            h = h > 0.0f ? h : 0.0f;
            in[o] = bf16_round(h);
        }
        l0 = 1;
    } else {
        for (int k = 0; k < net->n_in; k++) in[k] = net->verts[k] - loc[k % 3];
    }
    for (int l = l0; l < 4; l++) {
        const float *W = net->W[l], *b = net->b[l];
        for (int o = 0; o < dims[l + 1]; o++) {
            double acc = 0.0;
            const float *w = (bf16 ? net->Wb[l] : W) + (size_t)o * dims[l];
            for (int i = 0; i < dims[l]; i++) acc += (double)w[i] * (double)in[i];
            float v = (float)acc + b[o];
            v = v > 0.0f ? v : 0.0f;
            out[o] = (bf16 && l < 3) ? bf16_round(v) : v;
        }
        float *t = in; in = out; out = t;
    }
    memcpy(q_out, in, sizeof(float) * (size_t)net->n_out);
}

ORC_API void orc_dqn_forward(int n_in, int h1, int h2, int h3, int n_out, const float *const *W,
                             const float *const *b, const float *verts, const float *loc, int n, int bf16,
                             float *q) {
    orc_dqn net = {n_in, h1, h2, h3, n_out, {W[0], W[1], W[2], W[3]}, {b[0], b[1], b[2], b[3]}, verts,
                   NULL, {NULL, NULL, NULL, NULL}};
    if (bf16) dqn_prepare(&net);
    #pragma omp parallel
    {
        float *scratch = (float *)malloc(sizeof(float) * 2048);
        #pragma omp for schedule(static)
        for (int r = 0; r < n; r++) dqn_forward_one(&net, loc + (size_t)r * 3, bf16, q + (size_t)r * n_out, scratch);
        free(scratch);
    }
    if (bf16) dqn_release(&net);
}

static void chiu_map_t(float x, float y, float *xr, float *yr, float *zr) {
    x = 2.0f * x - 1.0f;
    y = 2.0f * y - 1.0f;
    float xx, yy, off;
    if (y > -x) {
        if (y < x) {
            xx = x;
            if (y > 0.0f) { off = 0.0f; yy = y; } else { off = 0.875f; yy = x + y; }
        } else {
            xx = y;
            if (x > 0.0f) { off = 0.125f; yy = y - x; } else { off = 0.25f; yy = -x; }
        }
    } else {
        if (y > x) {
            xx = -x;
            if (y > 0.0f) { off = 0.375f; yy = -x - y; } else { off = 0.5f; yy = -y; }
        } else {
            xx = -y;
            if (x > 0.0f) { off = 0.75f; yy = x; }
            else if (y != 0.0f) { off = 0.625f; yy = x - y; }
            else { *xr = 0.0f; *yr = 1.0f; *zr = 0.0f; return; }
        }
    }
    float c = 1.0f - xx * xx;
    float s = xx * sqrtf(2.0f - xx * xx);
    float phi = off + 0.125f * (yy / xx);
    float sp, cp;
    orc_sincos_turn(phi, &sp, &cp);
    *xr = s * cp;
    *yr = c;
    *zr = s * sp;
}

/* create_transformation_matrix(normal, position) = mat4(T, N, B, pos); world = M*(x,y,z,1);
 * direction = normalize(world - pos) */
static v3 grid_dir(float gx, float gy, v3 N, v3 T, v3 B, v3 pos) {
    float xh, yh, zh;
    chiu_map_t(gx / 12.0f, gy / 12.0f, &xh, &yh, &zh);
    v3 w = mk((T.x * xh + N.x * yh) + (B.x * zh + pos.x * 1.0f),
              (T.y * xh + N.y * yh) + (B.y * zh + pos.y * 1.0f),
              (T.z * xh + N.z * yh) + (B.z * zh + pos.z * 1.0f));
    return normalize3(mk(w.x - pos.x, w.y - pos.y, w.z - pos.z));
}

/* cos(theta) of the Chiu-map direction of (gx, gy): 1 - xx^2, xx = max(|2x-1|, |2y-1|)
 * (the octant branches of chiu_map_t select exactly that; the origin gives 1) -- the
 * same angle as the reference's dot(N, normalize(M v - p)) up to float rounding */
static float chiu_cos(float gx, float gy) {
    float x = 2.0f * (gx / 12.0f) - 1.0f, y = 2.0f * (gy / 12.0f) - 1.0f;
    float ax = fabsf(x), ay = fabsf(y);
    float xx = ax > ay ? ax : ay;
    return 1.0f - xx * xx;
}

static int dqn_sample(float *q, v3 N, v3 pos, uint64_t seed, uint32_t pix, uint32_t smp, uint32_t ev,
                      v3 *tp, v3 *dir_out) {
    v3 T, B;
    normal_frame(N, &T, &B);
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t ctr[4] = {pix, smp, ev, 0u}, o[4];
    orc_philox4x32_10(ctr, key, o);
    float rv = u01(o[0]);
    /* Q*cos per cell, then importance_sample_direction's sums (nn_rendering_helpers.cu:391-489)
     * in the fixed blocked order the device uses (rt_dqn.hip sample_from_q and the fused
     * k_dqn_mlp): 4 blocks of 36 cells; B_w = sum of qc = Q*cos over block w in cell order,
     * total = ((B_0 + B_1) + B_2) + B_3, P_0 = 0, P_{w+1} = P_w + B_w / total; the walk starts
     * in the first block w with P_{w+1} > rv from cum = P_w, cell by cell cum = cum + qd
     * (qd = qc / total), and takes the first cell with cum > rv and qd > 0 (on into the next
     * block if rounding leaves the block without one).  Inside the chosen block this is the
     * reference's own walk; the block sums only change the association of the float sums. */
    /* the cell jitters: one Philox draw per 4 cells (counter 1 + a/4), cell 4j + h takes the
     * two 16-bit halves of word h as (x, y) in [0, 1) */
    float bsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < 36; j++) {
        ctr[3] = 1u + (uint32_t)j;
        orc_philox4x32_10(ctr, key, o);
        for (int h = 0; h < 4; h++) {
            int a = 4 * j + h;
            int gxi = a / 12, gyi = a - gxi * 12;
            float c = chiu_cos((float)gxi + u16lo(o[h]), (float)gyi + u16hi(o[h]));
            float qc = q[a] * c;
            q[a] = qc;
            bsum[a / 36] = bsum[a / 36] + qc;
        }
    }
    float total = 0.0f;
    for (int w = 0; w < 4; w++) total = total + bsum[w];
    int act = -1;
    float P = 0.0f, qd_sel = 0.0f;
    for (int w = 0; w < 4 && act < 0; w++) {
        float Pn = P + bsum[w] / total;
        if (Pn > rv) {
            float cum = P;
            for (int a = 36 * w; a < 36 * w + 36 && act < 0; a++) {
                float qd = q[a] / total;
                cum = cum + qd;
                if (cum > rv && qd > 0.0f) { act = a; qd_sel = qd; }
            }
        }
        P = Pn;
    }
    *dir_out = mk(0.0f, 0.0f, 0.0f);
    if (act >= 0) {
        ctr[3] = 73u;
        orc_philox4x32_10(ctr, key, o);
        int gxi = act / 12, gyi = act - gxi * 12;
        v3 d = grid_dir((float)gxi + u01(o[0]), (float)gyi + u01(o[1]), N, T, B, pos);
        float c = dot3(N, d);
        const float RHO = 1.0f / (2.0f * 3.1415926535f);
        const float GRID_RHO = 1.0f / (12.0f * 12.0f);
        float pdf = RHO * (qd_sel / GRID_RHO);
        tp->x = (tp->x * c) / pdf;
        tp->y = (tp->y * c) / pdf;
        tp->z = (tp->z * c) / pdf;
        *dir_out = d;
    }
    return act;
}

ORC_API void orc_dqn_sample(const float *tri_all, int n_tri, float *q, const float *loc, const int32_t *tri,
                            const uint32_t *pix, int n, int sample, int bounce, uint64_t seed, float *tp,
                            float *dir_out, int32_t *action) {
    float *nrm = (float *)malloc(sizeof(float) * 3 * (size_t)n_tri);
    orc_triangle_normals(tri_all, n_tri, nrm);
    #pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++) {
        const float *nn = nrm + (size_t)tri[i] * 3;
        v3 t = mk(tp[i * 3], tp[i * 3 + 1], tp[i * 3 + 2]), d;
        action[i] = dqn_sample(q + (size_t)i * 144, mk(nn[0], nn[1], nn[2]),
                               mk(loc[i * 3], loc[i * 3 + 1], loc[i * 3 + 2]), seed, pix[i], (uint32_t)sample,
                               1u + (uint32_t)bounce, &t, &d);
        tp[i * 3] = t.x; tp[i * 3 + 1] = t.y; tp[i * 3 + 2] = t.z;
        dir_out[i * 3] = d.x; dir_out[i * 3 + 1] = d.y; dir_out[i * 3 + 2] = d.z;
    }
    free(nrm);
}

/* trace_ray: Ray(pos + dir*1e-5, dir) with the GPU hit rule; returns 1 if on a surface */
static int dqn_trace(const orc_scene *sc, const orc_params *p, v3 pos, v3 dir, v3 *loc, int *tri, v3 *tp,
                     uint64_t *casts) {
    v3 o = mk(pos.x + dir.x * 1e-5f, pos.y + dir.y * 1e-5f, pos.z + dir.z * 1e-5f);
    v3 d = normalize3(dir);
    hit_t h = closest_hit(sc, o, d, p->t_scale, 1);
    (*casts)++;
    if (h.tri < 0) { *tp = mk(tp->x * p->env_light, tp->y * p->env_light, tp->z * p->env_light); return 0; }
    if (h.tri >= sc->n_surf) {
        const float *e = sc->emission + (size_t)(h.tri - sc->n_surf) * 3;
        *tp = mk(tp->x * e[0], tp->y * e[1], tp->z * e[2]);
        return 0;
    }
    v3 D = mk(d.x * p->t_scale, d.y * p->t_scale, d.z * p->t_scale);
    *loc = mk(o.x + h.t * D.x, o.y + h.t * D.y, o.z + h.t * D.z);
    *tri = h.tri;
    const float *al = sc->albedo + (size_t)h.tri * 3;
    *tp = mk(tp->x * (al[0] / PI_F), tp->y * (al[1] / PI_F), tp->z * (al[2] / PI_F));
    return 1;
}

ORC_API int orc_render_dqn(const float *tri, const float *albedo, int n_surf, const float *emission,
                           const int32_t *light_group, int n_light, int n_in, int h1, int h2, int h3,
                           const float *const *W, const float *const *b, const float *verts, int bf16,
                           const orc_camera *cam, const orc_params *p, int x0, int y0, int w, int h,
                           float *out_rgb, uint64_t *out_casts) {
    orc_scene sc;
    scene_init(&sc, tri, albedo, n_surf, emission, light_group, n_light);
    orc_dqn net = {n_in, h1, h2, h3, 144, {W[0], W[1], W[2], W[3]}, {b[0], b[1], b[2], b[3]}, verts,
                   NULL, {NULL, NULL, NULL, NULL}};
    if (bf16) dqn_prepare(&net);
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    uint64_t total_casts = 0;
    #pragma omp parallel reduction(+:total_casts)
    {
        float *scratch = (float *)malloc(sizeof(float) * 2048);
        float q[144];
        #pragma omp for schedule(dynamic, 1)
        for (int yy = 0; yy < h; yy++) {
            for (int xx = 0; xx < w; xx++) {
                int px = x0 + xx, py = y0 + yy;
                uint32_t pix = (uint32_t)py * (uint32_t)p->width + (uint32_t)px;
                v3 acc = mk(0.0f, 0.0f, 0.0f);
                for (int s = 0; s < p->spp; s++) {
                    float r1, r2;
                    draw2(p->seed, pix, (uint32_t)s, 0u, &r1, &r2);
                    v3 o, d;
                    orc_params pg = *p;
                    pg.preset = 1;
                    camera_ray(cam, &pg, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
                    v3 tp = mk(1.0f, 1.0f, 1.0f), loc = o;
                    int tri_i = 0;
                    int alive = dqn_trace(&sc, p, o, d, &loc, &tri_i, &tp, &total_casts);
                    for (int bnc = 1; alive && bnc < p->max_bounces; bnc++) {
                        float locf[3] = {loc.x, loc.y, loc.z};
                        dqn_forward_one(&net, locf, bf16, q, scratch);
                        /* the kernel arithmetic (bf16 = 1) keeps the renderer's Q in bf16
                         * between the forward and the sampler (k_dqn_mlp<.., QB>); bf16 = 2:
                         * the bf16 forward with its fp32 Q (the statistical gate of that
                         * rounding, tests/test_dqn.py) */
                        if (bf16 == 1)
                            for (int a = 0; a < 144; a++) q[a] = bf16_round(q[a]);
                        const float *nn = sc.normal + (size_t)tri_i * 3;
                        v3 dir;
                        int act = dqn_sample(q, mk(nn[0], nn[1], nn[2]), loc, p->seed, pix, (uint32_t)s,
                                             1u + (uint32_t)bnc, &tp, &dir);
                        if (act < 0) {
                            total_casts++;
                            tp = mk(tp.x * p->env_light, tp.y * p->env_light, tp.z * p->env_light);
                            alive = 0;
                        } else {
                            alive = dqn_trace(&sc, p, loc, dir, &loc, &tri_i, &tp, &total_casts);
                        }
                    }
                    acc.x = acc.x + tp.x; acc.y = acc.y + tp.y; acc.z = acc.z + tp.z;
                }
                float fs = (float)p->spp;
                float *dst = out_rgb + ((size_t)yy * w + xx) * 3;
                dst[0] = acc.x / fs; dst[1] = acc.y / fs; dst[2] = acc.z / fs;
            }
        }
        free(scratch);
    }
    free(sc.normal);
    if (bf16) dqn_release(&net);
    if (out_casts) *out_casts = total_casts;
    return 0;
}

/* The same render in wavefront order with the Q values supplied by the caller: per bounce,
 * every live path's position goes out in one batch (path order: sample-major, then the
 * rect's pixels row-major) and q_fn returns their 144 Q values; the sampling, the traces
 * and the per-pixel sums are orc_render_dqn's (each path's arithmetic does not depend on the
 * batch, so with the network's own Q this equals orc_render_dqn).  The tests pass the GPU
 * forward (k_dqn_mlp through rt_dqn_forward) as q_fn: everything downstream of the bf16
 * GEMM is then checked bit for bit against the device render
 * (PretrainedPathtracer::render_frame, pre_trained_pathtracer.cu:188-491).  As the device
 * renderer does, the batch's Q is rounded to bf16 (RNE) before the sampler. */
typedef void (*orc_q_fn)(const float *loc, int n, float *q, void *user);

ORC_API int orc_render_dqn_wave(const float *tri, const float *albedo, int n_surf, const float *emission,
                                const int32_t *light_group, int n_light, const orc_camera *cam,
                                const orc_params *p, int x0, int y0, int w, int h, orc_q_fn q_fn, void *user,
                                float *out_rgb, uint64_t *out_casts) {
    orc_scene sc;
    scene_init(&sc, tri, albedo, n_surf, emission, light_group, n_light);
    const float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    const float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    const int n_pix = w * h, n = n_pix * p->spp;
    v3 *tp = (v3 *)malloc(sizeof(v3) * (size_t)n), *loc = (v3 *)malloc(sizeof(v3) * (size_t)n);
    int *tri_i = (int *)malloc(sizeof(int) * (size_t)n), *live = (int *)malloc(sizeof(int) * (size_t)n);
    float *bl = (float *)malloc(sizeof(float) * 3 * (size_t)n), *bq = (float *)malloc(sizeof(float) * 144 * (size_t)n);
    uint64_t total_casts = 0;
    int n_live = 0;
    for (int r = 0; r < n; r++) {
        const int s = r / n_pix, pi = r % n_pix;
        const int px = x0 + pi % w, py = y0 + pi / w;
        const uint32_t pix = (uint32_t)py * (uint32_t)p->width + (uint32_t)px;
        float r1, r2;
        draw2(p->seed, pix, (uint32_t)s, 0u, &r1, &r2);
        v3 o, d;
        orc_params pg = *p;
        pg.preset = 1;
        camera_ray(cam, &pg, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
        tp[r] = mk(1.0f, 1.0f, 1.0f);
        loc[r] = o;
        tri_i[r] = 0;
        if (dqn_trace(&sc, p, o, d, &loc[r], &tri_i[r], &tp[r], &total_casts)) live[n_live++] = r;
    }
    for (int bnc = 1; n_live > 0 && bnc < p->max_bounces; bnc++) {
        for (int k = 0; k < n_live; k++) {
            bl[3 * (size_t)k] = loc[live[k]].x;
            bl[3 * (size_t)k + 1] = loc[live[k]].y;
            bl[3 * (size_t)k + 2] = loc[live[k]].z;
        }
        q_fn(bl, n_live, bq, user);
        for (size_t i = 0; i < (size_t)n_live * 144; i++) bq[i] = bf16_round(bq[i]);
        int m = 0;
        for (int k = 0; k < n_live; k++) {
            const int r = live[k], s = r / n_pix, pi = r % n_pix;
            const uint32_t pix = (uint32_t)(y0 + pi / w) * (uint32_t)p->width + (uint32_t)(x0 + pi % w);
            const float *nn = sc.normal + (size_t)tri_i[r] * 3;
            v3 dir;
            const int act = dqn_sample(bq + (size_t)k * 144, mk(nn[0], nn[1], nn[2]), loc[r], p->seed, pix,
                                       (uint32_t)s, 1u + (uint32_t)bnc, &tp[r], &dir);
            int alive;
            if (act < 0) {
                total_casts++;
                tp[r] = mk(tp[r].x * p->env_light, tp[r].y * p->env_light, tp[r].z * p->env_light);
                alive = 0;
            } else {
                alive = dqn_trace(&sc, p, loc[r], dir, &loc[r], &tri_i[r], &tp[r], &total_casts);
            }
            if (alive) live[m++] = r;
        }
        n_live = m;
    }
    for (int pi = 0; pi < n_pix; pi++) {
        v3 acc = mk(0.0f, 0.0f, 0.0f);
        for (int s = 0; s < p->spp; s++) {
            const v3 t = tp[(size_t)s * n_pix + pi];
            acc.x = acc.x + t.x; acc.y = acc.y + t.y; acc.z = acc.z + t.z;
        }
        const float fs = (float)p->spp;
        float *dst = out_rgb + (size_t)pi * 3;
        dst[0] = acc.x / fs; dst[1] = acc.y / fs; dst[2] = acc.z / fs;
    }
    free(tp); free(loc); free(tri_i); free(live); free(bl); free(bq);
    free(sc.normal);
    if (out_casts) *out_casts = total_casts;
    return 0;
}

/* ================================================================== */
/* Expected-SARSA path (BASELINE config 3)                             */
/* ================================================================== */
/*
 * Restates (GPU_Rendering_Engine/Source/):
 *   radiance volume count / placement  radiance_volumes/radiance_map.cu:57-84,
 *                                      objects/triangle.cu:17-45 (area; rejection point picking)
 *   initial Q / CDF / irradiance       radiance_volumes/radiance_volume.cu:46-89
 *   KD tree + array form               radiance_volumes/radiance_tree.cu:10-246 (std::sort on
 *                                      position[dim]: oracle/orc_sort.cpp calls the same std::sort)
 *   nearest volume                     radiance_volumes/radiance_map.cu:149-203
 *   sector sampling                    radiance_volume.cu:191-244, radiance_map.cu:90-106
 *   TD target                          radiance_map.cu:110-146, radiance_volume.cu:304-307
 *   TD update + irradiance             radiance_volume.cu:93-112, 282-301
 *   CDF rebuild                        radiance_volume.cu:148-188
 *   render loop                        path_tracing/reinforcement_path_tracing.cu:26-120
 * Frame-synchronous TD: a frame reads the previous frame's
 * Q / CDF / irradiance; its TD targets are summed per (volume, sector) in
 * fixed point (round(target * 2^32), int64) with counts, then folded as the
 * running mean of alpha = 1/(1 + visits), clamped at 0.8/144.
 * RNG: volume placement counter (volume, attempt, 0xFFFF0001, 0), u01 of words
 * 0,1; sampling at bounce i counter (pixel, frame*spp + sample, 1+i, 0): words
 * 0,1,2 = r (sector), rx, ry in (0,1] like curand_uniform (uniform fallback: words 0,1).
 */
void orc_kd_sort(int32_t *v, int n, const float *pos4, int dim); /* orc_sort.cpp */

typedef struct {
    int dim, leaf, left, right;
    float data, px, py, pz, nx, ny, nz;
    int vol;
} orc_kd;

typedef struct {
    int n_vol, n_kd, kd_cap;
    float *pos;     /* [n][4] */
    float *nrm;     /* [n][3] */
    int32_t *surf;  /* [n] */
    float *frame;   /* [n][9] N T B */
    float *brdf;    /* [n] */
    float *cc, *ck; /* [n*144] cos of cell centre / corner directions */
    float *Q, *cdf, *accum;
    uint32_t *visits, *cnt;
    int64_t *sum;
    orc_kd *kd;
    float *tri_lum;
    uint32_t frames;
    uint64_t seed;
    int sample_max;                 /* 1: sample_max_direction_from_radiance_distribution */
    int inframe;                    /* 1: the reference's in-frame TD rule, one event at a time */
    uint64_t stat_paths, stat_zero; /* last frame: sum of per-pixel floor(path length mean), zero paths */
    uint64_t stat_null, stat_sector0, stat_cdf; /* last frame: failed CDF samples (null rays), CDF samples
                                                   that chose sector 0, all CDF samples */
    uint64_t stat_tie, stat_eqprobe; /* last frame: CDF samples whose draw equals an entry of the sampled
                                        row, searches in which a probe met cdf[mid] == r */
    /* scene (copied) */
    int n_surf, n_light;
    float *tri, *albedo, *emission, *normal;
    int32_t *light_group;
} orc_sarsa;

static float lum3(const float *c) {
    float mx = c[0] > c[1] ? c[0] : c[1];
    mx = mx > c[2] ? mx : c[2];
    float mn = c[0] < c[1] ? c[0] : c[1];
    mn = mn < c[2] ? mn : c[2];
    return 0.5f * (mx + mn);
}

/* Triangle::compute_area: float lengths/cosine, 1 - pow(cos,2) and sqrt in double */
static float tri_area(const float *v) {
    v3 a = mk(v[3] - v[0], v[4] - v[1], v[5] - v[2]);
    v3 b = mk(v[6] - v[0], v[7] - v[1], v[8] - v[2]);
    float e = sqrtf(dot3(a, a)) * sqrtf(dot3(b, b));
    float c = dot3(a, b) / e;
    float s = (float)sqrt(1.0 - (double)c * (double)c);
    return 0.5f * e * s;
}

typedef struct { int dim; float median; int vol, left, right; } kd_sub;

static int kd_build(orc_sarsa *m, kd_sub *subs, int *n_subs, int32_t *v, int n, int dim) {
    int me = (*n_subs)++;
    subs[me].dim = dim;
    subs[me].vol = -1;
    subs[me].left = subs[me].right = -1;
    if (n == 1) {
        subs[me].median = m->pos[4 * v[0] + dim];
        subs[me].vol = v[0];
        return me;
    }
    orc_kd_sort(v, n, m->pos, dim);
    int mi;
    if (n % 2 == 0) {
        mi = n / 2 - 1;
        subs[me].median = (m->pos[4 * v[mi] + dim] + m->pos[4 * v[mi + 1] + dim]) / 2;
    } else {
        mi = n / 2;
        subs[me].median = m->pos[4 * v[mi] + dim];
    }
    int l = kd_build(m, subs, n_subs, v, mi + 1, (dim + 1) % 3);
    int r = kd_build(m, subs, n_subs, v + mi + 1, n - mi - 1, (dim + 1) % 3);
    subs[me].left = l;
    subs[me].right = r;
    return me;
}

/* traverse_and_insert: children appended as a pair, left subtree first */
static void kd_insert(orc_sarsa *m, const kd_sub *subs, int s, int slot) {
    int last = m->n_kd - 1;
    const kd_sub *u = &subs[s];
    if (u->vol >= 0) {
        orc_kd *e = &m->kd[slot];
        memset(e, 0, sizeof(*e));
        e->dim = u->dim; e->leaf = 1; e->data = (float)u->vol; e->vol = u->vol;
        e->px = m->pos[4 * u->vol]; e->py = m->pos[4 * u->vol + 1]; e->pz = m->pos[4 * u->vol + 2];
        e->nx = m->nrm[3 * u->vol]; e->ny = m->nrm[3 * u->vol + 1]; e->nz = m->nrm[3 * u->vol + 2];
        return;
    }
    m->kd[slot].left = last + 1;
    m->kd[slot].right = last + 2;
    orc_kd c;
    memset(&c, 0, sizeof(c));
    c.dim = (u->dim + 1) % 3;
    c.data = subs[u->left].median;
    m->kd[m->n_kd++] = c;
    c.data = subs[u->right].median;
    m->kd[m->n_kd++] = c;
    kd_insert(m, subs, u->left, last + 1);
    kd_insert(m, subs, u->right, last + 2);
}

/* RadianceMap::get_radiance_volumes_count / uniformly_sample_radiance_volumes
 * (GPU/radiance_volumes/radiance_map.cu:58-84): floor(area / AREA_PER_SAMPLE) volumes per surface;
 * AREA_PER_SAMPLE (radiance_volumes_settings.h:12, 0.001f) as an argument */
ORC_API orc_sarsa *orc_sarsa_create_density(const float *tri, const float *albedo, int n_surf, const float *emission,
                                            const int32_t *light_group, int n_light, uint64_t seed,
                                            float area_per_sample) {
    orc_sarsa *m = (orc_sarsa *)calloc(1, sizeof(orc_sarsa));
    int nt = n_surf + n_light;
    m->n_surf = n_surf; m->n_light = n_light; m->seed = seed;
    m->tri = (float *)malloc(sizeof(float) * 9 * (size_t)(nt + 1));
    memcpy(m->tri, tri, sizeof(float) * 9 * (size_t)nt);
    m->albedo = (float *)malloc(sizeof(float) * 3 * (size_t)(n_surf + 1));
    memcpy(m->albedo, albedo, sizeof(float) * 3 * (size_t)n_surf);
    m->emission = (float *)malloc(sizeof(float) * 3 * (size_t)(n_light + 1));
    memcpy(m->emission, emission, sizeof(float) * 3 * (size_t)n_light);
    m->light_group = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_light + 1));
    memcpy(m->light_group, light_group, sizeof(int32_t) * (size_t)n_light);
    m->normal = (float *)malloc(sizeof(float) * 3 * (size_t)(nt + 1));
    orc_triangle_normals(m->tri, nt, m->normal);
    /* count, then place */
    int n = 0;
    for (int j = 0; j < n_surf; j++) n += (int)floorf(tri_area(tri + 9 * j) / area_per_sample);
    m->n_vol = n;
    m->pos = (float *)malloc(sizeof(float) * 4 * (size_t)(n + 1));
    m->nrm = (float *)malloc(sizeof(float) * 3 * (size_t)(n + 1));
    m->surf = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int x = 0;
    for (int j = 0; j < n_surf; j++) {
        const float *v = tri + 9 * j;
        int cnt = (int)floorf(tri_area(v) / area_per_sample);
        for (int i = 0; i < cnt; i++, x++) {
            float a1, a2;
            uint32_t attempt = 0;
            do {
                uint32_t ctr[4] = {(uint32_t)x, attempt++, 0xFFFF0001u, 0u}, o[4];
                orc_philox4x32_10(ctr, key, o);
                a1 = u01(o[0]);
                a2 = u01(o[1]);
            } while (a1 + a2 > 1.0f);
            for (int c = 0; c < 3; c++)
                m->pos[4 * x + c] = (v[c] + a1 * (v[3 + c] - v[c])) + a2 * (v[6 + c] - v[c]);
            m->pos[4 * x + 3] = 1.0f;
            for (int c = 0; c < 3; c++) m->nrm[3 * x + c] = m->normal[3 * j + c];
            m->surf[x] = j;
        }
    }
    size_t nS = (size_t)n * 144 + 1;
    m->frame = (float *)malloc(sizeof(float) * 9 * (size_t)(n + 1));
    m->brdf = (float *)malloc(sizeof(float) * (size_t)(n + 1));
    m->cc = (float *)malloc(sizeof(float) * nS);
    m->ck = (float *)malloc(sizeof(float) * nS);
    m->Q = (float *)malloc(sizeof(float) * nS);
    m->cdf = (float *)malloc(sizeof(float) * nS);
    m->accum = (float *)malloc(sizeof(float) * (size_t)(n + 1));
    m->visits = (uint32_t *)calloc(nS, sizeof(uint32_t));
    m->cnt = (uint32_t *)calloc(nS, sizeof(uint32_t));
    m->sum = (int64_t *)calloc(nS, sizeof(int64_t));
    const float Q0 = (1.f / (12.0f * 12.0f)) * 100.f;
    for (int i = 0; i < n; i++) {
        v3 N = mk(m->nrm[3 * i], m->nrm[3 * i + 1], m->nrm[3 * i + 2]);
        v3 P = mk(m->pos[4 * i], m->pos[4 * i + 1], m->pos[4 * i + 2]);
        v3 T, B;
        normal_frame(N, &T, &B);
        float *f = m->frame + 9 * (size_t)i;
        f[0] = N.x; f[1] = N.y; f[2] = N.z; f[3] = T.x; f[4] = T.y; f[5] = T.z; f[6] = B.x; f[7] = B.y; f[8] = B.z;
        float lum = lum3(albedo + 3 * m->surf[i]);
        m->brdf[i] = lum / PI_F;
        float irr = 0.0f;
        for (int gx = 0; gx < 12; gx++)
            for (int gy = 0; gy < 12; gy++) {
                int k = gx * 12 + gy;
                size_t at = (size_t)i * 144 + k;
                m->cc[at] = dot3(grid_dir((float)gx + 0.5f, (float)gy + 0.5f, N, T, B, P), N);
                m->ck[at] = dot3(grid_dir((float)gx, (float)gy, N, T, B, P), N);
                m->Q[at] = Q0;
                m->cdf[at] = (float)k * (1.f / (12.0f * 12.0f));
                irr = (float)((double)irr + ((double)m->cc[at] * ((double)lum / 3.14159265358979323846)) * (double)Q0);
            }
        m->accum[i] = irr;
    }
    m->tri_lum = (float *)malloc(sizeof(float) * (size_t)(nt + 1));
    for (int j = 0; j < n_surf; j++) m->tri_lum[j] = lum3(albedo + 3 * j);
    for (int j = 0; j < n_light; j++) m->tri_lum[n_surf + j] = lum3(emission + 3 * j);
    if (n > 0) {
        int32_t *idx = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
        for (int i = 0; i < n; i++) idx[i] = i;
        kd_sub *subs = (kd_sub *)malloc(sizeof(kd_sub) * (size_t)(2 * n));
        int n_subs = 0;
        int root = kd_build(m, subs, &n_subs, idx, n, 0);
        m->kd = (orc_kd *)calloc((size_t)(2 * n), sizeof(orc_kd));
        m->kd[0].dim = subs[root].dim;
        m->kd[0].data = subs[root].median;
        m->n_kd = 1;
        kd_insert(m, subs, root, 0);
        free(subs);
        free(idx);
    }
    return m;
}

ORC_API orc_sarsa *orc_sarsa_create(const float *tri, const float *albedo, int n_surf, const float *emission,
                                    const int32_t *light_group, int n_light, uint64_t seed) {
    return orc_sarsa_create_density(tri, albedo, n_surf, emission, light_group, n_light, seed, 0.001f);
}

ORC_API void orc_sarsa_destroy(orc_sarsa *m) {
    if (!m) return;
    free(m->pos); free(m->nrm); free(m->surf); free(m->frame); free(m->brdf); free(m->cc); free(m->ck);
    free(m->Q); free(m->cdf); free(m->accum); free(m->visits); free(m->cnt); free(m->sum); free(m->kd);
    free(m->tri_lum); free(m->tri); free(m->albedo); free(m->emission); free(m->light_group); free(m->normal);
    free(m);
}

ORC_API void orc_sarsa_info(const orc_sarsa *m, int32_t *n_vol, int32_t *n_kd) {
    *n_vol = m->n_vol;
    *n_kd = m->n_kd;
}

/* kd_nodes: n_kd x 12 words, the layout of rt_sarsa_volumes */
ORC_API void orc_sarsa_volumes(const orc_sarsa *m, float *pos, float *nrm, int32_t *surf, void *kd_nodes) {
    for (int i = 0; i < m->n_vol; i++) {
        if (pos) memcpy(pos + 3 * i, m->pos + 4 * i, sizeof(float) * 3);
        if (nrm) memcpy(nrm + 3 * i, m->nrm + 3 * i, sizeof(float) * 3);
        if (surf) surf[i] = m->surf[i];
    }
    if (kd_nodes) memcpy(kd_nodes, m->kd, sizeof(orc_kd) * (size_t)m->n_kd);
}

ORC_API void orc_sarsa_read(const orc_sarsa *m, float *q, float *cdf, uint32_t *visits, float *accum) {
    size_t nS = (size_t)m->n_vol * 144;
    if (q) memcpy(q, m->Q, sizeof(float) * nS);
    if (cdf) memcpy(cdf, m->cdf, sizeof(float) * nS);
    if (visits) memcpy(visits, m->visits, sizeof(uint32_t) * nS);
    if (accum) memcpy(accum, m->accum, sizeof(float) * (size_t)m->n_vol);
}

static float dist3(float ax, float ay, float az, float bx, float by, float bz) {
    float x = ax - bx, y = ay - by, z = az - bz;
    return sqrtf((x * x + y * y) + z * z);
}

/* find_closest_radiance_volume_iterative */
static int sarsa_nearest(const orc_sarsa *m, v3 p, v3 nrm) {
    int best = 0;
    float best_d = dist3(p.x, p.y, p.z, m->kd[0].px, m->kd[0].py, m->kd[0].pz);
    int stack[64], sp = 0;
    stack[sp++] = 0;
    while (sp > 0) {
        const orc_kd *e = &m->kd[stack[--sp]];
        if (e->leaf) {
            float d = dist3(e->px, e->py, e->pz, p.x, p.y, p.z);
            if (nrm.x == e->nx && nrm.y == e->ny && nrm.z == e->nz && d < best_d) {
                best = (int)e->data;
                best_d = d;
            }
        } else {
            float pc = e->dim == 0 ? p.x : (e->dim == 1 ? p.y : p.z);
            float delta = pc - e->data;
            int near_split = (delta * delta) < 0.003f;
            if (sp + 2 > 64) break;
            if (delta < 0.0f) {
                if (near_split) stack[sp++] = e->right;
                stack[sp++] = e->left;
            } else {
                if (near_split) stack[sp++] = e->left;
                stack[sp++] = e->right;
            }
        }
    }
    return best;
}

ORC_API void orc_sarsa_nearest(const orc_sarsa *m, const float *pos, const float *nrm, int n, int32_t *out) {
    #pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++)
        out[i] = sarsa_nearest(m, mk(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]),
                               mk(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
}

/* sample_direction_from_radiance_distribution: 0 = no sector found */
static int sarsa_sample(orc_sarsa *m, int rv, float r, float rx, float ry, int *sector, v3 *dir, float *pdf) {
    const float *cdf = m->cdf + (size_t)rv * 144;
    const float RHO = 1.0f / (2.0f * 3.1415926535f);
    const float GRID_RHO = 1.0f / (12.0f * 12.0f);
    int found = -1;
    float dv = 0.0f;
    /* instrumentation only (orc_sarsa_search_stats): the draw equals an entry of the row */
    int tie = 0, eq_probe = 0;
    for (int k = 0; k < 144; k++) tie |= cdf[k] == r;
    if (r <= cdf[0]) {
        found = 0;
        dv = cdf[0];
    } else {
        int start = 0, end = 143;
        while (start <= end) {
            int mid = (end + start) / 2;
            float mv = cdf[mid], pv = mid > 0 ? cdf[mid - 1] : 0.0f;
            eq_probe |= mv == r;
            if (r < mv && pv <= r) { found = mid; dv = mv - pv; break; }
            else if (mv < r) start = mid + 1;
            else end = mid - 1;
        }
    }
    if (tie) {
        #pragma omp atomic
        m->stat_tie += 1u;
    }
    if (eq_probe) {
        #pragma omp atomic
        m->stat_eqprobe += 1u;
    }
    if (found < 0) return 0;
    int sx = found / 12, sy = found - sx * 12;
    *sector = found;
    *pdf = RHO * (dv / GRID_RHO);
    const float *f = m->frame + 9 * (size_t)rv;
    *dir = grid_dir((float)sx + rx, (float)sy + ry, mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), mk(f[6], f[7], f[8]),
                    mk(m->pos[4 * rv], m->pos[4 * rv + 1], m->pos[4 * rv + 2]));
    return 1;
}

/* sample_max_direction_from_radiance_distribution (radiance_volume.cu:246-278): the first
 * sector of largest Q (strict <, scanned from sector 0), uniform within it; pdf from the
 * CDF step of that sector, which is 0 for sector 0 (last_pdf = cdf[0] there, :274). */
static void sarsa_sample_max(const orc_sarsa *m, int rv, float rx, float ry, int *sector, v3 *dir, float *pdf) {
    const float *q = m->Q + (size_t)rv * 144, *cdf = m->cdf + (size_t)rv * 144;
    const float RHO = 1.0f / (2.0f * 3.1415926535f);
    const float GRID_RHO = 1.0f / (12.0f * 12.0f);
    int mi = 0;
    float mq = q[0];
    for (int i = 0; i < 144; i++)
        if (mq < q[i]) { mq = q[i]; mi = i; }
    int sx = mi / 12, sy = mi - sx * 12;
    *sector = mi;
    float last = mi == 0 ? cdf[mi] : cdf[mi - 1];
    *pdf = RHO * ((cdf[mi] - last) / GRID_RHO);
    const float *f = m->frame + 9 * (size_t)rv;
    *dir = grid_dir((float)sx + rx, (float)sy + ry, mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), mk(f[6], f[7], f[8]),
                    mk(m->pos[4 * rv], m->pos[4 * rv + 1], m->pos[4 * rv + 2]));
}

ORC_API void orc_sarsa_set_sampling(orc_sarsa *m, int mode) { m->sample_max = mode == 1; }

ORC_API void orc_sarsa_stats(const orc_sarsa *m, uint64_t *path_floor_sum, uint64_t *zero_paths) {
    *path_floor_sum = m->stat_paths;
    *zero_paths = m->stat_zero;
}

/* instrumentation of the last frame: CDF samples, failed ones (the null ray), sector 0 taken */
ORC_API void orc_sarsa_sample_stats(const orc_sarsa *m, uint64_t *cdf_samples, uint64_t *null_samples,
                                    uint64_t *sector0) {
    *cdf_samples = m->stat_cdf;
    *null_samples = m->stat_null;
    *sector0 = m->stat_sector0;
}

/* The reference's own rule, applied in place event by event (sequential restatement of
 * RadianceVolume::temporal_difference_update, radiance_volume.cu:282-301, and
 * expected_sarsa_irradiance, :93-112): alpha from the sector's visits, the running update
 * clamped at RADIANCE_THRESHOLD, visits + 1, the volume's irradiance moved by the sector's
 * change times its corner cosine and BRDF.  One event at a time in the render's fixed
 * order (orc_render_sarsa runs serially in this mode): the reference's atomics and races
 * reduced to one interleaving, so the rule has a deterministic expected image. */
static void td_inframe(orc_sarsa *m, int rv, int sector, float target) {
    const float thr = (1.f / (12.0f * 12.0f)) * 0.8f;
    size_t k = (size_t)rv * 144 + sector;
    uint32_t vs = m->visits[k];
    float alpha = 1.f / (1.f + (float)vs);
    float q_old = m->Q[k];
    float upd = ((1.f - alpha) * q_old) + (alpha * target);
    upd = upd > thr ? upd : thr;
    m->visits[k] = vs + 1u;
    float cc = m->ck[k], brdf = m->brdf[rv];
    m->accum[rv] = (m->accum[rv] - ((q_old * cc) * brdf)) + ((upd * cc) * brdf);
    m->Q[k] = upd;
}

/* more instrumentation of the last frame's CDF samples: those whose draw equals some entry of
 * the sampled row (ties), and the searches in which a probe met cdf[mid] == r */
ORC_API void orc_sarsa_search_stats(const orc_sarsa *m, uint64_t *ties, uint64_t *equal_probes) {
    *ties = m->stat_tie;
    *equal_probes = m->stat_eqprobe;
}

ORC_API void orc_sarsa_set_td_mode(orc_sarsa *m, int mode) { m->inframe = mode == 1; }

static void td_add(orc_sarsa *m, int rv, int sector, float target) {
    if (m->inframe) {
        td_inframe(m, rv, sector, target);
        return;
    }
    int64_t v = (int64_t)llrintf(target * 4294967296.0f);
    size_t k = (size_t)rv * 144 + sector;
    #pragma omp atomic
    m->sum[k] += v;
    #pragma omp atomic
    m->cnt[k] += 1u;
}

/* path_trace_reinforcement_iterative with the frame-synchronous TD */
/* *null_ray (may be NULL): set when the path ends by tracing the zero direction of a failed
 * CDF search, whose radiance is NaN in the reference ((BRDF * 0) / pdf 0,
 * reinforcement_path_tracing.cu:101-108): it is not a zero-contribution path there */
static v3 sarsa_trace(orc_sarsa *m, const orc_params *p, uint32_t pix, uint32_t smp, v3 o, v3 d, uint64_t *casts,
                      int *null_ray) {
    orc_scene sc;
    sc.n_surf = m->n_surf; sc.n_light = m->n_light; sc.tri = m->tri; sc.albedo = m->albedo;
    sc.emission = m->emission; sc.light_group = m->light_group; sc.normal = m->normal;
    const float RHO = 1.0f / (2.0f * 3.1415926535f);
    const float IRR = (2.f * PI_F) / ((float)(12 * 12));
    v3 tp = mk(1.0f, 1.0f, 1.0f);
    int cur_rv = -1, cur_sector = -1;
    float cur_brdf = 0.0f;
    uint32_t key[2] = {(uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
    for (int i = 0; i < p->max_bounces; i++) {
        hit_t h = closest_hit(&sc, o, d, p->t_scale, p->hit_rule);
        (*casts)++;
        int is_surf = h.tri >= 0 && h.tri < sc.n_surf;
        v3 pos = o, nrm = mk(0.0f, 0.0f, 0.0f);
        if (is_surf) {
            v3 D = mk(d.x * p->t_scale, d.y * p->t_scale, d.z * p->t_scale);
            pos = mk(o.x + h.t * D.x, o.y + h.t * D.y, o.z + h.t * D.z);
            nrm = mk(sc.normal[3 * h.tri], sc.normal[3 * h.tri + 1], sc.normal[3 * h.tri + 2]);
        }
        if (i > 0) {
            if (cur_rv >= 0 && cur_sector >= 0) {
                float target;
                int next = -1;
                if (h.tri < 0) target = cur_brdf * p->env_light;
                else if (!is_surf) target = cur_brdf * m->tri_lum[h.tri];
                else {
                    next = sarsa_nearest(m, pos, nrm);
                    target = (m->accum[next] * IRR) * cur_brdf;
                }
                td_add(m, cur_rv, cur_sector, target);
                cur_rv = next;
                cur_sector = -1;
            }
        } else if (is_surf) {
            cur_rv = sarsa_nearest(m, pos, nrm);
        }
        if (h.tri < 0) return mk(tp.x * p->env_light, tp.y * p->env_light, tp.z * p->env_light);
        if (!is_surf) {
            const float *e = sc.emission + (size_t)(h.tri - sc.n_surf) * 3;
            return mk(tp.x * e[0], tp.y * e[1], tp.z * e[2]);
        }
        uint32_t ctr[4] = {pix, smp, 1u + (uint32_t)i, 0u}, rn[4];
        orc_philox4x32_10(ctr, key, rn);
        v3 sd;
        float pdf;
        if (cur_rv < 0) {
            float ct;
            sd = sample_dir(nrm, u01(rn[0]), u01(rn[1]), 0, &ct);
            pdf = RHO;
        } else if (m->sample_max) {
            sarsa_sample_max(m, cur_rv, u01_oc(rn[1]), u01_oc(rn[2]), &cur_sector, &sd, &pdf);
        } else if (!sarsa_sample(m, cur_rv, u01_oc(rn[0]), u01_oc(rn[1]), u01_oc(rn[2]), &cur_sector, &sd, &pdf)) {
            #pragma omp atomic
            m->stat_null += 1u;
            #pragma omp atomic
            m->stat_cdf += 1u;
            if (i + 1 >= p->max_bounces) return mk(0.0f, 0.0f, 0.0f);
            (*casts)++; /* the zero direction is traced and misses */
            if (null_ray) *null_ray = 1;
            return mk(tp.x * p->env_light, tp.y * p->env_light, tp.z * p->env_light);
        }
        if (cur_rv >= 0 && !m->sample_max) {
            #pragma omp atomic
            m->stat_cdf += 1u;
            if (cur_sector == 0) {
                #pragma omp atomic
                m->stat_sector0 += 1u;
            }
        }
        const float *al = sc.albedo + (size_t)h.tri * 3;
        float cos_theta = dot3(nrm, sd);
        cur_brdf = m->tri_lum[h.tri] / PI_F;
        tp.x = tp.x * (((al[0] / PI_F) * cos_theta) / pdf);
        tp.y = tp.y * (((al[1] / PI_F) * cos_theta) / pdf);
        tp.z = tp.z * (((al[2] / PI_F) * cos_theta) / pdf);
        o = mk(pos.x + sd.x * 1e-5f, pos.y + sd.y * 1e-5f, pos.z + sd.z * 1e-5f);
        d = normalize3(sd);
    }
    return mk(0.0f, 0.0f, 0.0f);
}

/* update_radiance_distribution (radiance_volume.cu:148-188) of volume v */
static void sarsa_rebuild_cdf(orc_sarsa *m, int v) {
    size_t b = (size_t)v * 144;
    float total = 0.0000000001f;
    for (int k = 0; k < 144; k++) {
        float t = m->Q[b + k] * m->cc[b + k];
        t = t > 0.0f ? t : 0.0f;
        total += t;
    }
    float prev = 0.0f;
    for (int k = 0; k < 144; k++) {
        float t = m->Q[b + k] * m->cc[b + k];
        t = t > 0.0f ? t : 0.0f;
        float rad = t / total + prev;
        m->cdf[b + k] = rad;
        prev = rad;
    }
}

/* update_radiance_distribution + the frame's TD fold */
static void sarsa_apply(orc_sarsa *m) {
    const float thr = (1.f / (12.0f * 12.0f)) * 0.8f;
    #pragma omp parallel for schedule(static)
    for (int v = 0; v < m->n_vol; v++) {
        size_t b = (size_t)v * 144;
        float brdf = m->brdf[v], accum = m->accum[v];
        for (int k = 0; k < 144; k++) {
            uint32_t n = m->cnt[b + k];
            if (n == 0u) continue;
            float sum = (float)((double)m->sum[b + k] * 2.3283064365386962890625e-10);
            uint32_t vis = m->visits[b + k];
            float q_old = m->Q[b + k];
            float q_new = (q_old * (float)vis + sum) / (float)(vis + n);
            q_new = q_new > thr ? q_new : thr;
            float cc = m->ck[b + k];
            accum = (accum - ((q_old * cc) * brdf)) + ((q_new * cc) * brdf);
            m->Q[b + k] = q_new;
            m->visits[b + k] = vis + n;
            m->cnt[b + k] = 0u;
            m->sum[b + k] = 0;
        }
        m->accum[v] = accum;
        sarsa_rebuild_cdf(m, v);
    }
}

/* The fold on host arrays (rt_sarsa_write's visits, the pending sums and counts of
 * rt_sarsa_td_device, rt_sarsa_apply): visits, sums, counts are n_vol x 144 */
ORC_API void orc_sarsa_set_visits(orc_sarsa *m, const uint32_t *visits) {
    memcpy(m->visits, visits, sizeof(uint32_t) * (size_t)m->n_vol * 144);
}

ORC_API void orc_sarsa_set_pending(orc_sarsa *m, const int64_t *sums, const uint32_t *counts) {
    memcpy(m->sum, sums, sizeof(int64_t) * (size_t)m->n_vol * 144);
    memcpy(m->cnt, counts, sizeof(uint32_t) * (size_t)m->n_vol * 144);
}

ORC_API void orc_sarsa_apply(orc_sarsa *m) { sarsa_apply(m); }

/* Q-table loader (rt_sarsa_load_q): Q from radiance_map_data.txt values, the irradiance
 * estimate of initialise_radiance_grid (radiance_volume.cu:46-63) over that Q, the CDF of
 * update_radiance_distribution; visits kept. */
ORC_API void orc_sarsa_load_q(orc_sarsa *m, const float *q) {
    memcpy(m->Q, q, sizeof(float) * (size_t)m->n_vol * 144);
    for (int v = 0; v < m->n_vol; v++) {
        size_t b = (size_t)v * 144;
        float lum = lum3(m->albedo + 3 * m->surf[v]);
        float irr = 0.0f;
        for (int k = 0; k < 144; k++)
            irr = (float)((double)irr + ((double)m->cc[b + k] * ((double)lum / 3.14159265358979323846)) *
                                            (double)m->Q[b + k]);
        m->accum[v] = irr;
        sarsa_rebuild_cdf(m, v);
    }
}

/* The TD accumulators one rectangle of the current frame adds (the frame is not applied):
 * out_sum/out_cnt get this rectangle's n_vol x 144 fixed-point target sums and counts, and
 * the map's accumulators are cleared again.  The rectangles of a frame's tiles add up to the
 * whole frame's accumulators (the multi-GPU exchange, rtmi.dist.sum_td). */
ORC_API int orc_sarsa_td_rect(orc_sarsa *m, const orc_camera *cam, const orc_params *p, int x0, int y0, int w,
                              int h, int64_t *out_sum, uint32_t *out_cnt) {
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    orc_params pg = *p;
    pg.preset = 1;
    uint32_t base = m->frames * (uint32_t)p->spp;
    uint64_t total = 0;
    #pragma omp parallel for schedule(dynamic, 1) reduction(+:total)
    for (int py = y0; py < y0 + h; py++) {
        for (int px = x0; px < x0 + w; px++) {
            uint32_t pix = (uint32_t)py * (uint32_t)p->width + (uint32_t)px;
            uint64_t casts = 0;
            for (int s = 0; s < p->spp; s++) {
                float r1, r2;
                draw2(p->seed, pix, base + (uint32_t)s, 0u, &r1, &r2);
                v3 o, d;
                camera_ray(cam, &pg, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
                (void)sarsa_trace(m, p, pix, base + (uint32_t)s, o, d, &casts, NULL);
            }
            total += casts;
        }
    }
    size_t n = (size_t)m->n_vol * 144;
    memcpy(out_sum, m->sum, sizeof(int64_t) * n);
    memcpy(out_cnt, m->cnt, sizeof(uint32_t) * n);
    memset(m->sum, 0, sizeof(int64_t) * n);
    memset(m->cnt, 0, sizeof(uint32_t) * n);
    return (int)(total > 0);
}

/* One frame's rectangle (x0, y0, w, h) of the width x height image (GPU-engine preset) into
 * out_rgb (w x h x 3, may be NULL): pixels row by row, each pixel's chunks in order (OpenMP
 * over rows; one thread in the in-frame TD mode).  The frame's TD is accumulated (or applied
 * in place, in-frame mode) but not folded; *paths / *zero: the frame statistics. */
static uint64_t sarsa_frame_rect(orc_sarsa *m, const orc_camera *cam, const orc_params *p, int x0, int y0, int w,
                                 int h, float *out_rgb, uint64_t *paths_out, uint64_t *zero_out) {
    float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    orc_params pg = *p;
    pg.preset = 1;
    uint64_t total = 0, paths = 0, zero = 0;
    int W = p->width;
    int S = p->spp_split <= 0 ? 1 : p->spp_split;
    int per = p->spp / S;
    uint32_t base = m->frames * (uint32_t)p->spp;
    m->stat_null = m->stat_sector0 = m->stat_cdf = 0;
    m->stat_tie = m->stat_eqprobe = 0;
    /* in-frame TD: one thread, pixels row by row, each pixel's chunks and samples in order */
    #pragma omp parallel for schedule(dynamic, 1) reduction(+:total, paths, zero) if(!m->inframe)
    for (int py = y0; py < y0 + h; py++) {
        for (int px = x0; px < x0 + w; px++) {
            uint32_t pix = (uint32_t)py * (uint32_t)W + (uint32_t)px;
            v3 acc = mk(0.0f, 0.0f, 0.0f);
            uint64_t casts = 0;
            for (int c = 0; c < S; c++) {
                v3 part = mk(0.0f, 0.0f, 0.0f);
                for (int s = c * per; s < (c + 1) * per; s++) {
                    float r1, r2;
                    draw2(p->seed, pix, base + (uint32_t)s, 0u, &r1, &r2);
                    v3 o, d;
                    camera_ray(cam, &pg, cy, sy, cx, sx, px, py, r1, r2, &o, &d);
                    int null_ray = 0;
                    v3 L = sarsa_trace(m, p, pix, base + (uint32_t)s, o, d, &casts, &null_ray);
                    part.x = part.x + L.x; part.y = part.y + L.y; part.z = part.z + L.z;
                    /* path_trace_reinforcement (reinforcement_path_tracing.cu:28-41): a
                     * zero-contribution path (a NaN one, null_ray, is not); its path length is
                     * its ray casts */
                    if (!null_ray && (L.x + L.y + L.z) / 3.f < 0.0001f) zero++;
                }
                if (c == 0) acc = part;
                else { acc.x = acc.x + part.x; acc.y = acc.y + part.y; acc.z = acc.z + part.z; }
            }
            if (out_rgb) {
                float fs = (float)p->spp;
                float *dst = out_rgb + ((size_t)(py - y0) * w + (px - x0)) * 3;
                dst[0] = acc.x / fs; dst[1] = acc.y / fs; dst[2] = acc.z / fs;
            }
            total += casts;
            paths += casts / (uint64_t)p->spp; /* int(total_path_lengths / SAMPLES_PER_PIXEL) */
        }
    }
    *paths_out = paths;
    *zero_out = zero;
    return total;
}

/* `frames` frames of the whole width x height image (GPU-engine preset); out_rgb = last frame */
ORC_API int orc_render_sarsa(orc_sarsa *m, const orc_camera *cam, const orc_params *p, int frames, float *out_rgb,
                             uint64_t *out_casts) {
    uint64_t total = 0;
    for (int f = 0; f < frames; f++) {
        uint64_t paths = 0, zero = 0;
        total += sarsa_frame_rect(m, cam, p, 0, 0, p->width, p->height, out_rgb, &paths, &zero);
        m->stat_paths = paths;
        m->stat_zero = zero;
        sarsa_apply(m);
        m->frames++;
    }
    if (out_casts) *out_casts = total;
    return 0;
}

/* A rectangle of the current frame, not applied (the map is left as it was, apart from the
 * in-frame mode's in-place updates): the bounded CPU-baseline sample of bench.py. */
ORC_API int orc_render_sarsa_rect(orc_sarsa *m, const orc_camera *cam, const orc_params *p, int x0, int y0, int w,
                                  int h, float *out_rgb, uint64_t *out_casts) {
    uint64_t paths = 0, zero = 0;
    uint64_t total = sarsa_frame_rect(m, cam, p, x0, y0, w, h, out_rgb, &paths, &zero);
    size_t n = (size_t)m->n_vol * 144;
    memset(m->sum, 0, sizeof(int64_t) * n);
    memset(m->cnt, 0, sizeof(uint32_t) * n);
    if (out_casts) *out_casts = total;
    return 0;
}

/* ================================================================== */
/* Neural-Q TD targets                        */
/* ================================================================== */
/* compute_td_targets (GPU/deep_learning/nn_rendering_helpers.cu:91-140): target =
 * reward + max_a(Q(s',a) cos_a) * discount (reward alone when terminal == 1); the max starts
 * at the raw Q of action 0 and weights actions 1.. by the cosine of a jittered direction in
 * their cell (here the Chiu map's cos with the sampler's Philox jitters: counter
 * (pix, sample, 1 + bounce, 1 + a/2)), as rt_dqn_td_targets_device. */
static void td_targets_ev(uint64_t seed, const float *next_q, const int32_t *terminal, const float *reward,
                          const float *discount, const uint32_t *pix, uint32_t sample, uint32_t ev, int n,
                          float *target) {
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int b = 0; b < n; b++) {
        if (terminal[b] == 1) { target[b] = reward[b]; continue; }
        const float *q = next_q + (size_t)b * 144;
        float best = q[0];
        for (int a2 = 0; a2 < 144; a2 += 2) {
            uint32_t ctr[4] = {pix[b], sample, ev, 1u + (uint32_t)(a2 >> 1)};
            uint32_t o[4];
            orc_philox4x32_10(ctr, key, o);
            for (int h = 0; h < 2; h++) {
                int a = a2 + h;
                if (a == 0) continue;
                int gxi = a / 12, gyi = a - gxi * 12;
                float c = chiu_cos((float)gxi + u01(o[2 * h]), (float)gyi + u01(o[2 * h + 1]));
                float t = q[a] * c;
                if (best < t) best = t;
            }
        }
        target[b] = reward[b] + best * discount[b];
    }
}

ORC_API void orc_td_targets(uint64_t seed, const float *next_q, const int32_t *terminal, const float *reward,
                            const float *discount, const uint32_t *pix, int sample, int bounce, int n,
                            float *target) {
    td_targets_ev(seed, next_q, terminal, reward, discount, pix, (uint32_t)sample, 1u + (uint32_t)bounce, n, target);
}

/* ================================================================== */
/* Neural-Q training frame                                             */
/* ================================================================== */
/* NeuralQPathtracer::render_frame (GPU/deep_learning/neural_q_pathtracer.cu:226-600) in the
 * reference's per-ray arrays, one ray per pixel (id = y * width + x), in its order:
 *   per sample: initialise_ray (:604-643);
 *     per bounce b: (b > 0) Q of every ray's position, then sample_batch_ray_directions_epsilon_greedy
 *       (nn_rendering_helpers.cu:330-389): greedy rows importance_sample_direction (dqn_sample; a
 *       row whose Q admits no cell keeps its direction and takes action 0), explore rows a
 *       uniformly chosen jittered cell; trace_ray (:646-745; GPU hit rule; throughput, path length
 *       and the rays_finished flag only for paths still contributing, state 0); (b > 0) per batch
 *       of `batch` rays the learning rule (:420-513): Q at the new positions, compute_td_targets,
 *       trainer.update on the positions before the trace and the sampled actions;
 *       sample_random_scene_pos_for_terminated_rays (nn_rendering_helpers.cu:241-277: the new
 *       position stored with y and z exchanged, state 2); leave the loop once no path bounced;
 *     update_total_throughput, sum_path_lengths, sum_zero_contribution_light_paths; epsilon decays;
 *   update_device_buffer: total / spp.
 * The network is not evaluated here.  q_fn(loc, n, q) returns Q [n][144] of n positions and
 * step_fn(prev, action, target, n) runs one update and returns its loss; they are called exactly
 * where the reference evaluates and updates its network: q_fn once over all rays before
 * sampling, then per batch q_fn on the batch's new positions followed by step_fn.
 * The state the update trains on.  The reference is built with TRAIN_ON_POSITION false
 * (constants/deep_learning_settings.h:10): the network's input is the scene's vertices in the
 * ray's coordinate system, ray_vertices = vertices - ray_locations
 * (convert_vertices_to_point_coord_system, nn_rendering_helpers.cu:281-298), which is also this
 * project's network input (nn_vertices - loc).  ray_vertices is converted at the top of the
 * bounce (:292), from every ray's position before the trace, and copied to prev_ray_vertices after
 * the trace (:405-408); trainer.update reads prev_ray_vertices (:487-489).  So S_t is the position
 * before the trace for every ray, whether the trace ends on a surface, a light or nothing:
 * `prev` below, set for every ray.  prev_ray_locations, which trace_ray writes on surface hits
 * only (:714-716), is read only under TRAIN_ON_POSITION true (:482-485), a build the reference
 * does not ship and whose 3-input network this project does not have; variant 5 restates that
 * array instead, as a control that the comparison tells the two apart.
 * Conventions of this project that the restatement adopts where the reference's own cannot be
 * reproduced or differ without effect on the algorithm: the ray id is
 * y * width + x (the reference: SCREEN_HEIGHT * x + y, its pixel-to-thread map); a sample's loss
 * is summed over the batches in double and rounded to float once (the reference adds floats,
 * :276, :508); a restart's rejection loop stops after 64 attempts and then mirrors the point
 * into the triangle (Triangle::sample_position_on_plane loops without a bound; 2^-64); the random
 * numbers are Philox draws keyed as follows, not cuRAND's.
 * Philox events (pixel, frame * spp + sample, event, counter): 0 the camera jitter, 1 + b the
 * greedy sampler, 0x1000 + b the epsilon draw (word 0, (0, 1]) and the exploration cell (word 1)
 * and its jitters (words 2, 3), 0x2000 + b a restart's surface, 0x3000 + b (counter = attempt) its
 * point, 0x4000 + b the targets' cell jitters.
 * variant (negative controls of the tests; 0 = the algorithm): 1 the targets draw from event
 * 1 + b; 2 the restart position without the y/z exchange; 3 throughput also updated for
 * restarted rays (state 2); 4 next-state Q of every batch taken before the bounce's first update;
 * 5 the update's state taken from prev_ray_locations (written on surface hits only).
 * counters [8]: greedy rows, explore rows, greedy rows with no selectable cell, misses, light
 * hits, restarts, second restarts of a ray within a sample, rays still live after the last
 * bounce of a sample. */
typedef float (*orc_step_fn)(const float *prev, const int32_t *action, const float *target, int n, void *user);

ORC_API int orc_neuralq_frame(const float *tri, const float *albedo, int n_surf, const float *emission,
                              const int32_t *light_group, int n_light, const orc_camera *cam,
                              const orc_params *p, int batch, int frame, float *eps_io, float eps_min,
                              float eps_decay, orc_q_fn q_fn, orc_step_fn step_fn, void *user, int variant,
                              float *out_rgb, float *stats, uint64_t *out_casts, float *o_loc, float *o_tp,
                              float *o_total, int32_t *o_tri, uint32_t *o_state, uint32_t *o_bounces,
                              int32_t *o_action, float *o_reward, float *o_discount, int32_t *o_terminal,
                              uint64_t *counters) {
    if (batch <= 0 || p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->max_bounces < 1 || n_surf <= 0) return -1;
    orc_scene sc;
    scene_init(&sc, tri, albedo, n_surf, emission, light_group, n_light);
    const float cy = (float)cos((double)cam->yaw_y), sy = (float)sin((double)cam->yaw_y);
    const float cx = (float)cos((double)cam->yaw_x), sx = (float)sin((double)cam->yaw_x);
    const int n = p->width * p->height;
    const uint32_t key[2] = {(uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
    const float RHO = 1.0f / (2.0f * 3.1415926535f);
    float *lum = (float *)malloc(sizeof(float) * (size_t)(n_surf + n_light));
    for (int j = 0; j < n_surf; j++) lum[j] = lum3(albedo + 3 * (size_t)j);
    for (int j = 0; j < n_light; j++) lum[n_surf + j] = lum3(emission + 3 * (size_t)j);
    float *prev = (float *)malloc(sizeof(float) * 3 * (size_t)n), *dir = (float *)malloc(sizeof(float) * 3 * (size_t)n);
    float *q = (float *)malloc(sizeof(float) * 144 * (size_t)n), *target = (float *)malloc(sizeof(float) * (size_t)n);
    uint32_t *pix = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    int *restarts = (int *)malloc(sizeof(int) * (size_t)n);
    float *loc = o_loc, *tp = o_tp, *total = o_total, *reward = o_reward, *discount = o_discount;
    int32_t *rtri = o_tri, *action = o_action, *terminal = o_terminal;
    uint32_t *state = o_state, *bounces = o_bounces;
    uint64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, casts = 0;
    float eps = *eps_io;
    for (int i = 0; i < 3 * n; i++) total[i] = 0.0f;
    for (int i = 0; i < n; i++) terminal[i] = 0;
    const uint32_t base = (uint32_t)frame * (uint32_t)p->spp;
    for (int s = 0; s < p->spp; s++) {
        const uint32_t smp = base + (uint32_t)s;
        double loss = 0.0;
        for (int i = 0; i < n; i++) {
            float r1, r2;
            draw2(p->seed, (uint32_t)i, smp, 0u, &r1, &r2);
            v3 o, d;
            orc_params pg = *p;
            pg.preset = 1;
            camera_ray(cam, &pg, cy, sy, cx, sx, i % p->width, i / p->width, r1, r2, &o, &d);
            loc[3 * i] = prev[3 * i] = o.x; loc[3 * i + 1] = prev[3 * i + 1] = o.y; loc[3 * i + 2] = prev[3 * i + 2] = o.z;
            dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
            tp[3 * i] = tp[3 * i + 1] = tp[3 * i + 2] = 1.0f;
            rtri[i] = -1;
            state[i] = 0u;
            reward[i] = 0.0f;
            discount[i] = 1.0f;
            bounces[i] = (uint32_t)p->max_bounces;
            action[i] = 0;
            pix[i] = (uint32_t)i;
            restarts[i] = 0;
        }
        for (int b = 0; b < p->max_bounces; b++) {
            if (b > 0) {
                q_fn(loc, n, q, user);
                for (int i = 0; i < n; i++) {
                    const float *nn = sc.normal + (size_t)rtri[i] * 3;
                    const v3 N = mk(nn[0], nn[1], nn[2]);
                    const v3 pos = mk(loc[3 * i], loc[3 * i + 1], loc[3 * i + 2]);
                    v3 t = mk(tp[3 * i], tp[3 * i + 1], tp[3 * i + 2]);
                    const int upd = state[i] == 0u || (variant == 3 && state[i] == 2u);
                    uint32_t ctr[4] = {pix[i], smp, 0x1000u + (uint32_t)b, 0u}, o[4];
                    orc_philox4x32_10(ctr, key, o);
                    if (u01_oc(o[0]) > eps) {
                        v3 tn = t, d;
                        const int act = dqn_sample(q + (size_t)i * 144, N, pos, p->seed, pix[i], smp, 1u + (uint32_t)b,
                                                   &tn, &d);
                        cnt[0]++;
                        if (act >= 0) {
                            dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
                            action[i] = act;
                            if (upd) t = tn;
                        } else {
                            action[i] = 0;
                            cnt[2]++;
                        }
                    } else {
                        const float u = u01_oc(o[1]) - 0.0001f;
                        int idx = (int)(u * 144.0f);
                        idx = idx < 0 ? 0 : (idx > 143 ? 143 : idx);
                        const int gx = idx / 12, gy = idx - gx * 12;
                        v3 T, B;
                        normal_frame(N, &T, &B);
                        const v3 d = grid_dir((float)gx + u01(o[2]), (float)gy + u01(o[3]), N, T, B, pos);
                        if (upd) {
                            const float c = dot3(N, d);
                            t = mk((t.x * c) / RHO, (t.y * c) / RHO, (t.z * c) / RHO);
                        }
                        dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
                        action[i] = idx;
                        cnt[1]++;
                    }
                    tp[3 * i] = t.x; tp[3 * i + 1] = t.y; tp[3 * i + 2] = t.z;
                }
            }
            int finished = 1;
            for (int i = 0; i < n; i++) {
                const v3 pos = mk(loc[3 * i], loc[3 * i + 1], loc[3 * i + 2]);
                const v3 dr = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
                const v3 o = mk(pos.x + dr.x * 1e-5f, pos.y + dr.y * 1e-5f, pos.z + dr.z * 1e-5f);
                const v3 d = normalize3(dr);
                const hit_t h = closest_hit(&sc, o, d, p->t_scale, 1);
                casts++;
                /* S_t of the update: the position the ray's vertices were converted at (see above) */
                if (variant != 5 || (h.tri >= 0 && h.tri < n_surf)) {
                    prev[3 * i] = pos.x; prev[3 * i + 1] = pos.y; prev[3 * i + 2] = pos.z;
                }
                const uint32_t st = state[i];
                const int upd = st == 0u || (variant == 3 && st == 2u);
                v3 t = mk(tp[3 * i], tp[3 * i + 1], tp[3 * i + 2]);
                if (h.tri < 0 || h.tri >= n_surf) {
                    const int light = h.tri >= 0;
                    cnt[light ? 4 : 3]++;
                    reward[i] = light ? lum[h.tri] * 200.0f : 0.0f;
                    discount[i] = 0.0f;
                    if (upd) {
                        if (light) {
                            const float *e = emission + (size_t)(h.tri - n_surf) * 3;
                            t = mk(t.x * e[0], t.y * e[1], t.z * e[2]);
                        } else {
                            t = mk(t.x * p->env_light, t.y * p->env_light, t.z * p->env_light);
                        }
                    }
                    if (st == 0u) bounces[i] = (uint32_t)b;
                    state[i] = 1u;
                    terminal[i] = 1;
                } else {
                    const v3 D = mk(d.x * p->t_scale, d.y * p->t_scale, d.z * p->t_scale);
                    loc[3 * i] = o.x + h.t * D.x; loc[3 * i + 1] = o.y + h.t * D.y; loc[3 * i + 2] = o.z + h.t * D.z;
                    rtri[i] = h.tri;
                    if (upd) {
                        const float *al = albedo + (size_t)h.tri * 3;
                        t = mk(t.x * (al[0] / PI_F), t.y * (al[1] / PI_F), t.z * (al[2] / PI_F));
                    }
                    if (st == 0u) finished = 0;
                    reward[i] = 0.0f;
                    discount[i] = lum[h.tri];
                    terminal[i] = 0;
                }
                tp[3 * i] = t.x; tp[3 * i + 1] = t.y; tp[3 * i + 2] = t.z;
            }
            if (b > 0) {
                const uint32_t ev = variant == 1 ? 1u + (uint32_t)b : 0x4000u + (uint32_t)b;
                if (variant == 4) q_fn(loc, n, q, user);
                for (int b0 = 0; b0 < n; b0 += batch) {
                    const int nb = batch < n - b0 ? batch : n - b0;
                    float *qb = q + (size_t)b0 * 144;
                    if (variant != 4) q_fn(loc + 3 * (size_t)b0, nb, qb, user);
                    td_targets_ev(p->seed, qb, terminal + b0, reward + b0, discount + b0, pix + b0, smp, ev, nb,
                                  target + b0);
                    loss += (double)step_fn(prev + 3 * (size_t)b0, action + b0, target + b0, nb, user);
                }
            }
            for (int i = 0; i < n; i++) {
                if (state[i] != 1u) continue;
                uint32_t ctr[4] = {pix[i], smp, 0x2000u + (uint32_t)b, 0u}, o[4];
                orc_philox4x32_10(ctr, key, o);
                int sf = (int)((float)n_surf * u01_oc(o[0]));
                sf = sf < n_surf ? sf : n_surf - 1;
                const float *v = tri + (size_t)sf * 9;
                float a1, a2;
                uint32_t attempt = 0;
                ctr[2] = 0x3000u + (uint32_t)b;
                do {
                    ctr[3] = attempt++;
                    orc_philox4x32_10(ctr, key, o);
                    a1 = u01_oc(o[0]);
                    a2 = u01_oc(o[1]);
                } while (a1 + a2 > 1.0f && attempt < 64u);
                if (a1 + a2 > 1.0f) { a1 = 1.0f - a1; a2 = 1.0f - a2; }
                float pt[3];
                for (int c = 0; c < 3; c++) pt[c] = (v[c] + a1 * (v[3 + c] - v[c])) + a2 * (v[6 + c] - v[c]);
                loc[3 * i] = pt[0];
                loc[3 * i + 1] = variant == 2 ? pt[1] : pt[2];
                loc[3 * i + 2] = variant == 2 ? pt[2] : pt[1];
                rtri[i] = sf;
                state[i] = 2u;
                cnt[5]++;
                if (++restarts[i] == 2) cnt[6]++;
            }
            if (finished) break;
        }
        uint64_t sum_b = 0, zero = 0;
        for (int i = 0; i < n; i++) {
            for (int c = 0; c < 3; c++) total[3 * i + c] = total[3 * i + c] + tp[3 * i + c];
            sum_b += bounces[i];
            if (tp[3 * i] < 0.0001f && tp[3 * i + 1] < 0.0001f && tp[3 * i + 2] < 0.0001f) zero++;
            if (state[i] == 0u) cnt[7]++;
        }
        const float dec = eps - eps_decay;
        eps = dec > eps_min ? dec : eps_min;
        if (stats) {
            stats[3 * s + 0] = (float)sum_b / ((float)p->height * (float)p->width);
            stats[3 * s + 1] = (float)loss;
            stats[3 * s + 2] = (float)zero;
        }
    }
    const float fs = (float)p->spp;
    if (out_rgb)
        for (int i = 0; i < 3 * n; i++) out_rgb[i] = total[i] / fs;
    *eps_io = eps;
    if (out_casts) *out_casts = casts;
    if (counters) memcpy(counters, cnt, sizeof(cnt));
    free(lum); free(prev); free(dir); free(q); free(target); free(pix); free(restarts);
    free(sc.normal);
    return 0;
}
