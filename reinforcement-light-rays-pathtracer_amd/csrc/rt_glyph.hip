// rt_glyph.hip — radiance-volume glyphs (the "radiance-volume glyphs" section of rtmi.h): the
// picture the reference judges a radiance map or a Q-network with.  Selected surface points are
// each drawn as a hemisphere of 12 x 12 coloured sectors inside the scene
// (RENDER_SAVED_RADIANCE_VOLUMES, GPU/constants/image_settings.h:15;
// RadianceVolume::read_radiance_volumes_to_surfaces, GPU/radiance_volumes/radiance_volume.cu:375-515;
// the CPU engine's build_radiance_volume_shapes / build_radiance_magnitude_volume_shapes,
// CPU/radiance_volumes/radiance_volume.cpp:100-174).
//
// The reference appends the glyphs' 288 diffuse triangles per volume to the scene, overwrites
// their normals by hand and path traces everything.  Here the glyphs are an overlay: the mesh
// lives in a triangle soup of its own with its own exact BVH (rt_bvh.cpp), k_glyph_view casts
// each camera ray against the scene and against that soup, and the unlit sector colours are
// composited over a base frame.  The scene, its tables and the glyph set are read only.
//
// Host side (no GPU): the mesh (glyph_mesh = get_vertices + build_surfaces) and the sector
// colours (glyph_colours).  The file reader is rt_selected_read (rt_sarsa_host.cpp, the Q-table
// parser).
//
// k_glyph_view: the camera-hit frame of rt_view.hpp (one lane per (pixel, chunk), a wave over
// 16 x 4 pixels at split 1, the shuffle fold of the chunk sums) and k_probe's LDS stack column for
// the BVH walks.  Per sample two casts of the same camera ray -- the scene's (the frame's routes:
// the rectangle cull or the scan; the scene's BVH where its accel mode turns it on) and the
// glyph soup's (its BVH, or the plain scan: RTMI_GLYPH_BVH=0) -- and the winner rule of the
// scan over the soup "scene surfaces, glyph triangles, lights".  Every route gives the same
// hits bit for bit, so a pixel does not depend on it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtmi.h"
#include "rt_hostframe.hpp"
#include "rt_view.hpp"

namespace rt {
namespace {

static_assert(kGlyphSectors == RT_GLYPH_SECTORS && kGlyphTris == RT_GLYPH_TRIS && kGlyphSectors == kGridRes * kGridRes,
              "a glyph is the 12 x 12 grid, two triangles per sector");

// The view: see the head of the file.  SBVH / GBVH: the scene's / the glyph soup's cast takes
// the exact BVH (closest_hit_bvh, its stack in the lane's LDS column; the two walks run one
// after the other and share it).  cull: the scene's cast takes the cull of the wave's pixel
// rectangle (launch_glyph_view: view_cull_wanted).  The lane layout, the trips and the fold are
// rt_view.hpp's.
// out_tri / out_glyph / out_sector / out_t (each may be null): the scene's own hit (-1: miss),
// the winning glyph and its sector (-1: no glyph won) and the winner's t (+inf: a miss) of
// sample a.sample_base, by output pixel.
template <bool SBVH, bool GBVH>
__global__ __launch_bounds__(256) void k_glyph_view(const RenderLaunch a, const GlyphSet g, int cull,
                                                    int32_t* __restrict__ out_tri, int32_t* __restrict__ out_glyph,
                                                    int32_t* __restrict__ out_sector, float* __restrict__ out_t) {
    __shared__ int s_stk[(SBVH || GBVH) ? kBvhMaxDepth * 256 : 1];
    ViewLane v;
    if (!view_lane(a, &v)) return;
    const float4* __restrict__ shade = a.scene.shade;
    const int n_surf = a.scene.n_surf;
    int* const stk = s_stk + ((SBVH || GBVH) ? (int)threadIdx.x : 0);
    const f3 o = make3(a.cam_x, a.cam_y, a.cam_z);
    uint64_t cm[kRenderCullWords];
    view_cull<1>(a, v, !SBVH && cull, cm);
    // what the pixel shows where no glyph wins and a base was given (the same for every sample)
    f3 base = make3(0.f, 0.f, 0.f);
    if (v.valid && g.base != nullptr) {
        const float* b = g.base + (size_t)v.pix * 3;
        base = make3(b[0], b[1], b[2]);
    }
    view_frame(a, v, [&](int s, bool first) {
        f3 d;
        const Hit hs = view_camera_hit<1, SBVH>(a, v, s, cull, cm, o, stk, &d);
        Hit hg;
        hg.t = 0.0f;
        hg.tri = -1;
        if (v.valid) {
            if constexpr (GBVH)
                hg = closest_hit_bvh<1>(g.soup, o, d, a.t_scale, stk);
            else
                hg = closest_hit<1>(g.soup.isect, g.soup.n_tri, o, d, a.t_scale);
        }
        // the scan over "surfaces, glyph triangles, lights" keeps the first triangle of least t
        const bool gwin = (hg.tri >= 0) && ((hs.tri < 0) || (hg.t < hs.t) || ((hg.t == hs.t) && (hs.tri >= n_surf)));
        f3 c = make3(0.f, 0.f, 0.f);
        if (gwin) {
            const int qd = hg.tri >> 1;  // glyph * 144 + sector
            const float4 col = g.colour[qd];
            c = make3(col.x, col.y, col.z);
            if (g.shade) {
                const float4 nq = g.qnormal[qd];
                const float f = 0.25f + 0.75f * fmaxf(-((nq.x * d.x + nq.y * d.y) + nq.z * d.z), 0.f);
                c = make3(c.x * f, c.y * f, c.z * f);
            }
        } else if (v.valid) {
            if (g.base != nullptr) {
                c = base;
            } else if (hs.tri < 0) {
                c = make3(a.env_light, a.env_light, a.env_light);
            } else {  // a surface's albedo, a light's emission
                const float4 e = shade[hs.tri * kShadeF4 + (hs.tri < n_surf ? 4 : 3)];
                c = make3(e.x, e.y, e.z);
            }
        }
        if (first) {
            const size_t op = v.op(a);
            view_write_tri(op, out_tri, hs.tri);
            if (out_glyph != nullptr) out_glyph[op] = gwin ? hg.tri / kGlyphTris : -1;
            if (out_sector != nullptr) out_sector[op] = gwin ? (hg.tri % kGlyphTris) >> 1 : -1;
            if (out_t != nullptr) out_t[op] = gwin ? hg.t : (hs.tri >= 0 ? hs.t : __builtin_inff());
        }
        return c;
    });
}

}  // namespace

// the scene's camera rays take the rectangle cull where view_cull_wanted says, or the
// scene's BVH when the launch's view of the scene carries one
hipError_t launch_glyph_view(const RenderLaunch& a, const GlyphSet& g, int32_t* out_tri, int32_t* out_glyph,
                             int32_t* out_sector, float* out_t, hipStream_t stream) {
    if (a.n_blocks <= 0) return hipSuccess;
    if (a.out == nullptr || a.hit_rule != 1) return hipErrorInvalidValue;
    if (g.soup.n_tri > 0 && (g.soup.isect == nullptr || g.colour == nullptr || g.qnormal == nullptr))
        return hipErrorInvalidValue;
    if (!view_split_ok(a)) return hipErrorInvalidValue;
    const bool sbvh = a.scene.bvh_nodes != nullptr;
    const bool gbvh = g.soup.n_tri > 0 && g.soup.bvh_nodes != nullptr;
    const int cull = !sbvh && view_cull_wanted(a);
    const dim3 grid((unsigned)(a.n_blocks * a.split));
    KernelTimer kt(KT_SARSA_VIEW, stream);
    if (sbvh && gbvh)
        hipLaunchKernelGGL((k_glyph_view<true, true>), grid, dim3(256), 0, stream, a, g, cull, out_tri, out_glyph, out_sector, out_t);
    else if (sbvh)
        hipLaunchKernelGGL((k_glyph_view<true, false>), grid, dim3(256), 0, stream, a, g, cull, out_tri, out_glyph, out_sector, out_t);
    else if (gbvh)
        hipLaunchKernelGGL((k_glyph_view<false, true>), grid, dim3(256), 0, stream, a, g, cull, out_tri, out_glyph, out_sector, out_t);
    else
        hipLaunchKernelGGL((k_glyph_view<false, false>), grid, dim3(256), 0, stream, a, g, cull, out_tri, out_glyph, out_sector, out_t);
    return hipGetLastError();
}

}  // namespace rt

// ---- host side -------------------------------------------------------------------------------

struct rt_glyphs {
    rt_ctx* ctx = nullptr;
    int device = 0;
    int n = 0;
    rt_scene* mesh = nullptr;     // the soup as a device scene of its own (288 n surfaces, no light), accel BVH; null: n = 0
    float4* d_colour = nullptr;   // [144 n]
    float4* d_qnormal = nullptr;  // [144 n]
    int bvh_nodes = 0;
};

namespace {

int err(int code, const std::string& m) { return rt::set_error(code, m.c_str()); }

#define RT_HIPG(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return err(RT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// get_vertices + build_surfaces (radiance_volume.cu:442-515) of one glyph: rtmi.h rt_glyph_mesh
void glyph_mesh_one(const float* pos, const float* nrm, float D, float* tri_v, float* quad_normal) {
    using rt::f3;
    constexpr int R = rt::kGridRes;
    const f3 P = rt::make3(pos[0], pos[1], pos[2]);
    const f3 N = rt::make3(nrm[0], nrm[1], nrm[2]);
    f3 T, B;
    rt::normal_frame(N, &T, &B);
    f3 V[R + 1][R + 1];
    for (int x = 0; x <= R; ++x)
        for (int y = 0; y <= R; ++y) {
            float xh, yh, zh;
            rt::chiu_map((float)x / (float)R, (float)y / (float)R, &xh, &yh, &zh);
            const float xs = xh * D, ys = yh * D, zs = zh * D;
            V[x][y] = rt::make3((T.x * xs + N.x * ys) + (B.x * zs + P.x), (T.y * xs + N.y * ys) + (B.y * zs + P.y),
                                (T.z * xs + N.z * ys) + (B.z * zs + P.z));
        }
    auto put = [](float* dst, const f3& a, const f3& b, const f3& c) {
        const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        memcpy(dst, v, sizeof(v));
    };
    for (int x = 0; x < R; ++x)
        for (int y = 0; y < R; ++y) {
            const int k = x * R + y;
            const f3 v0 = V[x][y], v1 = V[x + 1][y], v2 = V[x][y + 1], v3 = V[x + 1][y + 1];
            put(tri_v + (size_t)(2 * k) * 9, v0, v2, v1);
            put(tri_v + (size_t)(2 * k + 1) * 9, v1, v2, v3);
            if (quad_normal) {
                const f3 mid = rt::make3((((v0.x + v1.x) + v2.x) + v3.x) / 4.f, (((v0.y + v1.y) + v2.y) + v3.y) / 4.f,
                                         (((v0.z + v1.z) + v2.z) + v3.z) / 4.f);
                const f3 nq = rt::normalize(rt::make3(mid.x - P.x, mid.y - P.y, mid.z - P.z));
                quad_normal[3 * k + 0] = nq.x;
                quad_normal[3 * k + 1] = nq.y;
                quad_normal[3 * k + 2] = nq.z;
            }
        }
}

// diam: one diameter per glyph, or (one_diameter) a single one for all of them
int glyph_mesh(const float* pos, const float* normal, int n, const float* diam, bool one_diameter, float* tri_v,
               float* quad_normal) {
    if (n < 0) return err(RT_E_INVALID, "rt_glyph_mesh: n < 0");
    if (!diam) return err(RT_E_INVALID, "rt_glyph_mesh: NULL argument");
    for (int g = 0; g < (one_diameter ? 1 : n); ++g)
        if (!(diam[g] > 0.0f) || !std::isfinite(diam[g]))
            return err(RT_E_INVALID, "rt_glyph_mesh: the diameter must be finite and > 0");
    if (n > 0 && (!pos || !normal || !tri_v)) return err(RT_E_INVALID, "rt_glyph_mesh: NULL argument");
    for (int g = 0; g < n; ++g) {
        const float* N = normal + (size_t)3 * g;
        if (!finite3(pos + (size_t)3 * g) || !finite3(N))
            return err(RT_E_INVALID, "rt_glyph_mesh: glyph " + std::to_string(g) + " has a non-finite position or normal");
        if (N[0] == 0.0f && N[1] == 0.0f && N[2] == 0.0f)
            return err(RT_E_INVALID, "rt_glyph_mesh: glyph " + std::to_string(g) + " has a zero normal");
    }
    for (int g = 0; g < n; ++g)
        glyph_mesh_one(pos + (size_t)3 * g, normal + (size_t)3 * g, diam[one_diameter ? 0 : g],
                       tri_v + (size_t)g * rt::kGlyphTris * 9,
                       quad_normal ? quad_normal + (size_t)g * rt::kGlyphSectors * 3 : nullptr);
    return RT_OK;
}

int glyph_colours(const float* values, int n, int mode, float* rgb) {
    if (n < 0) return err(RT_E_INVALID, "rt_glyph_colours: n < 0");
    if (mode != RT_GLYPH_RATIO && mode != RT_GLYPH_MAGNITUDE)
        return err(RT_E_INVALID, "rt_glyph_colours: bad mode " + std::to_string(mode));
    if (n > 0 && (!values || !rgb)) return err(RT_E_INVALID, "rt_glyph_colours: NULL argument");
    constexpr int S = rt::kGlyphSectors;
    for (size_t i = 0; i < (size_t)n * S; ++i)
        if (!std::isfinite(values[i]))
            return err(RT_E_INVALID, "rt_glyph_colours: glyph " + std::to_string(i / S) + " has a non-finite value");
    for (int g = 0; g < n; ++g) {
        const float* v = values + (size_t)g * S;
        float* out = rgb + (size_t)g * S * 3;
        if (mode == RT_GLYPH_RATIO) {  // build_surfaces: the ratio to the row's largest value, red over green
            float m = 0.f;
            for (int k = 0; k < S; ++k)
                if (m < v[k]) m = v[k];
            for (int k = 0; k < S; ++k) {
                const float ratio = m == 0.f ? 0.f : v[k] / m;
                out[3 * k + 0] = ratio;
                out[3 * k + 1] = 1.f - ratio;
                out[3 * k + 2] = 0.f;
            }
        } else {  // build_radiance_magnitude_volume_shapes: grey, darker where the magnitude is larger
            float m = 0.0001f;
            for (int k = 0; k < S; ++k)
                if (fabsf(v[k]) > m) m = fabsf(v[k]);
            for (int k = 0; k < S; ++k) out[3 * k + 0] = out[3 * k + 1] = out[3 * k + 2] = 1.f - fabsf(v[k]) / m;
        }
    }
    return RT_OK;
}

// rgb (n x 3 floats per entry) as the device's float4 table
int upload_f4(float4* dst, const float* src, size_t entries) {
    std::vector<float4> tab(entries);
    for (size_t i = 0; i < entries; ++i) tab[i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.f);
    RT_HIPG(hipMemcpy(dst, tab.data(), sizeof(float4) * entries, hipMemcpyHostToDevice));
    return RT_OK;
}

// what the view refuses before any device work: values first (RT_E_INVALID), then the engine
int check_view_params(const rt_params* p) {
    if (!p) return err(RT_E_INVALID, "params is NULL");
    if (rt::params_size_bad(p)) return err(RT_E_INVALID, "bad image size / spp");
    if (const char* why = rt::params_split_refusal(p)) return err(RT_E_INVALID, why);
    if (p->preset != RT_PRESET_GPU) return err(RT_E_UNSUPPORTED, "the glyph view implements the GPU-engine preset");
    if (p->hit_rule != RT_HIT_RULE_GPU) return err(RT_E_UNSUPPORTED, "the glyph view implements the GPU engine's hit rule");
    return RT_OK;
}

// the glyph cast's route: the BVH unless RTMI_GLYPH_BVH=0 (read per call)
bool glyph_bvh_wanted() {
    const char* e = getenv("RTMI_GLYPH_BVH");
    return !(e && strcmp(e, "0") == 0);
}

// one view launch
int view_frame(const rt_scene* scene, const rt_glyphs* gl, const rt_camera* cam, const rt_params* p,
               const rt_glyph_view_opts* opts, uint32_t first_sample, const float* d_base, const rt::BlockDesc* d_blocks,
               int n_blocks, int out_pitch, float* d_out, int32_t* d_tri, int32_t* d_glyph, int32_t* d_sector, float* d_t,
               hipStream_t stream) {
    rt::RenderLaunch a = rt::render_launch(scene, cam, p);
    rt::fill_view_launch(&a, p, d_blocks, n_blocks, out_pitch, d_out, first_sample);
    rt::GlyphSet g;  // (an empty set: a soup of no triangles)
    if (gl->mesh) g.soup = glyph_bvh_wanted() ? rt::scene_launch_view(gl->mesh) : rt::scene_device(gl->mesh);
    g.colour = gl->d_colour;
    g.qnormal = gl->d_qnormal;
    g.base = d_base;
    g.shade = (opts && opts->shade != 0) ? 1 : 0;
    RT_HIPG(rt::launch_glyph_view(a, g, d_tri, d_glyph, d_sector, d_t, stream));
    return RT_OK;
}

// rt_glyphs_create / rt_glyphs_create_sized: diam as glyph_mesh takes it
int glyphs_create(rt_ctx* ctx, const float* pos, const float* normal, const float* values, int32_t n, const float* diam,
                  bool one_diameter, int colour_mode, rt_glyphs** out) {
    // (by value first, then the pointers: every refusal comes before any device work)
    if (n < 0 || n > RT_GLYPH_MAX)
        return err(RT_E_INVALID, "rt_glyphs_create: " + std::to_string(n) + " glyphs, outside [0, " + std::to_string(RT_GLYPH_MAX) + "]");
    if (!ctx || !out) return err(RT_E_INVALID, "rt_glyphs_create: ctx/out is NULL");
    *out = nullptr;
    if (n > 0 && (!pos || !normal || !values)) return err(RT_E_INVALID, "rt_glyphs_create: NULL argument");
    const size_t nq = (size_t)n * rt::kGlyphSectors, nt = (size_t)n * rt::kGlyphTris;
    std::vector<float> tri(nt * 9), qn(nq * 3), rgb(nq * 3);
    int rc = glyph_mesh(pos, normal, n, diam, one_diameter, tri.data(), qn.data());
    if (rc == RT_OK) rc = glyph_colours(values, n, colour_mode, rgb.data());
    if (rc != RT_OK) return rc;
    rt_glyphs* g = new (std::nothrow) rt_glyphs();
    if (!g) return err(RT_E_NOMEM, "out of host memory");
    g->ctx = ctx;
    g->device = rt::ctx_device(ctx);
    g->n = n;
    if (n == 0) {
        *out = g;
        return RT_OK;
    }
    // the soup as a scene of its own: 288 n surfaces and no light; the albedo is not used
    const std::vector<float> albedo(nt * 3, 0.f);
    rc = rt_scene_create(ctx, tri.data(), albedo.data(), (int)nt, nullptr, nullptr, nullptr, 0, &g->mesh);
    if (rc == RT_OK) rc = rt_scene_set_accel(g->mesh, RT_ACCEL_BVH);  // (the build, if the scene has none yet)
    if (rc == RT_OK) rc = rt_scene_accel_info(g->mesh, &g->bvh_nodes, nullptr, nullptr);
    hipError_t e = hipSuccess;
    if (rc == RT_OK) e = hipMalloc(&g->d_colour, sizeof(float4) * nq);
    if (rc == RT_OK && e == hipSuccess) e = hipMalloc(&g->d_qnormal, sizeof(float4) * nq);
    if (rc == RT_OK && e != hipSuccess) rc = err(RT_E_HIP, std::string("rt_glyphs_create: ") + hipGetErrorString(e));
    if (rc == RT_OK) rc = upload_f4(g->d_colour, rgb.data(), nq);
    if (rc == RT_OK) rc = upload_f4(g->d_qnormal, qn.data(), nq);
    if (rc != RT_OK) {
        const std::string msg = rt_last_error();  // (the destroy below must not lose it)
        (void)rt_glyphs_destroy(g);
        return err(rc, msg);
    }
    *out = g;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_glyph_mesh(const float* pos, const float* normal, int32_t n, float diameter, float* tri_v, float* quad_normal) {
    return glyph_mesh(pos, normal, n, &diameter, true, tri_v, quad_normal);
}

int rt_glyph_colours(const float* values, int32_t n, int mode, float* rgb) { return glyph_colours(values, n, mode, rgb); }

int rt_glyphs_create(rt_ctx* ctx, const float* pos, const float* normal, const float* values, int32_t n, float diameter,
                     int colour_mode, rt_glyphs** out) {
    return glyphs_create(ctx, pos, normal, values, n, &diameter, true, colour_mode, out);
}

int rt_glyphs_create_sized(rt_ctx* ctx, const float* pos, const float* normal, const float* values,
                           const float* diameters, int32_t n, int colour_mode, rt_glyphs** out) {
    if (n > 0 && n <= RT_GLYPH_MAX && !diameters) return err(RT_E_INVALID, "rt_glyphs_create_sized: diameters is NULL");
    const float none = 1.0f;  // (an empty set has no diameter to check)
    return glyphs_create(ctx, pos, normal, values, n, n > 0 ? diameters : &none, n <= 0, colour_mode, out);
}

int rt_glyphs_destroy(rt_glyphs* g) {
    if (!g) return RT_OK;
    (void)hipSetDevice(g->device);
    if (g->d_colour) (void)hipFree(g->d_colour);
    if (g->d_qnormal) (void)hipFree(g->d_qnormal);
    if (g->mesh) (void)rt_scene_destroy(g->mesh);
    delete g;
    return RT_OK;
}

int rt_glyphs_set_colours(rt_glyphs* g, const float* rgb) {
    if (!g) return err(RT_E_INVALID, "NULL argument");
    if (g->n == 0) return RT_OK;
    if (!rgb) return err(RT_E_INVALID, "rt_glyphs_set_colours: rgb is NULL");
    RT_HIPG(hipSetDevice(g->device));
    RT_HIPG(hipDeviceSynchronize());  // a view in flight still reads the table
    return upload_f4(g->d_colour, rgb, (size_t)g->n * rt::kGlyphSectors);
}

int rt_glyphs_info(const rt_glyphs* g, int32_t* n_glyphs, int32_t* n_tri, int32_t* bvh_nodes) {
    if (!g) return err(RT_E_INVALID, "NULL argument");
    if (n_glyphs) *n_glyphs = g->n;
    if (n_tri) *n_tri = g->n * rt::kGlyphTris;
    if (bvh_nodes) *bvh_nodes = g->bvh_nodes;
    return RT_OK;
}

int rt_render_glyph_view(rt_ctx* ctx, const rt_scene* scene, const rt_glyphs* gl, const rt_camera* cam,
                         const rt_params* params, const rt_glyph_view_opts* opts, uint32_t first_sample,
                         const float* base_rgb, float* out_rgb, int32_t* out_tri, int32_t* out_glyph, int32_t* out_sector,
                         float* out_t) {
    int rc = check_view_params(params);  // (by value first, then the pointers)
    if (rc != RT_OK) return rc;
    if (!ctx || !scene || !gl || !cam || !out_rgb) return err(RT_E_INVALID, "rt_render_glyph_view: NULL argument");
    if (gl->device != rt::ctx_device(ctx)) return err(RT_E_INVALID, "the glyph set belongs to another device");
    RT_HIPG(hipSetDevice(gl->device));
    const int W = params->width, H = params->height;
    const size_t np = (size_t)W * H;
    float *d_out, *d_base, *d_t;
    int32_t *d_tri, *d_glyph, *d_sector;
    rt::HostFrame f(0, 0, W, H);
    f.out(&d_out, out_rgb, sizeof(float) * 3 * np);
    f.in(&d_base, base_rgb, sizeof(float) * 3 * np);
    f.out(&d_tri, out_tri, sizeof(int32_t) * np);
    f.out(&d_glyph, out_glyph, sizeof(int32_t) * np);
    f.out(&d_sector, out_sector, sizeof(int32_t) * np);
    f.out(&d_t, out_t, sizeof(float) * np);
    const hipError_t e = f.begin();
    if (e == hipSuccess)
        rc = view_frame(scene, gl, cam, params, opts, first_sample, d_base, f.blocks(), f.n_blocks(), W, d_out, d_tri,
                        d_glyph, d_sector, d_t, 0);
    return f.finish(rc, e, "rt_render_glyph_view");
}

int rt_render_glyph_view_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_glyphs* gl, const rt_camera* cam,
                                      const rt_params* params, const rt_glyph_view_opts* opts, uint32_t first_sample,
                                      const float* d_base, const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                                      void* stream) {
    int rc = check_view_params(params);
    if (rc != RT_OK) return rc;
    if (!ctx || !scene || !gl || !cam) return err(RT_E_INVALID, "rt_render_glyph_view_tiles_device: NULL argument");
    if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !d_out))) return err(RT_E_INVALID, "bad tiles/out");
    if (gl->device != rt::ctx_device(ctx)) return err(RT_E_INVALID, "the glyph set belongs to another device");
    RT_HIPG(hipSetDevice(gl->device));
    if (n_tiles == 0) return RT_OK;
    const rt::BlockDesc* d_blocks = nullptr;
    int n_blocks = 0;
    rc = rt::ctx_blocks(ctx, tiles, n_tiles, tile_size, params->width, params->height, &d_blocks, &n_blocks);
    if (rc != RT_OK) return rc;
    return view_frame(scene, gl, cam, params, opts, first_sample, d_base, d_blocks, n_blocks, tile_size, d_out, nullptr,
                      nullptr, nullptr, nullptr, (hipStream_t)stream);
}

}  // extern "C"
