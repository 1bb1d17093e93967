/*
 * rtmi.h — C ABI of the MI355X-native path tracer (librtmi.so).
 *
 * The reference (callumPearce/Reinforcement-Light-Rays-Pathtracer) has no
 * FFI; its drop-in boundary for the hot path is the C++ scene-loader /
 * Camera / SDL frame-buffer API plus the render entry point.  Each entry
 * point below names the reference interface it replaces (paths relative to
 * the reference root; CPU/ = Old_CPU_Rendering_Engine/Source,
 * GPU/ = GPU_Rendering_Engine/Source).  The C++ facade in
 * reinforcement-light-rays-pathtracer_amd/host/ restores the reference's
 * class/function names on top of this ABI; Python binds it with ctypes.
 *
 * Conventions
 *  - every function returns RT_OK (0) or a negative RT_E* code; nothing
 *    throws across the ABI; rt_last_error() holds a thread-local message.
 *  - host pointers are caller-owned; device memory is owned by rt_ctx /
 *    rt_scene.  Functions named *_device take device pointers and a
 *    hipStream_t passed as void* and are asynchronous on that stream.
 *  - one host thread per rt_ctx; contexts on different GPUs may run
 *    concurrently (one process per GPU is the supported multi-GPU model).
 */
#ifndef RTMI_H
#define RTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_E_INVALID (-1)     /* bad argument */
#define RT_E_HIP (-2)         /* HIP runtime error */
#define RT_E_NOMEM (-3)       /* allocation failed */
#define RT_E_IO (-4)          /* file could not be opened / parsed */
#define RT_E_UNSUPPORTED (-5) /* valid request this build does not implement */
#define RT_E_INTERNAL (-6)    /* a self-check of the library failed */

#define RT_HIT_NONE (-1)
#define RT_HIT_TYPE_LIGHT 1u   /* enum IntersectionType AREA_LIGHT(_PLANE) */
#define RT_HIT_TYPE_SURFACE 2u /* enum IntersectionType SURFACE */

/* semantic presets */
#define RT_PRESET_CPU 0 /* Old_CPU_Rendering_Engine: recursive estimator, bounce cap semantics of
                           CPU/path_tracing/default_path_tracing.cpp:46-101 */
#define RT_PRESET_GPU 1 /* GPU_Rendering_Engine: iterative throughput,
                           GPU/path_tracing/default_path_tracing.cu:36-88 */

#define RT_HIT_RULE_CPU 0 /* predicate of the prebuilt CPU triangle.cpp.o (t > 1e-5, t < dist + 1e-5) */
#define RT_HIT_RULE_GPU 1 /* GPU/rays/ray.cu:38-141 (t < dist, dist starts at 999999) */

#define RT_SAMPLER_UNIFORM 0 /* the reference's sampler: cos(theta) = r1, pdf 1/(2*pi) */
#define RT_SAMPLER_COSINE 1  /* cosine-weighted: cos(theta) = sqrt(r1), pdf cos/pi */

typedef struct rt_ctx rt_ctx;
typedef struct rt_scene rt_scene;

/* Camera: CPU/camera.h:11-42 (position, yaw) and GPU/camera.cuh:11-36 (yaw_y, yaw_x). */
typedef struct {
    float pos[4];
    float yaw_y; /* CPU engine "yaw" */
    float yaw_x; /* GPU engine only; 0 for the CPU preset */
} rt_camera;

/* Render parameters: the reference's compile-time constants
 * (CPU/constants/ and GPU/constants/ headers) as a runtime struct. */
typedef struct {
    int32_t width, height; /* SCREEN_WIDTH / SCREEN_HEIGHT; FOCAL_LENGTH = height */
    int32_t spp;           /* SAMPLES_PER_PIXEL */
    int32_t max_bounces;   /* MAX_RAY_BOUNCES */
    int32_t sampler;       /* RT_SAMPLER_* */
    int32_t preset;        /* RT_PRESET_* */
    int32_t hit_rule;      /* RT_HIT_RULE_* */
    int32_t spp_split;     /* sample chunks per pixel (1,2,4,...,64; divides spp; 0 = 1).  Chunk c
                              sums samples [c*spp/S, (c+1)*spp/S) in order; the pixel is
                              (((P0 + P1) + P2) + ...) / spp.  Part of the result's definition:
                              keep it fixed across GPU counts for bit-identical images. */
    uint64_t seed;         /* Philox key; the reference's curand seed is 1984 */
    float env_light;       /* ENVIRONMENT_LIGHT (GPU preset) */
    float t_scale;         /* direction scale in the hit test (= SCREEN_HEIGHT in the reference) */
} rt_params;

/* Fill *p with the reference defaults of a preset:
 *   CPU: 512x512, 16 spp, cap 2, hit rule CPU   (CPU/constants/image_settings.h:9-12,
 *                                                monte_carlo_settings.h:8-9)
 *   GPU: 720x720, 32 spp, cap 80, hit rule GPU  (GPU/constants/image_settings.h:9-12,
 *                                                monte_carlo_settings.h:8-10)
 * seed 1984 (GPU/utils/cuda_helpers.cu:24). */
int rt_params_default(int preset, rt_params* p);

/* ---- context ---------------------------------------------------------- */
/* Replaces the device setup of GPU/main.cu:150-198 (cudaMalloc + pointer patching). */
int rt_ctx_create(int device_ordinal, rt_ctx** out);
int rt_ctx_destroy(rt_ctx* ctx);
const char* rt_last_error(void);

/* ---- scene construction (host side, no GPU) --------------------------- */
/* get_cornell_shapes: CPU/scenes/cornell_box_scene.cpp:3-205 (variant RT_PRESET_CPU:
 * one light plane, emission 1*(1,1,0.9)) and GPU/scenes/cornell_box_scene.cu:4 (variant
 * RT_PRESET_GPU: two AreaLights, emission 14*(0.9,0.9,0.9)).
 * Arrays must hold 36 surfaces / 2 lights (rt_cornell_counts). */
int rt_cornell_counts(int* n_surf, int* n_light);
int rt_cornell_geometry(int variant, float* tri_v /* n_surf x 9 */, float* albedo /* n_surf x 3 */,
                        float* light_v /* n_light x 9 */, float* emission /* n_light x 3 */,
                        int32_t* light_group /* n_light */);

/* load_scene for OBJ files with the GPU engine's semantics:
 * GPU/objects/object_importer.cu:8-412 (scale 2, (v1,v3,v2) order, per-scene materials and
 * lights, lights_in_obj for complex_light_room).  `scene_kind` selects the hard-coded
 * material/light block: 0 generic (white 0.75, no lights), 1 door_room, 2 archway,
 * 3 complex_light_room.  Two-pass: call with NULL arrays to get counts.
 * door_room variants: scene_kind = 1 | (bits << 8), the blocks the reference comments in
 * and out by hand (object_importer.cu).  0 = the door-room lights of :214-237, the red
 * material of :152-155 on triangles 24-35 and the blue of :161-163 on 12-23: the scene of
 * the thesis's door-room comparison renders (Images/door_room/default_128spp_50avg.png:
 * image mean and average path length match, tools/door_variants.py).  RT_DOOR_WHITE_DOOR
 * drops the red material (commented at HEAD), RT_DOOR_NO_BLUE the blue (active at HEAD),
 * RT_DOOR_ARCHWAY_LIGHTS uses the lights active at HEAD (:240-271, the archway's, outside
 * this room: a black image) instead of the door-room lights (commented at HEAD). */
#define RT_DOOR_WHITE_DOOR 1
#define RT_DOOR_NO_BLUE 2
#define RT_DOOR_ARCHWAY_LIGHTS 4
int rt_obj_geometry(const char* path, int scene_kind, float* tri_v, float* albedo, int* n_surf,
                    float* light_v, float* emission, int32_t* light_group, int* n_light,
                    float* nn_vertices /* Scene::vertices order, may be NULL */, int* n_nn_floats);

/* ---- device scene ------------------------------------------------------ */
/* Scene::load_* + the H2D copies of GPU/main.cu:160-180.  Copies the host arrays;
 * computes normals (CPU/objects/triangle.cpp:73-82) and per-triangle tangent frames. */
int rt_scene_create(rt_ctx* ctx, const float* tri_v, const float* albedo, int n_surf,
                    const float* light_v, const float* emission, const int32_t* light_group,
                    int n_light, rt_scene** out);
int rt_scene_destroy(rt_scene* scene);
/* Host copy of the normals the scene computed, (n_surf+n_light) x 3. */
int rt_scene_normals(const rt_scene* scene, float* out);

/* ---- the hot path -------------------------------------------------------- */
/* Ray::closest_intersection over a ray batch (CPU/rays/ray.cpp:14-28 + the hit predicate;
 * GPU/rays/ray.cu:16-141).  dir must be normalised (Ray::Ray does it).  out_t = hit distance
 * in t_scale units (+inf on miss); out_hit = (type<<30)|index, RT_HIT_NONE on miss; light
 * index = plane index (hit_rule CPU) or light-triangle index (hit_rule GPU). Host arrays. */
int rt_intersect(rt_ctx* ctx, const rt_scene* scene, const float* orig /* n x 3 */,
                 const float* dir /* n x 3 */, int n, float t_scale, int hit_rule,
                 float* out_t, int32_t* out_hit);
/* Same, device pointers, asynchronous on `stream` (hipStream_t). */
int rt_intersect_device(rt_ctx* ctx, const rt_scene* scene, const float* d_orig,
                        const float* d_dir, int n, float t_scale, int hit_rule, float* d_t,
                        int32_t* d_hit, void* stream);
/* Diagnostic: rt_intersect by a chosen hit-test method.  Every method returns the same
 * bits (the exact test decides; the filters only skip triangles it must reject):
 *   RT_ISECT_SCAN    the single-phase exact scan of every triangle
 *   RT_ISECT_FILTER  the fp32 two-phase filter (rays within the scene's filter bounds,
 *                    else RT_E_UNSUPPORTED)
 *   RT_ISECT_MFMA    the matrix-core filter of k_render_ps's bounce casts (a ray whose
 *                    origin is outside the scene's box + 1 keeps every triangle)
 * out_cand (optional, MFMA only): per ray, the triangles that reached the exact test. */
#define RT_ISECT_SCAN 0
#define RT_ISECT_FILTER 1
#define RT_ISECT_MFMA 2
#define RT_ISECT_BVH 3 /* the exact BVH path: built on first use if the scene has none, and kept
                          (this call may allocate); the scene's accel mode is not changed */
int rt_intersect_method(rt_ctx* ctx, const rt_scene* scene, const float* orig, const float* dir, int n,
                        float t_scale, int hit_rule, int method, float* out_t, int32_t* out_hit,
                        int32_t* out_cand);
/* Diagnostic: rt_intersect by the candidate route of the render kernels -- the exact test of a
 * ray's candidate triangles only, in index order, the rest shared by the ray's wave -- with the
 * candidates chosen by `source`:
 *   RT_CAND_TABLE  surf[n]: ray r is taken as a bounce ray leaving surface surf[r]; its
 *                  candidates come from the scene's bounce-ray candidate table for hit_rule
 *                  (built on first use and kept, as a render builds it).  out_masks (optional):
 *                  the masks the device lookup gave, words = ceil(n_tri / 64) per ray, bit
 *                  i % 64 of word i / 64 = triangle i.  The hits are rt_intersect's as long as
 *                  the table is sound for the rays.
 *   RT_CAND_GIVEN  masks_in[n][words]: the caller's candidates (the GPU preset's camera rays
 *                  take their tile's cull masks this way).  The hit is that of the scan
 *                  restricted to the ray's mask; a ray with an empty mask hits nothing.
 * pair_cap: the length of the wave's shared pair list, one the render kernels are built with:
 * RT_CAND_CAP_TABLE (scenes of at most 64 triangles) or RT_CAND_CAP_SHARED; anything else is
 * RT_E_INVALID.  RT_E_UNSUPPORTED: a scene of more than 256 triangles or on the BVH path, or
 * (RT_CAND_TABLE) no table for the scene at this hit_rule and t_scale (the CPU rule's serves
 * t_scale >= 256).  Never falls back to another method.  Replaces no reference interface. */
#define RT_CAND_TABLE 0
#define RT_CAND_GIVEN 1
#define RT_CAND_CAP_TABLE 96
#define RT_CAND_CAP_SHARED 256
int rt_intersect_cand(rt_ctx* ctx, const rt_scene* scene, const float* orig, const float* dir, int n, float t_scale,
                      int hit_rule, int source, const int32_t* surf, const uint64_t* masks_in, int pair_cap,
                      float* out_t, int32_t* out_hit, uint64_t* out_masks);

/* ---- acceleration structure for large scenes ----
 * The reference scans every triangle per ray (CPU/rays/ray.cpp:14-28, GPU/rays/ray.cu:
 * 16-141) and has no acceleration structure; Models/bunny.obj (4,968 triangles) and
 * Medieval_House.obj (2,663) make that scan the whole cost.  The BVH path returns the
 * scan's hit bit for bit (both hit rules): padded boxes that prove the exact test fails,
 * and a second BVH over the triangles' planes for the pairs a ray could graze (rt_bvh.cpp).  RT_ACCEL_AUTO (the
 * default) builds and uses it for scenes above RT_BVH_AUTO_MIN triangles; RT_ACCEL_SCAN
 * never uses it; RT_ACCEL_BVH builds it for any scene (A/B).  The default-sampler renders
 * (rt_render, rt_render_tiles_device), the Expected-SARSA, DQN and Neural-Q renders
 * (their trace kernels take the BVH when the scene's mode turns it on) and rt_intersect /
 * rt_intersect_device follow the mode. */
#define RT_ACCEL_AUTO 0
#define RT_ACCEL_SCAN 1
#define RT_ACCEL_BVH 2
#define RT_BVH_AUTO_MIN 256
int rt_scene_set_accel(rt_scene* scene, int mode);
/* nodes of the triangle BVH, its depth, nodes of the plane-space BVH (out pointers may
 * be NULL; zeros when the scene has no BVH) */
int rt_scene_accel_info(const rt_scene* scene, int* n_nodes, int* depth, int64_t* plane_nodes);
/* The bounce-ray candidate table of hit rule `hit_rule` (no reference counterpart: the
 * scene's preprocessing, like a BVH build): built on the first render that takes it.
 * built: 1 once on the device; build_s: host build + upload seconds; bytes: device bytes.
 * Out pointers may be NULL; zeros before the build or when no render took it. */
int rt_scene_ctab_info(const rt_scene* scene, int hit_rule, int* built, double* build_s, uint64_t* bytes);
/* Host only (no GPU): build the BVH of n triangles (n x 9 vertices, the rt_scene_create
 * order) and check its invariants (every triangle in one leaf of each tree, boxes nested
 * and holding their triangles, planes inside their plane-space leaves).  stats
 * (optional, 4 entries): nodes, depth, plane-space nodes, leaves.  RT_E_INTERNAL with
 * rt_last_error() naming the first violation. */
int rt_bvh_check(const float* tri_v, int n, int64_t* stats);

/* draw_default_path_tracing (CPU/path_tracing/default_path_tracing.cpp:5-18;
 * GPU kernel GPU/path_tracing/default_path_tracing.cu:7-34): render the rectangle
 * [x0,x0+w) x [y0,y0+h) of the params->width x params->height image.
 * out_rgb: w*h*3 floats, row-major (row = y-y0).  Synchronous; host memory. */
int rt_render(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params,
              int x0, int y0, int w, int h, float* out_rgb, uint64_t* out_ray_casts);

/* Tile-list render for image-tile partitioning across GPUs.  tiles: n_tiles x 2 int32
 * (host) pixel origins of tile_size x tile_size tiles (tile_size a multiple of 16).
 * d_out: device, n_tiles*tile_size*tile_size*3 floats, [tile][y][x][rgb].
 * d_casts: device uint64 (accumulated into, may be NULL).  Asynchronous on `stream`. */
int rt_render_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam,
                           const rt_params* params, const int32_t* tiles, int n_tiles,
                           int tile_size, float* d_out, uint64_t* d_casts, void* stream);

/* ---- next-event estimation: direct light by shadow rays (GPU preset) ---------
 * The reference's path tracer adds light only when a bounce ray happens to hit a light
 * triangle.  This is the same renderer with the standard variance reduction
 * beside it: at every surface hit one point of one light is sampled and tested with a shadow
 * ray.  Its expectation is rt_render's at the same max_bounces, exactly (consequence (a) below);
 * its indirect path is rt_render's path, ray for ray.  GPU preset only: RT_PRESET_CPU is
 * RT_E_UNSUPPORTED.
 *
 * Definition (normative; every line in binary32, -ffp-contract=off semantics, IEEE / and sqrt,
 * normalize(v) = v * (1 / sqrt(dot(v, v))), dot(a, b) = (ax bx + ay by) + az bz).
 * Sample s of pixel pix = y W + x starts with tp = (1,1,1), L = (0,0,0), depth = 0; its camera
 * ray is rt_render's (event 0).  Each cast ends in one of three ways:
 *   miss:         L += tp * env_light; the path ends.
 *   light hit:    at depth == 0, L += tp * Le (the camera sees the light); at depth > 0 nothing
 *                 (that light was sampled at the previous surface).  The path ends.
 *   surface hit   tri at pos = o + t D:
 *     depth + 1 == max_bounces: the path ends with nothing (rt_render would have no next cast, so
 *       no direct light is taken either);
 *     else the direct term, then -- unless flag RT_NEE_DIRECT_ONLY ends the path here -- the
 *       preset's own bounce unchanged (event 1 + depth, counter word 3 = 0), then ++depth.
 * The direct term at (tri, pos, depth):
 *   1. one Philox block w of counter (pix, s, 1 + depth, 0x4E454531) under the seed's key;
 *   2. r = u01(w0); light l = the first with r < cdf[l] (a light that catches the rest -- the last
 *      whose cdf exceeds its predecessor's -- exists only for a caller's own cdf: a built table ends at 1);
 *   3. u = u01(w1), v = u01(w2); if u + v > 1: u = 1 - u, v = 1 - v;  y = (v0 + u e1) + v e2 with
 *      the light's v0, e1 = v1 - v0, e2 = v2 - v0;
 *   4. Lv = y - pos, d2 = dot(Lv, Lv), d = normalize(Lv), cx = dot(N_tri, d), cy = |dot(N_l, d)|
 *      (lights emit from both faces: GPU/rays/ray.cu:78-112 has no facing test);
 *   5. d2 == 0, cx <= 0 or cy == 0: no cast, no contribution;
 *   6. else the ray o = pos + 1e-5f d along d, cast as a ray leaving tri like every other cast; the
 *      sample is visible iff the closest hit is triangle n_surf + l;
 *   7. visible: per channel L += ((tp brdf_tri) Le_l) (((cx cy) / d2) k_l), brdf_tri = albedo / pi
 *      under both samplers.
 * Visibility by the closest hit inherits the scan's tie rules (a surface coplanar with the light
 * at the same t wins, as for a bounce ray), is bit-identical on every cast route and needs no
 * second epsilon.  A point within rounding of an edge shared by two light triangles can land on
 * the neighbour and count as occluded (probability of the order 2^-24 per sample).
 * Light table (host, double, stored as float): w_l = area_l (Le.r + Le.g + Le.b), cdf[l] the
 * normalised running sum, k_l = (sum w) / (Le.r + Le.g + Le.b) (the reciprocal of the area pdf;
 * 0 for a light of weight 0, which is never chosen).  A scene without lights, or without
 * weight, is valid: no direct term is ever taken.
 * A sample's L takes its terms in path order; samples fold as everywhere (spp_split chunks in
 * sample order, chunk sums in chunk order, / spp).  Every closest-hit call counts as a cast,
 * shadow casts included.  Consequences: (a) the expectation equals rt_render's -- the direct term at
 * the surface of cast i stands for a light hit at cast i + 1 <= max_bounces - 1; (b) with no light
 * (or none of weight) image and casts equal rt_render's bit for bit.
 * out_stats (may be NULL): [0] paths (samples), [1] zero-contribution paths, L == (0,0,0) exactly.
 * flags: 0 or RT_NEE_DIRECT_ONLY, else RT_E_INVALID.  Other arguments, checks and texts: rt_render's
 * and rt_render_tiles_device's (d_stats: device uint64[2], accumulated into, may be NULL). */
#define RT_NEE_DIRECT_ONLY 1
int rt_render_nee(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params, int flags,
                  int x0, int y0, int w, int h, float* out_rgb, uint64_t* out_ray_casts, uint64_t* out_stats);
int rt_render_nee_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params,
                               int flags, const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                               uint64_t* d_casts, uint64_t* d_stats, void* stream);
/* Host only, no GPU.  The light table of light triangles light_v (n_light x 9) with emission
 * (n_light x 3): cdf and k, n_light floats each. */
int rt_nee_light_table(const float* light_v, const float* emission, int n_light, float* cdf, float* k);
/* Host only: steps 1-3 of the direct term for n draws (pix, s, depth): the light (-1 where the cdf
 * has no weight) and the point y (n x 3; zeros for no light), by the code the kernel runs. */
int rt_nee_sample(const float* light_v, const float* cdf, int n_light, uint64_t seed, const uint32_t* pix,
                  const uint32_t* s, const int32_t* depth, int n, int32_t* light, float* y);

/* ---- DQN Q-value sampling (BASELINE config 4) ---------------------------- */
typedef struct rt_dqn rt_dqn;

/* DyNet TextFileSaver format reader (the reference loads RMD/<scene>.model with
 * dynet::TextFileLoader, GPU/deep_learning/pre_trained_pathtracer.cu:45-53).  Parameters in
 * file order; each returned row-major [rows][cols] (DyNet stores column-major); a vector
 * ("{rows}" header) is returned with cols = 0 and holds rows values.  Call with values = NULL
 * to size: *n_params, *n_values. */
int rt_dynet_read(const char* path, int max_params, int32_t* rows, int32_t* cols, float* values,
                  int* n_params, int64_t* n_values);

/* DyNet TextFileSaver format writer (the reference saves its trained networks with
 * dynet::TextFileSaver, GPU_Rendering_Engine/Source/deep_learning/neural_q_pathtracer.cu:193 and
 * NN_Q_Value_Trainer/Source/main.cu:290, into Radiance_Map_Data/<name>.model):
 * "#Parameter# /_<k> {rows,cols} <bytes> ZERO_GRAD" (vectors "{rows}") then one line of
 * column-major "%+.8e " values; <bytes> counts that line with its newline.  values: the
 * n_params parameters concatenated, each row-major [rows][cols] (the rt_dynet_read layout;
 * cols = 0: a vector of rows values, "{rows}" header; cols = 1: an (rows, 1) matrix), so a
 * write -> read round trip returns the same floats and shapes bit for bit.  Non-finite
 * values are refused (RT_E_INVALID): DyNet's loader cannot parse them. */
int rt_dynet_write(const char* path, int n_params, const int32_t* rows, const int32_t* cols,
                   const float* values);

/* DQNetwork::initialize + the parameters it loads (NN_Builders/dq_network.cu:8-33,
 * fc_layer.cu:29-35): ReLU(W x + b) x 4, n_in -> hidden[0] -> hidden[1] -> hidden[2] -> n_out.
 * W[l]: row-major [out][in] fp32, b[l]: [out].  nn_vertices: Scene::vertices (n_in floats);
 * the network input is nn_vertices - ray position (nn_rendering_helpers.cu:280-298).
 * Stored on the device as bf16 for the MFMA forward.  n_out must be 144. */
int rt_dqn_create(rt_ctx* ctx, const float* nn_vertices, int n_in, const int32_t* hidden /* 3 */,
                  int n_out, const float* const* W /* 4 */, const float* const* b /* 4 */,
                  rt_dqn** out);
int rt_dqn_destroy(rt_dqn* dqn);
/* Kernel of the forward pass (same Q bit for bit; A/B measurement):
 * RT_DQN_MLP_AUTO (default) and RT_DQN_MLP_STREAM: the weight-streaming kernel (rt_dqn_mlp_rows
 * rays per workgroup, weight fragments from L2); RT_DQN_MLP_STATIONARY: the weight-stationary one
 * (weights resident in registers, one workgroup per CU) for the reference's 200-300-200
 * shape, the streaming one otherwise. */
#define RT_DQN_MLP_AUTO 0
#define RT_DQN_MLP_STREAM 1
#define RT_DQN_MLP_STATIONARY 2
int rt_dqn_set_mlp(rt_dqn* dqn, int mode);
/* Rays per workgroup of the weight-streaming forward kernel in this build (16 per M-tile):
 * the ray counts at which a launch takes one more workgroup, for tests and benchmarks. */
int rt_dqn_mlp_rows(void);
/* DQNetwork::network_inference on n ray positions (host arrays): q = n x 144. */
int rt_dqn_forward(rt_ctx* ctx, const rt_dqn* dqn, const float* loc /* n x 3 */, int n, float* q);
/* Same on device buffers, asynchronous on `stream`. */
int rt_dqn_forward_device(rt_ctx* ctx, const rt_dqn* dqn, const float* d_loc, int n, float* d_q,
                          void* stream);
/* save_selected_radiance_volumes_vals_nn / write_q_values_for_position
 * (GPU/deep_learning/q_value_extractor.cu:18-125): for each "x y z nx ny nz" line of
 * to_select_path, the network's Q values at x (rt_dqn_forward) normalised by their sum,
 * written as "x y z nx ny nz q0 .. q143" (selected_deep.txt); out_path is replaced. */
int rt_dqn_save_selected(rt_ctx* ctx, const rt_dqn* dqn, const char* to_select_path, const char* out_path);
/* importance_sample_direction (nn_rendering_helpers.cu:391-489) for n rays given their Q
 * values (host arrays; q is overwritten with Q*cos as in the reference).  tri: surface the
 * ray sits on; pix: global pixel id (RNG key); tp updated in place; action -1 = none. */
int rt_dqn_sample(rt_ctx* ctx, const rt_scene* scene, uint64_t seed, float* q, const float* loc,
                  const int32_t* tri, const uint32_t* pix, int n, int sample, int bounce, float* tp,
                  float* dir_out, int32_t* action);
/* PretrainedPathtracer::render_frame (pre_trained_pathtracer.cu:188-376), GPU-engine preset:
 * rectangle render into host memory, and tile-list render into device memory (stream-ordered;
 * synchronises the stream every few bounces to stop once all paths have ended).  Between the
 * forward and the sampler each ray's 144 Q values are kept in bf16 (round to nearest even of
 * the forward's fp32 Q, within the forward's own bf16 tolerance): the per-bounce Q buffer's
 * HBM round trip is half the bytes (the sampler itself is rt_dqn_sample's, on those values). */
int rt_render_dqn(rt_ctx* ctx, const rt_scene* scene, const rt_dqn* dqn, const rt_camera* cam,
                  const rt_params* params, int x0, int y0, int w, int h, float* out_rgb,
                  uint64_t* out_ray_casts);
int rt_render_dqn_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_dqn* dqn,
                               const rt_camera* cam, const rt_params* params, const int32_t* tiles,
                               int n_tiles, int tile_size, float* d_out, uint64_t* d_casts,
                               void* stream);

/* Direction sampling of rt_render_dqn / rt_render_dqn_tiles_device, a property of the network
 * handle (as rt_dqn_set_mlp; rt_sarsa_set_sampling is the map's):
 * RT_DQN_SAMPLE_CDF (default) importance_sample_direction, rt_dqn_sample's sampler on the bf16 Q;
 * RT_DQN_SAMPLE_MAX the reference's sample_max_direction (nn_rendering_helpers.cu:491-553), the
 *   sampler of the thesis's fig:1_spp_max_dir (4_critical_evaluation.tex): every bounce leaves
 *   through the cell of highest estimated radiance.  For a ray at bounce b >= 1 on surface `tri`
 *   (shading frame N, T, B) at position pos, with Q[0..143] the fp32 forward at pos,
 *   rt_dqn_forward's value bit for bit (the view's rule; not the bf16 copy the CDF renderer keeps):
 *     action   max_idx = 0, max_q = 0.0f; for k = 0..143: if (Q[k] > max_q) take k (:513-522).
 *              The first cell of the largest positive Q; a row with nothing above zero, or all
 *              NaN, gives 0; a NaN never wins, +inf wins, -0.0f does not beat 0.0f.  The scan
 *              runs on raw Q, not Q x cos, as the reference's.  There is always an action, so
 *              there is always a cast.
 *     dir      what the CDF sampler gives for that cell: Philox counter (pix, sample, 1 + b, 73)
 *              under the params' seed, words o; gx = action / 12, gy = action % 12;
 *              dir = grid_direction(gx + u01(o[0]), gy + u01(o[1]), N, T, B, pos).
 *     tp       c = dot(N, dir), pdf = RHO * 2.0f, tp = (tp * c) / pdf per channel, the multiply
 *              and the divide each rounded once.  The constant pdf is the reference's (:547): it
 *              is not the density the direction was drawn with, so the estimator is biased on
 *              purpose -- the mode shows where the network points, it does not converge to
 *              the reference image.
 *   The reference also draws rv = curand_uniform (:508) and never uses it; with a counter-based
 *   generator an unused draw consumes nothing, so none is made.
 *   The frame is otherwise rt_render_dqn's: the camera pass, the bounce loop with its early
 *   stop, the accumulation.  A pixel does not depend on the tile list,
 *   RTMI_DQN_RAYS_IN_FLIGHT, the forward kernel (rt_dqn_set_mlp), the cast route, or the route
 *   of the action: inside the streaming forward's epilogue on its LDS tile (4 B per ray leave
 *   the kernel), or (RT_DQN_MLP_STATIONARY networks, RTMI_DQN_MAX_FUSED=0 in the environment,
 *   read per call) k_dqn_argmax on the fp32 Q the forward wrote.
 * Another mode, or a NULL handle: RT_E_INVALID. */
#define RT_DQN_SAMPLE_CDF 0
#define RT_DQN_SAMPLE_MAX 1
int rt_dqn_set_sampling(rt_dqn* dqn, int mode);
int rt_dqn_get_sampling(const rt_dqn* dqn, int* mode);
/* RT_DQN_SAMPLE_MAX's sampler alone for n rays given their Q values (host arrays, rt_dqn_sample's
 * arguments and checks): action, direction and throughput as defined above; q is read and not
 * modified; the action comes from k_dqn_argmax. */
int rt_dqn_sample_max(rt_ctx* ctx, const rt_scene* scene, uint64_t seed, const float* q, const float* loc,
                      const int32_t* tri, const uint32_t* pix, int n, int sample, int bounce, float* tp,
                      float* dir_out, int32_t* action);
/* Statistics of the last rt_render_dqn or rt_render_dqn_tiles_device on this context, in either
 * sampling mode -- how the thesis reads fig:1_spp_max_dir: paths = the call's valid rays
 * (its pixels x spp); zero_paths = those whose final throughput, the value added to the pixel,
 * has every channel < 1e-4f (THROUGHPUT_THRESHOLD of sum_zero_contribution_light_paths,
 * nn_rendering_helpers.cu:555-568; a NaN channel is not below it, so such a ray is not
 * counted).  The sum of path lengths is the cast count the render already returns (a path's
 * length is its ray casts), so there is no third counter.  A blocking copy: after the
 * stream-ordered entry synchronise the stream first.  Either pointer may be NULL.  Before any
 * counted render on the context: RT_E_INVALID.  A tile render's sums cover the call's tiles (add
 * them over ranks).  Counted by one small kernel per pass that reads the throughputs; it
 * changes no pixel and no cast count.
 * rt_dqn_enable_stats(ctx, on): the kernel is launched only by renders after on != 0 (default
 * off; a property of the context).  Measured on BASELINE config 4's frame the counting cost more
 * than the run-to-run spread of the frame itself, so a frame that does not
 * ask for the statistics runs exactly the launches it ran before they existed; after a render
 * with the statistics off rt_dqn_render_stats returns RT_E_INVALID. */
int rt_dqn_enable_stats(rt_ctx* ctx, int on);
int rt_dqn_render_stats(const rt_ctx* ctx, uint64_t* paths, uint64_t* zero_paths);

/* The Q-network view: the network's irradiance estimate at every camera hit, the network's
 * side of the thesis's comparison (Images/neural_q_visualisation.png beside
 * expected_sarsa_visualisation.png, 4_critical_evaluation.tex); it replaces no reference
 * interface.  The map's side is rt_render_irradiance.
 *
 * Per sample s in [first_sample, first_sample + spp) of every pixel: the camera ray
 * rt_render_dqn casts for sample index s (k_dqn_camera: jitter draw2(pix, s, 0, seed), pixel
 * key y * W + x), its closest hit under the GPU hit rule and t_scale, the hit point p being the
 * one the renderer hands the network at bounce 1.  At a hit on surface `tri`:
 *   Q[0..143]  the fp32 forward at p, rt_dqn_forward's value bit for bit (not the bf16 copy the
 *              renderer keeps between forward and sampler);
 *   c_k = chiu_cos(gx + 0.5f, gy + 0.5f), k = gx * 12 + gy: the cell-centre cosine, in float32
 *              1 - xx * xx with xx = max(|2 (g / 12) - 1|) over the two coordinates;
 *   t_k = Q_k * c_k (one rounded multiply, never contracted into the sum);
 *   B_w = (t_36w + t_36w+1) + .. + t_36w+35, added one after another in k order, w = 0..3;
 *   S = ((B_0 + B_1) + B_2) + B_3 (sample_from_q's blocking);
 *   L = (S * brdf[tri]) * ((2 pi) / 144), brdf[tri] the luminance / pi a radiance volume on that
 *              surface carries, the constant rt_render_irradiance's;
 *   the sample is (L, L, L), or with tint != 0 albedo * (L / luminance), 0 where the luminance is 0;
 *   action = the first k of largest t_k: a scan from k = 0 that replaces on >, from -inf, so a
 *              NaN never wins (0 if no t_k exceeds -inf).
 * A light gives its emission, a miss params->env_light.  The pixel is
 * (((v_s0 + v_s0+1) + ..) / (float)spp, folded in sample order whatever number of sample slots
 * a pass holds.  spp_split, max_bounces and sampler are ignored.
 *
 * How to read the number: for a volume whose Q row is q, rt_sarsa_write makes the map's
 * estimate initial_irradiance(c, q, luminance) * (2 pi / 144); a network that returns q at that
 * point gives the same value up to the rounding of a 144-term fp32 sum against a double one.
 * So this view and rt_render_irradiance with k = 1 are on one scale, and their difference
 * shows where the network departs from the map it was fitted to.
 *
 * out_tri / out_pos / out_q / out_action (each may be NULL) describe sample first_sample:
 * out_tri -1 for a miss and >= n_surf for a light; out_pos and out_q zeros and out_action -1
 * unless a surface was hit.  The network, the scene and its tables are read only; the call
 * uses the context's DQN workspace as rt_render_dqn does.  A pixel does not depend on the tile
 * list, RTMI_DQN_RAYS_IN_FLIGHT, the forward kernel (rt_dqn_set_mlp), the cast route, or the
 * route of the reduction: inside the streaming forward's epilogue on its LDS tile, or (out_q
 * requested, RT_DQN_MLP_STATIONARY networks, RTMI_DQN_VIEW_FUSED=0 in the environment, read
 * per call) k_dqn_view_reduce on the Q the forward wrote.
 * Refused before any device work: NULL required pointers, an unknown mode, size or spp <= 0
 * (RT_E_INVALID); another preset or hit rule than the GPU engine's (RT_E_UNSUPPORTED).
 * n_tiles == 0 is RT_OK. */
#define RT_DQN_VIEW_IRRADIANCE 0
typedef struct {
    int32_t mode; /* RT_DQN_VIEW_IRRADIANCE */
    int32_t tint; /* != 0: times the surface's albedo / luminance, as rt_irr_opts.tint */
} rt_dqn_view_opts;
int rt_render_dqn_view(rt_ctx* ctx, const rt_scene* scene, const rt_dqn* dqn, const rt_camera* cam,
                       const rt_params* params, const rt_dqn_view_opts* opts, uint32_t first_sample,
                       float* out_rgb /* W x H x 3 */, int32_t* out_tri, float* out_pos /* W x H x 3 */,
                       float* out_q /* W x H x 144 */, int32_t* out_action /* W x H */);
int rt_render_dqn_view_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_dqn* dqn,
                                    const rt_camera* cam, const rt_params* params,
                                    const rt_dqn_view_opts* opts, uint32_t first_sample,
                                    const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                                    void* stream);

/* ---- Neural-Q training ---------------------------
 * The learning rule of NeuralQPathtracer::render_frame
 * (GPU/deep_learning/neural_q_pathtracer.cu:420-513), which the reference runs through
 * DyNet on the host, on device buffers in fp32: parameters, gradients and Adam moments
 * live on the device; rt_dqn_trainer_params copies the weights out (row-major, the
 * rt_dqn_create layout) to rebuild the bf16 inference network. */
typedef struct rt_dqn_trainer rt_dqn_trainer;
/* DQNetwork::initialize (NN_Builders/dq_network.cu:8-33) with the given parameters +
 * dynet::AdamTrainer(model) (neural_q_pathtracer.cu:47): DyNet defaults beta1 0.9,
 * beta2 0.999, eps 1e-8, global gradient-norm clipping at 5; learning_rate (DyNet 1e-3). */
int rt_dqn_trainer_create(rt_ctx* ctx, const float* nn_vertices, int n_in, const int32_t* hidden /* 3 */,
                          int n_out, const float* const* W /* 4 */, const float* const* b /* 4 */,
                          float learning_rate, rt_dqn_trainer** out);
int rt_dqn_trainer_destroy(rt_dqn_trainer* trainer);
int rt_dqn_trainer_params(const rt_dqn_trainer* trainer, float* const* W /* 4 */, float* const* b /* 4 */);
/* The gradients of the last training step (d loss / d parameter, as the backward pass wrote
 * them: before the clipping scale is applied), in the layout of rt_dqn_trainer_params.
 * Like rt_dqn_trainer_params a blocking copy (it waits for the device); a step left in
 * flight on another stream must be synchronised by the caller first.  RT_E_INVALID if no
 * step has run on this trainer. */
int rt_dqn_trainer_gradients(const rt_dqn_trainer* trainer, float* const* W /* 4 */, float* const* b /* 4 */);
/* Steps 5-7 of the training loop (neural_q_pathtracer.cu:478-513) on n rays: forward on the
 * current states (network input nn_vertices - loc), pick the taken actions, loss =
 * sum (target - q_a)^2 (sum_batches), backward, trainer.update().  Device arrays:
 * d_loc n x 3, d_action n (an action outside [0, n_out) contributes nothing), d_target n.
 * loss_out / grad_norm_out (host, optional; either one synchronises the stream): the loss
 * and the gradient L2 norm before clipping. */
int rt_dqn_train_step_device(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* d_loc, const int32_t* d_action,
                             const float* d_target, int n, float* loss_out, float* grad_norm_out, void* stream);
/* compute_td_targets (GPU/deep_learning/nn_rendering_helpers.cu:91-140): target =
 * reward + max_a(Q(s',a) cos_a) * discount, reward alone where terminal == 1; action 0 is
 * not cosine-weighted (as in the reference); cos_a of a jittered direction in cell a
 * (Philox: pixel, sample, event 1 + bounce).  d_next_q: n x 144 row-major. */
int rt_dqn_td_targets_device(rt_ctx* ctx, uint64_t seed, const float* d_next_q, const int32_t* d_terminal,
                             const float* d_reward, const float* d_discount, const uint32_t* d_pix, int sample,
                             int bounce, int n, float* d_target, void* stream);
/* Q of n positions from the trainer's current parameters: the forward pass that
 * rt_dqn_train_step_device and rt_neuralq_render_frame run (fp32, not the bf16 inference
 * network of rt_dqn_forward), its output copied to d_q (device, n x n_out row-major).
 * d_loc: device, n x 3.  Read-only for the trainer: parameters, Adam moments and the update
 * count are untouched (the workspace may grow).  Asynchronous on `stream`. */
int rt_dqn_trainer_forward_device(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* d_loc, int n, float* d_q,
                                  void* stream);

/* ---- Q-network fit to a radiance map (the reference's NN_Q_Value_Trainer) ----
 * The supervised stage between rt_sarsa_save_q and rt_render_dqn
 * (NN_Q_Value_Trainer/Source/main.cu:118-294): the network is fitted to the rows
 * "position -> all Q values" of a trained radiance map, squared distance over every output,
 * Adam, batches of 128 rows, 100 epochs, an 80/20 train/test split with the test error per
 * epoch.  It runs on an rt_dqn_trainer, so a fitted network can go on into rt_neuralq_create
 * or, through rt_dqn_trainer_params, into rt_dqn_create / rt_dynet_write.  DyNet is not
 * available: parity is against the fp64 restatement, unpinned against DyNet itself.
 *
 * rt_dqn_fit_order: the split and the shuffle (main.cu:126 std::random_shuffle, :147-156
 *   rand() / RAND_MAX < 0.8), host only, with Philox in place of rand().  Row i draws the
 *   Philox4x32-10 block of key (seed lo, seed hi) and counter (i, 0, 0, RT_DQN_FIT_TAG): word 3
 *   is 0 in every render draw and 0x566F726F in the Voronoi palette, so the stream is apart
 *   from both.  u = (w0 >> 8) 2^-24; the row trains if u < train_fraction (compared in float),
 *   else it is a test row.  order: the training rows, then the test rows, each set ascending
 *   in (w1, i) -- a random permutation, ties broken by the index.  train_fraction in (0, 1]
 *   (the reference: 0.8); n >= 0. */
#define RT_DQN_FIT_TAG 0x51466974u /* "QFit" */
int rt_dqn_fit_order(uint64_t seed, int32_t n, float train_fraction, int32_t* order /* n */, int32_t* n_train);
/* One update of main.cu:192-238 on n rows: forward on the positions (network input
 * nn_vertices - loc, main.cu:25-36), loss = sum_b sum_a (target - q)^2
 * (sum_batches(squared_distance)), backward, trainer.update().  The output gradient is
 * q > 0 ? -2 (target - q) : 0 for every element: a dead output counts in the loss and passes
 * no gradient, as in rt_dqn_train_step_device.  Device arrays: d_loc n x 3, d_target n x n_out
 * (row-major; any 4-byte alignment: the result does not depend on it).  Otherwise as
 * rt_dqn_train_step_device: asynchronous on `stream`, either out pointer synchronises, the loss
 * and the gradient norm before clipping; the trainer's update count advances, so fit steps and
 * Neural-Q steps on one trainer share Adam's time. */
int rt_dqn_fit_step_device(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* d_loc /* n x 3 */,
                           const float* d_target /* n x n_out */, int n, float* loss_out, float* grad_norm_out,
                           void* stream);
/* The middle of that step alone, on the caller's device arrays (for measurement and checks):
 * the loss sum (target - q)^2 over d_q and d_target (n x n_out each) and the output gradient
 * into d_dq (n x n_out, every element written).  Nothing of the trainer but its reduction
 * scratch is touched.  loss_out (host, optional) synchronises the stream. */
int rt_dqn_fit_loss_device(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* d_q, const float* d_target, int n,
                           float* d_dq, float* loss_out, void* stream);
/* The test loop of main.cu:241-277: sum_b ||target_b - Q(loc_b)||^2 with no update.  The
 * forward runs in chunks of RT_DQN_FIT_ERROR_CHUNK rows, so the trainer's workspace does not
 * grow with n.  Each difference is the fp32 target - q; its square and every sum are double,
 * in an order that depends on n and n_out alone: bit-identical run to run.  Parameters,
 * moments, gradients and the update count are untouched.  n = 0 gives 0.  error_out (host,
 * required) synchronises the stream. */
#define RT_DQN_FIT_ERROR_CHUNK 4096
int rt_dqn_fit_error_device(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* d_loc, const float* d_target,
                            int n, double* error_out, void* stream);
/* The data set of a fit: the reference's radiance_map_data (host arrays pos n x 3, q n x
 * n_actions, e.g. rt_qtable_read's or rt_sarsa_volumes' + rt_sarsa_read's), uploaded once in
 * the order of rt_dqn_fit_order(seed, n, train_fraction): every batch and the test set are
 * contiguous device slices.  The trainer is borrowed (as rt_neuralq_create borrows it) and
 * must outlive the fit.  RT_E_INVALID: n_actions differs from the trainer's output width,
 * batch_size <= 0, n <= 0, a value that is not finite (an in-frame RT_SARSA_SAMPLE_MAX map can
 * hold infinities), or a split that leaves no training row.  An empty test set is allowed
 * (its error is 0). */
typedef struct rt_dqn_fit rt_dqn_fit;
int rt_dqn_fit_create(rt_ctx* ctx, rt_dqn_trainer* trainer, const float* pos, const float* q, int32_t n,
                      int32_t n_actions, uint64_t seed, float train_fraction, int32_t batch_size,
                      rt_dqn_fit** out);
int rt_dqn_fit_destroy(rt_dqn_fit* fit);
/* n_batches = ceil(n_train / batch_size); any pointer may be NULL */
int rt_dqn_fit_info(const rt_dqn_fit* fit, int32_t* n_train, int32_t* n_test, int32_t* n_batches,
                    int32_t* epochs_done);
/* One pass of main.cu:186-284: rt_dqn_fit_step_device on the n_batches batches in order (the
 * last one ragged), then rt_dqn_fit_error_device on the test rows under the updated
 * parameters.  Nothing waits for the device between batches; the steps' float losses are
 * added on the device in double, in batch order; the call synchronises once, at its end.
 * loss_out / error_out (host, each may be NULL): the reference's printed "Loss:" and
 * "Error:". */
int rt_dqn_fit_epoch(rt_ctx* ctx, rt_dqn_fit* fit, double* loss_out, double* error_out, void* stream);

/* NeuralQPathtracer (GPU/deep_learning/neural_q_pathtracer.cu:226-600): renders while
 * training `trainer`'s network, on the device.  Per sample: initialise_ray (:604-643); per
 * bounce b until no path is bouncing or max_bounces: (b > 0) the network's Q at every ray's
 * position and sample_batch_ray_directions_epsilon_greedy (nn_rendering_helpers.cu:330-389:
 * importance_sample_direction with probability 1 - epsilon, else a uniform cell), trace_ray
 * (:646-745: rewards 0 / light luminance x 200, discount = the surface's luminance,
 * throughput on contributing paths), (b > 0) the learning rule per batch of batch_size rays
 * (compute_td_targets on the new positions, trainer.update on the old ones with the sampled
 * actions, neural_q_pathtracer.cu:420-513), sample_random_scene_pos_for_terminated_rays
 * (:241-277, restarted rays learn but no longer contribute; the point is stored with y and
 * z exchanged, as the reference stores it).  After a sample epsilon = max(epsilon -
 * decay, min) (:543-546).  The frame is the throughput summed over the samples / spp.
 * Reference settings: batch 4096, epsilon 0.05 / 0.05 / 0.01 (deep_learning_settings.h).
 * stats (optional, spp x 3 floats): per sample the nn_training_stats.txt values (:553-583):
 * average path length (sum of termination bounces / pixels), loss (summed over batches),
 * zero-contribution paths (every channel < THROUGHPUT_THRESHOLD).  out_rgb: W x H x 3 or
 * NULL.  Pixel ids key the RNG (Philox; seed = params->seed); successive frames continue
 * the sample sequence. */
typedef struct rt_neuralq rt_neuralq;
int rt_neuralq_create(rt_ctx* ctx, const rt_scene* scene, rt_dqn_trainer* trainer, int batch_size,
                      float epsilon_start, float epsilon_min, float epsilon_decay, rt_neuralq** out);
int rt_neuralq_destroy(rt_neuralq* nq);
int rt_neuralq_epsilon(const rt_neuralq* nq, float* epsilon);
int rt_neuralq_render_frame(rt_ctx* ctx, rt_neuralq* nq, const rt_camera* cam, const rt_params* params,
                            float* out_rgb, float* stats, uint64_t* out_ray_casts);
/* The per-ray arrays as the last frame left them (host copies, one ray per pixel, id =
 * y * width + x; for checks): position, throughput, throughput summed over the frame's samples
 * (n x 3 each), surface of the position, state (0 contributing, 1 terminal, 2 restarted),
 * bounce of termination, sampled action, reward, discount, terminal flag (n each).  NULL
 * outputs are skipped; n_rays (optional) receives n, so a first call with only n_rays sizes
 * the buffers.  RT_E_INVALID before the first frame.  A blocking copy. */
int rt_neuralq_read_rays(const rt_neuralq* nq, float* loc, float* throughput, float* total, int32_t* tri,
                         uint32_t* state, uint32_t* bounces, int32_t* action, float* reward, float* discount,
                         int32_t* terminal, int32_t* n_rays);

/* ---- Expected-SARSA radiance volumes (BASELINE config 3) ------------------ */
typedef struct rt_sarsa rt_sarsa;

/* RadianceMap::RadianceMap (GPU/radiance_volumes/radiance_map.cu:8-55): floor(area/0.001)
 * radiance volumes per surface, placed by rejection point picking (Philox stream of `seed`
 * in place of rand()), each with Q = 100/144 per sector, CDF k/144 and the irradiance of
 * initialise_radiance_grid (radiance_volume.cu:46-89); the KD tree of radiance_tree.cu in
 * its array form.  The map lives on the context's device. */
int rt_sarsa_create(rt_ctx* ctx, const rt_scene* scene, uint64_t seed, rt_sarsa** out);
/* The same with the volume density as an argument: floor(area / area_per_sample) volumes per
 * surface -- AREA_PER_SAMPLE (GPU/constants/radiance_volumes_settings.h:12), a compile-time
 * constant of the reference (0.001f) that its thesis runs varied (Images/door_room/
 * sarsa_128_344_volumes.bmp, 4_critical_evaluation.tex:240-245).  area_per_sample must be a
 * finite float > 0; rt_sarsa_create(...) is rt_sarsa_create_density(..., 0.001f, ...). */
int rt_sarsa_create_density(rt_ctx* ctx, const rt_scene* scene, uint64_t seed, float area_per_sample,
                            rt_sarsa** out);
int rt_sarsa_destroy(rt_sarsa* sarsa);
/* sizes: volumes, KD array elements, frames rendered so far (any pointer may be NULL) */
int rt_sarsa_info(const rt_sarsa* sarsa, int32_t* n_volumes, int32_t* n_nodes, uint32_t* frames);
/* Nearest-volume search of find_closest_radiance_volume_iterative
 * (GPU/radiance_volumes/radiance_map.cu:149-203).  Both modes return the same volume
 * for every query: RT_SARSA_SEARCH_KD walks the reference's KD array;
 * RT_SARSA_SEARCH_GRID (default) answers from a per-normal uniform grid when the
 * nearest same-normal volume is provably a leaf the KD walk visits and is unique,
 * and walks the KD array otherwise (counted in kd_fallbacks). */
#define RT_SARSA_SEARCH_KD 0
#define RT_SARSA_SEARCH_GRID 1
int rt_sarsa_set_search(rt_sarsa* sarsa, int mode);
/* Direction sampling at a surface with a radiance volume:
 * RT_SARSA_SAMPLE_CDF (default) RadianceVolume::sample_direction_from_radiance_distribution
 *   (radiance_volume.cu:191-244), the CDF by inverse transform;
 * RT_SARSA_SAMPLE_MAX sample_max_direction_from_radiance_distribution (:246-278): the first
 *   sector of largest Q (of the previous frame), uniform within it, pdf = RHO x its CDF step
 *   / GRID_RHO -- 0 for sector 0, as the reference computes it (the path's throughput is
 *   then infinite).  TD learning is the same in both modes. */
#define RT_SARSA_SAMPLE_CDF 0
#define RT_SARSA_SAMPLE_MAX 1
int rt_sarsa_set_sampling(rt_sarsa* sarsa, int mode);
/* TD learning rule (replaces the reference's in-kernel update,
 * GPU/radiance_volumes/radiance_volume.cu:282-301 temporal_difference_update and :93-112
 * expected_sarsa_irradiance, called from radiance_map.cu:90-146):
 * RT_SARSA_TD_FRAME (default) every TD target of a frame goes into a per-sector
 *   fixed-point sum and count; the frame end folds them into Q in closed form (the running
 *   mean alpha = 1/(1 + visits) gives) -- deterministic, bit-exact against oracle/, the same
 *   on any GPU count;
 * RT_SARSA_TD_INFRAME the reference's own rule: each event updates the sector's Q, visits
 *   and the volume's irradiance in place while the frame renders (later targets of the same
 *   frame see it; concurrent updates race as in the reference).  The CDFs still change only
 *   at the frame end (update_radiance_volume_distributions).  SAMPLE_MAX then scans the
 *   live Q at every sample, as the reference's scan of its radiance grid does.  Not
 *   reproducible run to run (a launch with one active lane is: the events then run in the
 *   restatement's order); one GPU only: rt_sarsa_td_device and a tile render with apply = 0
 *   return RT_E_UNSUPPORTED in this mode.
 * RT_SARSA_TD_OFF no learning: a frame samples the map as it stands (the CPU engine's
 *   draw_importance_sampling_path_tracing, Old_CPU_Rendering_Engine/Source/path_tracing/
 *   importance_sampling_path_tracing.cpp, on the GPU engine's map).  The render kernels are
 *   instantiated with the TD event, its atomics and its irradiance load compiled out; no
 *   sum, count, Q, visit, irradiance or CDF changes and nothing is applied at the frame end
 *   (rt_render_sarsa_tiles_device ignores `apply`, so a frame splits across GPUs with no
 *   exchange).  `frames` still advances, so successive frames draw fresh samples and can be
 *   averaged; rt_sarsa_frame_stats works as before; RT_SARSA_SAMPLE_MAX reads the stored
 *   arg-max.  A frame's image, casts and statistics are those a RT_SARSA_TD_FRAME frame of
 *   the same map gives, bit for bit. */
#define RT_SARSA_TD_FRAME 0
#define RT_SARSA_TD_INFRAME 1
#define RT_SARSA_TD_OFF 2
int rt_sarsa_set_td_mode(rt_sarsa* sarsa, int mode);
int rt_sarsa_get_td_mode(const rt_sarsa* sarsa, int* mode);
/* Paths in flight of the in-frame rule's render.  Its races -- and with them how fast a frame
 * learns -- depend on how many paths update the table at once: the reference's GTX 1070 Ti
 * holds at most 19 SMs x 2048 threads = 38,912.  lanes > 0 caps the render's persistent grid
 * at ceil(lanes / 256) workgroups of 256 lanes (the image and its statistics are then
 * rendered by fewer lanes, each taking more work items); 0 (default): the device's full
 * occupancy.  No effect on the frame-synchronous rule's results. */
int rt_sarsa_set_inframe_lanes(rt_sarsa* sarsa, int lanes);
/* Training statistics of the last frame rendered (GPU/main.cu:321-339, one line of
 * Radiance_Map_Data/sarsa_training_stats.txt per frame): path_floor_sum = the sum over the
 * frame's pixels of int(path lengths / spp) (path_trace_reinforcement,
 * reinforcement_path_tracing.cu:27-44; a path's length is its ray casts), zero_paths = the
 * paths whose mean radiance (r + g + b) / 3 < THROUGHPUT_THRESHOLD.  The reference's line is
 * "<path_floor_sum / pixels, integer division> 0 <zero_paths>".  For rt_render_sarsa_tiles_device
 * the sums cover the call's tiles (add them over ranks). */
int rt_sarsa_frame_stats(const rt_sarsa* sarsa, uint64_t* path_floor_sum, uint64_t* zero_paths);
/* On-disk formats of the reference's Q-tables.
 * rt_sarsa_save_q: RadianceMap::save_q_vals_to_file (GPU/radiance_volumes/radiance_map.cu:236-266):
 *   "144\n", then one line per volume in map order: "x y z Q0 .. Q143" (ostream defaults,
 *   6 significant digits).
 * rt_sarsa_save_selected: RadianceMap::save_selected_radiance_volumes_vals (radiance_map.cu:270-301):
 *   for each "x y z nx ny nz" line of to_select_path (RMD/selected_radiance_volumes/to_select.txt),
 *   the nearest volume (rt_sarsa_nearest) as "px py pz nx ny nz d0 .. d143" with its sector
 *   distribution (the CDF differenced: convert_radiance_distribution, radiance_volume.cu:332-336);
 *   out_path is replaced.  Both return RT_E_IO on file errors. */
int rt_sarsa_save_q(const rt_sarsa* sarsa, const char* path);
/* The Q-table back into a map: a file of rt_sarsa_save_q / save_q_vals_to_file, whose
 * volume positions must be this map's (same scene and seed: RT_E_INVALID otherwise).  Q is
 * set from the file (std::stof of the printed values), the irradiance estimate recomputed
 * as initialise_radiance_grid does for a Q grid (radiance_volume.cu:46-63), the CDF as
 * update_radiance_distribution (:148-188); visits are kept.  The reference reads its
 * per-volume files back only to draw them (read_radiance_volumes_from_file,
 * radiance_volume.cu:377-440); this resumes training or renders from a saved map.
 * save_q -> load_q -> save_q reproduces the file byte for byte. */
int rt_sarsa_load_q(rt_sarsa* sarsa, const char* path);
/* The same file without a map: load_radiance_map_data (NN_Q_Value_Trainer/Source/main.cu:73-116),
 * the input of the Q-network fit (rt_dqn_fit_create).  First line: the action count; then one
 * line "x y z Q0 .. Q(A-1)" per row; every value is strtof of its printed token (std::stof).
 * Host only.  Two passes, like rt_dynet_read: with pos and q NULL the call sizes (*n_rows,
 * *n_actions out); with both given, *n_rows and *n_actions hold on entry the sizes the arrays
 * were allocated for (the sizing pass's) and the file must still have them.  pos: n_rows x 3,
 * q: n_rows x n_actions.  Lines of blanks are skipped.  A missing file, a row with too few or
 * too many tokens, a token that is not a number, or an action count <= 0 returns RT_E_IO
 * with the line's number in the message.  rt_sarsa_load_q reads through the same parser. */
int rt_qtable_read(const char* path, int32_t* n_rows, int32_t* n_actions, float* pos /* n x 3 */,
                   float* q /* n x n_actions */);
int rt_sarsa_save_selected(rt_ctx* ctx, const rt_sarsa* sarsa, const char* to_select_path,
                           const char* out_path);
int rt_sarsa_search_stats(const rt_sarsa* sarsa, int32_t* mode, int32_t* n_classes, int64_t* grid_cells,
                          uint64_t* kd_fallbacks);
/* host copies: pos n x 3, normal n x 3, surface index n, KD array n_nodes x 12 words
 * {dim, leaf, left, right (int32), data, px, py, pz, nx, ny, nz (float), vol (int32)} */
int rt_sarsa_volumes(const rt_sarsa* sarsa, float* pos, float* normal, int32_t* surface,
                     float* kd_nodes);
/* Q-table (radiance_grid), CDF (radiance_distribution), visits (n x 144, sector x*12+y) and
 * irradiance_accum (n) after the last applied frame; NULL pointers are skipped. */
int rt_sarsa_read(const rt_sarsa* sarsa, float* q, float* cdf, uint32_t* visits,
                  float* irradiance);
/* The counterpart of rt_sarsa_read: host arrays into the volumes [v0, v0 + n) of the map.  Q is
 * set from q (n x 144); the irradiance estimate and the CDF (with its row ends and arg-max)
 * are recomputed as rt_sarsa_load_q does, by the same code, with no text file in between;
 * visits (n x 144) are set, or kept when NULL.  Pending TD sums are left alone.  What a
 * multi-GPU bake gathers into: each rank bakes a slice, the Q rows are gathered, every rank
 * writes them.  RT_E_INVALID for a range outside the map; n = 0 is RT_OK. */
int rt_sarsa_write(rt_sarsa* sarsa, int v0, int n, const float* q /* n x 144 */,
                   const uint32_t* visits /* n x 144, or NULL: kept */);
/* Fill the volumes [v0, v0 + n) from ground truth, on the device (k_bake, csrc/rt_bake.hip): the
 * CPU engine's map, whose volumes are filled by sampling the incoming radiance per sector at
 * construction (Old_CPU_Rendering_Engine/Source/radiance_volumes/radiance_map.cpp,
 * radiance_volume.cpp), for the GPU engine's 12 x 12 scalar grid.  With rad what
 * rt_probe_radiance gives for {pos = the volume's position, tri = its surface, ids = v} under
 * the same params and first_sample, bit for bit (a volume's sector k is the probe's: both
 * frames are normal_frame of the surface's stored normal):
 *   Q[v][k] = max(vol_brdf[v] * ((rad.r + rad.g) + rad.b) / 3, RADIANCE_THRESHOLD)
 *   (vol_brdf = the surface's luminance / pi; NaN gives the floor), visits[v][k] = spp, the
 *   sector's pending TD sum and count = 0,
 * then the volume's irradiance estimate and CDF as rt_sarsa_write computes them from that Q.
 * vol_brdf * luminance is what the TD rule's own targets converge to; its floor keeps every
 * sector's pdf above zero, so a render from a baked map stays unbiased; visits = spp makes
 * later training weigh the baked value as spp observations.  Nothing moves to the host.  A
 * volume's result depends on neither v0, n, the entry's internal batching nor the cast route.
 * Asynchronous on `stream` unless out_casts (the closest-hit calls, host) is given.
 * RT_E_INVALID for a range outside the map and whatever rt_probe_radiance refuses in params
 * (spp <= 0, spp_split not dividing spp, max_bounces < 1, bad sampler / hit_rule);
 * RT_E_UNSUPPORTED for a preset other than RT_PRESET_GPU; the map is then untouched.  n = 0 is
 * RT_OK; max_bounces = 1 gives the floor everywhere and 0 casts. */
int rt_sarsa_bake(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_params* params, int v0,
                  int n, uint32_t first_sample, uint64_t* out_casts /* may be NULL */, void* stream);
/* An expected-value sweep of the volumes [v0, v0 + n), on the device (k_sweep, csrc/rt_sweep.hip):
 * the Expected-SARSA target of a sector is one cast long, and evaluated from every volume's own
 * position instead of along camera paths it is value iteration over the map -- every sector of
 * every volume visited equally, no pixels, and light travels one bounce further per sweep.  For
 * volume v, sector k and sample s in [first_sample, first_sample + params->spp):
 *   the first ray of rt_sarsa_bake's (v, k, s): Philox counter (v * 144 + k, s, 1, 73),
 *     grid_direction in the surface's shading frame, o = pos + dir * 1e-5f, d = normalize(dir);
 *   one closest hit under params->hit_rule and params->t_scale (the bake's cast routes);
 *   target (float32, as the render's TD event forms it, brdf = vol_brdf[v] = the surface's
 *     luminance / pi):  brdf * env_light for a miss, brdf * the light's luminance for a light,
 *     (irradiance[u] * (2 pi / 144)) * brdf for a surface, u = the nearest volume the render
 *     finds for the hit point o + t * (d * t_scale) with the hit surface's stored normal (the
 *     map's search mode; volume 0 where no volume has that normal);
 *   llrint(target * 2^32) joins the sector's pending TD sum and 1 its pending count: the
 *     accumulators a tile render leaves with apply = 0 (rt_sarsa_td_device).
 * The sweep reads only the irradiance estimates as they stand when it starts (Jacobi: it never
 * sees its own results) and writes only the pending sums and counts of its range.  apply != 0
 * then runs rt_sarsa_apply on the stream: the running mean with alpha = 1 / (1 + visits), the
 * RADIANCE_THRESHOLD floor, the irradiance increments and the CDFs.  A sector always receives
 * exactly spp targets: spp_split, max_bounces, sampler, width and height are ignored.  A volume's
 * deposit depends on neither v0, n, the kernel's chunking, the cast route nor the search mode.
 * `scene` is the scene the map was made for.  Asynchronous on `stream` unless out_casts
 * (n * 144 * spp, host) is given.  Refused as rt_sarsa_bake refuses (a range outside the map,
 * spp <= 0, a bad hit_rule: RT_E_INVALID; a preset other than RT_PRESET_GPU: RT_E_UNSUPPORTED),
 * and RT_E_UNSUPPORTED unless the map's TD mode is RT_SARSA_TD_FRAME; the map is then untouched.
 * n = 0 deposits nothing and is RT_OK. */
int rt_sarsa_sweep(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_params* params, int v0,
                   int n, uint32_t first_sample, int apply, uint64_t* out_casts /* may be NULL */,
                   void* stream);
/* visits[v][k] = 0 for the volumes [v0, v0 + n), nothing else (stream-ordered).  The next applied
 * targets then replace Q instead of joining its mean, (Q * 0 + sum) / (0 + n): forget + sweep is
 * a pure Jacobi step, sweep alone averages with what the map knows.  On several GPUs every rank
 * forgets the whole swept range, sweeps its own slice with apply = 0, the sums are all-reduced and
 * every rank applies (rtmi.dist.sarsa_sweep): a separate entry so that this stays bit-identical
 * across ranks.  RT_E_INVALID for a range outside the map; n = 0 is RT_OK. */
int rt_sarsa_forget(rt_sarsa* sarsa, int v0, int n, void* stream);
/* RadianceMap::find_closest_radiance_volume_iterative (radiance_map.cu:149-203), n queries. */
int rt_sarsa_nearest(rt_ctx* ctx, const rt_sarsa* sarsa, const float* pos, const float* normal,
                     int n, int32_t* out);
/* draw_reinforcement_path_tracing + update_radiance_volume_distributions per frame
 * (reinforcement_path_tracing.cu:6-120, GPU/main.cu:296-350), GPU-engine preset: `frames`
 * frames of params->spp samples, each frame learning from the previous frame's Q-table;
 * out_rgb = the last frame (W x H x 3), out_ray_casts = casts of all frames. */
int rt_render_sarsa(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_camera* cam,
                    const rt_params* params, int frames, float* out_rgb, uint64_t* out_ray_casts);
/* One frame over a tile list into device memory (stream-ordered).  apply = 0 leaves the
 * frame's TD sums in the map's accumulators (rt_sarsa_td_device: int64 fixed-point sums,
 * uint32 counts, n x 144 each) for a cross-GPU sum before rt_sarsa_apply. */
int rt_render_sarsa_tiles_device(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa,
                                 const rt_camera* cam, const rt_params* params,
                                 const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                                 uint64_t* d_casts, int apply, void* stream);
int rt_sarsa_td_device(rt_sarsa* sarsa, void** d_sum, void** d_count, int64_t* n_entries);
int rt_sarsa_apply(rt_sarsa* sarsa, void* stream);

/* Radiance-map views: the reference GPU engine's PATH_TRACING_METHOD 2 (GPU/main.cu:414-495,
 * GPU/path_tracing/voronoi_trace.cu, RadianceMap::set_voronoi_colours / get_voronoi_colour,
 * radiance_map.cu:205-225): every camera hit drawn in the colour of its nearest radiance volume.
 *
 * rt_sarsa_voronoi_palette: set_voronoi_colour's random colours (host only).  Volume v gets
 *   u(w0), u(w1), u(w2), u = (x >> 8) 2^-24, of the Philox4x32-10 block with key (seed lo, seed hi)
 *   and counter (v, 0, 0, 0x566F726F): word 3 is 0 in every render draw, so the stream is apart
 *   from them (the reference draws three rand() / RAND_MAX per volume).
 * rt_sarsa_set_view_colours: the map's per-volume colour table (rgb: n_volumes x 3, host; NULL =
 *   the palette of the map's own seed, which a map that never had it called draws with).
 * rt_render_volume_view: per sample s in [first_sample, first_sample + spp) of every pixel, the
 *   camera ray rt_render_sarsa casts for sample index s (jitter: event 0 of counter
 *   (y W + x, s, 0, 0)), its closest hit under params->hit_rule and t_scale, the hit point
 *   o + t (d t_scale), its nearest volume by the map's current search mode, and that volume's
 *   colour; (1, 1, 1) for a light or a miss (voronoi_trace.cu:31-37).  The pixel is the sum of
 *   its spp_split chunk sums in order, divided by spp.  max_bounces, sampler and env_light are
 *   ignored.  out_rgb: W x H x 3.  out_tri, out_vol, out_pos (W x H [x 3], each may be NULL)
 *   describe sample first_sample: the triangle (-1 miss, >= n_surf a light), the volume (-1
 *   unless a surface was hit) and the hit point (zeros unless a surface was hit).  The map is
 *   read only, in every TD mode (only rt_sarsa_search_stats' kd_fallbacks may grow).
 * rt_render_volume_view_tiles_device: the same view over a tile list into device memory,
 *   stream-ordered; tiles and output layout as rt_render_sarsa_tiles_device. */
int rt_sarsa_voronoi_palette(uint64_t seed, int32_t n_volumes, float* rgb /* n_volumes x 3 */);
int rt_sarsa_set_view_colours(rt_sarsa* sarsa, const float* rgb);
int rt_render_volume_view(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_camera* cam,
                          const rt_params* params, uint32_t first_sample, float* out_rgb, int32_t* out_tri,
                          int32_t* out_vol, float* out_pos);
int rt_render_volume_view_tiles_device(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa,
                                       const rt_camera* cam, const rt_params* params, uint32_t first_sample,
                                       const int32_t* tiles, int n_tiles, int tile_size, float* d_out,
                                       void* stream);

/* The k nearest radiance volumes, and the irradiance render of the map on top of them: the CPU
 * engine's fifth drawing mode, draw_radiance_map_path_tracing
 * (Old_CPU_Rendering_Engine/Source/path_tracing/precompute_irradiance_path_tracing.cpp:3-53): one
 * camera ray per sample, no bounce, the pixel the map's own irradiance estimate at the hit point,
 * interpolated over the closest volumes (RadianceMap::get_irradiance_estimate,
 * radiance_map.cpp:93-128; RadianceTree::find_closest_radiance_volumes(n, max_dist, position,
 * normal), radiance_tree.cpp:111-177; CLOSEST_QUERY_COUNT and MAX_DIST,
 * constants/radiance_volumes_settings.h:14-15).
 *
 * rt_sarsa_knn (k_sarsa_knn): for query (p, N) let S be the volumes v whose stored normal equals
 *   N component by component under float == (the reference's rv_normal != vec3(normal) test) and
 *   whose distance d(v) = sqrtf((x x + y y) + z z) of vol_pos[v] - p, every operation rounded on
 *   its own, is < radius.  The result is the min(k, |S|) members of S ascending by (d, v): nearest
 *   first, equal float distances by volume index.  out_vol, out_dist: n x k, unused slots -1 and
 *   +inf; out_count: that number.  A query with a non-finite coordinate, or a normal no volume has,
 *   finds nothing.  The result of a query depends on neither n nor its place in the list.
 *   The search reads the per-normal grid of the map (whatever rt_sarsa_set_search says), which
 *   answers exactly up to rt_sarsa_knn_reach's radius: the grid's accept radius,
 *   sqrt(MAX_DIST) * 0.999 ~ 0.0547; 0 for a map without a grid (host only).
 *   Unlike the reference: its tree walk prunes subtrees by |delta| < max_dist and never tests a
 *   volume's own distance, so with fewer than n volumes in range it can return farther ones.  This
 *   entry never returns a volume at or beyond radius.  Expected neighbours at the reach are
 *   pi reach^2 / area_per_sample: 9.4 at the default 0.001, under 1 at 0.01.
 *   RT_E_INVALID: k outside [1, RT_SARSA_KNN_MAX] or radius not > 0 (both checked before any
 *   pointer), NULL arguments, radius beyond the reach; RT_E_UNSUPPORTED: a map without a grid
 *   (there is no other method behind it).
 * rt_render_irradiance (k_sarsa_irr): per sample s in [first_sample, first_sample + spp) of every
 *   pixel, rt_render_volume_view's camera ray, closest hit and hit point (out_tri and out_pos are
 *   that call's, bit for bit); at a surface hit the opts->k nearest volumes of (hit point, the
 *   surface's stored normal) within opts->radius as rt_sarsa_knn finds them, e_i = irradiance[v_i]
 *   * ((2 pi) / 144) of each (rt_sarsa_read's fourth array), nearest first, and
 *     RT_IRR_MEAN: L = ((e_0 + e_1) + ..) / count -- the reference (its barycentric branch tests
 *                  u + v + w == 1.f on floats and in practice falls through to this mean);
 *     RT_IRR_CONE: w_i = 1 - d_i / radius, L = ((w_0 e_0 + w_1 e_1) + ..) / ((w_0 + w_1) + ..),
 *                  the mean where the weights sum to 0;
 *   L = 0 with no volume in range (the reference returns vec3(0)).  The sample is (L, L, L), or
 *   with opts->tint != 0 albedo * (L / luminance), luminance = 0.5 (max + min) of the albedo (the
 *   reference's irradiance *= diffuse_c; 0 where the luminance is 0).  A light gives its emission,
 *   a miss params->env_light.  Every operation is IEEE fp32, rounded once.  The pixel is the sum of
 *   its spp_split chunk sums in order, divided by spp.  max_bounces and sampler are ignored.
 *   out_vol, out_dist (W x H x k, may be NULL): the volumes of sample first_sample and their
 *   distances (-1, +inf: none, or no surface hit).  The map is read only in every TD mode, and
 *   not even rt_sarsa_search_stats' kd_fallbacks moves.  Refusals as rt_sarsa_knn's (opts->k,
 *   opts->radius and opts->weight by value first) and rt_render_volume_view's.
 * rt_render_irradiance_tiles_device: the same over a tile list into device memory, stream-ordered;
 *   tiles and output layout as rt_render_sarsa_tiles_device. */
#define RT_SARSA_KNN_MAX 8
#define RT_IRR_MEAN 0 /* the reference: the plain average of the volumes found */
#define RT_IRR_CONE 1 /* weights 1 - d / radius */
typedef struct {
    int32_t k;      /* volumes to interpolate over, [1, RT_SARSA_KNN_MAX] (CLOSEST_QUERY_COUNT) */
    float radius;   /* (0, rt_sarsa_knn_reach] */
    int32_t weight; /* RT_IRR_MEAN / RT_IRR_CONE */
    int32_t tint;   /* != 0: times the surface's albedo / luminance */
} rt_irr_opts;
int rt_sarsa_knn_reach(const rt_sarsa* sarsa, float* radius);
int rt_sarsa_knn(rt_ctx* ctx, const rt_sarsa* sarsa, const float* pos /* n x 3 */, const float* normal /* n x 3 */,
                 int n, int k, float radius, int32_t* out_vol /* n x k */, float* out_dist /* n x k, may be NULL */,
                 int32_t* out_count /* n, may be NULL */);
int rt_render_irradiance(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_camera* cam,
                         const rt_params* params, const rt_irr_opts* opts, uint32_t first_sample, float* out_rgb,
                         int32_t* out_tri, float* out_pos, int32_t* out_vol /* W x H x k */,
                         float* out_dist /* W x H x k */);
int rt_render_irradiance_tiles_device(rt_ctx* ctx, const rt_scene* scene, rt_sarsa* sarsa, const rt_camera* cam,
                                      const rt_params* params, const rt_irr_opts* opts, uint32_t first_sample,
                                      const int32_t* tiles, int n_tiles, int tile_size, float* d_out, void* stream);

/* ---- ground-truth incident radiance at surface points ------------------------
 * Replaces no reference interface: the thesis judges what a radiance map or a Q-network
 * learned against "the true incident radiance distribution" at selected points, "calculated by
 * firing 4096 sampled light paths per sector and averaging their incident radiance
 * approximation" (Descriptions/write_up/chapters/4_critical_evaluation.tex:92-110,
 * Images/true_distribution.png beside expected_sarsa_visualisation.png and
 * neural_q_visualisation.png); the reference ships the picture and no code for it.
 *
 * Point p lies on surface tri[p] and takes the scene's normal and tangent frame of that
 * surface, as rt_dqn_sample does.  Sector k = gx * 12 + gy is the sampler's cell k.  Sample s in
 * [first_sample, first_sample + params->spp) of (p, k), Philox pixel word pix = ids[p] * 144 + k:
 *   dir = the direction rt_dqn_sample returns for pixel pix, sample s, bounce 0 when it selects
 *         cell k: grid_dir(gx + u, gy + v), (u, v) = u01 of words 0, 1 of the block with
 *         counter (pix, s, 1, 73) -- computed directly, not through a Q vector;
 *   the ray o = pos + dir * 1e-5f (a multiply, then an add), d = normalize(dir), throughput
 *         (1, 1, 1): nothing is multiplied in at the probed point, the value is incoming radiance;
 *   from there the tail of a GPU-preset rt_render path at depth 1: depth == max_bounces before a
 *         cast ends the path with 0; a miss gives tp * env_light, a light tp * emission, a
 *         surface takes the preset's bounce step with params->sampler (event 1 + depth, counter
 *         word 3 = 0); hit rule params->hit_rule, scale params->t_scale.  width, height and
 *         preset are ignored.
 * out_rad[p][k] = the mean of the paths' values L; out_irr[p][k] = the mean of L * c, c =
 * dot(N, d) of the sample's first ray; both by rt_params' sum definition (spp_split chunks, each
 * summed in sample order, folded ((P0 + P1) + P2) + .., divided by (float)spp; here spp_split may
 * be any divisor of spp).  out_dir[p][k] = dir of sample first_sample.  out_casts = closest-hit
 * calls.  A point's result depends on the scene, params, pos[p], tri[p], ids[p] and first_sample
 * alone -- not on n, the point's place in the list, the launch or the cast route (the scene's
 * bounce-ray candidate table where it has or may build one, the exact BVH when the accel mode
 * turns it on, the filter or the scan otherwise: the same hits) -- and is bit-identical run to
 * run: a multi-GPU split is a split of the point list, and batches of first_sample combine
 * into longer means and give error bars.
 * RT_E_INVALID: a NULL required pointer, n < 0, tri[p] outside [0, n_surf), ids[p] >= 2^32 / 144,
 * spp <= 0 or a split that does not divide it, max_bounces < 1.  n = 0: RT_OK, nothing written.
 * max_bounces = 1: zeros and 0 casts (out_dir is still written).
 * rt_probe_radiance_device: the same on device pointers, asynchronous on `stream`; d_casts is
 * accumulated into; tri and ids are not checked on the host: a point that fails the checks
 * above gets zeros, casts nothing and leaves its out_dir unwritten.  The chunk sums live in a workspace of the context: its probes run one
 * after another. */
#define RT_PROBE_SECTORS 144
int rt_probe_radiance(rt_ctx* ctx, const rt_scene* scene, const rt_params* params, const float* pos /* n x 3 */,
                      const int32_t* tri /* n */, const uint32_t* ids /* n */, int n, uint32_t first_sample,
                      float* out_rad /* n x 144 x 3 */, float* out_irr /* n x 144 x 3, may be NULL */,
                      float* out_dir /* n x 144 x 3, may be NULL */, uint64_t* out_casts /* may be NULL */);
int rt_probe_radiance_device(rt_ctx* ctx, const rt_scene* scene, const rt_params* params, const float* d_pos,
                             const int32_t* d_tri, const uint32_t* d_ids, int n, uint32_t first_sample,
                             float* d_rad, float* d_irr, float* d_dir, uint64_t* d_casts, void* stream);

/* ---- radiance-volume glyphs ------------------------------------------------------
 * The picture the reference judges a radiance map or a Q-network with (thesis ch. 4,
 * Images/expected_sarsa_visualisation.png, neural_q_visualisation.png, true_distribution.png):
 * selected surface points, each drawn as a hemisphere of 12 x 12 coloured sectors inside the
 * scene.  GPU engine: RENDER_SAVED_RADIANCE_VOLUMES (GPU/constants/image_settings.h:15) makes
 * Scene::load_custom_scene (GPU/scenes/scene.cu:41-46) call
 * RadianceVolume::read_radiance_volumes_to_surfaces = read_radiance_volumes_from_file +
 * get_vertices + build_surfaces (GPU/radiance_volumes/radiance_volume.cu:375-515); CPU engine:
 * build_radiance_volume_shapes / build_radiance_magnitude_volume_shapes
 * (CPU/radiance_volumes/radiance_volume.cpp:100-174).  The inputs are the files of
 * rt_sarsa_save_selected, rt_dqn_save_selected and tools/true_distribution.py.
 *
 * Unlike the reference, which appends 288 diffuse triangles per volume to the scene (with
 * hand-written normals) and path traces everything, the glyphs here are an overlay view: the
 * mesh never enters an rt_scene, is unlit, and is composited over any frame the library renders.
 *
 * rt_selected_read: read_radiance_volumes_from_file (radiance_volume.cu:377-440), host only.  One
 *   row "x y z nx ny nz d0 .. d143" per line, every value strtof of its token, through the parser
 *   of rt_qtable_read; lines of blanks are skipped.  Two passes like rt_qtable_read: with pos,
 *   normal and values NULL the call sizes (*n out); with all three given, *n holds on entry the
 *   row count the arrays were allocated for and the file must still have it.  A missing file, a
 *   row with too few or too many tokens, or a token that is not a number returns RT_E_IO with the
 *   line's number in the message.
 * rt_glyph_mesh: get_vertices + build_surfaces (radiance_volume.cu:442-515), host only.  For a
 *   glyph at P with normal N (used as given: the reference does not normalise what it reads) and
 *   diameter D (the reference's DIAMETER, 0.15f, which acts as a radius): (T, B) = the frame of N
 *   (create_normal_coordinate_system); for x, y in 0..12, (xh, yh, zh) = Chiu's map of
 *   (x / 12.f, y / 12.f), each times D in one rounded multiply (xs, ys, zs), and
 *     V[x][y].c = (T.c * xs + N.c * ys) + (B.c * zs + P.c)
 *   Quad k = x * 12 + y (the sector of every other entry point) gives triangle 2k = (V[x][y],
 *   V[x][y+1], V[x+1][y]) and 2k + 1 = (V[x+1][y], V[x][y+1], V[x+1][y+1]), the reference's
 *   (v0, v2, v1) and (v1, v2, v3).  quad_normal[k] = normalize(mid - P), mid = (((v0 + v1) + v2)
 *   + v3) / 4.f per component: what build_surfaces writes over the triangles' normals.
 *   RT_E_INVALID: a non-finite input, a zero normal, D not > 0.
 * rt_glyph_colours: the sector colours, host only.
 *   RT_GLYPH_RATIO (the GPU engine, build_surfaces): m = 0; scanning k upward m = v[k] wherever
 *     m < v[k]; ratio = v[k] / m (0 for a row whose m stays 0); colour (ratio, 1.f - ratio, 0).
 *   RT_GLYPH_MAGNITUDE (the CPU engine, build_radiance_magnitude_volume_shapes): m starts at
 *     0.0001f and takes |v[k]| where that is larger; colour grey 1.f - |v[k]| / m.
 *   Non-finite values: RT_E_INVALID.
 *
 * rt_glyphs_create: a glyph set on the context's device, 0 <= n <= RT_GLYPH_MAX (n = 0 is a valid
 *   empty set): rt_glyph_mesh's triangles as an intersection-record soup of its own, the exact BVH
 *   of rt_bvh.cpp built over it at once, rt_glyph_colours(colour_mode)'s table and the quad
 *   normals.  rt_glyphs_create_sized: the same with a diameter per glyph (diameters: n), for a
 *   picture that mixes sizes.  rt_glyphs_set_colours replaces the table (rgb: n x 144 x 3, the
 *   caller's own).
 *   rt_glyphs_info: glyphs, triangles (288 n), nodes of the BVH (pointers may be NULL).
 *
 * rt_render_glyph_view (k_glyph_view, csrc/rt_glyph.hip): per sample s in [first_sample,
 *   first_sample + spp) of every pixel, rt_render_volume_view's camera ray (jitter draw2(pix, s,
 *   0, seed), camera_ray<1>); H_s its closest hit in the scene under the GPU hit rule and t_scale
 *   (k_sarsa_view's route, or the scene's BVH where its accel mode turns it on: the same hits);
 *   H_g its closest hit in the glyph soup under the same rule.  The winner is the hit of the scan
 *   over the soup "scene surfaces, then glyph triangles, then lights": the glyph wins iff
 *   t_g < t_s, or t_g == t_s and H_s is a light.
 *   The sample's value: glyph triangle j gives glyph j / 288, sector (j % 288) / 2 and that
 *   sector's colour, with opts->shade != 0 every channel times
 *     0.25f + 0.75f * fmaxf(-((nq.x * d.x + nq.y * d.y) + nq.z * d.z), 0.f)
 *   (nq the sector's quad normal, d the ray direction, every operation rounded once; the mesh is
 *   two-sided, as the hit test is).  Otherwise base_rgb[pixel] where a base was given; without a
 *   base a surface gives its albedo, a light its emission and a miss params->env_light.
 *   The pixel is the sum of its spp_split chunk sums in order, divided by (float)spp
 *   (k_sarsa_view's fold).  max_bounces and sampler are ignored.
 *   base_rgb: host W x H x 3 or NULL; out_rgb: W x H x 3, required.  out_tri, out_glyph,
 *   out_sector, out_t (W x H, each may be NULL) describe sample first_sample: out_tri the scene's
 *   own hit, rt_render_volume_view's out_tri bit for bit, glyph in front or not; out_glyph and
 *   out_sector -1 unless a glyph won; out_t the winner's t, +inf for a miss.
 *   The scene, its tables and the glyph set are read only.  A pixel depends on neither the tile
 *   list nor the glyph cast's route: the BVH, or with RTMI_GLYPH_BVH=0 in the environment (read
 *   per call) the plain scan of the soup.
 *   Refused before any device work, params by value first: size or spp <= 0, a bad spp_split
 *   (RT_E_INVALID); another preset or hit rule than the GPU engine's (RT_E_UNSUPPORTED); then
 *   NULL required pointers (RT_E_INVALID).  rt_glyphs_create checks n before its pointers.
 *   The launches are timed under RT_KT_SARSA_VIEW.
 * rt_render_glyph_view_tiles_device: the same over a tile list into device memory,
 *   stream-ordered; tiles and output layout as rt_render_sarsa_tiles_device; d_base: the whole
 *   W x H x 3 image on the device, or NULL.  n_tiles == 0 is RT_OK. */
#define RT_GLYPH_MAX 256      /* glyphs per set: 73,728 triangles */
#define RT_GLYPH_SECTORS 144
#define RT_GLYPH_TRIS 288     /* triangles per glyph */
#define RT_GLYPH_RATIO 0
#define RT_GLYPH_MAGNITUDE 1
typedef struct rt_glyphs rt_glyphs;
typedef struct {
    int32_t shade; /* != 0: the sector colour times 0.25 + 0.75 max(-nq.d, 0) */
} rt_glyph_view_opts;
int rt_selected_read(const char* path, int32_t* n, float* pos /* n x 3 */, float* normal /* n x 3 */,
                     float* values /* n x 144 */);
int rt_glyph_mesh(const float* pos, const float* normal, int32_t n, float diameter,
                  float* tri_v /* n x 288 x 9 */, float* quad_normal /* n x 144 x 3, may be NULL */);
int rt_glyph_colours(const float* values /* n x 144 */, int32_t n, int mode, float* rgb /* n x 144 x 3 */);
int rt_glyphs_create(rt_ctx* ctx, const float* pos, const float* normal, const float* values, int32_t n,
                     float diameter, int colour_mode, rt_glyphs** out);
int rt_glyphs_create_sized(rt_ctx* ctx, const float* pos, const float* normal, const float* values,
                           const float* diameters /* n */, int32_t n, int colour_mode, rt_glyphs** out);
int rt_glyphs_destroy(rt_glyphs* glyphs);
int rt_glyphs_set_colours(rt_glyphs* glyphs, const float* rgb /* n x 144 x 3 */);
int rt_glyphs_info(const rt_glyphs* glyphs, int32_t* n_glyphs, int32_t* n_tri, int32_t* bvh_nodes);
int rt_render_glyph_view(rt_ctx* ctx, const rt_scene* scene, const rt_glyphs* glyphs, const rt_camera* cam,
                         const rt_params* params, const rt_glyph_view_opts* opts, uint32_t first_sample,
                         const float* base_rgb, float* out_rgb, int32_t* out_tri, int32_t* out_glyph,
                         int32_t* out_sector, float* out_t);
int rt_render_glyph_view_tiles_device(rt_ctx* ctx, const rt_scene* scene, const rt_glyphs* glyphs,
                                      const rt_camera* cam, const rt_params* params,
                                      const rt_glyph_view_opts* opts, uint32_t first_sample, const float* d_base,
                                      const int32_t* tiles, int n_tiles, int tile_size, float* d_out, void* stream);

/* Device self-tests of numeric building blocks (no reference counterpart): every
 * bit-exact claim against oracle/ rests on them.  result[0] = mismatches, result[1] = the
 * lowest mismatching input bits (0xffffffff: none).
 * RT_SELFTEST_RCP: the kernels' correctly-rounded reciprocal (Cramer's 1/detA, normalize)
 *   vs IEEE 1.0f / x over all 2^32 floats;
 * RT_SELFTEST_DIV12: the grid-coordinate x / 12 (Chiu map) vs IEEE over its domain,
 *   +0 and |x| in [2^-100, 2^100];
 * RT_SELFTEST_DIVRHO: the estimator's x / RHO vs IEEE over all 2^32 floats;
 * RT_SELFTEST_SQRT_POS: the sampling's square root without range guards vs sqrtf over its
 *   domain, +0 and [2^-96, FLT_MAX];
 * RT_SELFTEST_RCP_IN: the reciprocal without its range guard vs IEEE 1.0f / x over its domain,
 *   |x| in [2^-125, 2^125];
 * RT_SELFTEST_PHILOX_PX: the Philox block split into its pixel, event and sample parts vs the
 *   whole block, all four words, 2^24 counters (pixel, sample, event, 0) for each of two keys, with
 *   the pixel's words wave-uniform and per lane; result[1] = form << 25 | key << 24 |
 *   pixel index << 12 | sample << 2 | event of the lowest mismatch. */
#define RT_SELFTEST_RCP 1
#define RT_SELFTEST_DIV12 2
#define RT_SELFTEST_DIVRHO 3
#define RT_SELFTEST_SQRT_POS 4
#define RT_SELFTEST_RCP_IN 5
#define RT_SELFTEST_PHILOX_PX 6
int rt_selftest(rt_ctx* ctx, int which, uint64_t* result /* 2 */);

/* Host-side checks of the CPU-preset primary-ray cull (k_cull_ps; no GPU needed).
 * rt_filter_build: the per-triangle filter records of the two-phase hit test
 * (5 x float4 per triangle, layout rt_internal.hpp kFiltF4) for the triangle soup
 * tri_v (n x 9, surfaces then lights: the rt_scene_create order).
 * rt_rect_candidates: bit i of masks[i / 64] = triangle i may be the hit of a camera
 * ray through a pixel of [px0, px1] x [py0, py1] (inclusive); the other triangles
 * certainly fail the exact test for every such ray (RT_PRESET_CPU parameters).
 * Replaces no reference interface: it exposes the kernel's own cull so tests can check
 * it against the CPU restatement's hits (Ray::closest_intersection, CPU/rays/ray.cpp:14-28). */
int rt_filter_build(const float* tri_v, int n, float* out_filt /* n x 20 */);
int rt_rect_candidates(const float* filt, int n_tri, const rt_camera* cam, const rt_params* params,
                       int px0, int py0, int px1, int py1, uint64_t* masks /* ceil(n_tri / 64) */);
/* rt_rect_candidates by the route the kernels take: the camera-and-triangle half of the cull
 * once per triangle (what k_cull_forms writes for a launch), the rectangle half after it.
 * The same float operations on the same operands: the masks equal rt_rect_candidates' bit for
 * bit, which is what tests hold it to. */
int rt_rect_candidates_forms(const float* filt, int n_tri, const rt_camera* cam, const rt_params* params,
                             int px0, int py0, int px1, int py1, uint64_t* masks /* ceil(n_tri / 64) */);
/* The same masks computed by the kernel (k_cull_ps) for the launch rt_render would make
 * for the rectangle (x0, y0, w, h): 4 words per wave, waves in launch order (16x16 blocks
 * row-major, `spp_split` workgroups each, 4 waves per workgroup).  *n_words: capacity of
 * out on entry, words written on return. */
int rt_cull_masks_device(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, const rt_params* params,
                         int x0, int y0, int w, int h, uint64_t* out, int64_t* n_words);
/* Host-side check of the bounce-ray candidate table (rt_ctab.cpp): a render builds it on first
 * use for a scene of at most 256 triangles -- hit rule RT_HIT_RULE_CPU (k_render_ps's bounce
 * casts, t_scale >= 256) or RT_HIT_RULE_GPU (the GPU-engine renders' and the DQN renderer's
 * bounce casts; the GPU-engine renders' camera rays take the cull of their 16x4 pixel
 * rectangle) -- and the bounce casts take their candidates from it (RT_CTAB=0 in the
 * environment: never built).  For the triangle soup tri_v (n <= 256, the first n_surf
 * surfaces: the rt_scene_create order) build the table of `hit_rule` and look up each ray
 * (surf: the surface its origin lies on, orig, dir: n_rays x 3, dir unit length) as the kernels
 * do: bit i % 64 of masks[r * words + i / 64] (words = ceil(n / 64)) = triangle i is a
 * candidate of ray r; every other triangle fails the exact test under that rule (rule CPU:
 * t_scale >= 256) for it (rays the table does not cover get every triangle).  stats (optional,
 * 4 entries): patches, patches kept whole, candidate bits over all (patch, bin) entries,
 * grazing-table bits.  Replaces no reference interface: tests check it against the CPU
 * restatement's pass sets of Triangle::intersects (CPU/rays/ray.cpp:14-28; GPU/rays/ray.cu:63-64). */
int rt_ctab_candidates(const float* tri_v, int n, int n_surf, int hit_rule, const int32_t* surf, const float* orig,
                       const float* dir, int n_rays, uint64_t* masks, int64_t* stats);

/* Live kernel timing (no reference counterpart; bench.py's roofline): while enabled, every
 * launch of the kernel families below is bracketed by a HIP event pair on its own launch
 * stream.  rt_ktime_enable(1) clears the totals and starts, rt_ktime_enable(0) stops;
 * rt_ktime_read waits for the recorded launches and returns the total milliseconds and the
 * launch count of one family since the last enable. */
#define RT_KT_RENDER_PS 0     /* k_render_ps: CPU preset (configs 1-2, the bench kernel) */
#define RT_KT_RENDER 1        /* k_render: GPU preset (config 5) */
#define RT_KT_SARSA_RENDER 2  /* k_sarsa_render (config 3) */
#define RT_KT_SARSA_APPLY 3   /* k_sarsa_apply */
#define RT_KT_DQN_MLP 4       /* k_dqn_mlp: the Q-network forward (config 4) */
#define RT_KT_DQN_BOUNCE 5    /* k_dqn_bounce: Q.cos sampling + trace; in rt_render_dqn_view, k_dqn_view_reduce */
#define RT_KT_DQN_CAMERA 6    /* k_dqn_camera */
#define RT_KT_SARSA_VIEW 7    /* k_sarsa_view: the radiance-map view (rt_render_volume_view); k_glyph_view (rt_render_glyph_view) */
#define RT_KT_SARSA_NEAREST 8 /* k_sarsa_nearest: rt_sarsa_nearest's queries (without its copies) */
#define RT_KT_PROBE 9         /* k_probe: rt_probe_radiance's paths (without its fold) */
#define RT_KT_BAKE 10         /* k_bake: rt_sarsa_bake's paths (without its finish); k_sweep: rt_sarsa_sweep (without its apply) */
#define RT_KT_COUNT 11
int rt_ktime_enable(int on);
int rt_ktime_read(int kernel, double* total_ms, int64_t* launches);
const char* rt_ktime_name(int kernel);

/* SDLScreen::PutPixelSDL pack rule (CPU/sdl/sdl_screen.cpp:100-112). Host arrays. */
int rt_pack_argb(const float* rgb, int n, uint32_t* out_argb);

/* SDLScreen::SDL_SaveImage replacement: 32-bit BMP of an ARGB buffer (headless). */
int rt_save_bmp(const char* path, const uint32_t* argb, int width, int height);
/* The same frame as an 8-bit RGB PNG (the thesis images, Images/<scene>/reference.png;
 * SURVEY.md §8(f) item 4); stored deflate blocks, no compression. */
int rt_save_png(const char* path, const uint32_t* argb, int width, int height);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_H */
