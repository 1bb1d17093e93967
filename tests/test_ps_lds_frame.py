"""k_render_ps's table-route variant keeps its surfaces' shading frames in LDS (rt_kernels.hip:
k_render_ps's staging, ps_body): after the exact-test records the workgroup stages, per triangle,
N, T, B and the one fold colour it needs (48 bytes: [N.xyz, F.x] [T.xyz, F.y] [B.xyz, F.z]), and
every read of the shading records inside ps_body -- park, the claimed and the pending sample's
frame, ps_fold, the emission rows -- is served from that copy.  The LDS for it comes from the wave
blocks: slot codes are bytes, and at per_chunk <= 4 so are the queue's entries (k << 6 | lane
< 256); above that the wave block keeps its wide size.  The layout is a constant of the kernel's
template, picked by the launcher, so the two sides of per_chunk 4 | 5 are two instances.

The yardstick is test_ps_pipeline.py's and test_ps_settle.py's: CPU preset, t_scale 256, the table
route asserted, the uint32 view of the image and the ray casts against the CPU restatement
(oracle.render).  The tests pin image and casts, not the mechanism; the shapes are the ones at
which the layout can go wrong: both sides of the per_chunk boundary, 64 pixels per wave (queue
entries up to 255), the bench's wave, a clipped workgroup with a pixel-less wave, a scene that
fills the last record of the layout (64 triangles, code 61 in a slot, triangle 63's emission),
both fold rows, the variant's general loop, and hit rule 1.  Nothing here depends on the layout:
the file passes on the kernel before the change as well.
"""
import dataclasses

import numpy as np
import pytest

CROWDED_CAM = ((0.0, -0.8, 0.0, 1.0), 1.5708)  # test_ps_settle.py's view: position, yaw_y
T_SCALE = 256.0
SAMPLERS = ["RT_SAMPLER_UNIFORM", "RT_SAMPLER_COSINE"]


def stacked_sheets_geometry(g, n_quads):
    """g with n_quads more surface quads (two grey triangles each) appended to g.tri, each the way
    test_ps_settle.py's sheet_geometry appends its one: the light quad's vertices moved into the
    room along the light's normal, in the light triangles' vertex order.  Quad k lies 0.02 (k + 1)
    below the light and is shrunk about the quad's centre by 1 - (k + 1) / 16, so the stack is an
    inverted pyramid: every quad, the last one most of all, is seen from the room, and the light
    is seen past the rims."""
    v = g.light.reshape(-1, 3, 3).astype(np.float32)
    n = np.cross(v[0, 2] - v[0, 0], v[0, 1] - v[0, 0])  # the light's normal, into the room
    n = (n / np.linalg.norm(n)).astype(np.float32)
    ceil_n = np.cross(g.tri[6, 6:9] - g.tri[6, 0:3], g.tri[6, 3:6] - g.tri[6, 0:3])
    assert np.dot(n, ceil_n) > 0  # the same winding as a ceiling triangle (Cornell's triangle 6)
    centre = v.reshape(-1, 3).mean(axis=0).astype(np.float32)
    quads = []
    for k in range(n_quads):
        s = np.float32(1.0 - (k + 1) / 16.0)
        quads.append((centre + s * (v - centre) + np.float32(0.02 * (k + 1)) * n).reshape(-1, 9))
    sheets = np.concatenate(quads).astype(np.float32)
    grey = np.full((sheets.shape[0], 3), 0.5, np.float32)
    return dataclasses.replace(g, tri=np.concatenate([g.tri, sheets]).astype(np.float32),
                               albedo=np.concatenate([g.albedo, grey]).astype(np.float32))


def many_lights_geometry(g):
    """test_ps_pipeline.py's: g with its light quad cut into nine coplanar triangles that cover the
    same quad, same emission and light group (more than the light pre-test takes: kPsSplitLights 8)."""
    assert g.n_light == 2 and np.array_equal(g.emission[0], g.emission[1]) and g.light_group[0] == g.light_group[1]
    half = np.float32(0.5)
    parts = []
    for t in g.light:
        a, b, c = t[0:3], t[3:6], t[6:9]
        ab, bc, ca = (a + b) * half, (b + c) * half, (c + a) * half
        parts += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    p, q, r = parts.pop()
    m = (p + q) * half
    parts += [(p, m, r), (m, q, r)]
    light = np.stack([np.concatenate(t) for t in parts]).astype(np.float32)
    k = light.shape[0]
    return dataclasses.replace(g, light=light, emission=np.repeat(g.emission[:1], k, axis=0),
                               light_group=np.repeat(g.light_group[:1], k))


def test_appended_scenes_have_the_stated_sizes(rtmi_mod):
    """On the CPU: the largest scene fills the table route's 64 triangles (62 surfaces, so the
    highest slot code is 61 and the last staged record is light triangle 63), its quads lie inside
    the room below the light, and the many-lights scene is past the pre-test's limit."""
    c = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    assert c.n_surf == 36 and c.n_light == 2 and c.n_tri == 38
    g = stacked_sheets_geometry(c, 13)
    assert g.n_surf == 62 and g.n_light == 2 and g.n_tri == 64
    assert g.albedo.shape == (62, 3) and g.all_triangles().shape[0] == 64
    lo, hi = c.tri.reshape(-1, 3).min(axis=0), c.tri.reshape(-1, 3).max(axis=0)
    new = g.tri[36:].reshape(-1, 3)
    assert np.all(new >= lo) and np.all(new <= hi)
    # distinct planes, 0.02 apart: no two quads (nor a quad and the light) within the window's eps
    up = int(np.argmax(np.abs(np.cross(c.light[0, 6:9] - c.light[0, 0:3], c.light[0, 3:6] - c.light[0, 0:3]))))
    levels = np.unique(np.round(g.tri[36:].reshape(-1, 3)[:, up], 4))
    assert levels.size == 13 and not np.any(np.isclose(levels, c.light[0, up], atol=1e-2))
    m = many_lights_geometry(c)
    assert m.n_light == 9 and m.n_surf == 36 and m.n_tri == 45


@pytest.fixture(scope="module")
def cornell(rtmi_mod, gpu_ctx):
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


@pytest.fixture(scope="module")
def largest(rtmi_mod, gpu_ctx):
    g = stacked_sheets_geometry(rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU), 13)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


@pytest.fixture(scope="module")
def many_lights(rtmi_mod, gpu_ctx):
    g = many_lights_geometry(rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU))
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


def _check(rtmi_mod, oracle_mod, gpu_ctx, scene, cam=None, lit=True, rule=None, **params):
    g, sc = scene
    rule = rtmi_mod.RT_HIT_RULE_CPU if rule is None else rule
    pos, yaw_y = cam if cam is not None else (rtmi_mod.CAMERAS["cornell"], 0.0)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=T_SCALE, hit_rule=rule, **params)
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(rule)["built"]  # the table route was taken
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(pos, yaw_y=yaw_y), oracle_mod.params_from(p))
    print(f"{params}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.any(img > 0) or not lit  # (light reaches the frame: the folds ran)


# (spp, split) -> per_chunk = spp / split: 3, 4 (64 pixels per wave: entries up to 255), 4, 4 (the
# bench's wave: one pixel) in the byte layout; 5 (the first wide one), 8, 10 (the largest) wide
BOUNDARY = [(3, 1), (4, 1), (16, 4), (256, 64), (5, 1), (8, 1), (40, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spp,split", BOUNDARY)
def test_layout_boundary(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, sampler):
    """Cornell at 40 x 24: the workgroups of the right-hand column are clipped, and at split 1 one
    of their waves has no pixel."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=40, height=24, spp=spp, spp_split=split,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_fold_rows(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler):
    """The crowded view at the bench's wave shape: settled light folds and depth-1 light hits, so
    the fold colour (row 3 for the uniform sampler, row 4 for the cosine one) and the emission are
    read from the staged records."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, width=32, height=32, spp=256, spp_split=64,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spp,split", [(16, 4), (8, 1)])
def test_largest_scene(rtmi_mod, oracle_mod, gpu_ctx, largest, spp, split, sampler):
    """62 surfaces and 2 lights: slot codes up to 61, and the staged records fill the last slot of
    the layout (the records are the last thing in the workgroup's LDS at both wave-block sizes; a
    write past a wave block lands in its neighbour's slots or the exact-phase blocks and shows in
    the image)."""
    g, _ = largest
    assert g.n_surf == 62 and g.n_tri == 64
    _check(rtmi_mod, oracle_mod, gpu_ctx, largest, width=40, height=24, spp=spp, spp_split=split,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("max_bounces", [0, 1])
def test_general_loop_few_bounces(rtmi_mod, oracle_mod, gpu_ctx, cornell, max_bounces, sampler):
    """max_bounces 0 (the pre-test is off: every sample parks its value) and 1 (a surface hit ends
    the path; a light hit folds through the first surface)."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=32, height=32, spp=16, spp_split=4, max_bounces=max_bounces,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_general_loop_pretest_off(rtmi_mod, oracle_mod, gpu_ctx, many_lights, sampler):
    """Nine light triangles: the pre-test is off, so the variant's general loop shades at depth 1
    and folds through both bounces, all from the staged records."""
    g, _ = many_lights
    assert g.n_light == 9 and g.n_tri <= 64
    _check(rtmi_mod, oracle_mod, gpu_ctx, many_lights, width=32, height=32, spp=16, spp_split=4,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
def test_hit_rule_1(rtmi_mod, oracle_mod, gpu_ctx, cornell):
    """The other hit rule's table and instance (the CPU preset reaches it: the table for rule 1
    serves every t_scale), at the bench's wave shape."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, rule=rtmi_mod.RT_HIT_RULE_GPU, width=40, height=24, spp=256,
           spp_split=64)
