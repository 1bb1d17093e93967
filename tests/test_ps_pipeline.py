"""k_render_ps's pipelined bounce loop (rt_kernels.hip: the first loop of ps_body): with the
pooled trip, a sample whose cast hit a surface with one bounce left is kept by its lane as
pending, and its light pre-test runs in the lane's next trip, between the issue of the next
sample's table lookup and the first use of the loaded words -- or, once the wave's queue has
drained, after the loop.

The yardstick is test_ps_pool.py's: Cornell, CPU preset, t_scale 256, the table route asserted,
the uint32 view of the image and the ray casts against the CPU restatement (oracle.render).
The shapes are the smallest at which the new order can go wrong: one trip and then the drain;
several trips with pending samples carried across claims; a wave whose queue is empty.

The table route's other loop (ps_body's second) with bounces left runs when the pre-test is off:
Cornell with its light quad cut into more triangles than the pre-test takes.
"""
import dataclasses

import numpy as np
import pytest

# test_ps_pool.py's view: of those tried, the one whose workgroups defer the most samples
CROWDED_CAM = ((0.0, -0.8, 0.0, 1.0), 1.5708)  # position, yaw_y
# the bench camera turned round: it faces away from the box, every camera ray misses
AWAY_CAM = ((0.0, 0.0, -3.0, 1.0), 3.14159265)


@pytest.fixture(scope="module")
def cornell(rtmi_mod, gpu_ctx):
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


def _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=None, lit=True, primaries_only=False, **params):
    g, sc = cornell
    pos, yaw_y = cam if cam is not None else (rtmi_mod.CAMERAS["cornell"], 0.0)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=256.0, **params)
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(rtmi_mod.RT_HIT_RULE_CPU)["built"]  # the table route was taken
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(pos, yaw_y=yaw_y), oracle_mod.params_from(p))
    print(f"{params}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    if primaries_only:  # the oracle on the CPU says so: no path continues, the queues are empty
        assert ref_casts == p.width * p.height * p.spp
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.any(img > 0) or not lit  # (light reaches the frame: the folds ran)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(16, 4), (17, 5)])
def test_one_trip_then_drain(rtmi_mod, oracle_mod, gpu_ctx, cornell, width, height):
    """spp 1, split 1: per_chunk is 1 and a wave's queue holds at most 64 entries, so the loop
    runs one trip and every pre-test runs after it.  17 x 5 is clipped: one wave of its
    workgroups has no pixel, one is partly valid.  (64 or 85 samples: the frame may be black.)"""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, lit=False, width=width, height=height, spp=1, spp_split=1)


@pytest.mark.gpu
def test_drain_lists_deferrals(rtmi_mod, oracle_mod, gpu_ctx, cornell):
    """spp 4, split 4 at 32 x 32 from the crowded view: one trip per wave again, so all its
    deferrals (about 0.8 % of the 4,096 samples pass the pre-test) are listed after the loop,
    and the pooled trip runs on them."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, width=32, height=32, spp=4, spp_split=4)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split,width", [(40, 4, 32), (256, 64, 16)])
def test_pending_across_claims(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, width):
    """Several trips per wave, pending samples carried across claims: per_chunk 10 (the largest
    the launcher sends to k_render_ps) and the bench's shape."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=width, height=16, spp=spp, spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split", [(1, 1), (40, 4)])
def test_empty_queue(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split):
    """Every camera ray misses (the oracle's casts are width x height x spp): the loop and the
    drain see nothing pending, and the frame is black."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=AWAY_CAM, lit=False, primaries_only=True, width=32, height=16,
           spp=spp, spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [0, 1, 2])
@pytest.mark.parametrize("spp,split", [(4, 4), (40, 4)])
def test_max_bounces(rtmi_mod, oracle_mod, gpu_ctx, cornell, max_bounces, spp, split):
    """per_chunk 1 and 10.  At max_bounces 0 and 1 nothing is ever pending (0: the pre-test is
    off and the old loop runs; 1: a surface hit ends the path with 0 on the spot)."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=32, height=16, spp=spp, spp_split=split,
           max_bounces=max_bounces)


def many_lights_geometry(g):
    """g with its light quad (two triangles) cut into nine coplanar triangles that cover the same
    quad, same emission and light group: each triangle into four at its edges' midpoints (the
    orientation kept), the last of the eight halved once more."""
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
    n = light.shape[0]
    return dataclasses.replace(g, light=light, emission=np.repeat(g.emission[:1], n, axis=0),
                               light_group=np.repeat(g.light_group[:1], n))


@pytest.fixture(scope="module")
def many_lights(rtmi_mod, gpu_ctx):
    g = many_lights_geometry(rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU))
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [1, 2])
@pytest.mark.parametrize("spp,split", [(4, 4), (40, 4)])
def test_general_loop_on_table_route(rtmi_mod, oracle_mod, gpu_ctx, many_lights, max_bounces, spp, split):
    """Nine light triangles: more than the light pre-test takes (kPsSplitLights 8), so the
    table-route kernel runs its general loop with bounces left -- shading at depth 1, the folds
    through both bounces, nothing deferred and an empty pooled trip.  per_chunk 1 and 10."""
    g, _ = many_lights
    assert g.n_light == 9 and g.n_tri <= 64
    _check(rtmi_mod, oracle_mod, gpu_ctx, many_lights, width=32, height=16, spp=spp, spp_split=split,
           max_bounces=max_bounces)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["RT_SAMPLER_UNIFORM", "RT_SAMPLER_COSINE"])
def test_both_samplers(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler):
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=32, height=16, spp=40, spp_split=4, max_bounces=2,
           sampler=getattr(rtmi_mod, sampler))
