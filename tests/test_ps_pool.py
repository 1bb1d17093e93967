"""k_render_ps's pooled trip (rt_kernels.hip: ps_pool): the table-route kernel defers the
retraces of the light pre-test to one trip of the whole workgroup, between two barriers that
all four waves reach.

The yardstick is the existing bit-exactness: every case renders the Cornell scene with the CPU
preset on the table route and compares against the CPU restatement (oracle.render) on the
uint32 view of the image, and requires equal ray casts.  t_scale stays at 256 (the table
serves the CPU hit rule from there, test_ctab.py) whatever the frame's height.
"""
import numpy as np
import pytest

# inside the box, close under the ceiling light, turned to a side wall (the CPU preset's camera
# has no pitch): of the views tried, the one whose workgroups defer the most samples
CROWDED_CAM = ((0.0, -0.8, 0.0, 1.0), 1.5708)  # position, yaw_y


@pytest.fixture(scope="module")
def cornell(rtmi_mod, gpu_ctx):
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


def _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=None, lit=True, **params):
    g, sc = cornell
    pos, yaw_y = cam if cam is not None else (rtmi_mod.CAMERAS["cornell"], 0.0)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=256.0, **params)
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(rtmi_mod.RT_HIT_RULE_CPU)["built"]  # the table route was taken
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(pos, yaw_y=yaw_y), oracle_mod.params_from(p))
    print(f"{params}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.any(img > 0) or not lit  # (light reaches the frame: the folds ran)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(40, 24), (17, 9)])
def test_clipped_frames(rtmi_mod, oracle_mod, gpu_ctx, cornell, width, height):
    """Workgroups along the clip have waves without a valid pixel and one partially valid wave:
    they skip the bounce loop and still reach both pool barriers and serve the pool."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=width, height=height, spp=256, spp_split=64)
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=width, height=height, spp=8, spp_split=2)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split,width", [(4, 1, 32), (8, 8, 32), (256, 64, 16), (40, 4, 32)])
def test_sample_and_split_shapes(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, width):
    """per_chunk 4 (four pixels per lane group), 1, the bench's shape, and 10: at per_chunk 16
    (spp 64, split 4) the sample slots and queues take 64 KB, past the 40 KB up to which the
    launcher sends k_render_ps; 10 samples per lane (40 KB exactly) is the largest it still gets."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=width, height=16, spp=spp, spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [0, 1, 2, 3])
def test_max_bounces(rtmi_mod, oracle_mod, gpu_ctx, cornell, max_bounces):
    """Deferral needs max_bounces 2 (the pre-test's retrace at depth 1); at 0 and 1 the pre-test
    never fires -- the barriers run regardless.  (max_bounces 0: nothing but directly seen
    light, the frame may be black.)  The kernel keeps deferral off beyond 2, but no launch gets
    there: the CPU preset's renders refuse max_bounces 3 ("supports max_bounces <= 2") before any
    kernel runs, as they did before the pooled trip, and that is what the case of 3 pins."""
    if max_bounces == 3:
        g, sc = cornell
        p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=256.0, width=32, height=16, spp=64,
                                    spp_split=16, max_bounces=3)
        with pytest.raises(rtmi_mod.RtError, match="max_bounces <= 2"):
            rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"]), p)
        return
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, lit=max_bounces > 0, width=32, height=16, spp=64, spp_split=16,
           max_bounces=max_bounces)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["RT_SAMPLER_UNIFORM", "RT_SAMPLER_COSINE"])
def test_both_samplers(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler):
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, width=32, height=16, spp=64, spp_split=16, max_bounces=2,
           sampler=getattr(rtmi_mod, sampler))


@pytest.mark.gpu
def test_crowded_pool(rtmi_mod, oracle_mod, gpu_ctx, cornell):
    """The fullest pool found.  The case was meant to put more than 64 deferred samples into one
    workgroup, so that a second wave serves the pool; no Cornell view does.  The kernel's own
    counters (an RT_PROF build, max_pool) give the largest count of a workgroup as 28 for this
    view, 17-25 for twelve others inside and outside the box at 32 x 32 x 256 spp, split 64, and
    34 over the 512 x 512 bench frame: the light pre-test passes for under 1 % of a
    workgroup's 1024 samples.  The other waves and the further steps of the pool are covered by
    running this file against a build with RT_PS_POOL_SPAN=4."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, width=32, height=32, spp=256, spp_split=64)
