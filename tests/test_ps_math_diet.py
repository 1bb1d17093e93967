"""k_render_ps's sampling math without the work the image does not need (rt_math.hpp, ps_body):

  * sqrt_rn_pos: v_sqrt_f32 and the neighbour correction alone, for +0 and [2^-96, FLT_MAX];
  * rcp_rn_in: v_rcp_f32 and the Newton step alone, for |x| in [2^-125, 2^125]; with sqrt_rn_pos
    the guard-free normalize_unit of ps_shade_dir and of the primary phase's camera ray;
  * the Philox block split by what its products depend on (philox_pix, philox_ev,
    philox_finish): the pixel's words once per lane, or once per wave on the scalar unit when the
    wave holds one pixel (split 64, the ONEPX instances).

Proofs: the two float forms against sqrtf and IEEE division over every float of their domains,
and the split against philox4x32_10 over 2^24 counters per key, with the pixel's words wave-uniform
and per lane -- on the device, through rt_selftest; the split also on the host under the
sanitizers (tools/sanitize/philox_split_main.cpp).  Renders: image words and casts equal to the
CPU restatement (oracle.render) at the shapes where the change takes another path: one pixel per
wave on both sides of the per_chunk values 4 and 1, several pixels per wave, max_bounces 0, 1, 2
(the pipelined loop, the general loop), a seed with a high word, and a frame whose waves are partly
or wholly outside it.  The renders pin image and casts, not the mechanism: they pass on the kernel
before the change as well.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_SCALE = 256.0  # (the table route serves it at every frame size: test_ps_lds_frame.py)
SAMPLERS = ["RT_SAMPLER_UNIFORM", "RT_SAMPLER_COSINE"]
RULES = ["RT_HIT_RULE_CPU", "RT_HIT_RULE_GPU"]
RT_SELFTEST_SQRT_POS, RT_SELFTEST_RCP_IN, RT_SELFTEST_PHILOX_PX = 4, 5, 6  # include/rtmi.h


def test_host_philox_split_under_sanitizers(tmp_path):
    """The RT_HD split compiles on the host and gives philox4x32_10's words over the device
    self-test's counters and the Random123 known answers; AddressSanitizer and UBSan on."""
    exe = str(tmp_path / "philox_split_san")
    subprocess.run(["c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "sanitize", "philox_split_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "philox_split: ok" in r.stdout and "33554432 counters" in r.stdout and " 0 mismatches" in r.stdout


def test_header_declares_the_new_selftests():
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for name, val in [("RT_SELFTEST_SQRT_POS", 4), ("RT_SELFTEST_RCP_IN", 5), ("RT_SELFTEST_PHILOX_PX", 6)]:
        assert f"#define {name} {val}\n" in src


@pytest.mark.gpu
@pytest.mark.parametrize("which,name", [(RT_SELFTEST_SQRT_POS, "RT_SELFTEST_SQRT_POS"),
                                        (RT_SELFTEST_RCP_IN, "RT_SELFTEST_RCP_IN"),
                                        (RT_SELFTEST_PHILOX_PX, "RT_SELFTEST_PHILOX_PX")])
def test_device_exhaustive_selftest(rtmi_mod, gpu_ctx, which, name):
    """Zero mismatches over the whole domain (sqrt: +0 and every float of [2^-96, FLT_MAX]; rcp:
    every float of both signs with |x| in [2^-125, 2^125]; Philox: all four words of 2^24 counters
    for each of two keys, the pixel's words through the scalar unit and per lane)."""
    res = (ctypes.c_uint64 * 2)()
    rtmi_mod.check(rtmi_mod.lib().rt_selftest(gpu_ctx.handle, which, res))
    print(f"{name}: {int(res[0])} mismatches, first {hex(int(res[1]))}")
    assert int(res[0]) == 0, (name, int(res[0]), hex(int(res[1])))
    assert int(res[1]) == 0xFFFFFFFF  # no mismatching input recorded


@pytest.mark.gpu
def test_selftest_refuses_codes_past_the_last(rtmi_mod, gpu_ctx):
    res = (ctypes.c_uint64 * 2)()
    assert rtmi_mod.lib().rt_selftest(gpu_ctx.handle, 0, res) == -1
    assert rtmi_mod.lib().rt_selftest(gpu_ctx.handle, 99, res) == -1


@pytest.fixture(scope="module")
def cornell(rtmi_mod, gpu_ctx):
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


def _check(rtmi_mod, oracle_mod, gpu_ctx, scene, rule="RT_HIT_RULE_CPU", sampler="RT_SAMPLER_UNIFORM", lit=True, **params):
    g, sc = scene
    rule = getattr(rtmi_mod, rule)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=T_SCALE, hit_rule=rule, sampler=getattr(rtmi_mod, sampler),
                                **params)
    cam = rtmi_mod.CAMERAS["cornell"]
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(cam), p)
    assert sc.ctab_info(rule)["built"]  # the table route was taken
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(cam), oracle_mod.params_from(p))
    print(f"{params} {sampler} rule {rule}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.any(img > 0) or not lit  # (light reaches the frame)


# (spp, split): one pixel per wave at per_chunk 4 (the bench's wave) and 1; then 4, 16 and 64
# pixels per wave (64 / split: per-lane pixel words), the last one at per_chunk 8, the wide layout
SHAPES = [(256, 64), (64, 64), (64, 16), (16, 4), (8, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spp,split", SHAPES)
def test_shapes(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, sampler, rule):
    """Cornell at 40 x 24 (the right-hand column of workgroups is clipped), max_bounces 2: the
    pipelined loop, its pre-test's event 2 and the settled folds' re-draw of event 1."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, rule=rule, sampler=sampler, width=40, height=24, spp=spp,
           spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("max_bounces", [0, 1])
@pytest.mark.parametrize("spp,split", [(64, 64), (16, 4)])
def test_few_bounces(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, max_bounces, sampler):
    """max_bounces 0 (every sample ends at its camera ray: only the primary phase draws) and 1 (no
    sample is ever pending), with the pixel's words uniform and per lane."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler=sampler, width=40, height=24, spp=spp, spp_split=split,
           max_bounces=max_bounces, lit=max_bounces > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spp,split", [(256, 64), (16, 4)])
def test_seed_high_word(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, sampler):
    """The key's high word enters the pixel's words (M1 (hi(M0 pixel) ^ k1))."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler=sampler, width=40, height=24, spp=spp, spp_split=split,
           seed=(0x1234ABCD << 32) | 1984)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("spp,split", [(64, 64), (16, 4), (8, 1)])
def test_partly_invalid_waves(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split, sampler):
    """17 x 33: at split 64 a wave is one pixel, inside the frame or wholly outside it (the wave's
    pixel words come from its first lane); at splits 4 and 1 waves hold valid and invalid pixels."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, sampler=sampler, width=17, height=33, spp=spp, spp_split=split)
