"""The primary-ray cull in two halves (rt_cull.hpp: cull_forms + rect_cull_forms).

k_render_ps and k_cull_ps no longer evaluate rect_cull per wave: a small kernel computes the
camera-and-triangle half once per launch key (k_cull_forms), the wave finishes the test for its
pixel rectangle, and the rectangle itself is a closed form of the wave's position instead of a
reduction over the lanes.  The split runs rect_cull's float operations on the same operands in
the same order, so equality with the definition (rt_rect_candidates) is exact:
  CPU: rt_rect_candidates_forms == rt_rect_candidates, every scene, rule, yaw, frame and rectangle;
  GPU: rt_cull_masks_device == rt_rect_candidates over each wave's valid pixels, at the frame
       sizes and splits where the closed-form rectangle could go wrong.
"""
import ctypes
import os

import numpy as np
import pytest

CAM = (0.0, 0.0, -3.0, 1.0)
YAWS = (0.0, 0.2, -0.1, 1.3)
FRAMES = ((512, 512), (40, 24), (17, 33))
SCENES = ("cornell", "Medieval_House", "bunny", "complex_light_room", "archway", "door_room")


def _scene(rtmi_mod, kind):
    if kind == "cornell":
        return rtmi_mod.cornell_geometry(0), CAM
    from conftest import MODELS
    known = kind in rtmi_mod.CAMERAS
    g = rtmi_mod.obj_geometry(os.path.join(MODELS, kind + ".obj"), kind if known else "generic")
    return g, (rtmi_mod.CAMERAS[kind] if known else CAM)


def _rects(W, H):
    """(px0, py0, px1, py1) inclusive: single pixels, one row, a 16x4 block (whole and clipped),
    a rectangle touching each image edge, the whole image"""
    r = [(x, y, x, y) for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 3, H - 2),
                                   (1, H // 2))]
    r.append((0, H // 3, W - 1, H // 3))  # one row
    for x0, y0 in ((0, 0), (16 * ((W - 1) // 16), 4 * ((H - 1) // 4)), (16 * (W // 32), 4 * (H // 8))):
        r.append((x0, y0, min(x0 + 15, W - 1), min(y0 + 3, H - 1)))  # 16x4, the last ones clipped
    r.append((0, H // 4, min(3, W - 1), H // 2))          # left edge
    r.append((max(W - 4, 0), H // 4, W - 1, H // 2))      # right edge
    r.append((W // 4, 0, W // 2, min(2, H - 1)))          # top edge
    r.append((W // 4, max(H - 3, 0), W // 2, H - 1))      # bottom edge
    r.append((0, 0, W - 1, H - 1))
    return r


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("kind", SCENES)
def test_split_cull_equals_definition(rtmi_mod, kind, rule):
    geom, cam_pos = _scene(rtmi_mod, kind)
    filt = rtmi_mod.filter_records(geom.all_triangles())
    culled = kept = 0
    for yaw in YAWS:
        cam = rtmi_mod.camera(cam_pos, yaw_y=yaw)
        for (W, H) in FRAMES:
            p = rtmi_mod.default_params(0, width=W, height=H, spp=8, hit_rule=rule)
            for rect in _rects(W, H):
                want = rtmi_mod.rect_candidates(filt, cam, p, *rect)
                got = rtmi_mod.rect_candidates(filt, cam, p, *rect, forms=True)
                assert np.array_equal(got, want), (kind, rule, yaw, W, H, rect, np.flatnonzero(got != want)[:8])
                kept += int(want.sum())
                culled += int((~want).sum())
    # the cases exercise both answers
    assert kept > 0 and culled > 0, (kept, culled)


def _device_masks(rtmi_mod, ctx, sc, cam, p, rect, split):
    nb = ((rect[2] + 15) // 16) * ((rect[3] + 15) // 16)
    n = nb * split * 4 * 4
    out = np.zeros(n, np.uint64)
    nw = ctypes.c_int64(n)
    rtmi_mod.api.check(rtmi_mod.lib().rt_cull_masks_device(
        ctx.handle, sc.handle, ctypes.byref(cam), ctypes.byref(p), *rect,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(nw)))
    assert nw.value == n
    return out.reshape(nb, split, 4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("yaw", [0.0, 0.2])
@pytest.mark.parametrize("size", [(40, 24), (17, 33)])
@pytest.mark.parametrize("kind", ["cornell", "complex_light_room"])  # one mask word, three
def test_device_masks_equal_host_definition(rtmi_mod, gpu_ctx, kind, size, yaw, rule):
    geom, cam_pos = _scene(rtmi_mod, kind)
    filt = rtmi_mod.filter_records(geom.all_triangles())
    W, H = size
    cam = rtmi_mod.camera(cam_pos, yaw_y=yaw)
    host = {}
    empty_waves = 0
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        for split in (1, 2, 4, 8, 16, 32, 64):
            p = rtmi_mod.default_params(0, width=W, height=H, spp=64, spp_split=split, hit_rule=rule)
            out = _device_masks(rtmi_mod, gpu_ctx, sc, cam, p, (0, 0, W, H), split)
            lg = split.bit_length() - 1
            bi = 0
            for by in range(0, H, 16):
                for bx in range(0, W, 16):
                    for part in range(split):
                        for w in range(4):
                            q = (part << (8 - lg)) + ((np.arange(64) + 64 * w) >> lg)
                            px, py = bx + (q & 15), by + (q >> 4)
                            ok = (px < W) & (py < H)
                            got = out[bi, part, w]
                            if not ok.any():
                                empty_waves += 1
                                assert not got.any(), (split, bx, by, part, w)
                                continue
                            r = (int(px[ok].min()), int(py[ok].min()), int(px[ok].max()), int(py[ok].max()))
                            if r not in host:
                                m = rtmi_mod.rect_candidates(filt, cam, p, *r)
                                host[r] = np.zeros(256, bool)
                                host[r][:m.size] = m
                            bits = np.unpackbits(got.view(np.uint8), bitorder="little").astype(bool)
                            assert np.array_equal(bits, host[r]), (split, bx, by, part, w, r)
                    bi += 1
    assert empty_waves > 0  # waves left with no valid pixel are among the cases
