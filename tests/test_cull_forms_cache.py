"""The forms buffer of the primary-ray cull (rt_capi.cpp ctx_cull_forms) and k_render_ps's use of it.

A context keeps, per stream, the rows k_cull_forms wrote and the key they were computed for
(camera, frame size, t_scale, hit rule, scene); an unchanged key launches nothing.  A stale
buffer would cull with another camera's forms, so after every change of the key the masks and a
render on the long-lived context must equal those of a fresh context bit for bit -- which also
pins that the forms kernel runs on the render's stream ahead of it.
"""
import ctypes
import os

import numpy as np
import pytest

W, H = 48, 40
CAM_A = ((0.0, 0.0, -3.0, 1.0), 0.0)
CAM_B = ((0.3, -0.2, -2.5, 1.0), 0.25)


def _masks(rtmi_mod, ctx, sc, cam, p):
    split = max(1, p.spp_split)
    nb = ((p.width + 15) // 16) * ((p.height + 15) // 16)
    n = nb * split * 4 * 4
    out = np.zeros(n, np.uint64)
    nw = ctypes.c_int64(n)
    rtmi_mod.api.check(rtmi_mod.lib().rt_cull_masks_device(
        ctx.handle, sc.handle, ctypes.byref(cam), ctypes.byref(p), 0, 0, p.width, p.height,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(nw)))
    return out


def _render(rtmi_mod, torch, ctx, sc, cam, p, stream):
    tiles = np.array([(x, y) for y in range(0, p.height, 16) for x in range(0, p.width, 16)], np.int32)
    with torch.cuda.stream(stream):
        out = torch.zeros((len(tiles), 16, 16, 3), device="cuda")
        casts = torch.zeros(1, dtype=torch.int64, device="cuda")
        rtmi_mod.render_tiles_device(ctx, sc, cam, p, tiles, 16, out.data_ptr(), casts.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy(), int(casts.item())


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("spp,split", [(8, 4), (64, 64)])
def test_forms_follow_the_key(rtmi_mod, spp, split, sampler):
    import torch
    from conftest import MODELS
    g_a = rtmi_mod.cornell_geometry(0)
    g_b = rtmi_mod.obj_geometry(os.path.join(MODELS, "door_room.obj"), "door_room")
    s0 = torch.cuda.current_stream()
    s1 = torch.cuda.Stream()

    def params(**kw):
        return rtmi_mod.default_params(0, **{"width": W, "height": H, "spp": spp, "spp_split": split,
                                             "sampler": sampler, **kw})
    ts = params().t_scale
    cam_d = (rtmi_mod.CAMERAS["door_room"], 0.1)
    # (scene, camera, params, stream): each step changes one part of the key
    steps = [("a", CAM_A, params(), s0), ("a", CAM_B, params(), s0), ("a", CAM_A, params(), s0),
             ("a", CAM_A, params(t_scale=2.0 * ts), s0), ("a", CAM_A, params(width=40, height=24), s0),
             ("b", cam_d, params(width=40, height=24), s0), ("b", cam_d, params(hit_rule=1), s0),
             ("a", CAM_B, params(), s1), ("a", CAM_A, params(), s0), ("a", CAM_A, params(), s1),
             ("a", CAM_A, params(), s1)]
    with rtmi_mod.Context(0) as ctx, rtmi_mod.Scene(ctx, g_a) as sa, rtmi_mod.Scene(ctx, g_b) as sb:
        for i, (which, (pos, yaw), p, stream) in enumerate(steps):
            cam = rtmi_mod.camera(pos, yaw_y=yaw)
            geom, sc = (g_a, sa) if which == "a" else (g_b, sb)
            got_img, got_casts = _render(rtmi_mod, torch, ctx, sc, cam, p, stream)
            got_masks = _masks(rtmi_mod, ctx, sc, cam, p)
            with rtmi_mod.Context(0) as fresh, rtmi_mod.Scene(fresh, geom) as fs:
                want_masks = _masks(rtmi_mod, fresh, fs, cam, p)
                want_img, want_casts = _render(rtmi_mod, torch, fresh, fs, cam, p, s0)
            assert np.array_equal(got_masks, want_masks), i
            assert got_casts == want_casts, (i, got_casts, want_casts)
            assert np.array_equal(got_img, want_img), i
            assert want_casts > 0


@pytest.mark.gpu
def test_scene_rebuilt_at_the_same_address(rtmi_mod):
    """A scene destroyed and another created may get the same device address for its filter
    records: the key's generation tells them apart."""
    g_a = rtmi_mod.cornell_geometry(0)
    g_c = rtmi_mod.cornell_geometry(0)
    g_c.tri = np.ascontiguousarray(g_c.tri * np.float32(0.75))  # same counts, other triangles
    cam = rtmi_mod.camera(CAM_A[0])
    p = rtmi_mod.default_params(0, width=W, height=H, spp=8, spp_split=4)
    with rtmi_mod.Context(0) as ctx:
        with rtmi_mod.Scene(ctx, g_a) as sc:
            _masks(rtmi_mod, ctx, sc, cam, p)
        with rtmi_mod.Scene(ctx, g_c) as sc:
            got = _masks(rtmi_mod, ctx, sc, cam, p)
            got_img, got_casts = rtmi_mod.render(ctx, sc, cam, p)
    with rtmi_mod.Context(0) as fresh, rtmi_mod.Scene(fresh, g_c) as fs:
        want = _masks(rtmi_mod, fresh, fs, cam, p)
        want_img, want_casts = rtmi_mod.render(fresh, fs, cam, p)
    assert np.array_equal(got, want)
    assert got_casts == want_casts and np.array_equal(got_img, want_img)


@pytest.mark.gpu
def test_no_forms_buffer_keeps_the_image(rtmi_mod, monkeypatch):
    """Without the buffer (allocation failed) the kernels run the whole cull: the same result."""
    geom = rtmi_mod.cornell_geometry(0)
    cam = rtmi_mod.camera(CAM_B[0], yaw_y=CAM_B[1])
    p = rtmi_mod.default_params(0, width=W, height=H, spp=16, spp_split=4)
    with rtmi_mod.Context(0) as ctx, rtmi_mod.Scene(ctx, geom) as sc:
        want_masks = _masks(rtmi_mod, ctx, sc, cam, p)
        want_img, want_casts = rtmi_mod.render(ctx, sc, cam, p)
    monkeypatch.setenv("RT_FORMS_TEST_FAIL", "1")
    with rtmi_mod.Context(0) as ctx, rtmi_mod.Scene(ctx, geom) as sc:
        got_masks = _masks(rtmi_mod, ctx, sc, cam, p)
        got_img, got_casts = rtmi_mod.render(ctx, sc, cam, p)
    assert np.array_equal(got_masks, want_masks)
    assert got_casts == want_casts and np.array_equal(got_img, want_img)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split", [(16, 4), (32, 8), (256, 64)])
def test_render_equals_oracle(rtmi_mod, oracle_mod, spp, split):
    """40 x 24 (clipped blocks) with the CPU preset: the image bit for bit, the casts equal."""
    geom = rtmi_mod.cornell_geometry(0)
    p = rtmi_mod.default_params(0, width=40, height=24, spp=spp, spp_split=split)
    with rtmi_mod.Context(0) as ctx, rtmi_mod.Scene(ctx, geom) as sc:
        img, casts = rtmi_mod.render(ctx, sc, rtmi_mod.camera(CAM_A[0]), p)
    ref, ref_casts = oracle_mod.render(geom, oracle_mod.camera(CAM_A[0]), oracle_mod.params_from(p))
    assert casts == ref_casts, (casts, ref_casts)
    assert np.array_equal(img, ref)
