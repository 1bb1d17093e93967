"""k_render_ps's in-wave settle (rt_kernels.hip: pretest_pending in ps_body's pipelined loop): a
terminal ray whose light pre-test passes is traced on the spot by its wave -- lane j tests
triangle j against the passing lane's ray, and the scan's window (t < best + eps, in index order)
runs over the triangles that pass -- instead of being deferred to a pooled trip of the workgroup.

The yardstick is test_ps_pipeline.py's: CPU preset, t_scale 256, the table route asserted, the
uint32 view of the image and the ray casts against the CPU restatement (oracle.render).  The
tests pin image and casts, not the mechanism.

Shapes: passes settled inside the loop's pre-tests, several per wave (the bench's wave shape and
per_chunk 10); one trip, so every settle happens in the drain after the loop; a workgroup with a
pixel-less and a partly valid wave (no barrier but the casts barrier is left for it to reach);
and a scene in which the window's tie rule decides the hit: a surface sheet 1e-3 below the
light, so that the light (the later index) wins for steep rays and the sheet for grazing ones.

Serial settle loop (a one-off count from an RT_PROF build, prof slot 8, not asserted here): on
the crowded 32 x 32 x 256 shape below, the largest number of lanes settled in one pre-test pass
was 6 (2,660 passes in 4,096 trips), and 7 over the bench frame:
the settle loop runs more than once per pass.
"""
import dataclasses

import numpy as np
import pytest

# test_ps_pool.py's view: of those tried, the one whose workgroups pass the pre-test most often
CROWDED_CAM = ((0.0, -0.8, 0.0, 1.0), 1.5708)  # position, yaw_y
T_SCALE = 256.0
EPS = np.float32(1e-5)  # kEps: the window's eps in t; 2.56e-3 world units along the ray at t_scale 256
SHEET_DELTA = 1e-3      # world units between the light and the sheet


def sheet_geometry(g, delta=SHEET_DELTA):
    """g with one more surface quad (two triangles, grey) appended to g.tri: the light quad's
    vertices moved into the room along the light's normal by delta, in the light triangles' vertex
    order -- the ceiling triangles' winding (both face the room)."""
    v = g.light.reshape(-1, 3, 3).astype(np.float32)
    n = np.cross(v[0, 2] - v[0, 0], v[0, 1] - v[0, 0])  # the light's normal, into the room
    n = (n / np.linalg.norm(n)).astype(np.float32)
    ceil_n = np.cross(g.tri[6, 6:9] - g.tri[6, 0:3], g.tri[6, 3:6] - g.tri[6, 0:3])
    assert np.dot(n, ceil_n) > 0  # the same winding as a ceiling triangle (Cornell's triangle 6)
    sheet = (v + np.float32(delta) * n).reshape(-1, 9).astype(np.float32)
    grey = np.full((sheet.shape[0], 3), 0.5, np.float32)
    return dataclasses.replace(g, tri=np.concatenate([g.tri, sheet]).astype(np.float32),
                               albedo=np.concatenate([g.albedo, grey]).astype(np.float32))


def _terminal_rays(g, n, seed):
    """n rays as the kernel forms them (o = pos + 1e-5 sd, d = sd / |sd| in float32, sd uniform
    over the hemisphere of the surface's normal) from area-weighted points of Cornell's surfaces
    but the ceiling: every such point lies below the light."""
    rng = np.random.default_rng(seed)
    src = np.array([i for i in range(36) if not 6 <= i <= 13])
    v = g.tri[src].reshape(-1, 3, 3).astype(np.float64)
    N = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])  # into the room
    area = 0.5 * np.linalg.norm(N, axis=1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    j = rng.choice(len(src), n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    f = a + b > 1
    a[f], b[f] = 1 - a[f], 1 - b[f]
    pos = (v[j, 0] + a[:, None] * (v[j, 1] - v[j, 0]) + b[:, None] * (v[j, 2] - v[j, 0])).astype(np.float32)
    nn = N[j]
    T = np.where((np.abs(nn[:, 0]) > np.abs(nn[:, 1]))[:, None],
                 np.stack([nn[:, 2], 0 * nn[:, 0], -nn[:, 0]], 1), np.stack([0 * nn[:, 0], -nn[:, 2], nn[:, 1]], 1))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(nn, T)
    r1, r2 = rng.random(n), rng.random(n)
    st = np.sqrt(1 - r1 * r1)
    sd = ((st * np.cos(2 * np.pi * r2))[:, None] * B + r1[:, None] * nn +
          (st * np.sin(2 * np.pi * r2))[:, None] * T).astype(np.float32)
    o = (pos + np.float32(1e-5) * sd).astype(np.float32)
    ln = np.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2]).astype(np.float32)
    return o, (sd / ln[:, None]).astype(np.float32)


def test_sheet_scene_has_both_kinds_of_tie(rtmi_mod, oracle_mod):
    """On the CPU, from the restatement's pass sets (oracle.pass_masks, the call test_ctab.py
    uses) and its t values: of 200,000 terminal rays from points below the light, 3,095 have a
    sheet triangle and a light triangle both passing at delta = 1e-3; 2,803 of them with
    |dt| < eps (the later index, the light, wins the window) and 292 with |dt| > eps (the sheet
    wins).  (At delta = 2e-3: 1,652 and 1,434.)"""
    g = sheet_geometry(rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU))
    assert g.n_surf == 38 and g.n_tri == 40 and g.n_tri <= 64
    tri = np.ascontiguousarray(g.all_triangles(), np.float32)
    o, d = _terminal_rays(g, 200000, seed=10)
    passes = oracle_mod.pass_masks(tri, o, d, T_SCALE, 0)[:, 0]
    sheet_bits, light_bits = np.uint64(3 << 36), np.uint64(3 << 38)
    both = ((passes & sheet_bits) != 0) & ((passes & light_bits) != 0)
    grp = np.zeros(0, np.int32)
    # (each pair alone, as two surfaces: the t of the one that passes; +inf for a miss)
    t_sheet, _ = oracle_mod.intersect(tri[36:38], 2, 0, grp, o[both], d[both], T_SCALE, 0)
    t_light, _ = oracle_mod.intersect(tri[38:40], 2, 0, grp, o[both], d[both], T_SCALE, 0)
    assert np.all(np.isfinite(t_sheet)) and np.all(np.isfinite(t_light))
    dt = np.abs(t_light - t_sheet)
    near, far = int(np.count_nonzero(dt < EPS)), int(np.count_nonzero(dt > EPS))
    print(f"both pass: {int(both.sum())}, |dt| < eps: {near}, |dt| > eps: {far}")
    assert near >= 100 and far >= 100


@pytest.fixture(scope="module")
def cornell(rtmi_mod, gpu_ctx):
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


@pytest.fixture(scope="module")
def sheet(rtmi_mod, gpu_ctx):
    g = sheet_geometry(rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU))
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        yield g, sc


def _check(rtmi_mod, oracle_mod, gpu_ctx, scene, cam=None, lit=True, **params):
    g, sc = scene
    pos, yaw_y = cam if cam is not None else (rtmi_mod.CAMERAS["cornell"], 0.0)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=T_SCALE, **params)
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(rtmi_mod.RT_HIT_RULE_CPU)["built"]  # the table route was taken
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(pos, yaw_y=yaw_y), oracle_mod.params_from(p))
    print(f"{params}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.any(img > 0) or not lit  # (light reaches the frame: the folds ran)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split", [(256, 64), (40, 4)])
def test_settle_in_the_loop(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split):
    """Crowded view, 32 x 32: several trips per wave, so passes are settled inside the loop's
    pre-tests, several per wave.  The bench's wave shape (a wave is one pixel) and per_chunk 10."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, width=32, height=32, spp=spp, spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,spp,split", [(32, 32, 4, 4), (16, 4, 1, 1)])
def test_settle_in_the_drain(rtmi_mod, oracle_mod, gpu_ctx, cornell, width, height, spp, split):
    """per_chunk 1: one trip per wave, so every pre-test, and every settle, runs in the drain after
    the loop.  (16 x 4 at 1 spp is 64 samples: the frame may be black.)"""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, lit=False, width=width, height=height, spp=spp,
           spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("spp,split", [(256, 64), (1, 1)])
def test_clipped_workgroup(rtmi_mod, oracle_mod, gpu_ctx, cornell, spp, split):
    """17 x 5: at split 1 one wave of a workgroup has no pixel and one is partly valid; at split 64
    (a wave is one pixel) a workgroup has three pixel-less waves beside a valid one, or four.  A
    pixel-less wave reaches the casts barrier and nothing else."""
    _check(rtmi_mod, oracle_mod, gpu_ctx, cornell, cam=CROWDED_CAM, lit=False, width=17, height=5, spp=spp,
           spp_split=split)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["RT_SAMPLER_UNIFORM", "RT_SAMPLER_COSINE"])
@pytest.mark.parametrize("view", ["crowded", "default"])
@pytest.mark.parametrize("max_bounces", [0, 1, 2])
def test_window_tie_rule(rtmi_mod, oracle_mod, gpu_ctx, sheet, max_bounces, view, sampler):
    """The sheet scene (test_sheet_scene_has_both_kinds_of_tie): a settled ray that passes both the
    sheet and the light ends on the light when the two are within eps in t, on the sheet otherwise,
    as the scan's window in index order decides.  max_bounces 2 at the bench's wave shape; 0 and 1
    (nothing is ever pending) at a smaller one."""
    g, _ = sheet
    assert g.n_tri <= 64
    shape = dict(width=32, height=32, spp=256, spp_split=64) if max_bounces == 2 else \
        dict(width=32, height=16, spp=4, spp_split=4)
    _check(rtmi_mod, oracle_mod, gpu_ctx, sheet, cam=CROWDED_CAM if view == "crowded" else None, lit=False,
           max_bounces=max_bounces, sampler=getattr(rtmi_mod, sampler), **shape)
