"""The Q-network view (rt_render_dqn_view[_tiles_device]): the network's irradiance estimate at
every camera hit, on rt_render_irradiance's scale.

  * the reduction of a ray's 144 Q values -- cell-centre cosines, the blocked fold, the action --
    restated once in numpy float32 (reduce_rows / shade below) and checked against itself without
    a GPU on random rows, rows with ties and rows with NaN;
  * on the GPU every output against its own definition, bit for bit: out_tri against
    orc_primary_hits, out_pos against the positions the restated DQN renderer hands its network at
    bounce 1 (orc_render_dqn_wave), both against rt_render_volume_view, out_q against rt_dqn_forward
    at out_pos, out_rgb and out_action against the restatement applied to out_q (the hit points
    differ from rt_render_volume_view's in the last bits: see test_gpu_view_equals_restatement);
  * row counts around the forward's workgroup tile, a frame without a surface hit, passes over
    sample slots, every route (fused, unfused, with out_q, stationary, scan, BVH, tiles), that a
    view changes nothing, and the scale against the map's own irradiance render.
Every pixel of every frame enters every comparison; the frames are at most 32 x 32 pixels
(the row-count frames are W x 1).
"""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from conftest import MODELS, ROOT

F = np.float32
SEED = 1984
ENV = 0.25           # env_light of the GPU frames: a miss is visible
PI_F = F(3.14159265358979323846)
IRR_SCALE = (F(2) * PI_F) / F(144)   # rt_render_irradiance's kIrrScale
NEG_INF = F(-np.inf)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def header_define(name):
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(-?\d+)", src, flags=re.M)
    assert m, name
    return int(m.group(1))


# ---- the restatement (numpy float32, every operation rounded on its own) ----------------

def cell_cos():
    """c_k = chiu_cos(gx + 0.5, gy + 0.5), k = gx * 12 + gy: 1 - xx * xx with
    xx = max(|2 (g / 12) - 1|) over the two coordinates."""
    g = np.arange(12, dtype=F) + F(0.5)
    a = np.abs(F(2) * (g / F(12)) - F(1))
    xx = np.maximum(a[:, None], a[None, :])
    c = (F(1) - xx * xx).reshape(144)
    assert c.dtype == F
    return c


def reduce_rows(q):
    """(S, action) of Q rows (n, 144): t_k = Q_k c_k; B_w = t_36w + t_36w+1 + .. one after another;
    S = ((B_0 + B_1) + B_2) + B_3; action = the first k of largest t_k, a scan from k = 0 that
    replaces on > starting from -inf (a NaN never wins; 0 if nothing exceeds -inf)."""
    q = np.ascontiguousarray(q, F).reshape(-1, 144)
    t = q * cell_cos()[None, :]
    assert t.dtype == F
    B = []
    for w in range(4):
        b = t[:, 36 * w].copy()
        for k in range(36 * w + 1, 36 * w + 36):
            b = b + t[:, k]
        B.append(b)
    S = ((B[0] + B[1]) + B[2]) + B[3]
    best = np.full(len(q), NEG_INF, F)
    act = np.zeros(len(q), np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(144):
            m = t[:, k] > best
            best = np.where(m, t[:, k], best)
            act = np.where(m, np.int32(k), act)
    assert S.dtype == F
    return S, act


def luminance(rgb):
    rgb = np.ascontiguousarray(rgb, F).reshape(-1, 3)
    return F(0.5) * (rgb.max(axis=1) + rgb.min(axis=1))


def shade(S, tri, albedo, tint):
    """L = (S brdf[tri]) kIrrScale, brdf = luminance / pi; grey, or albedo (L / luminance) and 0
    where the luminance is 0."""
    lum = luminance(albedo)
    brdf = lum / PI_F
    L = (S * brdf[tri]) * IRR_SCALE
    assert L.dtype == F
    if not tint:
        return np.repeat(L[:, None], 3, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = L / lum[tri]
        rgb = np.ascontiguousarray(albedo, F)[tri] * g[:, None]
    return np.where((lum[tri] == 0)[:, None], F(0), rgb).astype(F)


# ---------------------------------------------------------------- CPU ----------

def test_exports_constant_and_struct(rtmi_mod):
    L = rtmi_mod.lib()
    for s in ("rt_render_dqn_view", "rt_render_dqn_view_tiles_device"):
        assert s in rtmi_mod._lib.EXPORTS and hasattr(L, s)
    assert len(L.rt_render_dqn_view.argtypes) == 12 and len(L.rt_render_dqn_view_tiles_device.argtypes) == 12
    assert header_define("RT_DQN_VIEW_IRRADIANCE") == 0 == rtmi_mod.RT_DQN_VIEW_IRRADIANCE
    assert rtmi_mod.dqn.RT_DQN_VIEW_IRRADIANCE == rtmi_mod.RT_DQN_VIEW_IRRADIANCE
    assert ctypes.sizeof(rtmi_mod.RtDqnViewOpts) == 8
    assert callable(rtmi_mod.dqn.render_view) and callable(rtmi_mod.dqn.render_view_tiles_device)


def test_refusals_need_no_gpu(rtmi_mod):
    """NULL handles, outputs and options, an unknown mode, bad sizes, another preset or hit rule:
    all refused before a device is touched (no context exists here)."""
    R, L = rtmi_mod, rtmi_mod.lib()
    fp = np.zeros(8, F).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = np.zeros(8, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cam = R.camera(R.CAMERAS["cornell"])
    p = R.default_params(R.RT_PRESET_GPU, width=4, height=4, spp=1)
    o = R.RtDqnViewOpts(R.RT_DQN_VIEW_IRRADIANCE, 0)
    ref = ctypes.byref
    assert L.rt_render_dqn_view(None, None, None, ref(cam), ref(p), ref(o), 0, fp, None, None, None, None) == R._lib.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    assert L.rt_render_dqn_view_tiles_device(None, None, None, ref(cam), ref(p), ref(o), 0, ip, 1, 16, fp,
                                             None) == R._lib.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    # non-NULL handles that are never dereferenced: the value checks come first
    h = ctypes.c_void_p(1)
    assert L.rt_render_dqn_view(h, h, h, ref(cam), ref(p), ref(o), 0, None, None, None, None, None) == R._lib.RT_E_INVALID
    assert L.rt_render_dqn_view(h, h, h, ref(cam), ref(p), None, 0, fp, None, None, None, None) == R._lib.RT_E_INVALID
    assert L.rt_render_dqn_view(h, h, h, ref(cam), None, ref(o), 0, fp, None, None, None, None) == R._lib.RT_E_INVALID
    bad = R.RtDqnViewOpts(7, 0)
    for call in (lambda oo, pp: L.rt_render_dqn_view(h, h, h, ref(cam), ref(pp), ref(oo), 0, fp, None, None, None, None),
                 lambda oo, pp: L.rt_render_dqn_view_tiles_device(h, h, h, ref(cam), ref(pp), ref(oo), 0, ip, 1, 16, fp,
                                                                  None)):
        assert call(bad, p) == R._lib.RT_E_INVALID and b"mode" in L.rt_last_error()
        for kw in (dict(width=0), dict(height=-1), dict(spp=0)):
            q = R.default_params(R.RT_PRESET_GPU, **{**dict(width=4, height=4, spp=1), **kw})
            assert call(o, q) == R._lib.RT_E_INVALID, kw
        q = R.default_params(R.RT_PRESET_GPU, width=4, height=4, spp=1, hit_rule=R.RT_HIT_RULE_CPU)
        assert call(o, q) == R._lib.RT_E_UNSUPPORTED
        q = R.default_params(R.RT_PRESET_CPU, width=4, height=4, spp=1)
        assert call(o, q) == R._lib.RT_E_UNSUPPORTED
    q0 = R.default_params(R.RT_PRESET_GPU, width=4, height=4, spp=1, max_bounces=0)
    assert L.rt_render_dqn_view_tiles_device(h, h, h, ref(cam), ref(q0), ref(o), 0, None, 0, 16, None, None) == R._lib.RT_OK
    with pytest.raises(ValueError):
        R.dqn.render_view(None, None, None, cam, p, outputs=("depth",))


def test_cell_cosines():
    c = cell_cos().reshape(12, 12)
    assert np.array_equal(c, c.T)  # max(|x|, |y|) is symmetric
    assert np.all(c > 0) and np.all(c < 1)
    for gx in range(12):
        for gy in range(12):
            x = F(F(2) * F(F(gx + 0.5) / F(12)) - F(1))
            y = F(F(2) * F(F(gy + 0.5) / F(12)) - F(1))
            xx = max(abs(x), abs(y))
            assert c[gx, gy] == F(F(1) - F(xx * xx)), (gx, gy)
    # the mean of 1 - max(|x|, |y|)^2 over the square is 1/2 (sum c_k (2 pi / 144) = pi: the
    # hemisphere's cosine integral); the midpoint rule on 12 x 12 cells gives 73 / 144
    assert abs(float(c.astype(np.float64).sum()) - 73.0) < 1e-4


TIES = ((5, 60), (11, 132), (40, 51), (17, 61), (35, 134), (1, 12))


def restatement_rows():
    rng = np.random.default_rng(SEED)
    rows = [rng.uniform(0, 4, (64, 144)), rng.normal(size=(64, 144)) * 1e3,
            np.round(rng.uniform(0, 3, (64, 144))),           # many ties
            np.zeros((4, 144)), np.full((4, 144), 0.75)]
    q = np.concatenate(rows).astype(F)
    c = cell_cos()
    tie = np.zeros((6, 144), F)                                # equal largest t_k, in one block and across blocks
    for r, (k0, k1) in enumerate(TIES):
        assert c[k0] == c[k1] and k0 < k1                      # transposed cells (gx, gy), (gy, gx)
        tie[r, [k0, k1]] = 2.0
    nan = rng.uniform(0, 2, (8, 144)).astype(F)
    nan[0, 0] = np.nan
    nan[1, 143] = np.nan
    nan[2, :] = np.nan
    nan[3, 36:72] = np.nan
    nan[4, 7] = np.inf
    nan[5, :] = NEG_INF
    nan[6, 1:] = np.nan
    nan[7, :143] = np.nan
    return np.concatenate([q, tie, nan])


def test_restatement_against_itself():
    """reduce_rows against a scalar loop per row (the fold) and against the first arg-max of the
    non-NaN products (the action), and the fold against the double sum within its error bound."""
    q = restatement_rows()
    S, act = reduce_rows(q)
    c = cell_cos()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(q)):
            t = [F(q[r, k] * c[k]) for k in range(144)]
            B = []
            for w in range(4):
                b = t[36 * w]
                for k in range(36 * w + 1, 36 * w + 36):
                    b = F(b + t[k])
                B.append(b)
            s = F(F(F(B[0] + B[1]) + B[2]) + B[3])
            assert bits(s) == bits(S[r]) or (np.isnan(s) and np.isnan(S[r])), r
            tt = np.array(t, F)
            want = int(np.argmax(np.where(np.isnan(tt), NEG_INF, tt)))  # first index of the largest
            assert act[r] == want, (r, act[r], want)
    fin = np.isfinite(q).all(axis=1) & (q >= 0).all(axis=1)
    d = (q[fin].astype(np.float64) * c.astype(np.float64)).sum(axis=1)
    assert np.all(np.abs(S[fin] - d) <= 2 * 144 * 2.0 ** -24 * np.maximum(d, 1e-30))
    # ties take the first cell, NaN never wins, nothing above -inf gives 0
    n = len(q)
    assert list(act[n - 14:n - 8]) == [k0 for k0, _ in TIES]
    assert act[n - 8] != 0 and act[n - 6] == 0 and not 36 <= act[n - 5] < 72
    assert act[n - 4] == 7 and act[n - 3] == 0 and act[n - 2] == 0 and act[n - 1] == 143
    assert np.isnan(S[n - 6]) and np.isnan(S[n - 8])


def test_shade_restatement():
    alb = np.array([[0.75, 0.75, 0.75], [0.75, 0.15, 0.15], [0, 0, 0], [0.2, 0.9, 0.4]], F)
    S = np.array([1.0, 2.0, 3.0, 0.5], F)
    tri = np.arange(4)
    grey, tint = shade(S, tri, alb, False), shade(S, tri, alb, True)
    lum = luminance(alb)
    assert np.allclose(lum, [0.75, 0.45, 0.0, 0.55], rtol=1e-6)
    assert np.all(grey[:, 0] == grey[:, 1]) and np.all(tint[2] == 0) and grey[2, 0] == 0
    # a grey surface is its own tint; the tinted luminance is the grey value
    assert np.allclose(tint[0], grey[0], rtol=1e-6)
    assert np.allclose(luminance(tint), grey[:, 0], rtol=1e-6)
    assert np.allclose(grey[0, 0], 1.0 * 0.75 / np.pi * 2 * np.pi / 144, rtol=1e-6)


# ---------------------------------------------------------------- GPU ----------

def geometry(R, scene):
    if scene == "cornell":
        return R.cornell_geometry(R.RT_PRESET_GPU)
    return R.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


@functools.lru_cache(maxsize=None)
def door_model():
    import rtmi
    return rtmi.dqn.split_layers(rtmi.dqn.read_dynet(os.path.join(MODELS, "door_room_12_12.model")))


# (scene, network): the width classes of tests/test_dqn_forward_exact.py (the reference-shape
# body and the generic one) as exact networks, a selection network, the shipped model
NETS = {
    "exact-ref": ("cornell", lambda R, g: R.dqn.exact_weights(12, (200, 300, 200), "dense")),
    "exact-generic": ("cornell", lambda R, g: R.dqn.exact_weights(12, (96, 160, 96), "sparse")),
    "selection": ("door_room", lambda R, g: (*R.dqn.selection_weights(door_model()[0][0], door_model()[1][0],
                                                                      np.arange(56, 200), (200, 300, 200)),
                                             g.nn_vertices)),
    "door-model": ("door_room", lambda R, g: (*door_model(), g.nn_vertices)),
}


class World:
    def __init__(self, R, ctx, scene):
        self.R, self.ctx, self.scene = R, ctx, scene
        self.g = geometry(R, scene)
        self.sc = R.Scene(ctx, self.g)
        self.tri_all = self.g.all_triangles()
        self.nets = {}
        self._rm = None

    @property
    def rm(self):
        """a coarse radiance map, for rt_render_volume_view's camera hits"""
        if self._rm is None:
            self._rm = self.R.sarsa.RadianceMap(self.ctx, self.sc, SEED, 0.01)
        return self._rm

    def net(self, name):
        if name not in self.nets:
            scene, make = NETS[name]
            assert scene == self.scene
            W, b, verts = make(self.R, self.g)
            self.nets[name] = self.R.dqn.Dqn(self.ctx, verts, W, b)
        return self.nets[name]

    def close(self):
        for n in self.nets.values():
            n.close()
        if self._rm is not None:
            self._rm.close()
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(rtmi_mod, gpu_ctx):
    made = {}

    def get(scene):
        if scene not in made:
            made[scene] = World(rtmi_mod, gpu_ctx, scene)
        return made[scene]

    yield get
    for w in made.values():
        w.close()


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def params(R, w, h, spp=1, **kw):
    return R.default_params(R.RT_PRESET_GPU, width=w, height=h, spp=spp, env_light=ENV, **kw)


ALL = ("tri", "pos", "q", "action")


def expected_image(w, net, tri, pos, tint):
    """The view's sample values and actions from a frame's (tri, pos): the restatement on
    rt_dqn_forward(pos) at surface pixels, the emission at lights, env_light at misses."""
    g = w.g
    H, W_ = tri.shape
    rgb = np.full((H, W_, 3), F(ENV), F)
    act = np.full((H, W_), -1, np.int32)
    q = np.zeros((H, W_, 144), F)
    surf = (tri >= 0) & (tri < g.n_surf)
    light = tri >= g.n_surf
    rgb[light] = g.emission[tri[light] - g.n_surf]
    if surf.any():
        qs = net.forward(pos[surf])
        S, a = reduce_rows(qs)
        rgb[surf] = shade(S, tri[surf], g.albedo, tint)
        act[surf] = a
        q[surf] = qs
    return rgb, act, q, surf, light


def check_frame(w, net, cam, p, tint, first_sample=0):
    """One spp-1 frame with every output against its definition; returns (rgb, aov)."""
    R = w.R
    assert p.spp == 1
    rgb, aov = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint, first_sample=first_sample, outputs=ALL)
    tri, pos = aov["tri"], aov["pos"]
    want_rgb, want_act, want_q, surf, light = expected_image(w, net, tri, pos, tint)
    assert np.all(pos[~surf] == 0) and np.all(aov["q"][~surf] == 0) and np.all(aov["action"][~surf] == -1)
    assert np.array_equal(bits(aov["q"]), bits(want_q)), "out_q is not rt_dqn_forward(out_pos)"
    assert np.array_equal(aov["action"], want_act)
    assert np.array_equal(bits(rgb), bits(want_rgb))
    return rgb, aov, surf, light


def oracle_hits(oracle_mod, w, ocam, p, sample):
    """(tri of orc_primary_hits, the surface rays' positions handed to the network at bounce 1 by
    orc_render_dqn_wave in pixel order) for one sample index."""
    op = oracle_mod.params_from(p)
    op.spp, op.max_bounces = sample + 1, 2
    tri = oracle_mod.primary_hits(w.tri_all, w.g.n_surf, w.g.n_light, ocam, op, (0, 0, p.width, p.height),
                                  sample, sample + 1)[:, :, 0]
    locs = []

    def q_fn(loc):
        locs.append(loc.copy())
        return np.ones((len(loc), 144), F)

    oracle_mod.render_dqn_wave(w.g, ocam, op, q_fn)
    n_pix = p.width * p.height
    surf = (tri >= 0) & (tri < w.g.n_surf)
    if not locs:
        return tri, np.zeros((0, 3), F), surf
    # rays are ordered sample-major: skip the earlier samples' surface hits
    before = 0
    if sample > 0:
        all_tri = oracle_mod.primary_hits(w.tri_all, w.g.n_surf, w.g.n_light, ocam, op, (0, 0, p.width, p.height),
                                          0, sample)
        before = int(((all_tri >= 0) & (all_tri < w.g.n_surf)).sum())
    assert n_pix > 0
    return tri, locs[0][before:before + int(surf.sum())], surf


# the Cornell frame of the restatement test: pitched up from inside the opening, so that it shows
# surfaces, the ceiling light and the outside
CORNELL_VIEW = ((0.0, 0.0, -2.0, 1.0), {"yaw_x": -0.35})
CASES_1 = [(name, tint, first) for name in NETS for tint in (0, 1) for first in ((0,) if tint else (0, 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tint,first", CASES_1, ids=[f"{n}-tint{t}-s{f}" for n, t, f in CASES_1])
def test_gpu_view_equals_restatement(rtmi_mod, oracle_mod, worlds, name, tint, first):
    """20 x 12 (both image edges cut a 16 x 16 block), spp 1: every output bit for bit."""
    R = rtmi_mod
    w = worlds(NETS[name][0])
    net = w.net(name)
    pos, yaws = (R.CAMERAS[w.scene], {}) if w.scene != "cornell" else CORNELL_VIEW
    cam, ocam = R.camera(pos, **yaws), oracle_mod.camera(pos, **yaws)
    p = params(R, 20, 12)
    rgb, aov, surf, light = check_frame(w, net, cam, p, tint, first)
    tri, hit_pos, osurf = oracle_hits(oracle_mod, w, ocam, p, first)
    assert np.array_equal(aov["tri"], tri)
    assert np.array_equal(bits(aov["pos"][surf]), bits(hit_pos))
    miss = aov["tri"] < 0
    assert surf.sum() > 100 and np.all(rgb[miss] == F(ENV))
    assert np.all(rgb[light] == w.g.emission[aov["tri"][light] - w.g.n_surf])
    assert light.sum() > 0
    if w.scene == "cornell":
        assert miss.sum() > 0   # the frame shows all three kinds of sample
    n_act = len(np.unique(aov["action"][surf]))
    print(f"{name}: {surf.sum()} surface, {light.sum()} light, {miss.sum()} miss pixels, {n_act} distinct actions")
    assert np.any(aov["q"][surf] > 0)
    if not name.startswith("exact"):  # (an integer network's largest cell is the same everywhere)
        assert n_act > 1
    # rt_render_volume_view casts the same camera ray under the GPU hit rule: the same triangles.
    # Its hit points differ from the renderer's in the last bits (printed below) -- the renderer starts its ray 1e-5 along the direction and normalises the
    # direction again (trace_ray), the views do neither -- and the network is shown the
    # renderer's, so out_pos is pinned to orc_render_dqn_wave above and only bounded here, by
    # that offset.
    _, vtri, _, vpos = w.rm.view(cam, p, first_sample=first, aov=True)
    assert np.array_equal(aov["tri"], vtri)
    print(f"{name}: largest |out_pos - rt_render_volume_view's| {np.abs(aov['pos'] - vpos).max():.3g}, "
          f"{int((bits(aov['pos']) != bits(vpos)).any(axis=2).sum())} of {surf.sum()} hit points differ")
    assert np.abs(aov["pos"] - vpos).max() <= 1e-5


def floor_camera(R, oracle_mod):
    """inside the Cornell box, pitched at the floor: every camera ray lands on a surface"""
    pos = (0.0, 0.0, -0.5, 1.0)
    return R.camera(pos, yaw_x=FLOOR_PITCH), oracle_mod.camera(pos, yaw_x=FLOOR_PITCH)


FLOOR_PITCH = 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("exact-ref", "exact-generic"))
@pytest.mark.parametrize("route", ("fused", "unfused"))
def test_gpu_row_counts_around_the_tile(rtmi_mod, oracle_mod, worlds, name, route):
    """Surface-hit counts r - 1, r, r + 1 (r = rt_dqn_mlp_rows) and 1: W x 1 frames of a camera
    whose every ray hits a surface, the count asserted from out_tri."""
    R = rtmi_mod
    w = worlds("cornell")
    net = w.net(name)
    r = R.dqn.mlp_rows()
    cam, _ = floor_camera(R, oracle_mod)
    with env(RTMI_DQN_VIEW_FUSED=None if route == "fused" else "0"):
        for W_ in (r - 1, r, r + 1, 1):
            p = params(R, W_, 1)
            full = check_frame(w, net, cam, p, 0)            # out_q requested: the unfused route
            assert int(full[2].sum()) == W_, (W_, int(full[2].sum()))
            lean, aov = R.dqn.render_view(w.ctx, w.sc, net, cam, p, outputs=("tri", "action"))
            assert np.array_equal(bits(lean), bits(full[0])) and np.array_equal(aov["action"], full[1]["action"])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ("fused", "unfused"))
def test_gpu_no_surface_hit(rtmi_mod, worlds, route):
    """A camera facing out of the box: an empty list, every pixel env_light."""
    R = rtmi_mod
    w = worlds("cornell")
    cam = R.camera(R.CAMERAS["cornell"], yaw_y=float(np.pi))
    with env(RTMI_DQN_VIEW_FUSED=None if route == "fused" else "0"):
        for size, spp in (((20, 12), 1), ((5, 3), 3)):
            p = params(R, *size, spp=spp)
            rgb, aov = R.dqn.render_view(w.ctx, w.sc, w.net("exact-ref"), cam, p, outputs=ALL if spp == 1 else ("tri",))
            assert np.all(aov["tri"] == -1) and np.all(rgb == F(ENV))
            if spp == 1:
                assert not aov["q"].any() and not aov["pos"].any() and np.all(aov["action"] == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("exact-ref", "door-model"))
def test_gpu_passes_fold_in_sample_order(rtmi_mod, worlds, name):
    """spp 5 from sample 3 with two sample slots per pass: the one-pass frame, and the fold of
    five spp-1 frames in sample order."""
    R = rtmi_mod
    w = worlds(NETS[name][0])
    net = w.net(name)
    cam = R.camera(R.CAMERAS[w.scene])
    p5, p1 = params(R, 20, 12, spp=5), params(R, 20, 12, spp=1)
    n_pix = 2 * 256  # two 16 x 16 blocks
    one, aov1 = R.dqn.render_view(w.ctx, w.sc, net, cam, p5, tint=True, first_sample=3, outputs=("tri", "action"))
    with env(RTMI_DQN_RAYS_IN_FLIGHT=2 * n_pix):
        split, aov2 = R.dqn.render_view(w.ctx, w.sc, net, cam, p5, tint=True, first_sample=3, outputs=("tri", "action"))
    with env(RTMI_DQN_RAYS_IN_FLIGHT=1):
        single = R.dqn.render_view(w.ctx, w.sc, net, cam, p5, tint=True, first_sample=3)
    assert np.array_equal(bits(one), bits(split)) and np.array_equal(bits(one), bits(single))
    assert all(np.array_equal(aov1[k], aov2[k]) for k in aov1)
    acc = None
    for s in range(3, 8):
        v, a = R.dqn.render_view(w.ctx, w.sc, net, cam, p1, tint=True, first_sample=s, outputs=("tri", "action"))
        if s == 3:  # the outputs describe the first sample
            assert all(np.array_equal(a[k], aov1[k]) for k in a)
        acc = v if acc is None else acc + v
    assert acc.dtype == F
    assert np.array_equal(bits(acc / F(5)), bits(one))
    assert len(np.unique(one.reshape(-1, 3), axis=0)) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_gpu_routes_agree(rtmi_mod, worlds, name):
    """Fused, unfused and with out_q requested; streaming and stationary forward."""
    R = rtmi_mod
    w = worlds(NETS[name][0])
    net = w.net(name)
    cam = R.camera(R.CAMERAS[w.scene])
    p = params(R, 32, 32, spp=2)
    for tint in (0, 1):
        with env(RTMI_DQN_VIEW_FUSED="1"):
            fused, fa = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint, outputs=("action",))
        with env(RTMI_DQN_VIEW_FUSED="0"):
            unfused, ua = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint, outputs=("action",))
        default = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint)
        with_q, qa = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint, outputs=("q", "action"))
        for other in (unfused, default, with_q):
            assert np.array_equal(bits(fused), bits(other))
        assert np.array_equal(fa["action"], ua["action"]) and np.array_equal(fa["action"], qa["action"])
        assert np.array_equal(reduce_rows(qa["q"].reshape(-1, 144))[1][qa["action"].ravel() >= 0],
                              qa["action"].ravel()[qa["action"].ravel() >= 0])
        try:
            net.set_mlp(net.MLP_STATIONARY)
            stat, sa = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=tint, outputs=("action",))
        finally:
            net.set_mlp(net.MLP_AUTO)
        assert np.array_equal(bits(fused), bits(stat)) and np.array_equal(fa["action"], sa["action"])


@pytest.mark.gpu
def test_gpu_scan_equals_bvh(rtmi_mod, gpu_ctx):
    """The bunny in the Cornell box, 16 x 16: the exact BVH (k_dqn_camera<-1>) and the scan."""
    from test_bvh import bunny_cornell
    R = rtmi_mod
    g = bunny_cornell(R, R.RT_PRESET_GPU)
    W, b, verts = R.dqn.exact_weights(12, (200, 300, 200), "dense")
    cam = R.camera(R.CAMERAS["cornell"])
    p = params(R, 16, 16, spp=2)
    out = []
    with R.Scene(gpu_ctx, g) as sc, R.dqn.Dqn(gpu_ctx, verts, W, b) as net:
        for accel in (R.ACCEL_BVH, R.ACCEL_SCAN):
            sc.set_accel(accel)
            out.append(R.dqn.render_view(gpu_ctx, sc, net, cam, p, tint=True, outputs=ALL))
    (a, aa), (c, ca) = out
    assert np.array_equal(bits(a), bits(c))
    for k in ALL:
        assert np.array_equal(aa[k], ca[k]), k
    assert ((aa["tri"] >= 36) & (aa["tri"] < g.n_surf)).sum() > 0  # the bunny is in view


@pytest.mark.gpu
@pytest.mark.parametrize("T", (16, 32))
def test_gpu_tiles_equal_full_frame(rtmi_mod, worlds, T):
    import torch
    R = rtmi_mod
    w = worlds("door_room")
    net = w.net("door-model")
    cam = R.camera(R.CAMERAS["door_room"])
    W_, H = 30, 27
    p = params(R, W_, H, spp=3)
    full = R.dqn.render_view(w.ctx, w.sc, net, cam, p, tint=True, first_sample=5)
    origins = R.tiles.tile_origins(W_, H, T)
    pick = origins[np.random.default_rng(SEED).permutation(len(origins))]
    fill = -7.0
    out = torch.full((len(pick), T, T, 3), fill, dtype=torch.float32, device=torch.device("cuda", 0))
    R.dqn.render_view_tiles_device(w.ctx, w.sc, net, cam, p, pick, T, out.data_ptr(), 0, tint=True, first_sample=5)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, (x, y) in enumerate(pick):
        vw, vh = min(T, W_ - x), min(T, H - y)
        assert np.array_equal(bits(got[i, :vh, :vw]), bits(full[y:y + vh, x:x + vw])), (x, y)
        assert np.all(got[i, vh:] == fill) and np.all(got[i, :, vw:] == fill), (x, y)
    R.dqn.render_view_tiles_device(w.ctx, w.sc, net, cam, p, pick[:0], T, 0, 0)  # an empty list is a no-op
    if len(pick) > 1:  # a part of the list alone gives the same tiles
        out.fill_(fill)
        R.dqn.render_view_tiles_device(w.ctx, w.sc, net, cam, p, pick[:1], T, out.data_ptr(), 0, tint=True,
                                       first_sample=5)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(got[0]))


@pytest.mark.gpu
def test_gpu_view_is_read_only(rtmi_mod, worlds):
    """rt_dqn_forward at fixed points and a small rt_render_dqn frame, before and after a view."""
    R = rtmi_mod
    w = worlds("door_room")
    net = w.net("door-model")
    cam = R.camera(R.CAMERAS["door_room"])
    pts = np.random.default_rng(SEED).uniform(-1, 1, (300, 3)).astype(F)
    pr = R.default_params(R.RT_PRESET_GPU, width=24, height=20, spp=2, max_bounces=4)
    q0 = net.forward(pts)
    img0, casts0 = R.dqn.render(w.ctx, w.sc, net, cam, pr)
    for route in ("1", "0"):
        with env(RTMI_DQN_VIEW_FUSED=route):
            R.dqn.render_view(w.ctx, w.sc, net, cam, params(R, 32, 32, spp=3), tint=True, outputs=("tri", "action"))
        img1, casts1 = R.dqn.render(w.ctx, w.sc, net, cam, pr)
        assert casts1 == casts0 and np.array_equal(bits(img1), bits(img0))
        assert np.array_equal(bits(net.forward(pts)), bits(q0))
    assert img0.mean() > 0


@pytest.mark.gpu
def test_gpu_scale_against_the_map(rtmi_mod, oracle_mod, worlds):
    """Q = 0.75 in every volume of the map and from the network (last layer: zero weights, bias
    0.75): the view and rt_render_irradiance(k = 1, mean, no tint) agree to 2e-5 relative at every
    surface pixel where the map has a volume in range.  144 fp32 additions and 144 products at 2^-24
    each against the host's double fold rounded to float per step: 2 * 144 * 2^-24 = 1.7e-5."""
    R = rtmi_mod
    w = worlds("cornell")
    cam = R.camera(R.CAMERAS["cornell"])
    p = params(R, 32, 32)
    nn = np.unique(w.g.tri.reshape(-1, 3), axis=0).astype(F).ravel()  # the box's vertices as the network's inputs
    W, b = R.dqn.synthetic_weights(nn.size)
    W[3][:] = 0
    b[3][:] = 0.75
    with R.sarsa.RadianceMap(w.ctx, w.sc, SEED) as rm, R.dqn.Dqn(w.ctx, nn, W, b) as net:
        rm.write(np.full((rm.n_volumes, 144), 0.75, F))
        reach = rm.knn_reach()
        irr, tri, pos, vol, _ = rm.irradiance_view(cam, p, 1, None, R.RT_IRR_MEAN, False, aov=True)
        view, aov = R.dqn.render_view(w.ctx, w.sc, net, cam, p, outputs=("tri", "pos", "q"))
    assert np.array_equal(aov["tri"], tri)
    surf = (tri >= 0) & (tri < w.g.n_surf)
    assert np.all(aov["q"][surf] == F(0.75))
    have = surf & (vol[:, :, 0] >= 0)
    # the pixels left out, on the CPU: the nearest volume of the restated map is out of reach
    om = oracle_mod.Sarsa(w.g, SEED)
    vpos = om.volumes()[0]
    nrm = oracle_mod.normals(w.tri_all)[tri[surf]]
    near = om.nearest(pos[surf], nrm)
    d = np.linalg.norm(vpos[np.maximum(near, 0)].astype(np.float64) - pos[surf], axis=1)
    out_cpu = (near < 0) | (d >= reach)
    print(f"surface pixels {surf.sum()}, without a volume in range: device {int((surf & ~have).sum())}, "
          f"restated map {int(out_cpu.sum())}")
    assert out_cpu.mean() < 0.05 and (surf & ~have).sum() < 0.05 * surf.sum()
    rel = np.abs(view[have].astype(np.float64) - irr[have]) / irr[have]
    print(f"largest relative difference view / map {rel.max():.3g}")
    assert have.sum() > 500 and np.all(irr[have] > 0)
    assert rel.max() <= 2e-5
    assert np.array_equal(view[~surf], irr[~surf])  # lights and misses are the same samples
