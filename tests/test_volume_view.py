"""Radiance-map views (the reference's Voronoi mode, GPU/main.cu PATH_TRACING_METHOD 2):
rt_sarsa_voronoi_palette, rt_sarsa_set_view_colours, rt_render_volume_view[_tiles_device].

Everything is pinned against the existing restatement (oracle/):
  * the palette against Philox restated in numpy (no GPU);
  * the view's per-pixel triangle, hit point and nearest volume against orc_primary_hits, the
    camera ray restated in numpy float32 with the pinned intersect call's t, and
    orc_sarsa_nearest, in both search modes and at two volume densities;
  * the volumes once more, with no camera restatement, through the TD events that the
    restatement's render makes on each first hit's volume;
  * colours, the chunk fold, tile renders, and that a view leaves the map as it found it.
The shapes (50x39, 17x5, 1x1, 80x72 with 32-pixel tiles) leave most waves partly filled.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, PKG

SEED = 1984
PALETTE_WORD = 0x566F726F  # counter word 3 of the palette's Philox blocks


def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def palette_restated(oracle_mod, seed, n):
    """Volume v: u(w0), u(w1), u(w2) of Philox4x32-10 with key (seed lo, seed hi) and counter
    (v, 0, 0, PALETTE_WORD); u = (x >> 8) 2^-24."""
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = np.zeros((n, 3), np.float32)
    for v in range(n):
        w = oracle_mod.philox([v, 0, 0, PALETTE_WORD], key)
        out[v] = (w[:3] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return out


# ---------------------------------------------------------------- CPU ----------

@pytest.mark.parametrize("seed", (SEED, 0xFEDCBA9876543210))
def test_palette_equals_philox_restatement(rtmi_mod, oracle_mod, seed):
    for n in (0, 1, 1000):
        got = rtmi_mod.sarsa.voronoi_palette(seed, n)
        assert got.shape == (n, 3) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), palette_restated(oracle_mod, seed, n).view(np.uint32))
        assert got.tobytes() == rtmi_mod.sarsa.voronoi_palette(seed, n).tobytes()
    big = rtmi_mod.sarsa.voronoi_palette(seed, 1000)
    assert np.all((big >= 0) & (big < 1))
    assert np.array_equal(big[:1], rtmi_mod.sarsa.voronoi_palette(seed, 1))  # a volume's colour is its own
    assert len(np.unique(big, axis=0)) == 1000


def test_palette_seeds_differ_and_stream_is_apart_from_render_draws(rtmi_mod, oracle_mod):
    a, b = rtmi_mod.sarsa.voronoi_palette(1, 64), rtmi_mod.sarsa.voronoi_palette(2, 64)
    assert not np.array_equal(a, b)
    # the render draws' blocks have counter word 3 = 0: another block than the palette's
    w0 = oracle_mod.philox([5, 0, 0, 0], [1, 0])
    assert not np.array_equal((w0[:3] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), a[5])


def test_palette_refuses_invalid_arguments(rtmi_mod):
    L = rtmi_mod.lib()
    buf = np.zeros(3, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.rt_sarsa_voronoi_palette(SEED, -1, fp) == -1
    assert L.rt_sarsa_voronoi_palette(SEED, 1, None) == -1
    assert b"rgb" in L.rt_last_error()
    assert L.rt_sarsa_voronoi_palette(SEED, 0, None) == 0  # nothing to write
    assert L.rt_sarsa_set_view_colours(None, None) == -1
    with pytest.raises(rtmi_mod.RtError):
        rtmi_mod.sarsa.voronoi_palette(SEED, -5)


def test_colour_table_helpers(rtmi_mod):
    S = rtmi_mod.sarsa
    irr = S.irradiance_colours(np.array([0.0, 1.0, 4.0], np.float32))
    assert irr.dtype == np.float32 and np.array_equal(irr, np.array([[0] * 3, [0.25] * 3, [1] * 3], np.float32))
    vis = np.zeros((3, 144), np.uint32)
    vis[1, 7] = 9
    vis[2] = 1000
    v = S.visits_colours(vis)
    assert v.shape == (3, 3) and v[0, 0] == 0 and v[2, 0] == 1 and 0 < v[1, 0] < v[2, 0]
    q = np.zeros((4, 144), np.float32)
    q[1, 11] = 1                 # sector (0, 11): hue 0 (red), full value
    q[2, [4 * 12, 4 * 12 + 5]] = 2   # two maxima: the first, sector (4, 0): hue 1/3 (green), value 1/12
    q[3, 8 * 12 + 11] = 3        # hue 2/3 (blue)
    c = S.max_q_colours(q)
    assert np.allclose(c[0], [1 / 12, 0, 0]) and np.allclose(c[1], [1, 0, 0])
    assert np.allclose(c[2], [0, 1 / 12, 0]) and np.allclose(c[3], [0, 0, 1])
    assert not np.any(S.irradiance_colours(np.zeros(2, np.float32)))


# ---------------------------------------------------------------- GPU ----------

# (id, scene, width, height, camera yaws, hit rule): the scene set of every case
CASES = [
    ("door_room-50x39", "door_room", 50, 39, {}, 1),
    ("cornell-yaw_y", "cornell", 50, 39, {"yaw_y": 0.3}, 1),
    ("cornell-pitched", "cornell", 50, 39, {"yaw_x": 0.2}, 1),  # pitched: no rectangle cull
    ("archway-rule0", "archway", 50, 39, {}, 0),
    ("door_room-17x5", "door_room", 17, 5, {}, 1),
    ("door_room-1x1", "door_room", 1, 1, {}, 1),
]
CASE_IDS = [c[0] for c in CASES]
FIRST = (0, 5)


class World:
    """One scene's device scene, viewed map, oracle map and normals, shared by the tests; the
    twin map is rendered in lock-step with the viewed one and never viewed."""

    def __init__(self, rtmi_mod, oracle_mod, gpu_ctx, scene, area):
        self.rtmi, self.scene_name, self.area = rtmi_mod, scene, area
        self.g = geometry(rtmi_mod, scene)
        self.sc = rtmi_mod.Scene(gpu_ctx, self.g)
        self.ctx = gpu_ctx
        self.rm = rtmi_mod.sarsa.RadianceMap(gpu_ctx, self.sc, SEED, area)
        self.om = oracle_mod.Sarsa(self.g, SEED, 0.001 if area is None else area)
        self.tri_all = self.g.all_triangles()
        self.normals = oracle_mod.normals(self.tri_all)
        self._twin = None

    @property
    def twin(self):
        if self._twin is None:
            assert self.rm.frames == 0, "the twin must see every render of the viewed map"
            self._twin = self.rtmi.sarsa.RadianceMap(self.ctx, self.sc, SEED, self.area)
        return self._twin

    def close(self):
        for m in (self.rm, self._twin):
            if m is not None:
                m.close()
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(rtmi_mod, oracle_mod, gpu_ctx):
    made = {}

    def get(scene, area=None):
        if (scene, area) not in made:
            made[(scene, area)] = World(rtmi_mod, oracle_mod, gpu_ctx, scene, area)
        return made[(scene, area)]

    yield get
    for w in made.values():
        w.close()


def cameras(rtmi_mod, oracle_mod, scene, yaws):
    pos = rtmi_mod.CAMERAS[scene]
    return rtmi_mod.camera(pos, **yaws), oracle_mod.camera(pos, **yaws)


def view_params(rtmi_mod, width, height, hit_rule, spp=1, split=1, **kw):
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=width, height=height, spp=spp, spp_split=split,
                                   hit_rule=hit_rule, **kw)


def camera_dirs(oracle_mod, p, cam, s):
    """rt_oracle.c's camera_ray (GPU preset) for sample s of every pixel, in numpy float32:
    direction (H, W, 3)."""
    f = np.float32
    W, H = p.width, p.height
    key = [p.seed & 0xFFFFFFFF, (p.seed >> 32) & 0xFFFFFFFF]
    r1, r2 = np.zeros((H, W), f), np.zeros((H, W), f)
    for y in range(H):
        for x in range(W):
            w = oracle_mod.philox([y * W + x, s, 0, 0], key)
            u = (w[:2] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
            r1[y, x], r2[y, x] = u[0], u[1]
    px, py = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    dx = (px + r1) - f(W) / f(2)
    dy = (py + r2) - f(H) / f(2)
    dz = np.full((H, W), f(H), f)
    inv = f(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx * inv, dy * inv, dz * inv
    cy, sy = f(math.cos(float(f(cam.yaw_y)))), f(math.sin(float(f(cam.yaw_y))))
    cx, sx = f(math.cos(float(f(cam.yaw_x)))), f(math.sin(float(f(cam.yaw_x))))
    z, one = f(0), f(1)
    rx = (cy * dx + z * dy) + (-sy * dz + z * one)
    ry = (z * dx + one * dy) + (z * dz + z * one)
    rz = (sy * dx + z * dy) + (cy * dz + z * one)
    rw = (z * dx + z * dy) + (z * dz + one * one)
    qx = (one * rx + z * ry) + (z * rz + z * rw)
    qy = (z * rx + cx * ry) + (sx * rz + z * rw)
    qz = (z * rx + -sx * ry) + (cx * rz + z * rw)
    d = np.stack([qx, qy, qz], axis=2)
    assert d.dtype == f
    return d


def triangles_of_codes(codes, g, hit_rule):
    """rt_intersect's hit codes ((type << 30) | index) as checks against triangle indices:
    returns (triangle index or -1 where the code names one, light plane or -1 elsewhere)."""
    c = codes.astype(np.int64) & 0xFFFFFFFF
    miss = codes == -1
    typ, idx = c >> 30, c & 0x3FFFFFFF
    tri = np.where(miss, -1, np.where(typ == 2, idx, g.n_surf + idx))
    if hit_rule == 0:  # a light's index is its plane there
        return np.where(~miss & (typ == 1), -2, tri), np.where(~miss & (typ == 1), idx, -1)
    return tri, np.full(codes.shape, -1)


AOV_CASES = [(c, None) for c in CASES] + [(CASES[0], 0.1)]  # door_room at 344 volumes too
AOV_IDS = CASE_IDS + ["door_room-50x39-area0.1"]


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case,area", AOV_CASES, ids=AOV_IDS)
def test_gpu_view_aovs_equal_restatement(rtmi_mod, oracle_mod, gpu_ctx, worlds, case, area, first):
    _, scene, W, H, yaws, rule = case
    w = worlds(scene, area)
    S = rtmi_mod.sarsa
    p = view_params(rtmi_mod, W, H, rule)
    cam, ocam = cameras(rtmi_mod, oracle_mod, scene, yaws)
    got = {}
    for mode in (S.SEARCH_KD, S.SEARCH_GRID):  # (the grid mode is left on)
        w.rm.set_search(mode)
        got[mode] = w.rm.view(cam, p, first, aov=True)
    for a, b in zip(got[S.SEARCH_KD], got[S.SEARCH_GRID]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _, tri, vol, pos = got[S.SEARCH_GRID]
    n_surf = w.g.n_surf
    want_tri = oracle_mod.primary_hits(w.tri_all, n_surf, w.g.n_light, ocam, oracle_mod.params_from(p),
                                       (0, 0, W, H), first, first + 1)[:, :, 0]
    assert np.array_equal(tri, want_tri)
    surf = (tri >= 0) & (tri < n_surf)
    if W * H > 1:
        assert surf.any()
    assert np.all(vol[~surf] == -1) and not np.any(pos[~surf].view(np.uint32))
    # the hit point: o + t (d t_scale), separate multiply and add, t from the pinned intersect
    d = camera_dirs(oracle_mod, p, cam, first)
    o = np.broadcast_to(np.array(rtmi_mod.CAMERAS[scene][:3], np.float32), d.shape)
    t, codes = rtmi_mod.intersect(gpu_ctx, w.sc, o.reshape(-1, 3), d.reshape(-1, 3), p.t_scale, rule)
    t, codes = t.reshape(H, W), codes.reshape(H, W)
    ctri, cplane = triangles_of_codes(codes, w.g, rule)
    named = ctri != -2
    assert np.array_equal(ctri[named], tri[named])
    assert np.all(tri[~named] >= n_surf)
    assert np.array_equal(cplane[~named], w.g.light_group[tri[~named] - n_surf])
    D = d * np.float32(p.t_scale)
    want_pos = (o + t[:, :, None] * D).astype(np.float32)
    assert np.array_equal(pos[surf].view(np.uint32), want_pos[surf].view(np.uint32))
    assert np.array_equal(vol[surf], w.om.nearest(pos[surf], w.normals[tri[surf]]))
    assert np.all((vol[surf] >= 0) & (vol[surf] < w.rm.n_volumes))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_gpu_view_volumes_equal_td_event_counts(rtmi_mod, oracle_mod, worlds, case):
    """With the max-direction sampler and max_bounces 2, every path of the restatement whose
    camera ray hits a surface makes exactly one TD event, on that hit's nearest volume
    (sarsa_trace): its per-volume event counts are the histogram of the view's volumes."""
    _, scene, W, H, yaws, rule = case
    w = worlds(scene)
    cam, ocam = cameras(rtmi_mod, oracle_mod, scene, yaws)
    p = view_params(rtmi_mod, W, H, rule, max_bounces=2)
    fresh = oracle_mod.Sarsa(w.g, SEED)
    fresh.set_sampling(1)
    _, counts = fresh.td_rect(ocam, oracle_mod.params_from(p), (0, 0, W, H))
    per_volume = counts.reshape(fresh.n_volumes, 144).sum(axis=1)
    _, tri, vol, _ = w.rm.view(cam, p, 0, aov=True)
    assert per_volume.sum() == np.count_nonzero((tri >= 0) & (tri < w.g.n_surf)) > 0
    assert np.array_equal(per_volume, np.bincount(vol[vol >= 0], minlength=fresh.n_volumes))


def maps_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_view_colours_and_map_untouched(rtmi_mod, oracle_mod, worlds, case, first):
    _, scene, W, H, yaws, rule = case
    w = worlds(scene)
    S = rtmi_mod.sarsa
    cam, _ = cameras(rtmi_mod, oracle_mod, scene, yaws)
    p = view_params(rtmi_mod, W, H, rule)
    rm, twin = w.rm, w.twin
    one = np.float32(1)

    def expect(table, vol):
        return np.where((vol >= 0)[:, :, None], table[np.maximum(vol, 0)], one).astype(np.float32)

    # the palette of the map's seed (what a map that never had colours set draws with)
    if rm.frames > 0:
        rm.set_view_colours(None)
    rgb, _, vol, _ = rm.view(cam, p, first, aov=True)
    assert np.array_equal(rgb.view(np.uint32), expect(S.voronoi_palette(SEED, rm.n_volumes), vol).view(np.uint32))
    assert np.array_equal(rgb, rm.view(cam, p, first))  # the same image without the AOVs
    # two training frames on both maps, then the irradiance they learned as the table
    pt = view_params(rtmi_mod, W, H, rule, spp=2)
    for m in (rm, twin):
        m.render(cam, pt, 2)
    before, frames = rm.read(), rm.frames
    table = S.irradiance_colours(before[3])
    rm.set_view_colours(table)
    rgb = rm.view(cam, p, first)
    assert np.array_equal(rgb.view(np.uint32), expect(table, vol).view(np.uint32))
    st0 = rm.search_stats()
    rm.set_td_mode(S.TD_INFRAME)  # the in-frame rule's map is read only too
    assert np.array_equal(rgb, rm.view(cam, p, first))
    rm.set_td_mode(S.TD_FRAME)
    assert maps_equal(rm.read(), before) and rm.frames == frames
    assert rm.search_stats()["kd_fallbacks"] >= st0["kd_fallbacks"]
    # the viewed map goes on exactly as its twin that was never viewed
    (ia, ca), (ib, cb) = rm.render(cam, pt, 1), twin.render(cam, pt, 1)
    assert ca == cb and np.array_equal(ia, ib)
    assert maps_equal(rm.read(), twin.read()) and rm.frames == twin.frames == frames + 1
    rm.set_view_colours(None)


def fold(samples, split):
    """each chunk's samples added in order, the chunk sums added in order, / spp."""
    spp = len(samples)
    per = spp // split
    chunks = []
    for c in range(split):
        acc = np.zeros_like(samples[0])
        for s in samples[c * per:(c + 1) * per]:
            acc = acc + s
        chunks.append(acc)
    tot = chunks[0]
    for c in chunks[1:]:
        tot = tot + c
    assert tot.dtype == np.float32
    return tot / np.float32(spp)


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_view_fold_equals_single_sample_views(rtmi_mod, oracle_mod, worlds, case, first):
    _, scene, W, H, yaws, rule = case
    w = worlds(scene)
    cam, _ = cameras(rtmi_mod, oracle_mod, scene, yaws)
    w.rm.set_view_colours(None)
    singles = [w.rm.view(cam, view_params(rtmi_mod, W, H, rule), first + s) for s in range(8)]
    if W * H > 1:
        assert not np.array_equal(singles[0], singles[1])  # each sample re-jitters
    for split in (1, 4):
        got = w.rm.view(cam, view_params(rtmi_mod, W, H, rule, spp=8, split=split), first)
        assert np.array_equal(got.view(np.uint32), fold(singles, split).view(np.uint32)), split


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
def test_gpu_view_tiles_equal_full_view(rtmi_mod, oracle_mod, worlds, first):
    import torch
    w = worlds("door_room")
    W, H, T = 80, 72, 32
    cam, _ = cameras(rtmi_mod, oracle_mod, "door_room", {})
    p = view_params(rtmi_mod, W, H, 1, spp=4, split=2)
    w.rm.set_view_colours(None)
    full = w.rm.view(cam, p, first)
    origins = rtmi_mod.tiles.tile_origins(W, H, T)
    assert len(origins) == 9
    pick = origins[[8, 2, 4, 0, 7, 5]]  # scattered: corner, right-edge and bottom-edge tiles among them
    dev = torch.device("cuda", 0)
    fill = -7.0
    out = torch.full((len(pick), T, T, 3), fill, dtype=torch.float32, device=dev)
    w.rm.view_tiles_device(cam, p, pick, T, out.data_ptr(), 0, first)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k, (x, y) in enumerate(pick):
        vw, vh = min(T, W - x), min(T, H - y)
        assert np.array_equal(got[k, :vh, :vw], full[y:y + vh, x:x + vw]), (x, y)
        # the overhang of an edge tile is not written (as the SARSA tile render leaves it)
        assert np.all(got[k, vh:] == fill) and np.all(got[k, :, vw:] == fill), (x, y)
    w.rm.view_tiles_device(cam, p, pick[:0], T, 0, 0, first)  # an empty tile list is a no-op


@pytest.mark.gpu
def test_gpu_view_refuses_bad_arguments(rtmi_mod, oracle_mod, worlds):
    w = worlds("door_room")
    cam, _ = cameras(rtmi_mod, oracle_mod, "door_room", {})
    for bad in ({"spp": 0}, {"spp": 6, "split": 4}, {"spp": 9, "split": 3}, {"width": 0}):
        kw = {"width": 8, "height": 8, "hit_rule": 1}
        kw.update(bad)
        with pytest.raises(rtmi_mod.RtError) as e:
            w.rm.view(cam, view_params(rtmi_mod, kw.pop("width"), kw.pop("height"), kw.pop("hit_rule"), **kw))
        assert e.value.code == -1
    # max_bounces, sampler and env_light are ignored
    p = view_params(rtmi_mod, 8, 8, 1)
    q = view_params(rtmi_mod, 8, 8, 1, max_bounces=0, sampler=rtmi_mod.RT_SAMPLER_COSINE, env_light=3.0)
    assert np.array_equal(w.rm.view(cam, p), w.rm.view(cam, q))
    with pytest.raises(ValueError):
        w.rm.set_view_colours(np.zeros((3, 3), np.float32))


@pytest.mark.gpu
def test_gpu_facade_voronoi_trace_equals_view(rtmi_mod, gpu_ctx, tmp_path):
    """examples/reinforcement_main.cpp's method-2 loop (host/voronoi_trace.h) on a 24x20 screen:
    the saved frame is the Python view of the last frame's sample index, packed the same way."""
    exe = os.path.join(PKG, "build", "reinforcement_demo")
    assert os.path.exists(exe), f"{exe} missing: make -C {PKG}"
    obj = os.path.join(MODELS, "door_room.obj")
    out = str(tmp_path / "voronoi.bmp")
    r = subprocess.run([exe, "voronoi", obj, "1", "3", out, "24", "20"], capture_output=True, text=True, timeout=240,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("voronoi view") == 3
    raw = open(out, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 4 * 24 * 20
    got = np.frombuffer(raw[54:], dtype="<u4").reshape(20, 24)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=24, height=20, spp=1)
    with rtmi_mod.Scene(gpu_ctx, rtmi_mod.obj_geometry(obj, "door_room")) as sc, \
            rtmi_mod.sarsa.RadianceMap(gpu_ctx, sc, SEED) as rm:
        img = rm.view(rtmi_mod.camera(rtmi_mod.CAMERAS["door_room"]), p, first_sample=2)
    assert np.array_equal(got, rtmi_mod.pack_argb(img))
    assert len(np.unique(got)) > 20  # many volumes' colours, not a flat frame
