"""The k nearest radiance volumes (rt_sarsa_knn) and the irradiance render of the map on them
(rt_render_irradiance[_tiles_device]: the CPU engine's draw_radiance_map_path_tracing).

  * the search against its definition restated by brute force in numpy float32, bit for bit:
    volumes, distances and counts, for k in (1, 3, 8), two radii and three volume densities;
  * the render against rt_render_volume_view (triangle, hit point), rt_sarsa_knn (volumes,
    distances) and the numpy float32 restatement of the interpolation, bit for bit; the chunk
    fold, the tile render, and that the map is left exactly as it was;
  * on a map of equal Q everywhere, that equal values interpolate to themselves;
  * the facade's demo frame against the C ABI's.
The brute force is checked against itself without a GPU, on the restatement's (oracle/) map.
No query and no pixel is left out of any comparison.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, PKG, ROOT

SEED = 1984
F = np.float32
INF = F(np.inf)
KS = (1, 3, 8)
AREAS = (0.001, 0.004, 0.01)
# the counts (capped at 8) that the query set of each density covers, over both radii
CLAIMED_COUNTS = {0.001: (0, 1, 2, 3, 8), 0.004: (0, 1, 2, 3, 8), 0.01: (0, 1, 2, 3)}
N_VOLUME_QUERIES = 1500
MIN_TIES = 64


def header_define(name):
    import re
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(-?\d+)", src, flags=re.M)
    assert m, name
    return int(m.group(1))


def reach_of(max_dist=0.003):
    """sqrt(MAX_DIST) * 0.999 in float32: the grid's accept radius (rt_sarsa_knn_reach)."""
    return F(np.sqrt(F(max_dist)) * F(0.999))


def len3(dx, dy, dz):
    """rt_sarsa_search.hpp's len3: sqrtf((x x + y y) + z z), every operation rounded on its own."""
    assert dx.dtype == dy.dtype == dz.dtype == F
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


class Brute:
    """The definition by brute force: per query (p, N) the volumes whose normal equals N under
    float == and whose len3 distance is < radius, ascending by (distance, index)."""

    def __init__(self, vpos, vnrm):
        self.vpos = np.ascontiguousarray(vpos, F)
        self.vnrm = np.ascontiguousarray(vnrm, F)

    def neighbours(self, qpos, qnrm, radius):
        """For every query, (volumes, distances) of all of S, sorted."""
        qpos = np.ascontiguousarray(qpos, F).reshape(-1, 3)
        qnrm = np.ascontiguousarray(qnrm, F).reshape(-1, 3)
        out = [None] * len(qpos)
        # queries of one normal at a time (float ==: -0 equals +0, a NaN equals nothing)
        keys = np.unique(qnrm + F(0), axis=0) if len(qnrm) else np.zeros((0, 3), F)
        done = np.zeros(len(qpos), bool)
        for key in keys:
            if np.isnan(key).any():
                continue
            qs = np.nonzero((qnrm == key).all(axis=1))[0]
            vs = np.nonzero((self.vnrm == key).all(axis=1))[0]
            for lo in range(0, len(qs), 256):
                qi = qs[lo:lo + 256]
                d = len3(*[self.vpos[vs, c][None, :] - qpos[qi, c][:, None] for c in range(3)])
                inside = d < F(radius)
                for r, q in enumerate(qi):
                    v = vs[inside[r]]
                    dd = d[r][inside[r]]
                    order = np.lexsort((v, dd))
                    out[q] = (v[order].astype(np.int32), dd[order])
                    done[q] = True
        for q in np.nonzero(~done)[0]:
            out[q] = (np.zeros(0, np.int32), np.zeros(0, F))
        return out

    @staticmethod
    def top(nb, k):
        """rt_sarsa_knn's outputs for k from neighbours(): vol, dist (n, k), count (n)."""
        n = len(nb)
        vol = np.full((n, k), -1, np.int32)
        dist = np.full((n, k), INF, F)
        cnt = np.zeros(n, np.int32)
        for i, (v, d) in enumerate(nb):
            c = min(k, len(v))
            vol[i, :c], dist[i, :c], cnt[i] = v[:c], d[:c], c
        return vol, dist, cnt


def strided(n, count):
    return np.unique(np.linspace(0, n - 1, min(count, n)).astype(np.int64))


def tie_queries(brute, idx, reach):
    """Float midpoints M of a volume A (of idx) and one of its first four neighbours B, with
    len3(A - M) == len3(B - M) and nothing nearer to M: (M, normal, lower index of the pair)."""
    nb = brute.neighbours(brute.vpos[idx], brute.vnrm[idx], reach)
    mids, nrms, pairs = [], [], []
    for a, (v, _) in zip(idx, nb):
        for b in v[v != a][:4]:
            mids.append((brute.vpos[a] + brute.vpos[b]) * F(0.5))
            nrms.append(brute.vnrm[a])
            pairs.append((min(a, b), max(a, b)))
    mids, nrms = np.array(mids, F).reshape(-1, 3), np.array(nrms, F).reshape(-1, 3)
    keep, seen = [], set()
    for i, (v, d) in enumerate(brute.neighbours(mids, nrms, reach)):
        lo, hi = pairs[i]
        if len(v) >= 2 and d[0] == d[1] and v[0] == lo and v[1] == hi and (lo, hi) not in seen:
            seen.add((lo, hi))
            keep.append(i)
    keep = np.array(keep, np.int64)
    return mids[keep], nrms[keep], np.array([pairs[i][0] for i in keep], np.int32)


def class_normals(vnrm):
    return np.unique(vnrm + F(0), axis=0)


def synthetic_queries(brute):
    """Each class's normal at a volume of the class moved 1.0 along it (nothing in range), a
    normal of no class at a volume's position, a NaN and an infinite position."""
    cls = class_normals(brute.vnrm)
    first = np.array([np.nonzero((brute.vnrm == c).all(axis=1))[0][0] for c in cls])
    far = (brute.vpos[first] + F(1.0) * cls).astype(F)
    odd = np.array([[0.6, 0.0, 0.8]], F)
    assert not (cls == odd).all(axis=1).any()
    pos = np.concatenate([far, brute.vpos[:1], np.array([[np.nan, 0.1, 0.2], [0.1, np.inf, 0.2]], F)])
    nrm = np.concatenate([cls, odd, brute.vnrm[:2]])
    return pos, nrm


def capped_counts(*neighbour_lists):
    return sorted({min(len(v), 8) for nb in neighbour_lists for v, _ in nb})


# ---------------------------------------------------------------- CPU ----------

def test_constants_and_exports(rtmi_mod):
    assert header_define("RT_SARSA_KNN_MAX") == 8 == rtmi_mod.RT_SARSA_KNN_MAX
    assert header_define("RT_IRR_MEAN") == 0 == rtmi_mod.RT_IRR_MEAN
    assert header_define("RT_IRR_CONE") == 1 == rtmi_mod.RT_IRR_CONE
    L = rtmi_mod.lib()
    for s in ("rt_sarsa_knn_reach", "rt_sarsa_knn", "rt_render_irradiance", "rt_render_irradiance_tiles_device"):
        assert s in rtmi_mod._lib.EXPORTS and hasattr(L, s)
    assert ctypes.sizeof(rtmi_mod.RtIrrOpts) == 16


def test_refusals_by_value_need_no_gpu(rtmi_mod):
    L = rtmi_mod.lib()
    buf = np.zeros(8, F)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = np.zeros(8, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bad = [(0, 0.05), (9, 0.05), (-1, 0.05), (3, 0.0), (3, -0.01), (3, float("nan"))]
    for k, radius in bad:
        assert L.rt_sarsa_knn(None, None, fp, fp, 1, k, radius, ip, fp, ip) == -1, (k, radius)
        msg = L.rt_last_error()
        assert (b"k = " in msg) if not 1 <= k <= 8 else (b"radius" in msg), msg
        o = rtmi_mod.RtIrrOpts(k, radius, 0, 1)
        assert L.rt_render_irradiance(None, None, None, None, None, ctypes.byref(o), 0, fp, None, None, None,
                                      None) == -1
        assert L.rt_last_error() == msg
        assert L.rt_render_irradiance_tiles_device(None, None, None, None, None, ctypes.byref(o), 0, ip, 1, 16, fp,
                                                   None) == -1
        assert L.rt_last_error() == msg
    o = rtmi_mod.RtIrrOpts(3, 0.05, 7, 1)
    assert L.rt_render_irradiance(None, None, None, None, None, ctypes.byref(o), 0, fp, None, None, None, None) == -1
    assert b"weight" in L.rt_last_error()
    # good values, NULL handles / outputs / opts
    assert L.rt_sarsa_knn(None, None, fp, fp, 1, 3, 0.05, ip, fp, ip) == -1
    assert b"NULL" in L.rt_last_error()
    assert L.rt_sarsa_knn(None, None, fp, fp, -1, 3, 0.05, ip, fp, ip) == -1
    o = rtmi_mod.RtIrrOpts(3, 0.05, 0, 1)
    assert L.rt_render_irradiance(None, None, None, None, None, ctypes.byref(o), 0, fp, None, None, None, None) == -1
    assert b"NULL" in L.rt_last_error()
    assert L.rt_render_irradiance(None, None, None, None, None, None, 0, fp, None, None, None, None) == -1
    assert L.rt_sarsa_knn_reach(None, fp) == -1
    # rt_sarsa_set_td_mode refuses its mode the same way
    assert L.rt_sarsa_set_td_mode(None, 3) == -1 and b"TD mode" in L.rt_last_error()
    assert L.rt_sarsa_set_td_mode(None, 0) == -1 and b"NULL" in L.rt_last_error()


@pytest.fixture(scope="module")
def oracle_maps(oracle_mod):
    made = {}

    def get(area):
        if area not in made:
            om = oracle_mod.Sarsa(oracle_mod.cornell(1), SEED, area)
            pos, nrm, _, _ = om.volumes()
            made[area] = Brute(pos, nrm)
        return made[area]

    return get


@pytest.mark.parametrize("area,volumes", zip(AREAS, (24526, 6114, 2438)))
def test_brute_force_conditions_on_the_oracle_map(oracle_maps, area, volumes):
    """The restatement against itself, and the conditions the GPU test relies on: map sizes,
    tie queries, and the counts the query set covers."""
    b = oracle_maps(area)
    reach = reach_of()
    assert abs(float(reach) - 0.0547) < 1e-4
    assert len(b.vpos) == volumes and len(class_normals(b.vnrm)) == 14
    idx = strided(len(b.vpos), N_VOLUME_QUERIES)
    nb = b.neighbours(b.vpos[idx], b.vnrm[idx], reach)
    half = b.neighbours(b.vpos[idx], b.vnrm[idx], reach / F(2))
    for q, (v, d) in zip(idx, nb):
        assert v[0] == q and d[0] == 0 and np.all(np.diff(d) >= 0) and np.all(d < reach)
        assert np.all((b.vnrm[v] == b.vnrm[q]).all(axis=1)) and len(set(v.tolist())) == len(v)
        # ascending by (d, v): equal distances by index
        same = np.diff(d) == 0
        assert np.all(np.diff(v)[same] > 0)
    # a smaller radius or k gives a prefix
    for (v, d), (hv, hd) in zip(nb, half):
        n = int(np.count_nonzero(d < reach / F(2)))
        assert np.array_equal(hv, v[:n]) and np.array_equal(hd, d[:n])
    v8, d8, c8 = Brute.top(nb, 8)
    v3, d3, c3 = Brute.top(nb, 3)
    assert np.array_equal(v3, v8[:, :3]) and np.array_equal(c3, np.minimum(c8, 3))
    assert np.all(v8[np.arange(8)[None, :] >= c8[:, None]] == -1) and np.all(np.isinf(d8[v8 < 0]))
    # the tie queries
    mids, nrms, lower = tie_queries(b, idx, reach)
    assert len(mids) >= MIN_TIES
    tv, td, _ = Brute.top(b.neighbours(mids, nrms, reach), 1)
    assert np.array_equal(tv[:, 0], lower)
    # the synthetic queries find nothing
    spos, snrm = synthetic_queries(b)
    assert all(len(v) == 0 for v, _ in b.neighbours(spos, snrm, reach))
    counts = capped_counts(nb, half, b.neighbours(mids, nrms, reach), b.neighbours(spos, snrm, reach))
    assert set(CLAIMED_COUNTS[area]) <= set(counts), counts


# ---------------------------------------------------------------- GPU ----------

def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def gpu_params(rtmi_mod, width, height, hit_rule=1, spp=1, split=1, **kw):
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=width, height=height, spp=spp, spp_split=split,
                                   hit_rule=hit_rule, **kw)


class World:
    """One scene's device scene and map at one density, its volumes and normals, shared by the tests."""

    def __init__(self, rtmi_mod, oracle_mod, ctx, scene, area):
        self.rtmi, self.ctx, self.scene, self.area = rtmi_mod, ctx, scene, area
        self.g = geometry(rtmi_mod, scene)
        self.sc = rtmi_mod.Scene(ctx, self.g)
        self.rm = rtmi_mod.sarsa.RadianceMap(ctx, self.sc, SEED, area)
        pos, nrm, surf, _ = self.rm.volumes()
        self.brute = Brute(pos, nrm)
        self.surf = surf
        self.normals = oracle_mod.normals(self.g.all_triangles())
        self.reach = F(self.rm.knn_reach())
        self.trained = False

    def train(self, cam):
        """one learning frame, then a small bake: the estimates then differ from volume to volume"""
        if not self.trained:
            self.rm.render(cam, gpu_params(self.rtmi, 50, 39, spp=2), 1)
            self.rm.bake(self.sc, self.rtmi.default_params(self.rtmi.RT_PRESET_GPU, spp=4, spp_split=4, t_scale=39.0))
            self.trained = True

    def close(self):
        self.rm.close()
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(rtmi_mod, oracle_mod, gpu_ctx):
    made = {}

    def get(scene, area):
        if (scene, area) not in made:
            made[(scene, area)] = World(rtmi_mod, oracle_mod, gpu_ctx, scene, area)
        return made[(scene, area)]

    yield get
    for w in made.values():
        w.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SEARCH_WORLDS = [("cornell", 0.001), ("cornell", 0.004), ("cornell", 0.01), ("door_room", 0.004)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,area", SEARCH_WORLDS, ids=[f"{s}-{a}" for s, a in SEARCH_WORLDS])
def test_gpu_knn_equals_brute_force(rtmi_mod, worlds, scene, area):
    w = worlds(scene, area)
    b, rm, reach = w.brute, w.rm, w.reach
    assert bits(reach) == bits(reach_of()) and reach > 0
    idx = strided(len(b.vpos), N_VOLUME_QUERIES)
    assert len(idx) == N_VOLUME_QUERIES
    mids, mnrm, lower = tie_queries(b, idx, reach)
    assert len(mids) >= MIN_TIES
    # 2,000 camera hit points of the view (64 x 48: 3,072 pixels)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS[scene])
    _, tri, _, hpos = rm.view(cam, gpu_params(rtmi_mod, 64, 48), 0, aov=True)
    surf = (tri >= 0) & (tri < w.g.n_surf)
    hp, hn = hpos[surf][:2000], w.normals[tri[surf]][:2000]
    assert len(hp) == 2000
    spos, snrm = synthetic_queries(b)
    qpos = np.concatenate([b.vpos[idx], mids, hp, spos]).astype(F)
    qnrm = np.concatenate([b.vnrm[idx], mnrm, hn, snrm]).astype(F)
    n_syn, t0 = len(spos), len(idx)
    seen = set()
    for radius in (reach, reach / F(2)):
        nb = b.neighbours(qpos, qnrm, radius)
        seen |= set(capped_counts(nb))
        assert all(len(v) == 0 for v, _ in nb[-n_syn:])
        for k in KS:
            want = Brute.top(nb, k)
            got = rm.knn(qpos, qnrm, k, float(radius))
            print(f"{scene} {area} radius {float(radius):.5f} k {k}: {len(qpos)} queries, "
                  f"{int(np.count_nonzero(got[0] != want[0]))} volume, "
                  f"{int(np.count_nonzero(bits(got[1]) != bits(want[1])))} distance, "
                  f"{int(np.count_nonzero(got[2] != want[2]))} count mismatches")
            assert np.array_equal(got[0], want[0])
            assert np.array_equal(bits(got[1]), bits(want[1]))
            assert np.array_equal(got[2], want[2])
            if k == 1 and radius == reach:  # a tie goes to the lower index
                assert np.array_equal(got[0][t0:t0 + len(mids), 0], lower)
            if radius == reach and k == 3:
                # a query's result depends on neither n nor its place: n = 1, n = 257 (a partly
                # filled wave), the list reversed; n = 0 writes nothing
                for sel in (slice(7, 8), slice(100, 357), slice(None, None, -1)):
                    sub = rm.knn(qpos[sel], qnrm[sel], k, float(radius))
                    assert all(np.array_equal(bits(x), bits(y[sel])) for x, y in zip(sub, got))
                assert len(qpos[100:357]) == 257
                empty = rm.knn(qpos[:0], qnrm[:0], k, float(radius))
                assert empty[0].shape == (0, 3) and empty[2].shape == (0,)
    assert set(CLAIMED_COUNTS.get(area, ())) <= seen, sorted(seen)
    # radius None is the reach; the reach itself is accepted, the next float above it is not
    for x, y in zip(rm.knn(qpos[:50], qnrm[:50], 8), rm.knn(qpos[:50], qnrm[:50], 8, float(reach))):
        assert np.array_equal(bits(x), bits(y))
    with pytest.raises(rtmi_mod.RtError) as e:
        rm.knn(qpos[:4], qnrm[:4], 3, float(np.nextafter(reach, INF)))
    assert e.value.code == rtmi_mod._lib.RT_E_INVALID
    # NULL distances and counts are allowed; NULL volumes are not
    L = rtmi_mod.lib()
    vol = np.zeros((4, 3), np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    q4, n4 = np.ascontiguousarray(qpos[:4]), np.ascontiguousarray(qnrm[:4])
    args = (w.ctx.handle, rm.handle, q4.ctypes.data_as(fp), n4.ctypes.data_as(fp), 4, 3, float(reach))
    assert L.rt_sarsa_knn(*args, vol.ctypes.data_as(ip), None, None) == 0
    assert np.array_equal(vol, rm.knn(q4, n4, 3)[0])
    assert L.rt_sarsa_knn(*args, None, None, None) == -1
    # the search does not depend on the map's search mode, and moves none of its counters
    st = rm.search_stats()
    rm.set_search(rtmi_mod.sarsa.SEARCH_KD)
    kd = rm.knn(qpos[:300], qnrm[:300], 8)
    rm.set_search(rtmi_mod.sarsa.SEARCH_GRID)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(kd, rm.knn(qpos[:300], qnrm[:300], 8)))
    assert rm.search_stats() == st


# (id, scene, width, height, camera yaws, hit rule)
CASES = [
    ("door_room-50x39", "door_room", 50, 39, {}, 1),                  # lights in frame; the rectangle cull
    ("cornell-pitched", "cornell", 50, 39, {"yaw_x": 0.2}, 1),      # misses in frame; pitched: no cull
    ("door_room-pitched", "door_room", 50, 39, {"yaw_x": 0.3}, 1),  # lights, no cull
    ("cornell-rule0", "cornell", 17, 5, {}, 0),
    ("door_room-17x5", "door_room", 17, 5, {}, 1),
    ("door_room-1x1", "door_room", 1, 1, {}, 1),
]
CASE_IDS = [c[0] for c in CASES]
RENDER_AREA = 0.004
ENV = 0.25


def irr_scale():
    """rt_sarsa_search.hpp's kIrrScale: (2.f * pi_f) / 144.f"""
    return (F(2) * F(math.pi)) / F(144)


def lum_of(albedo):
    """tri_lum: 0.5f * (max + min)"""
    a = np.ascontiguousarray(albedo, F)
    return F(0.5) * (a.max(axis=1) + a.min(axis=1))


def restate(w, accum, tri, vol, dist, radius, weight, tint, env):
    """Steps 3-6 of rt_render_irradiance in numpy float32, from the AOVs of the sample."""
    g = w.g
    H, W, k = vol.shape
    e = accum[np.maximum(vol, 0)] * irr_scale()
    found = vol >= 0
    count = found.sum(axis=2)
    assert np.array_equal(found, np.arange(k)[None, None, :] < count[:, :, None])  # filled from the front
    wt = F(1) - dist / F(radius)
    we = wt * e
    zero = np.zeros((H, W), F)
    s, ws, wtot = zero.copy(), zero.copy(), zero.copy()
    for u in range(k):
        f = found[:, :, u]
        first = f & (u == 0)
        s = np.where(first, e[:, :, u], np.where(f, s + e[:, :, u], s))
        ws = np.where(first, we[:, :, u], np.where(f, ws + we[:, :, u], ws))
        wtot = np.where(first, wt[:, :, u], np.where(f, wtot + wt[:, :, u], wtot))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / count.astype(F)
        Lv = np.where((weight == w.rtmi.RT_IRR_CONE) & (wtot != 0), ws / wtot, mean)
        Lv = np.where(count == 0, F(0), Lv).astype(F)
        surf = (tri >= 0) & (tri < g.n_surf)
        ts = np.where(surf, tri, 0)
        rgb = np.repeat(Lv[:, :, None], 3, axis=2)
        if tint:
            lum = lum_of(g.albedo)[ts]
            rgb = np.where((lum == 0)[:, :, None], F(0), g.albedo.astype(F)[ts] * (Lv / lum)[:, :, None])
    light = tri >= g.n_surf
    em = np.ascontiguousarray(g.emission, F)[np.where(light, tri - g.n_surf, 0)]
    rgb = np.where(surf[:, :, None], rgb, np.where(light[:, :, None], em, F(env)))
    assert rgb.dtype == F
    return rgb, count


def fold(samples, split):
    """each chunk's samples added in order, the chunk sums added in order, / spp"""
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
    assert tot.dtype == F
    return tot / F(spp)


def case_setup(rtmi_mod, worlds, case):
    _, scene, W, H, yaws, rule = case
    w = worlds(scene, RENDER_AREA)
    w.train(rtmi_mod.camera(rtmi_mod.CAMERAS[scene]))
    return w, rtmi_mod.camera(rtmi_mod.CAMERAS[scene], **yaws), gpu_params(rtmi_mod, W, H, rule, env_light=ENV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_irradiance_equals_restatement(rtmi_mod, worlds, case):
    w, cam, p = case_setup(rtmi_mod, worlds, case)
    R = rtmi_mod
    rm = w.rm
    _, vtri, _, vpos = rm.view(cam, p, 0, aov=True)
    accum = rm.read()[3]
    assert len(np.unique(accum)) > len(accum) // 2  # the estimates differ from volume to volume
    surf = (vtri >= 0) & (vtri < w.g.n_surf)
    kinds = set()
    for k in KS:
        for radius in (w.reach, w.reach / F(2)):
            want_knn = rm.knn(vpos[surf], w.normals[vtri[surf]], k, float(radius))
            for weight in (R.RT_IRR_MEAN, R.RT_IRR_CONE):
                for tint in (True, False):
                    rgb, tri, pos, vol, dist = rm.irradiance_view(cam, p, k, float(radius), weight, tint, 0, aov=True)
                    assert np.array_equal(tri, vtri) and np.array_equal(bits(pos), bits(vpos))
                    assert np.array_equal(vol[surf], want_knn[0]) and np.array_equal(bits(dist[surf]), bits(want_knn[1]))
                    assert np.all(vol[~surf] == -1) and np.all(np.isposinf(dist[~surf]))
                    want, count = restate(w, accum, tri, vol, dist, radius, weight, tint, ENV)
                    assert np.array_equal(count[surf], want_knn[2])
                    bad = int(np.count_nonzero(bits(rgb) != bits(want)))
                    print(f"{case[0]} k {k} radius {float(radius):.5f} weight {weight} tint {tint}: "
                          f"{bad} of {rgb.size} values differ; counts {np.bincount(count[surf], minlength=k + 1)}")
                    assert np.array_equal(bits(rgb), bits(want))
                    assert np.array_equal(rgb, rm.irradiance_view(cam, p, k, float(radius), weight, tint))  # no AOVs
                    kinds |= {"light"} if (tri >= w.g.n_surf).any() else set()
                    kinds |= {"miss"} if (tri < 0).any() else set()
                    kinds |= {"none"} if (count[surf] == 0).any() else set()
                    kinds |= {"full"} if (count[surf] == k).any() else set()
    if case[0] == "door_room-50x39":
        assert {"light", "full"} <= kinds
    if case[0] == "cornell-pitched":
        assert {"miss", "full"} <= kinds
    # the defaults: k = 3, the reach, the mean, tinted, sample 0
    assert np.array_equal(rm.irradiance_view(cam, p), rm.irradiance_view(cam, p, 3, float(w.reach), R.RT_IRR_MEAN, True, 0))
    # max_bounces and sampler are ignored
    q = gpu_params(rtmi_mod, p.width, p.height, p.hit_rule, env_light=ENV, max_bounces=0, sampler=R.RT_SAMPLER_COSINE)
    assert np.array_equal(rm.irradiance_view(cam, p), rm.irradiance_view(cam, q))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_irradiance_fold_and_map_untouched(rtmi_mod, worlds, case):
    w, cam, p = case_setup(rtmi_mod, worlds, case)
    S, R, rm = rtmi_mod.sarsa, rtmi_mod, w.rm
    _, scene, W, H, _, rule = case
    before, frames, st = rm.read(), rm.frames, rm.search_stats()
    opts = dict(k=8, radius=None, weight=R.RT_IRR_CONE, tint=True)
    singles = [rm.irradiance_view(cam, p, first_sample=s, **opts) for s in range(4)]
    if W * H > 1:
        assert not np.array_equal(singles[0], singles[1])  # each sample re-jitters
    p4 = gpu_params(rtmi_mod, W, H, rule, spp=4, split=2, env_light=ENV)
    got = rm.irradiance_view(cam, p4, **opts)
    assert np.array_equal(bits(got), bits(fold(singles, 2)))
    # the AOVs of a multi-sample frame describe its first sample
    a4 = rm.irradiance_view(cam, p4, first_sample=1, aov=True, **opts)
    a1 = rm.irradiance_view(cam, p, first_sample=1, aov=True, **opts)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a4[1:], a1[1:]))
    for mode in (S.TD_INFRAME, S.TD_OFF, S.TD_FRAME):  # read only in every TD mode
        rm.set_td_mode(mode)
        assert np.array_equal(got, rm.irradiance_view(cam, p4, **opts))
        assert all(np.array_equal(x, y) for x, y in zip(rm.read(), before))
        assert rm.frames == frames and rm.search_stats() == st
    for badp in (dict(spp=0), dict(spp=6, split=4), dict(width=0)):
        kw = dict(width=8, height=8, hit_rule=1)
        kw.update(badp)
        with pytest.raises(R.RtError) as e:
            rm.irradiance_view(cam, gpu_params(rtmi_mod, kw.pop("width"), kw.pop("height"), kw.pop("hit_rule"), **kw))
        assert e.value.code == R._lib.RT_E_INVALID
    with pytest.raises(R.RtError) as e:
        rm.irradiance_view(cam, p, radius=float(np.nextafter(w.reach, INF)))
    assert e.value.code == R._lib.RT_E_INVALID


@pytest.mark.gpu
def test_gpu_irradiance_tiles_equal_full_render(rtmi_mod, worlds):
    import torch
    case = ("door_room-80x72", "door_room", 80, 72, {}, 1)
    w, cam, _ = case_setup(rtmi_mod, worlds, case)
    W, H, T = 80, 72, 32
    p = gpu_params(rtmi_mod, W, H, 1, spp=4, split=2, env_light=ENV)
    opts = dict(k=3, radius=None, weight=rtmi_mod.RT_IRR_MEAN, tint=True, first_sample=5)
    full = w.rm.irradiance_view(cam, p, **opts)
    origins = rtmi_mod.tiles.tile_origins(W, H, T)
    assert len(origins) == 9
    pick = origins[[8, 2, 4, 0, 7, 5]]  # scattered: corner, right-edge and bottom-edge tiles among them
    fill = -7.0
    out = torch.full((len(pick), T, T, 3), fill, dtype=torch.float32, device=torch.device("cuda", 0))
    w.rm.irradiance_view_tiles_device(cam, p, pick, T, out.data_ptr(), 0, **opts)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, (x, y) in enumerate(pick):
        vw, vh = min(T, W - x), min(T, H - y)
        assert np.array_equal(bits(got[i, :vh, :vw]), bits(full[y:y + vh, x:x + vw])), (x, y)
        assert np.all(got[i, vh:] == fill) and np.all(got[i, :, vw:] == fill), (x, y)  # the overhang is not written
    w.rm.irradiance_view_tiles_device(cam, p, pick[:0], T, 0, 0, **opts)  # an empty tile list is a no-op


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ("cornell", "door_room"))
def test_gpu_equal_values_interpolate_to_themselves(rtmi_mod, gpu_ctx, worlds, scene):
    """On a map whose every volume holds the same Q the neighbours of a point hold equal estimates
    (same normal, hence the same sector cosines): the k = 8 cone image is the k = 1 image to 1e-6
    relative wherever a volume is in range, and tinted it is albedo * const per surface."""
    w = worlds(scene, RENDER_AREA)
    R = rtmi_mod
    cam = R.camera(R.CAMERAS[scene])
    p = gpu_params(rtmi_mod, 50, 39, env_light=ENV)
    with R.sarsa.RadianceMap(gpu_ctx, w.sc, SEED, RENDER_AREA) as rm:
        rm.write(np.full((rm.n_volumes, 144), 0.37, F))
        one, tri, _, vol1, _ = rm.irradiance_view(cam, p, 1, None, R.RT_IRR_MEAN, False, aov=True)
        cone = rm.irradiance_view(cam, p, 8, None, R.RT_IRR_CONE, False)
        tinted = rm.irradiance_view(cam, p, 8, None, R.RT_IRR_CONE, True)
    surf = (tri >= 0) & (tri < w.g.n_surf)
    have = surf & (vol1[:, :, 0] >= 0)
    assert have.sum() > 1000 and np.all(one[have] > 0)
    assert np.array_equal(cone[~have], one[~have])
    rel = np.abs(cone[have].astype(np.float64) - one[have]) / one[have]
    print(f"{scene}: largest relative difference of the k = 8 cone image to the k = 1 image {rel.max():.3g}")
    assert rel.max() <= 1e-6
    alb, lum = w.g.albedo.astype(F), lum_of(w.g.albedo)
    want = np.where((lum[tri[have]] == 0)[:, None], F(0), alb[tri[have]] * (cone[have][:, :1] / lum[tri[have]][:, None]))
    assert np.array_equal(bits(tinted[have]), bits(want.astype(F)))
    # albedo * const per surface.  The volumes of one surface hold the same estimate up to the
    # rounding of their own cosine tables (grid_direction adds and subtracts the volume's position:
    # a few 2^-23 relative per cosine, averaged over 144 sectors), and the interpolation adds at most
    # 8 roundings: const is the same within 16 * 2^-23 = 2e-6 relative.
    for t in np.unique(tri[have]):
        px = tinted[have & (tri == t)].astype(np.float64)
        ch = alb[t] > 0
        c = px[:, ch] / alb[t][ch]
        assert np.all(np.abs(c - c.mean()) <= 2e-6 * c.mean()), t


@pytest.mark.gpu
def test_gpu_facade_irradiance_demo_equals_abi(rtmi_mod, gpu_ctx, tmp_path):
    """examples/reinforcement_main.cpp's irradiance mode (host/precompute_irradiance_path_tracing.h:
    precompute_radiance_volumes, then draw_radiance_map_path_tracing per frame) on a 24 x 20 screen
    saves the C ABI's frame of the same bake, packed by rt_pack_argb."""
    exe = os.path.join(PKG, "build", "reinforcement_demo")
    assert os.path.exists(exe), f"{exe} missing: make -C {PKG}"
    obj = os.path.join(MODELS, "door_room.obj")
    out = str(tmp_path / "irradiance.bmp")
    r = subprocess.run([exe, "irradiance", obj, "1", "2", "4", out, "24", "20", "3"], capture_output=True, text=True,
                       timeout=240, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("irradiance view, 3 closest volumes") == 2 and "precomputed 4 paths per sector" in r.stdout
    raw = open(out, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 4 * 24 * 20
    got = np.frombuffer(raw[54:], dtype="<u4").reshape(20, 24)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=24, height=20, spp=1)
    pb = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, spp=4, spp_split=4, t_scale=20.0)
    with rtmi_mod.Scene(gpu_ctx, rtmi_mod.obj_geometry(obj, "door_room")) as sc, \
            rtmi_mod.sarsa.RadianceMap(gpu_ctx, sc, SEED) as rm:
        rm.bake(sc, pb)
        img = rm.irradiance_view(rtmi_mod.camera(rtmi_mod.CAMERAS["door_room"]), p, 3, None, rtmi_mod.RT_IRR_MEAN, True,
                                 first_sample=1)
    assert np.array_equal(got, rtmi_mod.pack_argb(img))
    assert len(np.unique(got)) > 20
