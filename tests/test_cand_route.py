"""The candidate route of the render kernels, ray by ray (rt_intersect_cand): the device lookup
into the bounce-ray candidate table (rt_trace.hpp ctab_candidates) and the exact phase the wave
shares (closest_hit_cand: mf_exact_wave under rule 0, cand_exact_min under rule 1).

CPU: the restatement's masked scan (orc_intersect_masked) gives the scan's hit for any superset
of a ray's pass set -- the premise of the route -- and the ray sets below hold what they are
meant to (ties, t = +-0, few rays on a bin edge by accident).

GPU A: the device lookup on rays chosen against it (bin corners and edges of both cube-map
grids, face ties, origins on the surface's vertices, rays nearly in a plane, rays outside the
table's domain): sound at every t_scale the route serves, equal to the host lookup bit for bit
away from bin edges, and the route's (t, hit) the full scan's.
GPU B: the shared exact phase on masks chosen against it, one pattern per wave: against the
masked scan bit for bit.  Each wave's LDS block is exactly the render kernels' and the four are
adjacent, so a write past a block shows as a wrong hit in the next wave.
"""
import os

import numpy as np
import pytest

from conftest import MODELS
from ray_sets import _frame, bounce_rays
from test_mf_filter import edge_rays, surface_rays

T_SCALES = {0: (256.0, 512.0, 16384.0), 1: (1.0, 512.0, 16384.0)}  # what the table route serves
# candidates a lane tests itself before the shared phase (rt_trace.hpp RT_CTAB_OWN under rule 0,
# RT_CAND_OWN_MIN under rule 1's minimum fold)
OWN = {0: 3, 1: 0}
CAP_TABLE, CAP_SHARED = 96, 256  # RT_CAND_CAP_TABLE, RT_CAND_CAP_SHARED


def _geom(rtmi, kind):
    if kind == "cornell":
        return rtmi.cornell_geometry(0)
    if kind == "box":
        return box_geometry(rtmi)
    return rtmi.obj_geometry(os.path.join(MODELS, f"{kind}.obj"), kind)


def box_geometry(rtmi):
    """A closed axis-aligned box [-1, 1]^3, each face 4 x 4 quads of two triangles (192
    surfaces: every triangle has coplanar neighbours, so rays along shared edges tie), and a
    two-triangle light under its ceiling: 194 triangles, four live mask words."""
    k = 4
    g = np.linspace(-1.0, 1.0, k + 1)
    tris = []
    for ax in range(3):
        for side in (-1.0, 1.0):
            for i in range(k):
                for j in range(k):
                    def p(a, b):
                        v = np.zeros(3)
                        v[ax], v[(ax + 1) % 3], v[(ax + 2) % 3] = side, a, b
                        return v
                    a, b, c, d = p(g[i], g[j]), p(g[i + 1], g[j]), p(g[i + 1], g[j + 1]), p(g[i], g[j + 1])
                    tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
    tri = np.asarray(tris, np.float32)
    q = [np.array(v) for v in ((-0.3, -0.9, -0.3), (0.3, -0.9, -0.3), (0.3, -0.9, 0.3), (-0.3, -0.9, 0.3))]
    light = np.asarray([np.concatenate([q[0], q[1], q[2]]), np.concatenate([q[0], q[2], q[3]])], np.float32)
    return rtmi.Geometry(tri, np.full((tri.shape[0], 3), 0.75, np.float32), light,
                         np.full((2, 3), 10.0, np.float32), np.zeros(2, np.int32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _full_mask(n_tri):
    w = (n_tri + 63) // 64
    m = np.full(w, 0xFFFFFFFFFFFFFFFF, np.uint64)
    if n_tri % 64:
        m[-1] = np.uint64((1 << (n_tri % 64)) - 1)
    return m


def _random_bits(rng, n, n_tri, density):
    """(n, words) masks, each triangle's bit set with probability `density`"""
    w = (n_tri + 63) // 64
    b = np.zeros((n, w * 64), np.uint8)
    b[:, :n_tri] = rng.random((n, n_tri)) < density
    return np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(n, w)


def _mask_of(rows, n_tri):
    """(n, words) masks from a boolean (n, n_tri) matrix"""
    w = (n_tri + 63) // 64
    b = np.zeros((rows.shape[0], w * 64), np.uint8)
    b[:, :n_tri] = rows
    return np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(rows.shape[0], w)


def _oracle_scan(oracle, geom, o, d, ts, rule, masks=None):
    a = (geom.all_triangles(), geom.n_surf, geom.n_light, geom.light_group, o, d)
    return oracle.intersect(*a, ts, rule) if masks is None else oracle.intersect_masked(*a, masks, ts, rule)


def hit_triangles(oracle, geom, o, d, ts, rule, masks=None):
    """index of the triangle the (masked) scan hits (-1: none): the hit code with every light
    its own group, so that the CPU rule's codes name the triangle too"""
    own = np.arange(geom.n_light, dtype=np.int32)
    a = (geom.all_triangles(), geom.n_surf, geom.n_light, own, o, d)
    _, h = oracle.intersect(*a, ts, rule) if masks is None else oracle.intersect_masked(*a, masks, ts, rule)
    idx = h & 0x3FFFFFFF
    return np.where(h == -1, -1, np.where((h >> 30) & 3 == 2, idx, geom.n_surf + idx)).astype(np.int64)


# ---------------------------------------------------------------- ray sets ----------

def bin_critical(d):
    """A direction is bin-critical if a cube-map coordinate lands within nb * 2^-22 of a bin
    edge of the 16- or the 256-grid: x = u1 * nb / 2 in float32 as the host lookup computes it
    (rt_ctab.cpp ctab_lookup), |x - rint(x)| <= nb * 2^-22 -- 4 ulp of u1 around the edge, where
    the kernel's v_rcp_f32 (1 ulp) may pick the neighbouring bin."""
    d = np.ascontiguousarray(d, np.float32)
    ax = np.abs(d)
    fx = (ax[:, 0] >= ax[:, 1]) & (ax[:, 0] >= ax[:, 2])
    fy = ~fx & (ax[:, 1] >= ax[:, 2])
    m = np.where(fx, 0, np.where(fy, 1, 2))
    i = np.arange(d.shape[0])
    out = np.zeros(d.shape[0], bool)
    with np.errstate(all="ignore"):
        r = np.float32(1.0) / np.abs(d[i, m])
        for c in (1, 2):
            u1 = d[i, (m + c) % 3] * r + np.float32(1.0)
            for nb in (16, 256):
                x = u1 * np.float32(0.5 * nb)
                out |= np.abs(x.astype(np.float64) - np.rint(x)) <= nb * 2.0 ** -22
    return out


def _leave(pos, sd):
    """o, d of the ray leaving pos along sd as the kernels form it (bounce_rays' last lines)"""
    sd = sd.astype(np.float32)
    o = (pos + np.float32(1e-5) * sd).astype(np.float32)
    ln = np.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2]).astype(np.float32)
    return o, (sd / ln[:, None]).astype(np.float32)


def _surfaces(tri, n_surf):
    v = tri[:n_surf].reshape(-1, 3, 3).astype(np.float64)
    N = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])  # bounce_rays' orientation
    area = 0.5 * np.linalg.norm(N, axis=1)
    return v, N / np.linalg.norm(N, axis=1, keepdims=True), area


def _points(rng, v, area, n):
    j = rng.choice(v.shape[0], n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    f = a + b > 1
    a[f], b[f] = 1 - a[f], 1 - b[f]
    return j, (v[j, 0] + a[:, None] * (v[j, 1] - v[j, 0]) + b[:, None] * (v[j, 2] - v[j, 0])).astype(np.float32)


def _hemisphere(rng, N):
    out = np.zeros_like(N)
    for i, nn in enumerate(N):
        T, B = _frame(nn)
        r1, r2 = rng.random(), rng.random()
        st = np.sqrt(max(0.0, 1 - r1 * r1))
        out[i] = st * np.cos(2 * np.pi * r2) * B + r1 * nn + st * np.sin(2 * np.pi * r2) * T
    return out


def boundary_dirs(rng, n_bin, n_tie):
    """Directions through the corners and edges of the 16- and 256-grid bins of every cube face
    (n_bin), and on face ties |dx| = |dy|, |dy| = |dz|, all three equal (n_tie)."""
    s = np.zeros((n_bin + n_tie, 3))
    for i in range(n_bin):
        m, sign, nb = rng.integers(0, 3), rng.choice((-1.0, 1.0)), (16, 256)[i % 2]
        u = -1.0 + 2.0 * rng.integers(0, nb + 1) / nb
        nb2 = (16, 256)[rng.integers(0, 2)]
        v = -1.0 + 2.0 * rng.integers(0, nb2 + 1) / nb2 if i % 4 < 2 else rng.uniform(-1, 1)  # corner / edge
        if rng.random() < 0.5:
            u, v = v, u
        s[i, m], s[i, (m + 1) % 3], s[i, (m + 2) % 3] = sign, u, v
    for i in range(n_bin, n_bin + n_tie):
        sg = rng.choice((-1.0, 1.0), 3)
        m, c = rng.integers(0, 3), rng.uniform(0, 1)
        if i % 3 == 2:
            s[i] = sg  # all three equal
        else:  # two equal largest (c < 1) or two equal, the third larger (1 / c)
            s[i, m], s[i, (m + 1) % 3], s[i, (m + 2) % 3] = sg[0], sg[1], sg[2] * (c if i % 2 else 1.0 / max(c, 0.05))
    return s / np.linalg.norm(s, axis=1, keepdims=True)


GROUPS = ("bounce", "boundary", "origin", "outside", "grazing")
_TABLE_RAYS = {}


def table_rays(rtmi, kind):
    """The rays of part A for a scene: dict of surf, o, d, group (index into GROUPS), kind.

    The mixed set, 8,000 rays:
      bounce    the four kinds of bounce_rays: 4,510 uniform over the hemisphere, 80 each aimed
                at a vertex, nearly in some triangle's plane, nearly in their own plane
      boundary  2,000 placed on bin edges: 1,500 through corners and edges of the bins of both
                grids, 500 face ties (a tie is the outer edge of a cube face)
      origin    1,200 from the surface's own vertices and edge midpoints
      outside   50 the table does not cover
    and the grazing set, the rest of the same bounce_rays draw's kinds 1-3 (8,000; 3,000 for
    complex_light_room).  The walls of these scenes are axis-aligned, so a direction nearly in a
    wall's plane has a component of nearly 0: it lies along the centre line of a cube face, an
    edge of both grids.  5 % (aimed at a vertex) to 17 % of those kinds are bin-critical, which
    is why the mixed set, whose critical share is capped, holds few of them and they come as a
    set of their own, under every assertion but the cap."""
    if kind in _TABLE_RAYS:
        return _TABLE_RAYS[kind]
    geom = _geom(rtmi, kind)
    tri, n_surf = np.ascontiguousarray(geom.all_triangles(), np.float32), geom.n_surf
    rng = np.random.default_rng(97)
    v, N, area = _surfaces(tri, n_surf)
    sb, ob, db, kb = bounce_rays(tri, n_surf, 19000, seed=11)
    pick = np.concatenate([np.nonzero(kb == 0)[0][:4510]] + [np.nonzero(kb == q)[0][:80] for q in (1, 2, 3)])
    assert pick.size == 4750
    rest = np.setdiff1d(np.nonzero(kb > 0)[0], pick)[:3000 if kind == "complex_light_room" else 8000]
    parts = [(sb[pick], ob[pick], db[pick], 0, kb[pick]), (sb[rest], ob[rest], db[rest], 4, kb[rest])]
    # boundary: from random surface points, turned into the surface's hemisphere (-d lies on
    # an edge or a tie as d does)
    j, pos = _points(rng, v, area, 2000)
    s = boundary_dirs(rng, 1500, 500)
    s[np.einsum("ij,ij->i", s, N[j]) < 0] *= -1.0
    parts.append((j, *_leave(pos, s), 1, np.zeros(2000, int)))
    # origins on the surface's own vertices and edge midpoints (float32), hemisphere directions
    j = rng.integers(0, n_surf, 1200)
    c = rng.integers(0, 6, 1200)
    t32 = tri[:n_surf].reshape(-1, 3, 3)
    a, b = t32[j, c % 3], t32[j, (c % 3 + 1) % 3]
    pos = np.where((c < 3)[:, None], a, ((a + b) * np.float32(0.5)).astype(np.float32))
    parts.append((j, *_leave(pos, _hemisphere(rng, N[j])), 2, c))
    # outside the table's domain: origin off the plane, surface index out of range (twice),
    # non-unit direction, non-finite origin
    j, pos = _points(rng, v, area, 50)
    o, d = _leave(pos, _hemisphere(rng, N[j]))
    q = np.arange(50) % 5
    o[q == 0] += (np.float32(1e-3) * N[j[q == 0]]).astype(np.float32)
    j = j.copy()
    j[q == 1], j[q == 2] = -1, n_surf
    d[q == 3] *= np.float32(1.01)
    o[q == 4, 0] = np.nan
    parts.append((j, o, d, 3, q))
    n = sum(p[0].shape[0] for p in parts)
    perm = rng.permutation(n)  # the groups share waves
    out = {"surf": np.concatenate([p[0] for p in parts]).astype(np.int32)[perm],
           "o": np.concatenate([p[1] for p in parts])[perm], "d": np.concatenate([p[2] for p in parts])[perm],
           "group": np.concatenate([np.full(p[0].shape[0], p[3]) for p in parts])[perm],
           "kind": np.concatenate([p[4] for p in parts])[perm], "geom": geom, "tri": tri}
    out["critical"] = bin_critical(out["d"])
    _TABLE_RAYS[kind] = out
    return out


_PHASE_RAYS = {}


def phase_rays(rtmi, kind, n=20000):
    """The rays of part B: surface rays and edge / vertex rays (test_mf_filter.py), origins
    exactly on vertices (t = +-0 under rule 1), a few non-finite rays; shuffled."""
    if kind in _PHASE_RAYS:
        return _PHASE_RAYS[kind]
    geom = _geom(rtmi, kind)
    tri = np.ascontiguousarray(geom.all_triangles(), np.float32)
    rng = np.random.default_rng(5)
    o1, d1 = surface_rays(tri, n * 2 // 5, seed=3)
    o2, d2 = edge_rays(tri, n * 2 // 5, seed=4)
    n3 = n - o1.shape[0] - o2.shape[0]
    allv = tri.reshape(-1, 3)
    o3 = allv[rng.integers(0, allv.shape[0], n3)].copy()
    tgt = allv[rng.integers(0, allv.shape[0], n3)] + rng.normal(size=(n3, 3)).astype(np.float32) * np.float32(0.05)
    d3 = tgt - o3
    d3[np.linalg.norm(d3, axis=1) < 1e-3] = (0.0, 0.0, 1.0)
    d3 = (d3 / np.linalg.norm(d3, axis=1, keepdims=True)).astype(np.float32)
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    perm = rng.permutation(n)
    o, d = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])
    o[5, 0], d[70, 1], o[130, 2], d[200, 0] = np.nan, np.nan, np.inf, -np.inf
    d[300] = 0.0
    _PHASE_RAYS[kind] = (geom, tri, o, d)
    return _PHASE_RAYS[kind]


# ---------------------------------------------------------------- CPU ----------

SCENES = ["cornell", "door_room", "archway", "complex_light_room"]


@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("rule", [0, 1])
def test_masked_scan_of_a_superset_of_the_passes_is_the_scan(rtmi_mod, oracle_mod, kind, rule):
    """The premise of the route: the masked scan with every triangle, with exactly the pass
    set, and with the pass set plus random bits gives the full scan's (t, hit) bit for bit."""
    geom, tri, o, d = phase_rays(rtmi_mod, kind)
    n, n_tri = o.shape[0], tri.shape[0]
    ts = 512.0
    t, h = _oracle_scan(oracle_mod, geom, o, d, ts, rule)
    P = oracle_mod.pass_masks(tri, o, d, ts, rule)
    rng = np.random.default_rng(23)
    for name, m in (("full", np.tile(_full_mask(n_tri), (n, 1))), ("passes", P),
                    ("passes + random", P | _random_bits(rng, n, n_tri, 0.3))):
        tm, hm = _oracle_scan(oracle_mod, geom, o, d, ts, rule, m)
        assert np.array_equal(hm, h), name
        assert np.array_equal(_bits(tm), _bits(t)), name
    # and it is a restriction: without the scan's hit the ray hits something else or nothing
    hit = hit_triangles(oracle_mod, geom, o, d, ts, rule)
    m = P.copy()
    r = np.nonzero(hit >= 0)[0]
    m[r, hit[r] // 64] &= ~(np.uint64(1) << (hit[r] % 64).astype(np.uint64))
    tm, hm = _oracle_scan(oracle_mod, geom, o, d, ts, rule, m)
    left = hit_triangles(oracle_mod, geom, o, d, ts, rule, m)
    assert r.size > n // 2 and np.all(left[r] != hit[r])
    inm = (m[r, np.maximum(left[r], 0) // 64] >> (np.maximum(left[r], 0) % 64).astype(np.uint64)) & np.uint64(1)
    assert np.all((left[r] < 0) | (inm == 1)), "a hit outside the mask"
    assert np.all((hm == -1) == np.isinf(tm))
    assert np.all(_oracle_scan(oracle_mod, geom, o, d, ts, rule, np.zeros_like(P))[1] == -1)


@pytest.mark.parametrize("kind", SCENES)
def test_phase_rays_hold_ties_and_zero_distances(rtmi_mod, oracle_mod, kind):
    """The rays of part B are not trivial: some have two passing triangles at the same t or
    within the CPU rule's 1e-5 of each other, and some pass at t = +-0 under the GPU rule
    (origins on vertices)."""
    geom, tri, o, d = phase_rays(rtmi_mod, kind)
    n, n_tri = o.shape[0], tri.shape[0]
    for rule in (0, 1):
        P = oracle_mod.pass_masks(tri, o, d, 512.0, rule)
        t = np.full((n, n_tri), np.inf, np.float32)  # each passing triangle's own t
        for k in range(n_tri):
            one = np.zeros_like(P)
            one[:, k // 64] = P[:, k // 64] & (np.uint64(1) << np.uint64(k % 64))
            t[:, k] = _oracle_scan(oracle_mod, geom, o, d, 512.0, rule, one)[0]
        two = np.sort(t, axis=1)[:, :2].astype(np.float64)
        with np.errstate(invalid="ignore"):
            gap = two[:, 1] - two[:, 0]
        equal, near = int(np.sum(gap == 0.0)), int(np.sum(gap <= 1e-5))
        zero = int(np.sum((t == 0.0).any(axis=1)))
        neg_zero = int(np.sum(((t == 0.0) & np.signbit(t)).any(axis=1)))
        print(f"{kind} rule {rule}: {equal} rays with two equal t, {near} within 1e-5, {zero} with t = 0 "
              f"({neg_zero} with -0)")
        # The floors are an order below what the set is built to hold: 8,000 of the 20,000 rays
        # are aimed at edges and vertices, which two or more triangles share (2,000 at vertices
        # exactly: >= 200 near ties, a tenth of those exact); 4,000 start on a vertex, where
        # that vertex's triangles pass at t = +-0 under rule 1 (>= 500; the sign is det_t's, so
        # a good part are -0: >= 20).  Rule 0 asks t > 1e-5: no zero distances there.
        assert equal >= 20 and near >= 200, (equal, near)
        if rule == 1:
            assert zero >= 500 and neg_zero >= 20, (zero, neg_zero)
        else:
            assert zero == 0


@pytest.mark.parametrize("kind", SCENES)
def test_few_mixed_rays_are_bin_critical(rtmi_mod, kind):
    """At most 1 % of the mixed set outside its deliberately placed boundary rays is
    bin-critical, so the bit-for-bit comparison of the device masks with the host's covers the
    rest; the boundary rays are critical by construction and the grazing set largely."""
    R = table_rays(rtmi_mod, kind)
    g, c = R["group"], R["critical"]
    mixed = (g != GROUPS.index("boundary")) & (g != GROUPS.index("grazing"))
    assert int(np.sum(g != GROUPS.index("grazing"))) == 8000 and int(mixed.sum()) == 6000
    for i, name in enumerate(GROUPS):
        print(f"{kind}: {name}: {int(c[g == i].sum())} of {int((g == i).sum())} bin-critical")
    assert c[mixed].mean() <= 0.01, c[mixed].mean()
    assert c[g == GROUPS.index("boundary")].mean() >= 0.9  # they are where they were placed
    # every kind of bounce ray is there, and the rays the table serves lie in its domain
    assert all(int(np.sum((g == 0) & (R["kind"] == q))) >= 80 for q in range(4))


# ---------------------------------------------------------------- GPU ----------

@pytest.fixture(scope="module")
def scenes(rtmi_mod, gpu_ctx):
    """one device scene per kind for the module (its tables are built once, on first use)"""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = rtmi_mod.Scene(gpu_ctx, _geom(rtmi_mod, kind))
        return cache[kind]
    yield get
    for sc in cache.values():
        sc.close()


_HOST_MASKS = {}


def host_masks(rtmi, kind, rule):
    if (kind, rule) not in _HOST_MASKS:
        R = table_rays(rtmi, kind)
        _HOST_MASKS[kind, rule] = rtmi.ctab_candidates(R["tri"], R["geom"].n_surf, R["surf"], R["o"], R["d"],
                                                       hit_rule=rule)[0]
    return _HOST_MASKS[kind, rule]


_TABLE_RUNS = {}


def table_run(rtmi, ctx, scenes, kind, rule):
    """the table route on the scene's rays at every t_scale it serves, once per (scene, rule):
    {t_scale: (t, hit)}, the device masks, and a second pair cap where the scene has one"""
    if (kind, rule) not in _TABLE_RUNS:
        R = table_rays(rtmi, kind)
        sc = scenes(kind)
        cap = CAP_TABLE if R["tri"].shape[0] <= 64 else CAP_SHARED
        runs, masks = {}, None
        for ts in T_SCALES[rule]:
            t, h, m = rtmi.intersect_cand(ctx, sc, R["o"], R["d"], ts, rule, surf=R["surf"], pair_cap=cap, guard=64)
            n = R["o"].shape[0]
            assert np.all(_bits(t[n:]) == 0xA5A5A5A5) and np.all(_bits(h[n:]) == 0xA5A5A5A5)
            assert np.all(m[n:] == np.uint64(0xA5A5A5A5A5A5A5A5))
            assert masks is None or np.array_equal(masks, m[:n]), "the lookup does not depend on t_scale"
            runs[ts], masks = (t[:n], h[:n]), m[:n]
        other = None
        if cap == CAP_TABLE:
            other = rtmi.intersect_cand(ctx, sc, R["o"], R["d"], 512.0, rule, surf=R["surf"], pair_cap=CAP_SHARED)
        assert sc.ctab_info(rule)["built"]
        _TABLE_RUNS[kind, rule] = (runs, masks, other)
    return _TABLE_RUNS[kind, rule]


# Cornell: the grazing fold, one word; door_room: the fold under the GPU rule; archway: two
# words, no fold; complex_light_room: three words
TABLE_CASES = [("cornell", 0), ("door_room", 1), ("archway", 1), ("complex_light_room", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rule", TABLE_CASES)
def test_gpu_device_lookup_keeps_every_pass(rtmi_mod, oracle_mod, gpu_ctx, scenes, kind, rule):
    """Soundness of the kernel's own lookup: at every t_scale the route serves, every triangle
    that passes the exact test for a ray is among the candidates the device gave it -- the
    bin-critical rays included (the build widens the bins to cover the lookup's rounding)."""
    R = table_rays(rtmi_mod, kind)
    _, dev, _ = table_run(rtmi_mod, gpu_ctx, scenes, kind, rule)
    for ts in T_SCALES[rule]:
        missed = oracle_mod.pass_masks(R["tri"], R["o"], R["d"], ts, rule) & ~dev
        bad = np.nonzero(missed.any(axis=1))[0]
        assert bad.size == 0, (f"t_scale {ts}: {bad.size} rays miss a passing triangle, e.g. ray {bad[0]} "
                               f"({GROUPS[R['group'][bad[0]]]}, surface {R['surf'][bad[0]]}) words "
                               f"{[hex(int(x)) for x in missed[bad[0]]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rule", TABLE_CASES)
def test_gpu_device_masks_are_the_host_lookup(rtmi_mod, gpu_ctx, scenes, kind, rule, record_property):
    """Away from bin edges the device lookup (v_rcp_f32, its own face selection and fold branch)
    gives the host lookup's mask bit for bit.  Bin-critical rays may take the neighbouring bin:
    how many differ is reported, not gated (soundness covers them)."""
    R = table_rays(rtmi_mod, kind)
    _, dev, _ = table_run(rtmi_mod, gpu_ctx, scenes, kind, rule)
    host = host_masks(rtmi_mod, kind, rule)
    differ = (dev != host).any(axis=1)
    crit = R["critical"]
    print(f"{kind} rule {rule}: {int((differ & crit).sum())} of {int(crit.sum())} bin-critical rays differ "
          f"from the host lookup ({R['o'].shape[0]} rays)")
    record_property("critical_rays", int(crit.sum()))
    record_property("critical_rays_that_differ", int((differ & crit).sum()))
    bad = np.nonzero(differ & ~crit)[0]
    assert bad.size == 0, (f"{bad.size} rays off the bin edges differ, e.g. ray {bad[0]} "
                           f"({GROUPS[R['group'][bad[0]]]}) d {R['d'][bad[0]]} device "
                           f"{[hex(int(x)) for x in dev[bad[0]]]} host {[hex(int(x)) for x in host[bad[0]]]}")
    # the masks cull (else equality and soundness say little)
    served = R["group"] == GROUPS.index("bounce")
    pc = np.unpackbits(dev[served].view(np.uint8), axis=1).sum(axis=1)
    assert pc.mean() < 0.3 * R["tri"].shape[0], pc.mean()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rule", TABLE_CASES)
def test_gpu_table_route_hits_are_the_scan(rtmi_mod, oracle_mod, gpu_ctx, scenes, kind, rule):
    R = table_rays(rtmi_mod, kind)
    runs, _, other = table_run(rtmi_mod, gpu_ctx, scenes, kind, rule)
    for ts, (t, h) in runs.items():
        tc, hc = _oracle_scan(oracle_mod, R["geom"], R["o"], R["d"], ts, rule)
        bad = np.nonzero((h != hc) | (_bits(t) != _bits(tc)))[0]
        assert bad.size == 0, f"t_scale {ts}: {bad.size} rays differ from the scan, first {bad[:5]}"
    if other is not None:  # the one-word scenes are served at both pair caps
        assert np.array_equal(other[1], runs[512.0][1]) and np.array_equal(_bits(other[0]), _bits(runs[512.0][0]))
        assert np.array_equal(other[2], table_run(rtmi_mod, gpu_ctx, scenes, kind, rule)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rule", TABLE_CASES)
def test_gpu_rays_outside_the_table_keep_every_triangle(rtmi_mod, gpu_ctx, scenes, kind, rule):
    R = table_rays(rtmi_mod, kind)
    _, dev, _ = table_run(rtmi_mod, gpu_ctx, scenes, kind, rule)
    out = R["group"] == GROUPS.index("outside")
    assert out.sum() == 50
    assert np.all(dev[out] == _full_mask(R["tri"].shape[0])[None, :])
    assert not np.all(dev[~out] == _full_mask(R["tri"].shape[0])[None, :], axis=1).all()


# ---- B: the shared exact phase on given masks

def _subset(rng, live, k):
    """k of the triangle indices `live` (all of them if there are fewer)"""
    return rng.choice(live, size=min(k, live.size), replace=False)


def wave_patterns(n_tri, rule, cap):
    """The mask patterns, one per wave of 64 consecutive rays, in the order the waves take them
    (a workgroup's four waves get four different ones).  Each: (name, f(rng, P, hit) -> bool
    (64, n_tri)) with P the lanes' pass sets (bool) and hit their scan hits."""
    words = (n_tri + 63) // 64
    word = [np.arange(64 * w, min(64 * w + 64, n_tri)) for w in range(words)]
    everything = np.arange(n_tri)

    def full(rng, P, hit):
        return np.ones((64, n_tri), bool)

    def empty(rng, P, hit):
        return np.zeros((64, n_tri), bool)

    def heavy(lane):
        def f(rng, P, hit):
            m = np.zeros((64, n_tri), bool)
            m[lane] = True
            return m
        return f

    def staircase(rng, P, hit):  # lane i holds i candidates
        m = np.zeros((64, n_tri), bool)
        for i in range(64):
            m[i, _subset(rng, everything, i)] = True
        return m

    def staircase_word0(rng, P, hit):  # lane i holds the first i + 1 of word 0: lane 63 all 64
        m = np.zeros((64, n_tri), bool)
        for i in range(64):
            m[i, :min(i + 1, word[0].size)] = True
        return m

    def total(T, w):
        """the wave's pair total of word w after the own-lane tests is exactly T"""
        def f(rng, P, hit):
            own = OWN[rule]
            room = word[w].size - own
            q = np.zeros(64, int)
            for _ in range(T):
                q[rng.choice(np.nonzero(q < room)[0])] += 1
            m = np.zeros((64, n_tri), bool)
            for i in range(64):  # (own candidates first in index order: the lane's own tests take them)
                m[i, _subset(rng, word[w], own + q[i])] = True
            return m
        return f

    def only(ws):
        def f(rng, P, hit):
            m = np.zeros((64, n_tri), bool)
            for w in ws:
                m[:, word[w]] = rng.random((64, word[w].size)) < 0.5
            return m
        return f

    def sparse(rng, P, hit):  # 1-5 random triangles, never the scan's hit
        m = np.zeros((64, n_tri), bool)
        for i in range(64):
            m[i, _subset(rng, everything, rng.integers(1, 6))] = True
            if hit[i] >= 0:
                m[i, hit[i]] = False
        return m

    def passes(rng, P, hit):
        return P.copy()

    def superset(rng, P, hit):
        return P | (rng.random(P.shape) < 0.15)

    pats = [("full", full), ("empty", empty), ("full", full), ("heavy lane 0", heavy(0)),
            ("heavy lane 63", heavy(63)), ("passes", passes), ("heavy lane 31", heavy(31)), ("staircase", staircase),
            ("superset", superset), ("sparse", sparse)]
    if n_tri >= 64:
        pats.append(("staircase word 0", staircase_word0))
    for w in sorted({0, words - 1}):
        for T in (0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap):
            if T <= 64 * (word[w].size - OWN[rule]):
                pats.append((f"total {T} word {w}", total(T, w)))
    pats.append(("last word only", only([words - 1])))
    if words > 1:
        pats.append(("words 1 up only", only(range(1, words))))
    return pats


_PHASE_MASKS = {}


def phase_masks(rtmi, oracle, kind, rule, cap):
    """(names per wave, masks (n, words), superset rows) for the scene's part-B rays"""
    key = (kind, rule, cap)
    if key not in _PHASE_MASKS:
        geom, tri, o, d = phase_rays(rtmi, kind)
        n, n_tri = o.shape[0], tri.shape[0]
        Pm = oracle.pass_masks(tri, o, d, 512.0, rule)
        P = np.unpackbits(Pm.view(np.uint8), axis=1, bitorder="little")[:, :n_tri].astype(bool)
        hit = hit_triangles(oracle, geom, o, d, 512.0, rule)
        pats = wave_patterns(n_tri, rule, cap)
        rng = np.random.default_rng(1000 * rule + cap)
        rows = np.zeros((n, n_tri), bool)
        names = []
        for w in range((n + 63) // 64):
            name, f = pats[w % len(pats)]
            a, b = 64 * w, min(64 * w + 64, n)
            Pw, hw = np.zeros((64, n_tri), bool), np.full(64, -1)
            Pw[:b - a], hw[:b - a] = P[a:b], hit[a:b]
            rows[a:b] = f(rng, Pw, hw)[:b - a]
            names.append(name)
        sup = np.repeat(np.isin(names, ("full", "passes", "superset")), 64)[:n]
        _PHASE_MASKS[key] = (names, _mask_of(rows, n_tri), sup)
    return _PHASE_MASKS[key]


PHASE_CASES = [("cornell", CAP_TABLE), ("cornell", CAP_SHARED), ("archway", CAP_SHARED), ("box", CAP_SHARED)]


def test_wave_patterns_hold_what_they_name(rtmi_mod, oracle_mod):
    """(CPU) the masks of part B: the pair totals after the own-lane tests, the multi-window
    waves, a lane with all 64 of a word, empty waves between full ones."""
    for kind, cap in PHASE_CASES:
        n_tri = _geom(rtmi_mod, kind).n_tri
        for rule in (0, 1):
            names, masks, sup = phase_masks(rtmi_mod, oracle_mod, kind, rule, cap)
            pc = np.zeros((masks.shape[0], masks.shape[1]), int)  # candidates per ray and word
            for w in range(masks.shape[1]):
                pc[:, w] = np.unpackbits(masks[:, w:w + 1].view(np.uint8), axis=1).sum(axis=1)
            seen = set()
            for wv, name in enumerate(names[:len(names) - 1]):  # (whole waves)
                c = pc[64 * wv:64 * wv + 64]
                if name.startswith("total"):
                    T, w = int(name.split()[1]), int(name.split()[3])
                    assert c[:, [k for k in range(c.shape[1]) if k != w]].sum() == 0
                    assert np.maximum(c[:, w] - OWN[rule], 0).sum() == T and c[:, w].min() >= OWN[rule], name
                    seen.add(T)
                elif name == "empty":
                    assert c.sum() == 0 and names[wv - 1] == "full" and names[wv + 1] == "full"
                elif name == "full":
                    assert np.all(c.sum(axis=1) == n_tri)
                elif name == "staircase":
                    assert np.array_equal(c.sum(axis=1), np.minimum(np.arange(64), n_tri))
                elif name == "staircase word 0":
                    assert c[63, 0] == 64
            assert {0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap} <= seen, (kind, rule, seen)
            assert len(set(names[:4])) >= 3 and sup.sum() >= 64 * 3
    # Cornell's full wave: 2,432 pairs less the lanes' own, 26 windows at the table route's cap
    assert 64 * 38 == 2432 and -(-64 * 38 // CAP_TABLE) == 26 and CAP_TABLE % 38 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,cap", PHASE_CASES)
@pytest.mark.parametrize("rule", [0, 1])
def test_gpu_exact_phase_on_given_masks(rtmi_mod, oracle_mod, gpu_ctx, scenes, kind, cap, rule):
    """closest_hit_cand on the patterns above, at ray counts around the wave and the workgroup
    and one of 20,000: (t, hit) of every ray is the masked scan's bit for bit, the scan's own
    where the mask holds the pass set, nothing for an empty mask; nothing is written past n."""
    geom, tri, o, d = phase_rays(rtmi_mod, kind)
    names, masks, sup = phase_masks(rtmi_mod, oracle_mod, kind, rule, cap)
    sc = scenes(kind)
    tm, hm = _oracle_scan(oracle_mod, geom, o, d, 512.0, rule, masks)
    tf, hf = _oracle_scan(oracle_mod, geom, o, d, 512.0, rule)
    assert np.array_equal(hm[sup], hf[sup]) and np.array_equal(_bits(tm[sup]), _bits(tf[sup]))
    none = ~masks.any(axis=1)
    assert none.sum() >= 64 and np.all(hm[none] == -1) and np.all(np.isinf(tm[none]))
    for n in (1, 63, 64, 65, 255, 256, 257, o.shape[0]):
        # (the short counts start at different waves of the pattern list)
        a = 0 if n == o.shape[0] else 64 * (n % 7)
        t, h = rtmi_mod.intersect_cand(gpu_ctx, sc, o[a:a + n], d[a:a + n], 512.0, rule, masks=masks[a:a + n],
                                       pair_cap=cap, guard=96)
        assert np.all(_bits(t[n:]) == 0xA5A5A5A5) and np.all(_bits(h[n:]) == 0xA5A5A5A5), n
        bad = np.nonzero((h[:n] != hm[a:a + n]) | (_bits(t[:n]) != _bits(tm[a:a + n])))[0]
        assert bad.size == 0, (f"n = {n}: {bad.size} rays differ from the masked scan, e.g. ray {a + bad[0]} of "
                               f"wave '{names[(a + bad[0]) // 64]}': ({t[bad[0]]}, {h[bad[0]]}) for "
                               f"({tm[a + bad[0]]}, {hm[a + bad[0]]}); waves "
                               f"{sorted({names[(a + b) // 64] for b in bad})}")


@pytest.mark.gpu
def test_gpu_a_pass_at_the_start_distance_is_no_hit(rtmi_mod, oracle_mod, gpu_ctx, scenes):
    """The GPU rule's window starts at t = 999999 and accepts t < best: a triangle that passes
    at exactly 999999 is no hit (with `<=` it would be), one at 999998 is.  Rays into the box
    from 999998, 999999 and 1000000 in front of its near wall, t_scale 1: exact in float32."""
    geom = _geom(rtmi_mod, "box")
    tri = geom.all_triangles()
    xy = np.random.default_rng(1).uniform(-0.95, 0.95, (64, 2)).astype(np.float32)
    o = np.concatenate([np.concatenate([xy, np.full((64, 1), -1.0 - dist, np.float32)], axis=1)
                        for dist in (999998.0, 999999.0, 1000000.0)]).astype(np.float32)
    d = np.tile(np.asarray([0.0, 0.0, 1.0], np.float32), (192, 1))
    P = oracle_mod.pass_masks(tri, o, d, 1.0, 1)
    tc, hc = _oracle_scan(oracle_mod, geom, o, d, 1.0, 1)
    assert P.any(axis=1).all() and np.all(tc[:64] == 999998.0) and np.all(hc[64:] == -1)
    for masks in (P, np.tile(_full_mask(tri.shape[0]), (192, 1))):
        t, h = rtmi_mod.intersect_cand(gpu_ctx, scenes("box"), o, d, 1.0, 1, masks=masks)
        assert np.array_equal(h, hc) and np.array_equal(_bits(t), _bits(tc))


@pytest.mark.gpu
def test_gpu_intersect_cand_refuses_what_it_does_not_serve(rtmi_mod, gpu_ctx, scenes):
    """No silent fallback: a pair cap no render kernel pairs with the scene's mask words, a
    candidate bit past the last triangle -> RT_E_INVALID; the CPU rule's table below its
    t_scale, a scene of more than 256 triangles -> RT_E_UNSUPPORTED."""
    o = np.zeros((4, 3), np.float32)
    d = np.tile(np.asarray([0.0, 0.0, 1.0], np.float32), (4, 1))
    surf = np.zeros(4, np.int32)

    def code(sc, ts, rule, **kw):
        with pytest.raises(rtmi_mod.RtError) as e:
            rtmi_mod.intersect_cand(gpu_ctx, sc, o, d, ts, rule, **kw)
        return e.value.code

    arch, corn = scenes("archway"), scenes("cornell")
    assert code(arch, 512.0, 1, surf=surf, pair_cap=CAP_TABLE) == -1
    assert code(corn, 512.0, 0, surf=surf, pair_cap=64) == -1
    bad = np.zeros((4, 1), np.uint64)
    bad[2, 0] = np.uint64(1) << np.uint64(38)
    assert code(corn, 512.0, 0, masks=bad, pair_cap=CAP_TABLE) == -1
    assert code(corn, 255.0, 0, surf=surf, pair_cap=CAP_TABLE) == -5
    with rtmi_mod.Scene(gpu_ctx, rtmi_mod.obj_geometry(os.path.join(MODELS, "bunny.obj"), "generic")) as big:
        m = np.zeros((4, (big.geom.n_tri + 63) // 64), np.uint64)
        assert code(big, 512.0, 1, masks=m) == -5
        assert code(big, 512.0, 1, surf=surf) == -5
