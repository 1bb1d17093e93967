"""The exact BVH path (rt_trace.hpp closest_hit_bvh, rt_bvh.cpp) on crafted scenes.

The shipped meshes of test_bvh.py almost never reach the branches that hold the path's logic:
rule 0's fold of the candidates below cut = fl(fl(tmin + eps) + eps) in index order, its two
hand-offs to the scan (more than kBvhCand candidates; a fold that could climb to the cut), exact
ties under both rules, a leaf at the depth cap, the coincident-centroid halving, one- and
two-triangle trees, and scenes at the ends of the ranges the build's bounds are made for.  The
small synthetic families below reach each of them by construction.

Every ray of every set is kept (no generator discards one) and compared bit for bit: the BVH
against the scan and against the CPU restatement.  That a family reaches its corner is asserted
on the restatement alone (oracle.pass_t, oracle.intersect), in the unmarked tests, so those
claims hold without a GPU; the measured counts are in DESIGN.md §6.
"""
import ctypes

import numpy as np
import pytest

from test_bvh import _same

EPS = np.float32(1e-5)
T_SCALE = {0: 512.0, 1: 720.0}   # each hit rule at its engine's own SCREEN_HEIGHT
N_RAYS = 20_000
K_BVH_CAND = 4                   # rt_internal.hpp kBvhCand
K_BVH_MAX_DEPTH = 24             # rt_internal.hpp kBvhMaxDepth
RT_E_UNSUPPORTED = -5            # include/rtmi.h
N_SKIP = 15                      # deep: the geometric sequence in front of the cluster


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _geom(rtmi, tri):
    """A Geometry of surfaces only."""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    return rtmi.Geometry(tri, np.full((tri.shape[0], 3), 0.75, np.float32), np.zeros((0, 9), np.float32),
                         np.zeros((0, 3), np.float32), np.zeros((0,), np.int32))


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


TILT = _rotation((1.0, 2.0, 3.0), 0.7)   # a skew axis: no box of the tilted stack is flat


# ---------------------------------------------------------------------------------------------
# scene families
# ---------------------------------------------------------------------------------------------
STAIR_K = (2, 3, 4, 5, 6, 12)
STAIR_STEPS = (0.45, 0.9, 0.999, 1.0, 1.001, 1.9, 2.1)
STAIR_ORDERS = ("asc", "desc", "evenodd", "shuffle")


def sheet_order(K, order):
    """order[j] = the sheet stored at index pair j.  Rays from below meet sheet 0 first: `asc`
    lets the scan climb the staircase (its t is not tmin), `desc` walks it down to tmin,
    `evenodd` (0, 2, 4, .., 1, 3, ..) and the seeded shuffle stop part of the way."""
    if order == "asc":
        return np.arange(K)
    if order == "desc":
        return np.arange(K)[::-1].copy()
    if order == "evenodd":
        return np.concatenate([np.arange(0, K, 2), np.arange(1, K, 2)])
    return np.random.default_rng(100 + K).permutation(K)


def stairs(K, step, order, t_scale, rot=None, size=1.0, centre=(0.0, 0.0, 0.0)):
    """K squares of two triangles each, `size` wide, at z_k = k step 1e-5 t_scale (so a ray along
    z sees their t values step * 1e-5 apart), stored in the given sheet order; rot: rotated."""
    dz = step * 1e-5 * t_scale
    out = []
    for k in sheet_order(K, order):
        z = k * dz
        a, b, c, d = (0, 0, z), (size, 0, z), (size, size, z), (0, size, z)
        out += [a + b + c, a + c + d]
    t = np.array(out, np.float64).reshape(-1, 3)
    if rot is not None:
        t = t @ rot.T
    return (t + np.asarray(centre, np.float64)).astype(np.float32).reshape(-1, 9)


def stair_rays(K, step, t_scale, rot, seed, n=N_RAYS):
    """The ray sets of a stack, generated in the stack's own frame and rotated with it:
    oblique rays through the stack from both sides; rays starting on a sheet and between two
    sheets; directions with one and two components exactly +0.0 / -0.0 from origins in the planes
    of the (flat) boxes' faces; origins outside the scene box but within the origin bound (8);
    origins beyond it, NaN and inf components (the documented scan hand-off)."""
    rng = np.random.default_rng(seed)
    dz = step * 1e-5 * t_scale
    top = (K - 1) * dz
    O, D = [], []
    # oblique, from below and from above
    m = n * 11 // 20
    o = np.empty((m, 3))
    o[:, :2] = rng.uniform(-0.2, 1.2, (m, 2))
    below = np.arange(m) % 2 == 0
    o[:, 2] = np.where(below, -1.5, top + 1.5)
    tgt = np.empty((m, 3))
    tgt[:, :2] = rng.uniform(0.02, 0.98, (m, 2))
    tgt[:, 2] = 0.5 * top
    O.append(o)
    D.append(tgt - o)
    # on a sheet / between two sheets, any direction
    m = n * 4 // 20
    k = rng.integers(0, K, m)
    o = np.empty((m, 3))
    o[:, :2] = rng.uniform(0.0, 1.0, (m, 2))
    o[:, 2] = (k + 0.5 * (np.arange(m) % 2) * (k < K - 1)) * dz
    O.append(o)
    D.append(rng.normal(size=(m, 3)))
    # exact zero components: along and against each axis, and in each coordinate plane; the
    # origin has one coordinate in a face plane of the boxes (x, y in {0, 1}, z = z_k)
    m = n * 2 // 20
    d = rng.normal(size=(m, 3))
    kind = np.arange(m) % 12
    ax = kind % 3
    for a in range(3):
        two = (kind < 6) & (ax == a)            # two zero components: +-e_a
        d[two] = 0.0
        d[two, a] = np.where(kind[two] < 3, 1.0, -1.0)
        d[(kind >= 6) & (ax == a), a] = 0.0    # one zero component
    neg = rng.random((m, 3)) < 0.5
    d = np.where((d == 0.0) & neg, -0.0, d)
    o = rng.uniform(-0.5, 1.5, (m, 3))
    o[:, 2] = rng.uniform(-0.5, 0.5, m) + 0.5 * top
    face = rng.integers(0, 3, m)
    pick = rng.integers(0, 2, m).astype(np.float64)
    o[face == 0, 0] = pick[face == 0]
    o[face == 1, 1] = pick[face == 1]
    o[face == 2, 2] = rng.integers(0, K, np.count_nonzero(face == 2)) * dz
    O.append(o)
    D.append(d)
    # outside the scene box, inside the origin bound
    m = n * 2 // 20
    o = _unit(rng.normal(size=(m, 3))).astype(np.float64) * rng.uniform(3.0, 4.5, (m, 1))
    tgt = np.concatenate([rng.uniform(0, 1, (m, 2)), np.full((m, 1), 0.5 * top)], 1)
    O.append(o)
    D.append(tgt - o)
    # beyond the bound, non-finite
    m = n - sum(x.shape[0] for x in O)
    o = _unit(rng.normal(size=(m, 3))).astype(np.float64) * rng.uniform(15.0, 60.0, (m, 1))
    d = np.array([0.5, 0.5, 0.5 * top]) - o
    O.append(o)
    D.append(d)
    o = np.concatenate(O)
    d = np.concatenate(D)
    if rot is not None:
        zs = slice(O[0].shape[0] + O[1].shape[0], O[0].shape[0] + O[1].shape[0] + O[2].shape[0])
        oz, dz_ = o[zs].copy(), d[zs].copy()
        o, d = o @ rot.T, d @ rot.T
        o[zs], d[zs] = oz, dz_   # the exact zeros stay in the world's axes
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), (d / nrm).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j in range(12):                 # the last rows: one non-finite component each
        (o if j % 2 else d)[n - 1 - j, j % 3] = bad[(j // 2) % 3]
    return o, d


def stair_cases(rule):
    """(name, triangles, origins, directions) of the stairs family under a rule: every K, step
    and order axis-aligned, and the 0.9 / 1.001 steps tilted (216 stacks)."""
    ts = T_SCALE[rule]
    for K in STAIR_K:
        for step in STAIR_STEPS:
            for order in STAIR_ORDERS:
                for rot in (None, TILT):
                    if rot is not None and step not in (0.9, 1.001):
                        continue
                    seed = (K * 10000 + int(round(step * 1000))) * 10 + STAIR_ORDERS.index(order) * 2 + (rot is None)
                    o, d = stair_rays(K, step, ts, rot, seed)
                    yield f"K{K}-s{step}-{order}-{'flat' if rot is None else 'tilt'}", \
                        stairs(K, step, order, ts, rot), o, d


def soup_rays(tri, seed, n=N_RAYS, aim_sigma=0.0):
    """The ray sets of a triangle soup: rays aimed at float points of the triangles and of their
    edges and vertices from shells around the scene; rays starting on a triangle (the point
    itself and the bounce loop's 1e-5 offset); directions with exact +-0 components from origins
    on the face planes of the triangles' boxes; origins between the scene box and the origin
    bound; origins beyond it, NaN and inf components."""
    rng = np.random.default_rng(seed)
    t = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
    vmax = float(np.abs(t).max())
    obound = max(8.0, 2.0 * vmax + 1.0)
    lo, hi = t.reshape(-1, 3).min(0).astype(np.float64), t.reshape(-1, 3).max(0).astype(np.float64)
    c, r = 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1e-3)

    def points(m, edge):
        i = rng.integers(0, t.shape[0], m)
        u = rng.random(m, dtype=np.float32)
        v = rng.random(m, dtype=np.float32)
        flip = u + v > 1
        u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
        if edge:
            side = rng.integers(0, 3, m)
            u[side == 0] = 0
            v[side == 1] = 0
            on_hyp = side == 2
            v[on_hyp] = 1 - u[on_hyp]
            u[::7] = 0     # vertices
            v[::7] = 0
        return (t[i, 0] + u[:, None] * (t[i, 1] - t[i, 0]) + v[:, None] * (t[i, 2] - t[i, 0])).astype(np.float32), i

    O, D = [], []
    for edge, m in ((False, n * 7 // 20), (True, n * 5 // 20)):
        p, _ = points(m, edge)
        o = c + _unit(rng.normal(size=(m, 3))) * rng.uniform(0.05, 1.0, (m, 1)) * min(r, vmax + 1.0)
        o = o.astype(np.float32)
        O.append(o)
        D.append(p.astype(np.float64) - o + aim_sigma * rng.normal(size=(m, 3)))
    m = n * 3 // 20
    p, _ = points(m, False)
    d = _unit(rng.normal(size=(m, 3)))
    p[::2] = p[::2] + EPS * d[::2]
    O.append(p)
    D.append(d.astype(np.float64))
    m = n * 2 // 20
    d = rng.normal(size=(m, 3))
    kind = np.arange(m) % 12
    ax = kind % 3
    for a in range(3):
        two = (kind < 6) & (ax == a)
        d[two] = 0.0
        d[two, a] = np.where(kind[two] < 3, 1.0, -1.0)
        d[(kind >= 6) & (ax == a), a] = 0.0
    d = np.where((d == 0.0) & (rng.random((m, 3)) < 0.5), -0.0, d)
    p, i = points(m, False)
    face = rng.integers(0, 3, m)
    box = np.where(rng.random((m, 3)) < 0.5, t[i].min(1), t[i].max(1))
    p[np.arange(m), face] = box[np.arange(m), face]
    # step back along the non-zero components so that the triangle is ahead of the origin
    O.append((p - 0.25 * min(r, 1.0) * np.where(d == 0.0, 0.0, np.sign(d))).astype(np.float32))
    D.append(d)
    m = n * 2 // 20
    p, _ = points(m, False)
    shell = rng.uniform(vmax * 1.05 + 0.5, obound * 0.95, (m, 1))
    o = _unit(rng.normal(size=(m, 3)))
    o = (o / np.abs(o).max(1, keepdims=True) * shell).astype(np.float32)   # max-norm: inside obound
    O.append(o)
    D.append(p.astype(np.float64) - o)
    m = n - sum(x.shape[0] for x in O)
    o = (_unit(rng.normal(size=(m, 3))) * rng.uniform(1.5 * obound, 6.0 * obound, (m, 1))).astype(np.float32)
    O.append(o)
    D.append(c - o)
    o = np.concatenate(O).astype(np.float32)
    d = np.concatenate(D)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    d = (d / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j in range(12):
        (o if j % 2 else d)[n - 1 - j, j % 3] = bad[(j // 2) % 3]
    return o, d


BASE_TRI = np.array([[-0.6, -0.4, 0.1], [0.7, -0.3, -0.2], [0.05, 0.8, 0.3]], np.float32)


def twin_cases():
    """(name, triangles): one triangle 2, 3, 4 and 5 times (4 fills rule 0's candidate list, 5
    overflows it); its three cyclic vertex orders and their reversed windings (a near tie from
    different rounding); two triangles sharing an edge."""
    for m in (2, 3, 4, 5):
        yield f"same-x{m}", np.tile(BASE_TRI.reshape(1, 9), (m, 1))
    perm = [BASE_TRI[[j, (j + 1) % 3, (j + 2) % 3]] for j in range(3)]
    perm += [p[[0, 2, 1]] for p in perm]
    yield "orders", np.array(perm, np.float32).reshape(-1, 9)
    far = np.array([-0.5, 0.6, -0.7], np.float32)
    yield "shared-edge", np.array([BASE_TRI, np.array([BASE_TRI[1], BASE_TRI[0], far])], np.float32).reshape(-1, 9)


def centred_triangles(n, p_lo, p_hi, seed):
    """n triangles whose bounding boxes all have centre exactly 0: v0 = -p, v1 = +p and
    |v2_i| <= |p_i|; every padded-box centroid coincides, so the build can only halve the list."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(p_lo, p_hi, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    v2 = p * rng.uniform(-1.0, 1.0, (n, 3))
    return np.concatenate([-p, p, v2], 1).astype(np.float32)


def deep_scene():
    """The depth-cap scene: N_SKIP triangles at x = 20^-k of size 0.3 * 20^-k, which the binned
    split can only peel off one a level, in front of 2,048 triangles with one common box centre,
    which it can only halve: the cap (level kBvhMaxDepth - 1) arrives with more than kLeafMax
    triangles left in a leaf."""
    k = np.arange(N_SKIP, dtype=np.float64)
    x, s = 20.0 ** -k, 0.3 * 20.0 ** -k
    z = np.zeros_like(x)
    seq = np.stack([x, 0.1 * s, z, x + s, 0.1 * s, 0.2 * s, x, 1.1 * s, 0.3 * s], 1)
    return np.concatenate([seq.astype(np.float32), centred_triangles(2048, 0.002, 0.01, 5)], 0)


def deep_rays(seed, n=N_RAYS):
    """Rays aimed into the cluster at the origin: along all six axes (exact axis directions and
    jittered ones), at random from a shell around it, and the soup sets of the whole scene."""
    rng = np.random.default_rng(seed)
    m = n // 4
    axis = np.arange(m) % 6
    o = np.zeros((m, 3))
    o[np.arange(m), axis % 3] = np.where(axis < 3, 1.0, -1.0) * rng.uniform(0.02, 0.6, m)
    exact = np.arange(m) % 4 == 0
    tgt = rng.uniform(-0.008, 0.008, (m, 3))
    d = tgt - o
    o[~exact] += rng.uniform(-0.004, 0.004, (np.count_nonzero(~exact), 3))
    for a in range(3):   # the exact rows: +-e_a with true zeros, through a point near the origin
        row = exact & (axis % 3 == a)
        d[row] = 0.0
        d[row, a] = -np.sign(o[row, a])
        o[row] += np.where(np.arange(3) == a, 0.0, 1.0) * rng.uniform(-0.004, 0.004, (np.count_nonzero(row), 3))
    m2 = n // 4
    o2 = _unit(rng.normal(size=(m2, 3))).astype(np.float64) * rng.uniform(0.011, 0.5, (m2, 1))
    d2 = rng.uniform(-0.008, 0.008, (m2, 3)) - o2
    o3, d3 = soup_rays(deep_scene(), seed + 1, n - m - m2)
    o = np.concatenate([o, o2]).astype(np.float32)
    d = _unit(np.concatenate([d, d2]))
    return np.concatenate([o, o3]), np.concatenate([d, d3])


def fan_scene():
    return centred_triangles(40, 0.3, 1.0, 6)


def tiny_cases():
    yield "one", BASE_TRI.reshape(1, 9)
    yield "two", np.array([BASE_TRI, BASE_TRI[[0, 2, 1]] + np.float32(0.25)], np.float32).reshape(2, 9)


def wide_scene():
    """400 triangles with centres in +-300 and sizes 10^U(-4, 2): tiny triangles among
    coordinates of several hundred units."""
    rng = np.random.default_rng(8)
    c = rng.uniform(-300, 300, (400, 1, 3))
    s = 10.0 ** rng.uniform(-4, 2, (400, 1, 1))
    return (c + s * rng.normal(size=(400, 3, 3))).astype(np.float32).reshape(-1, 9)


def needle_scene():
    """300 needles: the third vertex 1e-4 (relative to the first edge) off that edge."""
    rng = np.random.default_rng(9)
    v0 = rng.uniform(-2, 2, (300, 3))
    e1 = rng.normal(size=(300, 3))
    e1 *= rng.uniform(0.3, 2.0, (300, 1)) / np.linalg.norm(e1, axis=1, keepdims=True)
    perp = np.cross(e1, rng.normal(size=(300, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    v2 = v0 + rng.uniform(0.1, 0.9, (300, 1)) * e1 + 1e-4 * np.linalg.norm(e1, axis=1, keepdims=True) * perp
    return np.concatenate([v0, v0 + e1, v2], 1).astype(np.float32)


def huge_triangles():
    """300 triangles about 1e6 from the origin: outside the ranges the BVH's bounds hold for."""
    rng = np.random.default_rng(10)
    c = rng.choice([-1e6, 1e6], (300, 1, 3)) + rng.uniform(-50, 50, (300, 1, 3))
    return (c + rng.normal(size=(300, 3, 3))).astype(np.float32).reshape(-1, 9)


def soup_cases(family):
    """(name, triangles, origins, directions) of the families that use the soup ray sets."""
    if family == "twins":
        for j, (name, tri) in enumerate(twin_cases()):
            yield (name, tri) + soup_rays(tri, 20 + j)
    elif family == "deep":
        yield ("deep", deep_scene()) + deep_rays(30)
    elif family == "fan":
        yield ("fan", fan_scene()) + soup_rays(fan_scene(), 31)
    elif family == "tiny":
        for j, (name, tri) in enumerate(tiny_cases()):
            yield (name, tri) + soup_rays(tri, 32 + j)
    elif family == "ranges":
        yield ("wide", wide_scene()) + soup_rays(wide_scene(), 34)
        yield ("needles", needle_scene()) + soup_rays(needle_scene(), 35)
        # aimed a little off, so that needles are grazed and missed as well
        yield ("needles-near", needle_scene()) + soup_rays(needle_scene(), 36, aim_sigma=2e-4)
    else:
        raise KeyError(family)


SOUP_FAMILIES = ("twins", "deep", "fan", "tiny", "ranges")


def cases(family, rule):
    return stair_cases(rule) if family == "stairs" else soup_cases(family)


# ---------------------------------------------------------------------------------------------
# CPU: the host build on every family, and what the families reach (the restatement alone)
# ---------------------------------------------------------------------------------------------
def _bvh_check(rtmi, tri):
    tri = np.ascontiguousarray(tri, np.float32)
    stats = (ctypes.c_int64 * 4)()
    rc = rtmi.lib().rt_bvh_check(tri.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), tri.shape[0], stats)
    return rc, list(stats)


def _scan(oracle, tri, o, d, rule):
    return oracle.intersect(tri, tri.shape[0], 0, np.zeros(0, np.int32), o, d, T_SCALE[rule], rule)


def _cut(tmin):
    return (tmin + EPS) + EPS   # float32 throughout: fl(fl(tmin + eps) + eps)


def test_pass_t_equals_single_bit_masks(oracle_mod):
    """oracle.pass_t is closest_hit_masked's per-triangle code: entry (r, i) is what
    intersect_masked returns for ray r with triangle i alone in the mask (its t, or no hit)."""
    for rule in (0, 1):
        tri = stairs(3, 0.9, "evenodd", T_SCALE[rule], TILT)
        o, d = stair_rays(3, 0.9, T_SCALE[rule], TILT, 77, 4000)
        pt = oracle_mod.pass_t(tri, o, d, T_SCALE[rule], rule)
        assert pt.shape == (4000, 6) and pt.dtype == np.float32
        for i in range(6):
            masks = np.full((4000, 1), 1 << i, np.uint64)
            t, h = oracle_mod.intersect_masked(tri, 6, 0, np.zeros(0, np.int32), o, d, masks, T_SCALE[rule], rule)
            assert np.array_equal(pt[:, i].view(np.uint32), t.view(np.uint32))
            assert np.array_equal(h != -1, np.isfinite(pt[:, i]))
        assert np.isfinite(pt).any(1).sum() > 2000


def test_families_build_on_the_host(rtmi_mod):
    """rt_bvh_check builds every family and finds the trees' invariants intact."""
    scenes = [(f"stairs {K}-{step}-{order}-{ts}", stairs(K, step, order, ts, rot))
              for K in STAIR_K for step in STAIR_STEPS for order in STAIR_ORDERS for rot in (None, TILT)
              for ts in T_SCALE.values()]
    scenes += [(f"{family} {name}", tri) for family in SOUP_FAMILIES for name, tri in _scenes_only(family)]
    for name, tri in scenes:
        rc, (nodes, depth, pnodes, leaves) = _bvh_check(rtmi_mod, tri)
        assert rc == 0, (name, rtmi_mod.lib().rt_last_error().decode())
        assert nodes == 2 * leaves - 1 and depth < K_BVH_MAX_DEPTH


def _scenes_only(family):
    if family == "twins":
        return list(twin_cases())
    if family == "deep":
        return [("deep", deep_scene())]
    if family == "fan":
        return [("fan", fan_scene())]
    if family == "tiny":
        return list(tiny_cases())
    return [("wide", wide_scene()), ("needles", needle_scene())]


def test_tree_shapes(rtmi_mod):
    """deep reaches the depth cap with leaves above kLeafMax = 4 triangles; the fan's 40
    triangles, split by halving alone, end in 16 leaves of two and three; the tiny trees are one
    leaf."""
    tri = deep_scene()
    rc, (nodes, depth, pnodes, leaves) = _bvh_check(rtmi_mod, tri)
    assert rc == 0 and tri.shape[0] == N_SKIP + 2048
    assert depth == K_BVH_MAX_DEPTH - 1
    assert leaves * 4 < tri.shape[0]
    rc, (nodes, depth, pnodes, leaves) = _bvh_check(rtmi_mod, fan_scene())
    assert rc == 0 and (depth, leaves) == (4, 16)   # 40 -> 20 -> 10 -> 5 -> 2 + 3
    for name, t in tiny_cases():
        rc, (nodes, depth, pnodes, leaves) = _bvh_check(rtmi_mod, t)
        assert rc == 0 and (nodes, depth, leaves) == (1, 0, 1)


def test_out_of_range_scene_is_refused(rtmi_mod):
    rc, _ = _bvh_check(rtmi_mod, huge_triangles())
    assert rc == RT_E_UNSUPPORTED


def _stairs_reach(oracle):
    """Over the rule-0 stairs family: rays with 2..kBvhCand triangles below the cut whose scan t
    is not tmin (the order-dependent fold), rays whose scan t reaches the cut (the
    bmax + eps <= cut hand-off), rays with more than kBvhCand triangles below the cut (the
    overflow hand-off); and the last of these under rule 1's arithmetic."""
    fold = climb = over = over1 = 0
    for name, tri, o, d in stair_cases(0):
        pt = oracle.pass_t(tri, o, d, T_SCALE[0], 0)
        t, h = _scan(oracle, tri, o, d, 0)
        tmin = pt.min(1)
        hit = np.isfinite(tmin)
        assert np.array_equal(hit, h != -1)
        cut = _cut(tmin)
        nc = (pt < cut[:, None]).sum(1)
        fold += np.count_nonzero(hit & (nc >= 2) & (nc <= K_BVH_CAND) & (t != tmin) & (t < cut))
        climb += np.count_nonzero(hit & (t >= cut))
        over += np.count_nonzero(hit & (nc > K_BVH_CAND))
    for name, tri, o, d in stair_cases(1):
        pt = oracle.pass_t(tri, o, d, T_SCALE[1], 1)
        tmin = pt.min(1)
        over1 += np.count_nonzero(np.isfinite(tmin) & ((pt < _cut(tmin)[:, None]).sum(1) > K_BVH_CAND))
    return fold, climb, over, over1


def test_stairs_reach_the_fold_and_both_hand_offs(oracle_mod):
    fold, climb, over, over1 = _stairs_reach(oracle_mod)
    print(f"stairs reach: fold {fold}, climb past the cut {climb}, overflow {over} (rule-1 arithmetic {over1})")
    assert fold >= 1000 and climb >= 1000 and over >= 1000 and over1 >= 1000


def _twins_reach(oracle, rule):
    n = 0
    for name, tri, o, d in soup_cases("twins"):
        pt = oracle.pass_t(tri, o, d, T_SCALE[rule], rule)
        t, h = _scan(oracle, tri, o, d, rule)
        tmin = pt.min(1)
        tied = np.isfinite(tmin)[:, None] & (pt == tmin[:, None])
        rows = tied.sum(1) >= 2
        first = tied.argmax(1)
        last = tri.shape[0] - 1 - tied[:, ::-1].argmax(1)
        if name.startswith("same"):   # copies of one triangle: every hit is an exact tie of them all
            assert np.array_equal(rows, h != -1) and np.all(tied.sum(1)[rows] == tri.shape[0])
        # the scan's index among the tied: the first under rule 1 (strict t < best); under rule 0
        # (t < best + eps) the last, where no other triangle is near (the copies, the edge pair)
        if rule == 1:
            assert np.array_equal(h[rows] & 0xffffff, first[rows])
        elif name != "orders":
            assert np.array_equal(h[rows] & 0xffffff, last[rows])
        if rule == 1 or name != "orders":
            assert np.array_equal(t[rows], tmin[rows])
        n += np.count_nonzero(rows)
    return n


@pytest.mark.parametrize("rule", [0, 1])
def test_twins_reach_exact_ties(oracle_mod, rule):
    n = _twins_reach(oracle_mod, rule)
    print(f"twins reach, rule {rule}: {n} rays with two or more triangles at bit-equal minimal t")
    assert n >= 1000


def test_deep_reaches_the_cluster(oracle_mod):
    tri = deep_scene()
    o, d = deep_rays(30)
    for rule in (0, 1):
        t, h = _scan(oracle_mod, tri, o, d, rule)
        n = np.count_nonzero((h != -1) & ((h & 0xffffff) >= N_SKIP))
        print(f"deep reach, rule {rule}: {n} rays hit a cluster triangle, {np.count_nonzero(h != -1)} hit")
        assert n >= 1000


# ---------------------------------------------------------------------------------------------
# GPU: the BVH against the scan and the restatement, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("family", ("stairs",) + SOUP_FAMILIES)
def test_bvh_crafted_matches_scan_and_oracle(rtmi_mod, oracle_mod, gpu_ctx, family, rule):
    ts = T_SCALE[rule]
    n = 0
    for name, tri, o, d in cases(family, rule):
        g = _geom(rtmi_mod, tri)
        with rtmi_mod.Scene(gpu_ctx, g) as sc:
            bvh = rtmi_mod.intersect_method(gpu_ctx, sc, o, d, ts, rule, rtmi_mod.ISECT_BVH)
            scan = rtmi_mod.intersect_method(gpu_ctx, sc, o, d, ts, rule, rtmi_mod.ISECT_SCAN)
        ref = _scan(oracle_mod, tri, o, d, rule)
        try:
            _same(scan, ref)
            _same(bvh, scan)
        except AssertionError as e:
            bad = np.flatnonzero((bvh[1] != scan[1]) | (bvh[0].view(np.uint32) != scan[0].view(np.uint32)))
            raise AssertionError(f"{family}/{name}, rule {rule}: {e}; {bad.size} rays differ from the scan, "
                                 f"first {bad[:5].tolist()}") from None
        n += 1
    assert n > 0


@pytest.mark.gpu
def test_bvh_crafted_deep_device_tree(rtmi_mod, gpu_ctx):
    """The device scene's tree of `deep` is the capped one (and built without being asked:
    2,063 triangles is above the automatic threshold)."""
    with rtmi_mod.Scene(gpu_ctx, _geom(rtmi_mod, deep_scene())) as sc:
        assert sc.accel_info()["depth"] == K_BVH_MAX_DEPTH - 1


def stairs_cornell(rtmi, preset, t_scale):
    """The Cornell box holding a 6-sheet ascending stack that faces the camera (step 0.9 at the
    render's t_scale: camera rays climb it to the cut) and a twin pair."""
    box = rtmi.cornell_geometry(preset)
    stack = stairs(6, 0.9, "asc", t_scale, None, 0.7, (-0.45, -0.3, 0.0))
    twin = (np.tile(BASE_TRI.reshape(1, 9), (2, 1)).reshape(-1, 3) * np.float32(0.4)
            + np.array([0.45, 0.45, -0.3], np.float32)).reshape(-1, 9)
    extra = np.concatenate([stack, twin], 0).astype(np.float32)
    tri = np.concatenate([box.tri, extra], 0)
    alb = np.concatenate([box.albedo, np.full((extra.shape[0], 3), 0.75, np.float32)], 0)
    return rtmi.Geometry(tri, alb, box.light, box.emission, box.light_group)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", [0, 1])
def test_bvh_crafted_render_matches_scan_and_oracle(rtmi_mod, oracle_mod, gpu_ctx, preset):
    """k_render<BVH> on the stack and the twins: image bits and cast count of the scan and of
    the restatement."""
    p = rtmi_mod.default_params(preset, width=64, height=64, spp=4, spp_split=2)
    g = stairs_cornell(rtmi_mod, preset, p.t_scale)
    cam_pos = rtmi_mod.CAMERAS["cornell"]
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        sc.set_accel(rtmi_mod.ACCEL_BVH)
        img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(cam_pos), p)
        sc.set_accel(rtmi_mod.ACCEL_SCAN)
        img_s, casts_s = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(cam_pos), p)
    assert casts == casts_s
    assert np.array_equal(img.view(np.uint32), img_s.view(np.uint32))
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(cam_pos), oracle_mod.params_from(p))
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("hit_rule", [1, 0])
def test_bvh_crafted_sarsa_frame_equals_scan(rtmi_mod, gpu_ctx, hit_rule):
    """One frame of a frozen radiance map over the same scene (k_sarsa_render_pq<.., BVH>, stack
    stride 64), BVH against scan, under both hit rules."""
    P = rtmi_mod.RT_PRESET_GPU
    p = rtmi_mod.default_params(P, width=64, height=64, spp=4, spp_split=2, hit_rule=hit_rule)
    g = stairs_cornell(rtmi_mod, P, p.t_scale)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"])
    out = {}
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        for accel in (rtmi_mod.ACCEL_BVH, rtmi_mod.ACCEL_SCAN):
            sc.set_accel(accel)
            with rtmi_mod.sarsa.RadianceMap(gpu_ctx, sc, 1984) as m:
                m.set_td_mode(rtmi_mod.sarsa.TD_OFF)
                out[accel] = m.render(cam, p, 1)
    (a, ca), (b, cb) = out[rtmi_mod.ACCEL_BVH], out[rtmi_mod.ACCEL_SCAN]
    assert ca == cb and a.mean() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_bvh_crafted_out_of_range_scene_keeps_the_scan(rtmi_mod, oracle_mod, gpu_ctx):
    """The Cornell box with 300 triangles a million units away: the BVH is refused on request,
    and the scene as created (automatic mode, above the threshold) renders and intersects as the
    scan."""
    box = rtmi_mod.cornell_geometry(0)
    far = huge_triangles()
    g = rtmi_mod.Geometry(np.concatenate([box.tri, far], 0),
                          np.concatenate([box.albedo, np.full((far.shape[0], 3), 0.75, np.float32)], 0),
                          box.light, box.emission, box.light_group)
    p = rtmi_mod.default_params(0, width=32, height=32, spp=2, spp_split=1)
    cam_pos = rtmi_mod.CAMERAS["cornell"]
    rng = np.random.default_rng(12)
    o = rng.uniform(-1, 1, (N_RAYS, 3)).astype(np.float32)
    d = _unit(rng.normal(size=(N_RAYS, 3)))
    with rtmi_mod.Scene(gpu_ctx, g) as sc:
        assert sc.accel_info()["nodes"] == 0
        got = rtmi_mod.intersect(gpu_ctx, sc, o, d, 512.0, 0)
        scan = rtmi_mod.intersect_method(gpu_ctx, sc, o, d, 512.0, 0, rtmi_mod.ISECT_SCAN)
        img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(cam_pos), p)
        with pytest.raises(rtmi_mod.RtError) as e:
            sc.set_accel(rtmi_mod.ACCEL_BVH)
        assert e.value.code == RT_E_UNSUPPORTED
        with pytest.raises(rtmi_mod.RtError):
            rtmi_mod.intersect_method(gpu_ctx, sc, o, d, 512.0, 0, rtmi_mod.ISECT_BVH)
        sc.set_accel(rtmi_mod.ACCEL_SCAN)
        img_s, casts_s = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(cam_pos), p)
    _same(got, scan)
    _same(got, oracle_mod.intersect(g.all_triangles(), g.n_surf, g.n_light, g.light_group, o, d, 512.0, 0))
    assert casts == casts_s and np.array_equal(img.view(np.uint32), img_s.view(np.uint32))
    ref, ref_casts = oracle_mod.render(g, oracle_mod.camera(cam_pos), oracle_mod.params_from(p))
    assert casts == ref_casts and np.array_equal(img.view(np.uint32), ref.view(np.uint32))
