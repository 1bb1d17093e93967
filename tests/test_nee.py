"""Next-event estimation for the GPU preset: rt_render_nee, rt_nee_light_table, rt_nee_sample.

The estimator is defined line by line in include/rtmi.h ("next-event estimation").  Here it is
restated in numpy float32 on top of the pinned pieces -- oracle.intersect for every cast,
oracle.philox (a vectorised Philox checked against it), oracle.primary_hits for the camera
rays, oracle.normals -- one depth level at a time over all paths of a frame, and
  * without a GPU: the light table and the sampler bit for bit, the sampler's distribution, the
    estimator's expectation against the pinned renderer (oracle.render), the argument checks;
  * on the GPU: image, casts and both stats bit for bit on every cast route, the no-light
    identity with rt_render, the tile entry, the expectation and the variance against rt_render
    itself, the reference's own Cornell render, the facade.
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, MODELS, PKG

f32 = np.float32
NEE_WORD = 0x4E454531
EPS = f32(1e-5)
PI = f32(3.14159265358979323846)
RHO = f32(1.0) / (f32(2.0) * PI)
BRANCHES = ("light_seen_depth0", "light_hit_deeper", "cx_skip", "occluded", "visible", "cap")


# ------------------------------------------------------------ the restatement ----------

def philox_np(c0, c1, c2, c3, seed):
    """Philox4x32-10 of counters (c0, c1, c2, c3) (broadcast) under the seed's key: (n, 4) uint32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)])
    m = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0 = (k0 + np.uint64(0x9E3779B9)) & m
        k1 = (k1 + np.uint64(0xBB67AE85)) & m
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(w):
    return (w >> np.uint32(8)).astype(np.float32) * f32(2.0 ** -24)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0) / np.sqrt(dot3(v, v))
        return v * inv[..., None]


_S = [f32(x) for x in (1.57079632679489662, -0.645964097506246254, 0.0796926262461670451, -0.00468175413531868810,
                       0.000160441184757112456)]
_C = [f32(x) for x in (-1.23370055013616983, 0.253669507901048014, -0.0208634807633529609, 0.000919260274839426046,
                       -0.0000252020423730606054)]


def sincos_turn_np(r):
    x = r * f32(4.0)
    q = np.rint(x)
    f = x - q
    qi = q.astype(np.int64) & 3
    f2 = f * f
    sp = np.full_like(f, _S[4])
    for c in (_S[3], _S[2], _S[1], _S[0]):
        sp = sp * f2
        sp = sp + c
    sp = sp * f
    cp = np.full_like(f, _C[4])
    for c in (_C[3], _C[2], _C[1], _C[0], f32(1.0)):
        cp = cp * f2
        cp = cp + c
    s = np.select([qi == 0, qi == 1, qi == 2], [sp, cp, -sp], -cp)
    c = np.select([qi == 0, qi == 1, qi == 2], [cp, -sp, -cp], sp)
    return s.astype(np.float32), c.astype(np.float32)


def normal_frame_np(n):
    """rt_math.hpp normal_frame per row: T, B = cross(n, T) in glm's order."""
    z = np.zeros(len(n), np.float32)
    a = np.stack([n[:, 2], z, -n[:, 0]], 1)
    b = np.stack([z, -n[:, 2], n[:, 1]], 1)
    T = normalize3(np.where((np.abs(n[:, 0]) > np.abs(n[:, 1]))[:, None], a, b)).astype(np.float32)
    B = np.stack([n[:, 1] * T[:, 2] - T[:, 1] * n[:, 2], n[:, 2] * T[:, 0] - T[:, 2] * n[:, 0],
                  n[:, 0] * T[:, 1] - T[:, 0] * n[:, 1]], 1)
    return T, B


def light_table_np(light_v, emission):
    """rt_nee_light_table restated: double, stored as float32."""
    v = np.asarray(light_v, np.float32).reshape(-1, 9).astype(np.float64)
    e = np.asarray(emission, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(v)
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    le = (e[:, 0] + e[:, 1]) + e[:, 2]
    w = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) * le
    w = np.where(w > 0.0, w, 0.0)
    total = 0.0
    for x in w:
        total += x
    cdf, k = np.zeros(n, np.float32), np.zeros(n, np.float32)
    run = 0.0
    for l in range(n):
        run += w[l]
        cdf[l] = np.float32(run / total) if total > 0.0 else 0.0
        k[l] = np.float32(total / le[l]) if w[l] > 0.0 else 0.0
    return cdf, k


def last_light_np(cdf):
    prev = np.concatenate([[f32(0.0)], cdf[:-1]])
    up = np.nonzero(cdf > prev)[0]
    return int(up[-1]) if len(up) else -1


def pick_np(cdf, last, r):
    """the first light l <= last with r < cdf[l], else last"""
    return np.minimum(np.searchsorted(cdf[:last + 1], r, side="right"), last).astype(np.int64)


def light_point_np(light_v, l, u, v):
    t = np.asarray(light_v, np.float32).reshape(-1, 9)[l]
    v0, e1, e2 = t[:, 0:3], t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]
    flip = u + v > f32(1.0)
    u = np.where(flip, f32(1.0) - u, u)
    v = np.where(flip, f32(1.0) - v, v)
    return (v0 + u[:, None] * e1) + v[:, None] * e2, u, v


def sample_np(light_v, cdf, seed, pix, s, depth):
    """rt_nee_sample restated: light (-1 without weight), y, and the folded (u, v)."""
    cdf = np.asarray(cdf, np.float32)
    n = len(pix)
    last = last_light_np(cdf) if len(cdf) else -1
    if last < 0:
        return np.full(n, -1, np.int32), np.zeros((n, 3), np.float32), None, None
    w = philox_np(pix, s, 1 + np.asarray(depth, np.int64), NEE_WORD, seed)
    l = pick_np(cdf, last, u01(w[:, 0]))
    y, u, v = light_point_np(light_v, l, u01(w[:, 1]), u01(w[:, 2]))
    return l.astype(np.int32), y.astype(np.float32), u, v


class Restated:
    """The NEE frame of a rectangle, restated.  image (h, w, 3), casts, path_casts (h, w): the casts
    that are not shadow casts per pixel, paths, zero_paths, branch counters."""

    def __init__(self, oracle, geom, cam_pos, p, flags, rect=None, yaw_y=0.0, yaw_x=0.0):
        x0, y0, w, h = rect if rect is not None else (0, 0, p.width, p.height)
        tri_all = np.ascontiguousarray(geom.all_triangles(), np.float32)
        n_surf, n_light = geom.n_surf, geom.n_light
        ids = np.arange(n_light, dtype=np.int32)  # a light hit reports its triangle under both rules
        N = oracle.normals(tri_all) if len(tri_all) else np.zeros((0, 3), np.float32)
        T, B = normal_frame_np(N)
        albedo = np.asarray(geom.albedo, np.float32).reshape(-1, 3)
        brdf = albedo / PI
        Le = np.asarray(geom.emission, np.float32).reshape(-1, 3)
        cdf, kk = light_table_np(geom.light, geom.emission)
        last = last_light_np(cdf) if n_light else -1
        seed, spp, ts, env = int(p.seed), p.spp, f32(p.t_scale), f32(p.env_light)
        self.branch = dict.fromkeys(BRANCHES, 0)

        ys, xs, ss = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(spp), indexing="ij")
        px, py, smp = xs.ravel(), ys.ravel(), ss.ravel()
        pix = (py.astype(np.uint64) * np.uint64(p.width) + px.astype(np.uint64)).astype(np.uint32)
        n = len(pix)
        # the camera ray (rt_trace.hpp camera_ray<1>)
        wd = philox_np(pix, smp, 0, 0, seed)
        dr = np.stack([(px.astype(np.float32) + u01(wd[:, 0])) - f32(p.width) / f32(2.0),
                       (py.astype(np.float32) + u01(wd[:, 1])) - f32(p.height) / f32(2.0),
                       np.full(n, f32(p.height))], 1)
        dr = normalize3(dr)
        cy_, sy_ = f32(np.cos(np.float64(f32(yaw_y)))), f32(np.sin(np.float64(f32(yaw_y))))
        cx_, sx_ = f32(np.cos(np.float64(f32(yaw_x)))), f32(np.sin(np.float64(f32(yaw_x))))
        z, one = f32(0.0), f32(1.0)
        rx = (cy_ * dr[:, 0] + z * dr[:, 1]) + (-sy_ * dr[:, 2] + z * one)
        ry = (z * dr[:, 0] + one * dr[:, 1]) + (z * dr[:, 2] + z * one)
        rz = (sy_ * dr[:, 0] + z * dr[:, 1]) + (cy_ * dr[:, 2] + z * one)
        rw = (z * dr[:, 0] + z * dr[:, 1]) + (z * dr[:, 2] + one * one)
        d = np.stack([(one * rx + z * ry) + (z * rz + z * rw), (z * rx + cx_ * ry) + (sx_ * rz + z * rw),
                      (z * rx + -sx_ * ry) + (cx_ * rz + z * rw)], 1).astype(np.float32)
        o = np.tile(np.asarray(cam_pos[:3], np.float32), (n, 1))
        tp = np.ones((n, 3), np.float32)
        L = np.zeros((n, 3), np.float32)
        path_casts = np.zeros(n, np.int64)
        self.casts = 0
        alive = np.arange(n)
        depth = 0
        self.first_hit = None

        def cast(oo, dd):
            t, code = oracle.intersect(tri_all, n_surf, n_light, ids, oo, dd, float(ts), p.hit_rule)
            kind = np.where(code == -1, 0, (code >> 30) & 3)  # 0 miss, 1 light, 2 surface
            return t, kind, code & 0x3FFFFFFF

        while len(alive):
            t, kind, idx = cast(o, d)
            self.casts += len(alive)
            path_casts[alive] += 1
            if depth == 0:
                self.first_hit = np.where(kind == 0, -1, np.where(kind == 1, n_surf + idx, idx))
            miss, light, surf = kind == 0, kind == 1, kind == 2
            L[alive[miss]] = L[alive[miss]] + tp[miss] * env
            if depth == 0:
                L[alive[light]] = L[alive[light]] + tp[light] * Le[idx[light]]
                self.branch["light_seen_depth0"] += int(light.sum())
            else:
                self.branch["light_hit_deeper"] += int(light.sum())
            if depth + 1 == p.max_bounces:
                self.branch["cap"] += int(surf.sum())
                break
            alive, o, d, tp, t, tri = alive[surf], o[surf], d[surf], tp[surf], t[surf], idx[surf]
            if not len(alive):
                break
            D = d * ts
            pos = o + t[:, None] * D
            # the direct term
            if last >= 0:
                w4 = philox_np(pix[alive], smp[alive], 1 + depth, NEE_WORD, seed)
                l = pick_np(cdf, last, u01(w4[:, 0]))
                y, _, _ = light_point_np(geom.light, l, u01(w4[:, 1]), u01(w4[:, 2]))
                Lv = y - pos
                d2 = dot3(Lv, Lv)
                sd = normalize3(Lv)
                with np.errstate(invalid="ignore", divide="ignore"):
                    cx = dot3(N[tri], sd)
                    cy = np.abs(dot3(N[n_surf + l], sd))
                    ok = (d2 != 0) & (cx > 0) & (cy > 0)
                    g = ((cx * cy) / d2) * kk[l]
                self.branch["cx_skip"] += int(((d2 != 0) & ~(cx > 0)).sum())
                fac = ((tp * brdf[tri]) * Le[l]) * g[:, None]
                if ok.any():
                    so = pos[ok] + EPS * sd[ok]
                    _, sk, si = cast(so, sd[ok])
                    self.casts += int(ok.sum())
                    vis = (sk == 1) & (si == l[ok])
                    who = alive[ok][vis]
                    L[who] = L[who] + fac[ok][vis]
                    self.branch["visible"] += int(vis.sum())
                    self.branch["occluded"] += int((~vis).sum())
            if flags & 1:
                break
            # the preset's bounce (rt_paths.hpp surface_step)
            wb = philox_np(pix[alive], smp[alive], 1 + depth, 0, seed)
            r1, r2 = u01(wb[:, 0]), u01(wb[:, 1])
            if p.sampler == 0:
                ct, st = r1, np.sqrt(f32(1.0) - r1 * r1)
            else:
                ct, st = np.sqrt(r1), np.sqrt(f32(1.0) - r1)
            sphi, cphi = sincos_turn_np(r2)
            sx, sz = st * cphi, st * sphi
            sdir = (sx[:, None] * B[tri] + ct[:, None] * N[tri]) + sz[:, None] * T[tri]
            if p.sampler == 0:
                tp = ((tp * brdf[tri]) * ct[:, None]) / RHO
            else:
                tp = tp * albedo[tri]
            o = (pos + EPS * sdir).astype(np.float32)
            d = normalize3(sdir).astype(np.float32)
            depth += 1

        self.per_sample = L.reshape(h, w, spp, 3)
        self.path_casts = path_casts.reshape(h, w, spp).sum(axis=2)
        self.paths = n
        self.zero_paths = int((~L.any(axis=1)).sum())

    def image(self, split, spp):
        split = max(1, split)
        per = spp // split
        tot = None
        for c in range(split):
            acc = np.zeros(self.per_sample.shape[:2] + (3,), np.float32)
            for j in range(c * per, (c + 1) * per):
                acc = acc + self.per_sample[:, :, j]
            tot = acc if tot is None else tot + acc
        return tot / f32(spp)


def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def gpu_params(rtmi_mod, **kw):
    kw.setdefault("spp_split", 1)
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- CPU ----------

def test_the_restatements_pieces_are_the_pinned_ones(oracle_mod):
    """The vectorised Philox and sincos_turn against oracle.philox and oracle.sincos_turn (the camera
    rays against oracle.primary_hits: in the estimator's test)."""
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    ctr[0] = (0, 0, 0, 0)
    ctr[1] = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, NEE_WORD)
    seed = 0x0123456789ABCDEF
    got = philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
    for c, g in zip(ctr, got):
        assert np.array_equal(oracle_mod.philox(c, (seed & 0xFFFFFFFF, seed >> 32)), g)
    r = np.concatenate([u01(rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)),
                        np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875], np.float32)])
    s, c = sincos_turn_np(r)
    for ri, si, ci in zip(r, s, c):
        ws, wc = oracle_mod.sincos_turn(float(ri))
        assert bits(si) == bits(f32(ws)) and bits(ci) == bits(f32(wc)), ri


def crafted_lights():
    """(name, light triangles, emission): zero-area lights first, in the middle and last; a single
    light; two lights of unequal emission; 256 equal lights (boundaries at k / 256)."""
    tri = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32)
    flat = np.array([2, 2, 2, 3, 3, 3, 4, 4, 4], np.float32)  # collinear: no area
    big = np.array([0, 0, 1, 2, 0, 1, 0, 3, 1], np.float32)
    out = [("zero-area", np.stack([flat, tri, flat, big, tri + 5, flat]),
            np.array([[1, 1, 1], [1, 2, 3], [9, 9, 9], [0.5, 0.5, 0.5], [4, 0, 0], [1, 1, 1]], np.float32)),
           ("single", tri[None], np.array([[3, 2, 1]], np.float32)),
           ("unequal", np.stack([tri, tri + 1]), np.array([[1, 1, 1], [10, 20, 30]], np.float32)),
           ("black-and-lit", np.stack([tri, big]), np.array([[0, 0, 0], [1, 1, 1]], np.float32)),
           ("no-weight", np.stack([flat, tri]), np.array([[1, 1, 1], [0, 0, 0]], np.float32))]
    many = np.tile(tri, (256, 1))
    many[:, 2::3] += np.arange(256, dtype=np.float32)[:, None]
    out.append(("equal-256", many, np.ones((256, 3), np.float32)))
    return out


def light_lists(rtmi_mod):
    g1, g2 = geometry(rtmi_mod, "cornell"), geometry(rtmi_mod, "complex_light_room")
    return [("cornell", g1.light, g1.emission), ("complex_light_room", g2.light, g2.emission)] + crafted_lights()


def test_light_table_and_sampler_bit_for_bit(rtmi_mod):
    G = rtmi_mod.Geometry
    rng = np.random.default_rng(5)
    for name, lv, em in light_lists(rtmi_mod):
        geom = G(np.zeros((0, 9), np.float32), np.zeros((0, 3), np.float32), lv, em, np.zeros(len(lv), np.int32))
        cdf, k = rtmi_mod.nee_light_table(geom)
        wc, wk = light_table_np(lv, em)
        assert np.array_equal(bits(cdf), bits(wc)) and np.array_equal(bits(k), bits(wk)), name
        if name == "no-weight":
            assert not cdf.any() and not k.any()
        else:
            assert cdf[last_light_np(cdf)] == 1.0 and np.all(np.diff(cdf) >= 0)
        if name == "zero-area":
            assert cdf[0] == 0 and cdf[2] == cdf[1] and cdf[5] == cdf[4] and list(k[[0, 2, 5]]) == [0, 0, 0]
        n = 4096
        pix = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        s = rng.integers(0, 1 << 16, n).astype(np.uint32)
        depth = rng.integers(0, 80, n).astype(np.int32)
        for seed in (1984, 0xFEDCBA9876543210):
            li, y = rtmi_mod.nee_sample(lv, cdf, seed, pix, s, depth)
            wl, wy, u, v = sample_np(lv, cdf, seed, pix, s, depth)
            assert np.array_equal(li, wl) and np.array_equal(bits(y), bits(wy)), name
            if name == "no-weight":
                assert np.all(li == -1) and not y.any()
                continue
            assert np.all(k[li] > 0), name  # a light without weight is never chosen
            # y inside its triangle: barycentrics in [0, 1] to one ulp-scaled margin.  Solved in double from
            # the float32 point: each coordinate carries at most 3 roundings of magnitudes <= the triangle's
            # largest |coordinate| M, so the barycentrics move by at most 3 ulp(M) / (shortest edge) ~ 8 eps M / e
            t = lv[li].astype(np.float64)
            e1, e2, r = t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3], y.astype(np.float64) - t[:, 0:3]
            a11, a12, a22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
            b1, b2 = (r * e1).sum(1), (r * e2).sum(1)
            det = a11 * a22 - a12 * a12
            bu, bv = (b1 * a22 - b2 * a12) / det, (b2 * a11 - b1 * a12) / det
            M = np.abs(t).max(1)
            margin = 8 * 2.0 ** -24 * M / np.sqrt(np.minimum(a11, a22)) + 2.0 ** -24
            assert np.all(bu >= -margin) and np.all(bv >= -margin) and np.all(bu + bv <= 1 + margin), name


def test_sampler_boundaries(rtmi_mod):
    """r exactly on a CDF boundary goes to the light above it; r above the last boundary of a caller's
    cdf goes to the last light whose cdf rises."""
    name, lv, em = crafted_lights()[-1]
    assert name == "equal-256"
    cdf, _ = light_table_np(lv, em)
    assert np.array_equal(cdf, (np.arange(1, 257) / 256).astype(np.float32))
    # counters whose r = u01(w0) is a multiple of 1 / 256: 2^-16 of all
    seed = 7
    pix = np.arange(1 << 20, dtype=np.uint32)
    z = np.zeros_like(pix)
    r = u01(philox_np(pix, 3, 1, NEE_WORD, seed)[:, 0])
    on = np.nonzero((r * f32(256.0)) == np.floor(r * f32(256.0)))[0]
    assert 4 <= len(on) <= 64  # expected 16
    li, _ = rtmi_mod.nee_sample(lv, cdf, seed, pix[on], z[on] + 3, z[on].astype(np.int32))
    assert np.array_equal(li, (r[on] * f32(256.0)).astype(np.int32))  # r == cdf[l - 1] is not below it
    assert np.array_equal(li, sample_np(lv, cdf, seed, pix[on], z[on] + 3, z[on])[0])
    # a caller's cdf that ends below 1, flat at the end: light 1 catches the rest
    own = np.array([0.25, 0.5, 0.5], np.float32)
    li, _ = rtmi_mod.nee_sample(lv[:3], own, seed, pix[:4096], z[:4096] + 3, z[:4096].astype(np.int32))
    r = r[:4096]
    assert (r >= 0.5).sum() > 1000
    assert np.array_equal(li, np.where(r < 0.25, 0, 1))
    with pytest.raises(rtmi_mod.RtError):
        rtmi_mod.nee_sample(lv[:2], np.array([0.5, 0.25], np.float32), seed, pix[:1], z[:1], z[:1].astype(np.int32))


# the 1 - 1e-6 quantile of chi-square by degrees of freedom (those the lists below need)
CHI2_Q = {1: 23.92812697687947, 2: 27.631021115871036, 9: 44.81093787062026, 23: 70.54955713680532}


def test_sampler_distribution_chi_square(rtmi_mod):
    """2^16 samples per list at a fixed seed: the light choice against its weights, and per light
    the point's barycentrics (u, v) over a 4 x 4 grid: the six cells below the diagonal u + v = 1 hold
    2/16 each, the four on it 1/16, the rest nothing (9 degrees of freedom).  The restatement is tested;
    the library's samples are its samples, bit for bit."""
    n = 1 << 16
    pix = np.arange(n, dtype=np.uint32) * np.uint32(2654435761)
    s = (np.arange(n) % 64).astype(np.uint32)
    depth = (np.arange(n) % 5).astype(np.int32)
    cell_p = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            cell_p[i, j] = 2 / 16 if i + j < 3 else (1 / 16 if i + j == 3 else 0.0)
    for name, lv, em in light_lists(rtmi_mod):
        if name in ("no-weight", "equal-256"):
            continue
        cdf, k = light_table_np(lv, em)
        li, y, u, v = sample_np(lv, cdf, 1984, pix, s, depth)
        got = rtmi_mod.nee_sample(lv, cdf, 1984, pix, s, depth)
        assert np.array_equal(got[0], li) and np.array_equal(bits(got[1]), bits(y))
        prob = np.diff(np.concatenate([[0.0], cdf.astype(np.float64)]))
        lit = prob > 0
        cnt = np.bincount(li, minlength=len(cdf))
        assert not cnt[~lit].any()
        if lit.sum() > 1:
            x2 = (((cnt[lit] - n * prob[lit]) ** 2) / (n * prob[lit])).sum()
            assert x2 < CHI2_Q[int(lit.sum()) - 1], (name, x2)
        for l in np.nonzero(lit)[0]:
            m = li == l
            if m.sum() < 1600:  # expected counts below 100 per cell of 16: too few to test
                continue
            iu = np.minimum((u[m] * 4).astype(int), 3)
            iv = np.minimum((v[m] * 4).astype(int), 3)
            c = np.zeros((4, 4))
            np.add.at(c, (iu, iv), 1)
            # (u + v == 1 exactly lands in a zero-area cell's corner at most: folded in with its neighbour)
            live = cell_p > 0
            assert c[~live].sum() <= 2, (name, l)
            e = m.sum() * cell_p[live]
            x2 = ((c[live] - e) ** 2 / e).sum()
            assert x2 < CHI2_Q[9], (name, l, x2)


# the estimator's definition against the pinned renderer: Cornell 24 x 24, 32 seeds x 64 spp
EST = dict(width=24, height=24, spp=64, max_bounces=4)
EST_SEEDS = tuple(range(500, 532))


def block_means(img, b):
    h, w, _ = img.shape
    return img.astype(np.float64).reshape(h // b, b, w // b, b, 3).mean(axis=(1, 3))


def z_scores(a, b):
    """per block and channel: (mean_a - mean_b) / standard error of the difference over the seeds"""
    a, b = np.asarray(a), np.asarray(b)
    d = a - b
    se = d.std(axis=0, ddof=1) / np.sqrt(d.shape[0])
    m = d.mean(axis=0)
    return np.where(se > 0, m / np.where(se > 0, se, 1), np.where(m == 0, 0.0, np.inf))


@functools.lru_cache(maxsize=None)
def pinned_blocks():
    import oracle
    import rtmi
    geom = geometry(rtmi, "cornell")
    out = []
    for seed in EST_SEEDS:
        p = gpu_params(rtmi, seed=seed, **EST)
        img, _ = oracle.render(geom, oracle.camera(rtmi.CAMERAS["cornell"]), oracle.params_from(p))
        out.append(block_means(img, 8))
    return np.array(out)


def test_estimator_has_the_renderers_expectation(rtmi_mod, oracle_mod):
    """The restated NEE image against oracle.render at the same max_bounces = 4: every 8 x 8 block
    and channel mean within |z| < 4.5 (standard error over the 32 seeds); and the direct-only
    restatement differs by z > 10 somewhere, so the comparison has power."""
    geom = geometry(rtmi_mod, "cornell")
    cam = rtmi_mod.CAMERAS["cornell"]
    full, direct = [], []
    for i, seed in enumerate(EST_SEEDS):
        p = gpu_params(rtmi_mod, seed=seed, **EST)
        r = Restated(oracle_mod, geom, cam, p, 0)
        full.append(block_means(r.image(1, p.spp), 8))
        if i == 0:  # the restated camera rays are the pinned ones
            hits = oracle_mod.primary_hits(geom.all_triangles(), geom.n_surf, geom.n_light, oracle_mod.camera(cam),
                                           oracle_mod.params_from(p), (0, 0, p.width, p.height), 0, p.spp)
            assert np.array_equal(r.first_hit.reshape(hits.shape), hits)
        if i < 8:
            d = Restated(oracle_mod, geom, cam, p, rtmi_mod.RT_NEE_DIRECT_ONLY)
            direct.append(block_means(d.image(1, p.spp), 8))
    ref = pinned_blocks()
    z = z_scores(full, ref)
    assert np.all(np.abs(z) < 4.5), np.abs(z).max()
    zd = z_scores(direct, ref[:8])
    assert np.abs(zd).max() > 10, np.abs(zd).max()


def test_abi_defines_and_refusals(rtmi_mod):
    src = open(os.path.join(os.path.dirname(PKG), "include", "rtmi.h")).read()
    assert "#define RT_NEE_DIRECT_ONLY 1" in src and rtmi_mod.RT_NEE_DIRECT_ONLY == 1
    assert "#define RT_KT_COUNT 11" in src and rtmi_mod.RT_KT_COUNT == 11
    L = rtmi_mod.lib()
    cam = rtmi_mod.camera()
    p = gpu_params(rtmi_mod, width=16, height=16)
    out = np.zeros((16, 16, 3), np.float32)
    fp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    one = ctypes.c_void_p(1)  # never dereferenced: every call below is refused before it looks
    args = lambda **kw: [kw.get("ctx", one), kw.get("scene", one), kw.get("cam", ctypes.byref(cam)),
                         kw.get("params", ctypes.byref(p)), kw.get("flags", 0), 0, 0, 16, 16, kw.get("out", fp), None, None]
    for bad in ("ctx", "scene", "cam", "out"):
        assert L.rt_render_nee(*args(**{bad: None})) == -1 and b"NULL" in L.rt_last_error(), bad
    assert L.rt_render_nee(*args(params=None)) == -1 and b"params is NULL" in L.rt_last_error()
    for flags in (2, 3, -1):
        assert L.rt_render_nee(*args(flags=flags)) == -1 and b"flags" in L.rt_last_error()
    pc = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, width=16, height=16)
    assert L.rt_render_nee(*args(params=ctypes.byref(pc))) == -5 and b"GPU preset" in L.rt_last_error()
    bad_split = gpu_params(rtmi_mod, width=16, height=16, spp=6, spp_split=4)
    assert L.rt_render_nee(*args(params=ctypes.byref(bad_split))) == -1 and b"spp_split" in L.rt_last_error()
    a = args()
    a[7] = 17
    assert L.rt_render_nee(*a) == -1 and b"rectangle" in L.rt_last_error()
    t = (ctypes.c_int32 * 2)(0, 0)
    tiles = lambda **kw: [kw.get("ctx", one), one, ctypes.byref(cam), kw.get("params", ctypes.byref(p)), kw.get("flags", 0),
                          kw.get("tiles", t), kw.get("n", 1), kw.get("size", 16), kw.get("out", one), None, None, None]
    assert L.rt_render_nee_tiles_device(*tiles(ctx=None)) == -1
    assert L.rt_render_nee_tiles_device(*tiles(flags=4)) == -1 and b"flags" in L.rt_last_error()
    assert L.rt_render_nee_tiles_device(*tiles(params=ctypes.byref(pc))) == -5
    assert L.rt_render_nee_tiles_device(*tiles(n=0)) == 0
    assert L.rt_render_nee_tiles_device(*tiles(out=None)) == -1
    assert L.rt_render_nee_tiles_device(*tiles(size=24)) == -1 and b"tile_size" in L.rt_last_error()
    assert L.rt_nee_light_table(None, None, 2, None, None) == -1 and L.rt_nee_light_table(None, None, 0, None, None) == 0
    assert L.rt_nee_light_table(None, None, -1, None, None) == -1
    assert L.rt_nee_sample(None, None, 1, 0, None, None, None, 3, None, None) == -1
    assert L.rt_nee_sample(None, None, 0, 0, None, None, None, 0, None, None) == 0


# ---------------------------------------------------------------- GPU ----------

# (id, scene, hit rule, t_scale or None for the default, exact BVH, expected route)
ROUTE_CASES = [
    ("cornell-table1", "cornell", 1, None, False),            # the table route, one mask word
    ("complex-table4", "complex_light_room", 1, None, False),  # four mask words, many lights
    ("cornell-bvh", "cornell", 1, None, True),
    ("cornell-rule0-scan", "cornell", 0, 64.0, False),         # no table below t_scale 256: the scan route
]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,rule,t_scale,bvh", [c[1:] for c in ROUTE_CASES], ids=[c[0] for c in ROUTE_CASES])
def test_bit_for_bit_against_the_restatement(rtmi_mod, oracle_mod, gpu_ctx, scene, rule, t_scale, bvh):
    """Image, cast count and both stats, 24 x 20 (not a multiple of 16: the clip), spp 4 at split 1
    and 2, max_bounces 1, 2, 4, both samplers, flags 0 and RT_NEE_DIRECT_ONLY, env_light 0 and
    0.25; and every branch of the definition reached over these, by the restatement's counters."""
    geom = geometry(rtmi_mod, scene)
    assert geom.n_tri <= 64 if scene == "cornell" else 64 < geom.n_tri <= 256
    cam_pos = rtmi_mod.CAMERAS[scene]
    cam = rtmi_mod.camera(cam_pos)
    reached = dict.fromkeys(BRANCHES, 0)
    kw = {} if t_scale is None else {"t_scale": t_scale}
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        if bvh:
            sc.set_accel(rtmi_mod.ACCEL_BVH)
        for mb in (1, 2, 4):
            for sampler in (0, 1):
                for flags in (0, rtmi_mod.RT_NEE_DIRECT_ONLY):
                    for env in (0.0, 0.25):
                        p = gpu_params(rtmi_mod, width=24, height=20, spp=4, max_bounces=mb, sampler=sampler,
                                       hit_rule=rule, env_light=env, **kw)
                        want = Restated(oracle_mod, geom, cam_pos, p, flags)
                        for k in BRANCHES:
                            reached[k] += want.branch[k]
                        for split in (1, 2):
                            p.spp_split = split
                            img, casts, st = rtmi_mod.render_nee(gpu_ctx, sc, cam, p, flags, stats=True)
                            tag = (mb, sampler, flags, env, split)
                            assert np.array_equal(bits(img), bits(want.image(split, p.spp))), tag
                            assert casts == want.casts, tag
                            assert st == {"paths": want.paths, "zero_paths": want.zero_paths}, tag
        if not bvh and t_scale is None:
            assert sc.ctab_info(rule)["built"]  # the table route was taken
        if t_scale is not None:
            assert not sc.ctab_info(rule)["built"]
    assert all(reached[k] > 0 for k in BRANCHES), reached


def without_lights(rtmi_mod, geom, keep_black):
    G = rtmi_mod.Geometry
    tri, alb = geom.tri, geom.albedo
    if keep_black:
        tri = np.concatenate([geom.tri, geom.light], 0)
        alb = np.concatenate([geom.albedo, np.zeros((geom.n_light, 3), np.float32)], 0)
    return G(np.ascontiguousarray(tri), np.ascontiguousarray(alb), np.zeros((0, 9), np.float32),
             np.zeros((0, 3), np.float32), np.zeros(0, np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("keep_black", [False, True])
def test_no_lights_equals_rt_render(rtmi_mod, gpu_ctx, keep_black):
    geom = without_lights(rtmi_mod, geometry(rtmi_mod, "cornell"), keep_black)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"])
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        for sampler, split in ((0, 1), (1, 4)):
            p = gpu_params(rtmi_mod, width=24, height=20, spp=8, spp_split=split, max_bounces=5, env_light=1.0,
                           sampler=sampler)
            a, ca = rtmi_mod.render(gpu_ctx, sc, cam, p)
            b, cb, st = rtmi_mod.render_nee(gpu_ctx, sc, cam, p, 0, stats=True)
            assert np.array_equal(bits(a), bits(b)) and ca == cb
            assert st["paths"] == 24 * 20 * 8 and a.any()


@pytest.mark.gpu
def test_same_paths_as_rt_render(rtmi_mod, oracle_mod, gpu_ctx):
    """With lights, flags 0 and the same seed the NEE frame's casts that are not shadow casts are
    rt_render's paths: per 8 x 8 pixel block at least rt_render's cast count -- and in fact equal,
    since a light hit ends both paths and nothing else ends either; both from the restatements,
    whose totals are the device's."""
    geom = geometry(rtmi_mod, "cornell")
    cam_pos = rtmi_mod.CAMERAS["cornell"]
    p = gpu_params(rtmi_mod, width=24, height=20, spp=4, max_bounces=6)
    want = Restated(oracle_mod, geom, cam_pos, p, 0)
    total_plain = 0
    for y in range(0, 20, 8):
        for x in range(0, 24, 8):
            h = min(8, 20 - y)
            _, c = oracle_mod.render(geom, oracle_mod.camera(cam_pos), oracle_mod.params_from(p), (x, y, 8, h))
            mine = int(want.path_casts[y:y + h, x:x + 8].sum())
            assert mine >= c and mine == c, (x, y, mine, c)
            total_plain += c
    assert want.casts > total_plain  # shadow casts were taken
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        cam = rtmi_mod.camera(cam_pos)
        _, c_nee = rtmi_mod.render_nee(gpu_ctx, sc, cam, p)
        _, c_plain = rtmi_mod.render(gpu_ctx, sc, cam, p)
    assert c_nee == want.casts and c_plain == total_plain


@pytest.mark.gpu
def test_tile_render_equals_rect_render(rtmi_mod, gpu_ctx):
    torch = pytest.importorskip("torch")
    geom = geometry(rtmi_mod, "cornell")
    W, H, T = 96, 64, 32
    p = gpu_params(rtmi_mod, width=W, height=H, spp=8, spp_split=2, max_bounces=4)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"])
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        full, casts_full, st_full = rtmi_mod.render_nee(gpu_ctx, sc, cam, p, 0, stats=True)
        world = 2  # the diagonal deal
        k = rtmi_mod.tiles.tiles_per_rank(W, H, T, world)
        gathered = np.zeros((world, k, T, T, 3), np.float32)
        casts = torch.zeros(1, dtype=torch.int64, device="cuda")
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for rank in range(world):
            idx = rtmi_mod.tiles.rank_tile_indices(W, H, T, rank, world)
            tiles = rtmi_mod.tiles.tile_origins(W, H, T)[idx]
            out = torch.zeros((len(tiles), T, T, 3), dtype=torch.float32, device="cuda")
            rtmi_mod.render_nee_tiles_device(gpu_ctx, sc, cam, p, 0, tiles, T, out.data_ptr(), casts.data_ptr(),
                                             stats.data_ptr(), stream)
            torch.cuda.synchronize()
            gathered[rank, :len(tiles)] = out.cpu().numpy()
    img = rtmi_mod.tiles.assemble(gathered, W, H, T, world)
    assert np.array_equal(bits(img), bits(full))
    assert int(casts.item()) == casts_full
    assert {"paths": int(stats[0].item()), "zero_paths": int(stats[1].item())} == st_full


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "door_room"])
def test_same_expectation_on_the_device(rtmi_mod, gpu_ctx, scene):
    """rt_render_nee against rt_render themselves, 48 x 48 with 16 x 16 blocks, max_bounces 4, 32 seeds
    x 64 spp: |z| < 4.5 everywhere; the direct-only frame exceeds z = 10 somewhere."""
    geom = geometry(rtmi_mod, scene)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS[scene])
    nee, plain, direct = [], [], []
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        for seed in EST_SEEDS:
            p = gpu_params(rtmi_mod, width=48, height=48, spp=64, max_bounces=4, seed=seed)
            nee.append(block_means(rtmi_mod.render_nee(gpu_ctx, sc, cam, p)[0], 16))
            plain.append(block_means(rtmi_mod.render(gpu_ctx, sc, cam, p)[0], 16))
            direct.append(block_means(rtmi_mod.render_nee(gpu_ctx, sc, cam, p, rtmi_mod.RT_NEE_DIRECT_ONLY)[0], 16))
    z = z_scores(nee, plain)
    print(f"{scene}: max |z| {np.abs(z).max():.2f}, direct-only max |z| {np.abs(z_scores(direct, plain)).max():.1f}")
    assert np.all(np.abs(z) < 4.5), np.abs(z).max()
    assert np.abs(z_scores(direct, plain)).max() > 10


@pytest.mark.gpu
def test_lower_variance_on_cornell(rtmi_mod, gpu_ctx):
    """Cornell 64 x 64, 16 spp, 8 seeds, the preset's 80 bounces: the per-pixel variance across the
    seeds, averaged over the image, is lower with next-event estimation than without (the ratio is
    printed and recorded in DESIGN.md section 7)."""
    geom = geometry(rtmi_mod, "cornell")
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"])
    a, b = [], []
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        for seed in range(8):
            p = gpu_params(rtmi_mod, width=64, height=64, spp=16, seed=900 + seed)
            a.append(rtmi_mod.render_nee(gpu_ctx, sc, cam, p)[0].astype(np.float64))
            b.append(rtmi_mod.render(gpu_ctx, sc, cam, p)[0].astype(np.float64))
    v_nee, v_plain = np.var(a, axis=0, ddof=1).mean(), np.var(b, axis=0, ddof=1).mean()
    print(f"variance: NEE {v_nee:.6g}, rt_render {v_plain:.6g}, ratio {v_nee / v_plain:.4f}")
    assert v_nee < v_plain


NEE_REF_SPP = 16


@pytest.mark.gpu
def test_cornell_matches_reference_render(rtmi_mod):
    """The reference's own GPU-engine render (Images/cornell/reference.png, 720 x 720, 4096 spp; block
    means in tests/golden/cornell_ref_stats.json) against the NEE frame, with the bounds
    test_gpu_preset_cornell_matches_reference_render has for the default render: mean |d| <= 0.5,
    max <= 3.0 of 255, image mean within 0.2 %.  At 16 spp, the smallest power of two at which the
    measured values are at most half the bounds: mean |d| 0.198, max 1.34, image mean 51.511 against
    51.553 (0.082 %).  At 8 spp: 0.269, 1.64, 0.048 % (the mean |d| above half its bound); at 32:
    0.162, 0.90, 0.054 %; at 256: 0.103, 0.56, 0.038 %.  rt_render at 16 spp: 6.82, 35.9, 12.7 %; it
    needs 1024 spp for 0.21."""
    ref = np.array(json.load(open(os.path.join(GOLDEN, "cornell_ref_stats.json")))["reference.png"]["means"])
    geom = geometry(rtmi_mod, "cornell")
    p = gpu_params(rtmi_mod, width=720, height=720, spp=NEE_REF_SPP, spp_split=16)
    with rtmi_mod.Context(0) as ctx, rtmi_mod.Scene(ctx, geom) as sc:
        img, _ = rtmi_mod.render_nee(ctx, sc, rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"]), p)
    rgb8 = rtmi_mod.metrics.argb_to_rgb8(rtmi_mod.pack_argb(img)).astype(np.float64)
    ours = rgb8.reshape(16, 45, 16, 45, 3).mean(axis=(1, 3))
    d = np.abs(ours - ref)
    print(f"spp {NEE_REF_SPP}: mean |d| {d.mean():.4f}, max {d.max():.4f}, image mean {ours.mean():.4f} vs {ref.mean():.4f}")
    assert d.mean() <= 0.5 and d.max() <= 3.0, (d.mean(), d.max())
    assert abs(ours.mean() - ref.mean()) <= 0.002 * ref.mean()


@pytest.mark.gpu
@pytest.mark.parametrize("direct_only", [0, 1])
def test_facade_equals_c_abi(rtmi_mod, gpu_ctx, tmp_path, direct_only):
    """examples/next_event_main.cpp (draw_next_event_path_tracing): its BMP is the C ABI's frame."""
    exe = os.path.join(PKG, "build", "next_event_demo")
    assert os.path.exists(exe), f"{exe} missing: make -C {PKG}"
    out = str(tmp_path / "nee.bmp")
    r = subprocess.run([exe, out, "4", str(direct_only), "64"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 4 * 64 * 64
    got = np.frombuffer(raw[54:], dtype="<u4").reshape(64, 64)
    geom = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)  # get_cornell_shapes of the facade
    p = gpu_params(rtmi_mod, width=64, height=64, spp=4)
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        img, _ = rtmi_mod.render_nee(gpu_ctx, sc, rtmi_mod.camera((0.0, 0.0, -3.0, 1.0)), p, direct_only)
    assert img.any() and np.array_equal(got, rtmi_mod.pack_argb(img))
