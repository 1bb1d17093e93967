"""Expected-value sweeps of the radiance map: rt_sarsa_sweep and rt_sarsa_forget (include/rtmi.h).

  * the deposit of a sweep against its restatement, bit for bit: numpy float32 on entries other
    tests pin (the probe's first directions, oracle.intersect's hits, the map's nearest-volume
    query), on every (spp, hit rule, env_light, range) case, every sector compared;
  * the fold: sweep(apply=True) == sweep(apply=False) + apply(); after forget() Q is the mean of
    the sweep's own targets; without it the visit-weighted mean; forget() moves visits only;
  * invariance of the pending sums under the split of the range, its order, the cast route, the
    search mode, spp_split and a second run; and that a sweep reads the irradiance estimates as
    they stood when it started (Jacobi);
  * rtmi.dist.sarsa_sweep at world size 1 and its two-rank split emulated on one GPU;
  * propagation: from a map at the floor, sweep 1 lifts exactly the sectors that see a light or
    the environment, sweep 2 some sector that sees a surface;
  * the argument checks; the C++ facade's sweep mode;
  * a swept map as a sampler (lower error than a fresh map's, unbiased) and its sector
    distributions against ground truth.
The small map is door_room at area_per_sample 0.1 (344 volumes; several surfaces carry none, so
the search's fallback to volume 0 takes part); Cornell serves the CPU hit rule's one-word
candidate table and, open at the front, the miss targets: no cast from a door_room volume leaves
that room under the GPU hit rule (CLOSED below; measured, and asserted in every case).  Before a
sweep the maps get seeded random Q rows (rm.write): on a fresh map every volume of a surface holds
one irradiance estimate, and a wrong nearest volume would pass.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import MODELS, PKG, ROOT

SEED = 1984
AREA = 0.1
S = 144
f32 = np.float32
THRESHOLD = f32(1.0) / (f32(12.0) * f32(12.0)) * f32(0.8)  # RADIANCE_THRESHOLD
IRR_SCALE = (f32(2.0) * f32(np.pi)) / f32(144.0)            # get_irradiance_estimate's 2 pi / 144
# The sampler tests' schedule, read from tools/sweep_map.py's curves (DESIGN.md section 7,
# "Expected-value sweeps"): from the issue's starting point, 8 replace sweeps of 8 casts, the frozen
# render's error falls for one sweep and then rises above the fresh map's, at 8, 32 and 64 casts per
# sweep alike; plain sweeps (the first replaces by itself: a fresh map has no visits) stop falling
# after the fifth, plus two: seven plain sweeps of 8 casts per sector, each with fresh samples
SWEEPS = 0
MEAN_SWEEPS = 7
SWEEP_SPP = 8


def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def gpu_params(rtmi_mod, **kw):
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, **kw)


# ---------------------------------------------------------------- CPU ----------

def test_new_symbols_are_exported(rtmi_mod):
    lib = rtmi_mod.lib()
    for name in ("rt_sarsa_sweep", "rt_sarsa_forget"):
        assert hasattr(lib, name), name
        assert name in rtmi_mod._lib.EXPORTS
    assert len(lib.rt_sarsa_sweep.argtypes) == 10 and len(lib.rt_sarsa_forget.argtypes) == 4
    assert hasattr(rtmi_mod.sarsa.RadianceMap, "sweep") and hasattr(rtmi_mod.sarsa.RadianceMap, "forget")
    from rtmi import dist as rdist
    assert callable(rdist.sarsa_sweep)


def header_define(name):
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    m = re.search(r"^#define\s+%s\s+(-?\d+)" % name, src, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_constants_agree(rtmi_mod):
    """include/rtmi.h, the binding and INTEGRATION.md agree on what a sweep needs: the TD modes, the
    timing slot k_sweep shares with k_bake (RT_KT_COUNT stays), and the entries' names"""
    sarsa = rtmi_mod.sarsa
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for name, value in (("RT_SARSA_TD_FRAME", sarsa.TD_FRAME), ("RT_SARSA_TD_INFRAME", sarsa.TD_INFRAME),
                        ("RT_SARSA_TD_OFF", sarsa.TD_OFF)):
        assert header_define(name) == value
    assert header_define("RT_KT_BAKE") == rtmi_mod.RT_KT_BAKE == 10
    assert header_define("RT_KT_COUNT") == rtmi_mod.RT_KT_COUNT == 11
    line = re.search(r"^#define\s+RT_KT_BAKE\s.*$", hdr, flags=re.M).group(0)
    assert "k_sweep" in line and "k_bake" in line
    assert sarsa.SECTORS == S
    assert "rt_sarsa_sweep" in doc and "rt_sarsa_forget" in doc and "RT_SARSA_TD_FRAME" in doc


def test_sweep_and_forget_refuse_null(rtmi_mod):
    lib = rtmi_mod.lib()
    p = gpu_params(rtmi_mod, spp=1)
    assert lib.rt_sarsa_sweep(None, None, None, ctypes.byref(p), 0, 0, 0, 1, None, None) == rtmi_mod._lib.RT_E_INVALID
    assert b"NULL" in lib.rt_last_error()
    assert lib.rt_sarsa_forget(None, 0, 0, None) == rtmi_mod._lib.RT_E_INVALID
    assert b"NULL" in lib.rt_last_error()


# ---------------------------------------------------------------- GPU ----------

def dot3(a, b):
    """the kernels' dot: (x + y) + z of the float32 products"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    """the kernels' normalize: v * (1 / sqrt(dot(v, v)))"""
    inv = f32(1.0) / np.sqrt(dot3(v, v))
    return v * inv[..., None]


def pending(rm):
    """the map's pending TD sums and counts, copied to the host as (n, 144)"""
    import torch
    from rtmi import dist as rdist
    s, c = rdist.td_tensors(rm, torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s.cpu().numpy().reshape(-1, S).copy(), c.cpu().numpy().reshape(-1, S).copy()


def same_maps(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


MISS, LIGHT, SURF = 0, 1, 2


class World:
    """A scene, the placement of its small map, seeded random Q rows and, per (hit rule, sample),
    the restated cast of every (volume, sector): computed once, shared, never changed."""

    def __init__(self, rtmi_mod, oracle_mod, ctx, scene, area=AREA):
        self.rtmi, self.oracle, self.ctx, self.name, self.area = rtmi_mod, oracle_mod, ctx, scene, area
        self.g = geometry(rtmi_mod, scene)
        self.sc = rtmi_mod.Scene(ctx, self.g)
        self.cam = rtmi_mod.camera(rtmi_mod.CAMERAS[scene])
        self.normals = self.sc.normals().reshape(-1, 3)  # the scene's stored normals, by triangle
        with self.new_map(written=False) as rm:
            self.n = rm.n_volumes
            self.pos, self.nrm, self.surf, _ = rm.volumes()
            self.fresh = rm.read()
        rng = np.random.default_rng(SEED)
        self.q0 = rng.uniform(0.05, 2.0, (self.n, S)).astype(np.float32)
        self.v0 = rng.integers(1, 9, (self.n, S)).astype(np.uint32)
        with self.new_map() as rm:
            self.start = rm.read()
        assert np.array_equal(self.start[0], self.q0) and np.array_equal(self.start[2], self.v0)
        self.irr = self.start[3]
        assert len(np.unique(self.irr)) > self.n // 2, "the irradiance estimates must differ from volume to volume"
        alb = np.asarray(self.g.albedo, np.float32)[self.surf]
        lum = f32(0.5) * (alb.max(axis=1) + alb.min(axis=1))  # Material luminance
        self.brdf = (lum / f32(np.pi)).astype(np.float32)
        em = np.asarray(self.g.emission, np.float32)
        self.light_lum = (f32(0.5) * (em.max(axis=1) + em.min(axis=1))).astype(np.float32)
        self._casts = {}

    def new_map(self, written=True):
        rm = self.rtmi.sarsa.RadianceMap(self.ctx, self.sc, SEED, self.area)
        if written:
            rm.write(self.q0, self.v0)
        return rm

    def cast(self, rule, t_scale, s):
        """sample s of every (volume, sector): kind (n, 144), the light's luminance where a light was
        hit, the hit surface and the nearest volume where a surface was"""
        key = (rule, float(t_scale), s)
        if key in self._casts:
            return self._casts[key]
        g, n = self.g, self.n
        p = gpu_params(self.rtmi, spp=1, max_bounces=1)
        dr = self.rtmi.probe.radiance(self.ctx, self.sc, p, self.pos, self.surf, np.arange(n), first_sample=s,
                                      want_irr=False, want_dir=True)["dir"]
        assert dr.dtype == np.float32 and dr.shape == (n, S, 3) and np.isfinite(dr).all()
        o = (self.pos[:, None, :] + dr * f32(1e-5)).reshape(-1, 3)
        d = normalize3(dr).reshape(-1, 3)
        t, hit = self.oracle.intersect(g.all_triangles(), g.n_surf, g.n_light, g.light_group, o, d, t_scale, rule)
        kind = np.full(n * S, SURF, np.int8)
        kind[hit == -1] = MISS
        light = (hit != -1) & ((hit >> 30) & 3 == 1)
        kind[light] = LIGHT
        idx = hit & 0x3FFFFFFF
        llum = np.zeros(n * S, np.float32)
        for li in np.unique(idx[light]):
            # rule 1 names the light triangle, rule 0 the light plane, whose triangles share one emission
            grp = self.light_lum[[li]] if rule == 1 else self.light_lum[g.light_group == li]
            assert len(grp) and np.all(grp == grp[0])
            llum[light & (idx == li)] = grp[0]
        surf = kind == SURF
        assert (idx[surf] < g.n_surf).all()
        # the hit point as the kernels form it: o + t * (d * t_scale), float32, unfused
        D = d[surf] * f32(t_scale)
        pt = o[surf] + t[surf, None] * D
        assert pt.dtype == np.float32
        with self.new_map(written=False) as rm:
            near = rm.nearest(pt, self.normals[idx[surf]])
        u = np.zeros(n * S, np.int64)
        u[surf] = near
        hs = np.full(n * S, -1, np.int64)
        hs[surf] = idx[surf]
        out = {"kind": kind.reshape(n, S), "llum": llum.reshape(n, S), "u": u.reshape(n, S), "hs": hs.reshape(n, S)}
        self._casts[key] = out
        return out

    def targets(self, rule, t_scale, s, env, irr=None):
        """the float32 TD target of sample s of every (volume, sector), and its cast"""
        c = self.cast(rule, t_scale, s)
        irr = self.irr if irr is None else irr
        b = self.brdf[:, None]
        tgt = np.where(c["kind"] == MISS, b * f32(env),
                       np.where(c["kind"] == LIGHT, b * c["llum"], (irr[c["u"]] * IRR_SCALE) * b))
        assert tgt.dtype == np.float32
        return tgt, c

    def deposit(self, p, first=0, irr=None):
        """the pending sums (int64) of a whole-map sweep: np.rint of the float32 product, summed"""
        tot = np.zeros((self.n, S), np.int64)
        for s in range(first, first + p.spp):
            tgt, _ = self.targets(p.hit_rule, p.t_scale, s, p.env_light, irr)
            fx = tgt * f32(4294967296.0)
            assert fx.dtype == np.float32
            tot += np.rint(fx).astype(np.int64)
        return tot

    def close(self):
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(rtmi_mod, oracle_mod, gpu_ctx):
    made = {}

    def get(scene, area=AREA):
        if (scene, area) not in made:
            made[(scene, area)] = World(rtmi_mod, oracle_mod, gpu_ctx, scene, area)
        return made[(scene, area)]

    yield get
    for w in made.values():
        w.close()


DEPOSIT_CASES = [(scene, spp, rule, env)
                 for scene, rules in (("door_room", (1, 0)),)
                 for spp in (1, 5, 8)
                 for rule in rules
                 for env in (0.0, 0.75)] + [("cornell", 8, 0, 0.5), ("cornell", 5, 0, 0.0),
                                            ("cornell", 1, 1, 0.75), ("cornell", 5, 1, 0.75), ("cornell", 8, 0, 0.75)]
# Whether a cast from a volume can leave the scene.  Under the GPU hit rule door_room is closed to
# its volumes: none of the casts of its 344-volume map misses, at any sample, so those env_light
# cases exercise no miss target (and check that the environment then adds nothing); under the CPU
# hit rule some of its casts miss, and the Cornell box is open at the front: there the env_light
# cases must contain miss targets.
CLOSED = {("door_room", 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("scene,spp,rule,env", DEPOSIT_CASES)
def test_gpu_deposit_equals_its_restatement(rtmi_mod, worlds, scene, spp, rule, env):
    """pending sums and counts of sweep(apply=False) == the restatement, every sector, bit for bit;
    the casts; Q, CDF, visits and irradiance untouched; nothing pending outside the range.  Ranges:
    the whole map, one volume, and [7, 7 + 130) (v0 != 0, no multiple of 64)."""
    w = worlds(scene)
    p = gpu_params(rtmi_mod, spp=spp, hit_rule=rule, env_light=env)
    want = w.deposit(p)
    # the case must be able to fail: a miss where the environment shines, a light, and one volume
    # seeing two different volumes of one surface
    tgt, c = w.targets(rule, p.t_scale, 0, env)
    misses = any((w.cast(rule, p.t_scale, s)["kind"] == MISS).any() for s in range(spp))
    assert misses == ((scene, rule) not in CLOSED), "the scene's openness is not what CLOSED says"
    if env > 0 and misses:
        assert (tgt[c["kind"] == MISS] > 0).any(), "no miss target: the case checks nothing"
    assert (c["kind"] == LIGHT).any() and (tgt[c["kind"] == LIGHT] > 0).any(), "no light target"
    two = False
    for v in range(w.n):
        sf = c["kind"][v] == SURF
        for j in np.unique(c["hs"][v][sf]):
            two = two or len(np.unique(tgt[v][sf & (c["hs"][v] == j)])) >= 2
        if two:
            break
    assert two, "no two distinct surface targets on one surface: a wrong nearest volume would pass"
    assert w.n > 7 + 130
    for v0, n in ((0, w.n), (w.n - 3, 1), (7, 130)):
        inr = np.zeros(w.n, bool)
        inr[v0:v0 + n] = True
        with w.new_map() as rm:
            casts = rm.sweep(w.sc, p, v0, n, apply=False)
            ps, pc = pending(rm)
            after = rm.read()
        assert casts == n * S * spp, (v0, n)
        assert same_maps(after, w.start), (v0, n)
        assert not ps[~inr].any() and not pc[~inr].any(), (v0, n)
        assert (pc[inr] == spp).all(), (v0, n)
        bad = ps[inr] != want[inr]
        assert np.array_equal(ps[inr], want[inr]), (v0, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def applied(w, q_old, vis_old, sums, counts):
    """k_sarsa_apply's fold in float32: (q_old * visits + f32(S 2^-32)) / (visits + n), floored"""
    s32 = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32)
    q = (q_old * vis_old.astype(np.float32) + s32) / (vis_old + counts.astype(np.uint32)).astype(np.float32)
    assert q.dtype == np.float32
    return np.where(q > THRESHOLD, q, THRESHOLD).astype(np.float32)


@pytest.mark.gpu
def test_gpu_apply_and_forget(rtmi_mod, worlds):
    """sweep(apply=True) is sweep(apply=False) then apply(); after forget() Q is the floored mean of
    the sweep's own targets and visits == spp; without it Q is the visit-weighted mean
    test_bake.py's warm-start test restates; forget() changes visits only."""
    w = worlds("door_room")
    spp = 5
    p = gpu_params(rtmi_mod, spp=spp, env_light=0.75)
    with w.new_map() as a, w.new_map() as b, w.new_map() as c:
        a.sweep(w.sc, p)
        b.sweep(w.sc, p, apply=False)
        sums, counts = pending(b)
        assert (counts == spp).all()
        b.apply()
        got = a.read()
        assert same_maps(got, b.read())
        ps, pc = pending(a)
        assert not ps.any() and not pc.any()
        # the visit-weighted running mean
        assert np.array_equal(got[0], applied(w, w.q0, w.v0, sums, counts))
        assert np.array_equal(got[2], w.v0 + spp)
        assert not np.array_equal(got[1], w.start[1]) and not np.array_equal(got[3], w.start[3])
        # forget: visits alone, also of a sub-range, with targets pending
        c.sweep(w.sc, p, apply=False)
        c.forget(7, 130)
        q, cdf, vis, irr = c.read()
        keep = np.r_[0:7, 137:w.n]
        assert not vis[7:137].any() and np.array_equal(vis[keep], w.v0[keep])
        assert same_maps((q, cdf, irr), (w.start[0], w.start[1], w.start[3]))
        s2, c2 = pending(c)
        assert np.array_equal(s2, sums) and np.array_equal(c2, counts)
        c.forget()
        assert not c.read()[2].any()
        c.apply()
        q, _, vis, _ = c.read()
        mean = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32) / f32(spp)
        assert np.array_equal(q, np.where(mean > THRESHOLD, mean, THRESHOLD))
        assert (vis == spp).all()
        assert (q > THRESHOLD).any() and not np.array_equal(q, got[0])


@pytest.mark.gpu
def test_gpu_sweep_is_invariant_and_jacobi(rtmi_mod, gpu_ctx, worlds):
    """One call, two halves, three ranges taken backwards, the exact BVH, the k-d search, spp_split 4
    and a second run: identical pending sums and cast totals; first_sample = spp: other sums.  Two
    half-range sweeps and one apply equal the whole-map sweep; applying between the halves does not:
    a sweep reads the irradiance as it stood when it started."""
    T = rtmi_mod.sarsa
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, spp=8, env_light=0.75)
    h = w.n // 2

    def run(fn, scene=None):
        with w.new_map() as rm:
            casts = fn(rm, scene or w.sc)
            return casts, pending(rm)

    casts, ref = run(lambda rm, sc: rm.sweep(sc, p, apply=False))
    assert casts == w.n * S * 8 and ref[0].any()

    def same(got):
        return got[0] == casts and np.array_equal(got[1][0], ref[0]) and np.array_equal(got[1][1], ref[1])

    assert same(run(lambda rm, sc: rm.sweep(sc, p, apply=False)))  # a second run
    assert same(run(lambda rm, sc: rm.sweep(sc, p, 0, h, apply=False) + rm.sweep(sc, p, h, apply=False)))
    cuts = [0, 65, 200, w.n]
    ranges = list(reversed(list(zip(cuts[:-1], cuts[1:]))))
    assert same(run(lambda rm, sc: sum(rm.sweep(sc, p, a, b - a, apply=False) for a, b in ranges)))
    assert same(run(lambda rm, sc: rm.sweep(sc, p, apply=False) + rm.sweep(sc, p, 11, 0, apply=False)))  # n = 0
    with rtmi_mod.Scene(gpu_ctx, w.g) as sb:
        sb.set_accel(rtmi_mod.ACCEL_BVH)
        assert same(run(lambda rm, sc: rm.sweep(sc, p, apply=False), sb))

    def kd(rm, sc):
        rm.set_search(T.SEARCH_KD)
        assert rm.search_stats()["mode"] == T.SEARCH_KD
        return rm.sweep(sc, p, apply=False)

    assert same(run(kd))
    p4 = gpu_params(rtmi_mod, spp=8, spp_split=4, env_light=0.75)
    p3 = gpu_params(rtmi_mod, spp=8, spp_split=3, max_bounces=1, sampler=1, width=3, height=5, env_light=0.75)
    p3.t_scale = p.t_scale
    assert same(run(lambda rm, sc: rm.sweep(sc, p4, apply=False)))
    assert same(run(lambda rm, sc: rm.sweep(sc, p3, apply=False)))  # ignored fields
    nxt = run(lambda rm, sc: rm.sweep(sc, p, first_sample=8, apply=False))
    assert nxt[0] == casts and not np.array_equal(nxt[1][0], ref[0])
    assert np.array_equal(nxt[1][0], w.deposit(p, first=8))
    # Jacobi
    with w.new_map() as one, w.new_map() as halves, w.new_map() as between:
        one.sweep(w.sc, p)
        halves.sweep(w.sc, p, 0, h, apply=False)
        halves.sweep(w.sc, p, h, apply=False)
        halves.apply()
        assert same_maps(one.read(), halves.read())
        between.sweep(w.sc, p, 0, h, apply=True)
        irr_mid = between.read()[3]
        between.sweep(w.sc, p, h, apply=False)
        second = pending(between)[0]
        between.apply()
        assert not np.array_equal(between.read()[0], one.read()[0])
        # the second half saw the first half's results, and nothing else
        assert np.array_equal(second[h:], w.deposit(p, irr=irr_mid)[h:]) and not second[:h].any()


@pytest.mark.gpu
@pytest.mark.parametrize("replace", [False, True])
def test_gpu_dist_sweep_world_1_and_emulated_split(rtmi_mod, worlds, replace):
    """rtmi.dist.sarsa_sweep without a process group is the plain call; its two-rank split, emulated
    on one GPU -- two maps sweep one slice each, their pending tensors are added into a third map's
    accumulators, which forgets (replace) and applies -- gives the same map, bit for bit."""
    import torch
    from rtmi import dist as rdist
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, spp=5, env_light=0.75)
    dev = torch.device("cuda", 0)
    slices = [rdist.sweep_slice(w.n, r, 2) for r in range(2)]
    assert slices[0][0] == 0 and slices[0][0] + slices[0][1] == slices[1][0] and sum(s[1] for s in slices) == w.n
    assert [rdist.sweep_slice(7, r, 3) for r in range(3)] == [(0, 3), (3, 2), (5, 2)]
    with w.new_map() as single, w.new_map() as plain, w.new_map() as r0, w.new_map() as r1, w.new_map() as tot:
        casts = rdist.sarsa_sweep(single, w.sc, p, first_sample=3, replace=replace)
        assert casts == w.n * S * 5
        if replace:
            plain.forget()
        plain.sweep(w.sc, p, first_sample=3)
        ref = single.read()
        assert same_maps(ref, plain.read())
        part = 0
        for rm, (v0, n) in zip((r0, r1), slices):
            part += rm.sweep(w.sc, p, v0, n, first_sample=3, apply=False)
        assert part == casts
        ts, tc = rdist.td_tensors(tot, dev)
        (s0, c0), (s1, c1) = rdist.td_tensors(r0, dev), rdist.td_tensors(r1, dev)
        ts.copy_(s0 + s1)
        tc.copy_(c0 + c1)
        torch.cuda.synchronize()
        if replace:
            tot.forget()
        tot.apply()
        assert same_maps(tot.read(), ref)
        assert (ref[2] == (5 if replace else w.v0 + 5)).all()


@pytest.mark.gpu
def test_gpu_light_propagates_one_bounce_per_sweep(rtmi_mod, worlds):
    """From a map at the floor everywhere, by replace sweeps of one cast per sector: after sweep 1
    exactly the sectors whose cast ended on a light or a miss (env_light > 0) are above the floor
    -- a surface target of a floor map is below brdf^2 2 pi floor < floor --, after sweep 2 some
    sector whose cast ended on a surface is."""
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, spp=1, env_light=0.75)
    floor = np.full((w.n, S), THRESHOLD, np.float32)
    with w.new_map(written=False) as rm:
        rm.write(floor)
        assert (rm.read()[0] == THRESHOLD).all()
        rm.forget()
        rm.sweep(w.sc, p, first_sample=0)
        q1, _, vis, irr1 = rm.read()
        tgt, c = w.targets(1, p.t_scale, 0, 0.75)
        lit = c["kind"] != SURF
        assert lit.any() and (~lit).any() and (tgt[lit] > THRESHOLD).all()
        assert np.array_equal(q1 > THRESHOLD, lit) and (vis == 1).all()
        rm.forget()
        rm.sweep(w.sc, p, first_sample=1)
        q2 = rm.read()[0]
        c2 = w.cast(1, p.t_scale, 1)
        assert (q2[c2["kind"] == SURF] > THRESHOLD).any(), "no light arrived over a surface"
        # and it is the restated second sweep of the first sweep's irradiance
        want = (w.deposit(gpu_params(rtmi_mod, spp=1, env_light=0.75), first=1, irr=irr1).astype(np.float64)
                * 2.0 ** -32).astype(np.float32)
        assert np.array_equal(q2, np.where(want > THRESHOLD, want, THRESHOLD))


@pytest.mark.gpu
def test_gpu_sweep_and_forget_refuse_bad_arguments(rtmi_mod, gpu_ctx, worlds):
    """each refusal has its code and a message, and leaves the map and its pending sums as they were:
    rt_sarsa_bake's refusals that apply to a sweep, and the TD modes without frame sums"""
    L = rtmi_mod._lib
    T = rtmi_mod.sarsa
    lib = rtmi_mod.lib()
    w = worlds("door_room")
    good = gpu_params(rtmi_mod, spp=8)
    with w.new_map() as rm:
        def call(ctx=gpu_ctx.handle, sc=w.sc.handle, m=rm.handle, p=good, v0=0, n=w.n, apply=1):
            rc = lib.rt_sarsa_sweep(ctx, sc, m, None if p is None else ctypes.byref(p), v0, n, 0, apply, None, None)
            return rc, lib.rt_last_error().decode()

        cases = [
            (dict(ctx=None), L.RT_E_INVALID), (dict(sc=None), L.RT_E_INVALID), (dict(m=None), L.RT_E_INVALID),
            (dict(p=None), L.RT_E_INVALID),
            (dict(v0=w.n - 1, n=2), L.RT_E_INVALID), (dict(v0=-1, n=1), L.RT_E_INVALID),
            (dict(v0=w.n + 1, n=0), L.RT_E_INVALID), (dict(n=-1), L.RT_E_INVALID),
            (dict(v0=2 ** 31 - 1, n=2 ** 31 - 1), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=0)), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=8, hit_rule=2)), L.RT_E_INVALID),
            (dict(p=rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, spp=8)), L.RT_E_UNSUPPORTED),
        ]
        for kw, code in cases:
            for apply in (0, 1):
                rc, msg = call(apply=apply, **kw)
                assert rc == code and msg, (kw, rc, msg)
        for mode in (T.TD_INFRAME, T.TD_OFF):
            rm.set_td_mode(mode)
            for n in (w.n, 1):
                rc, msg = call(n=n)
                assert rc == L.RT_E_UNSUPPORTED and "RT_SARSA_TD_FRAME" in msg, (mode, rc, msg)
            with pytest.raises(rtmi_mod.RtError) as e:
                rm.sweep(w.sc, good)
            assert e.value.code == L.RT_E_UNSUPPORTED
        rm.set_td_mode(T.TD_FRAME)
        for v0, n in ((w.n - 1, 2), (-1, 1), (w.n + 1, 0), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert lib.rt_sarsa_forget(rm.handle, v0, n, None) == L.RT_E_INVALID and lib.rt_last_error()
        rm.forget(w.n, 0)  # n = 0 at the end of the map
        assert rm.sweep(w.sc, good, w.n, 0) == 0
        assert same_maps(rm.read(), w.start)
        ps, pc = pending(rm)
        assert not ps.any() and not pc.any()


@pytest.mark.gpu
def test_gpu_facade_sweep_equals_binding(rtmi_mod, gpu_ctx, worlds, tmp_path):
    """examples/reinforcement_main.cpp's sweep mode (host/reinforcement_path_tracing.h:
    RadianceMap::sweep per sweep, then draw_importance_sampling_path_tracing per frame)
    on a 24 x 20 screen saves the frame the binding renders from the same sweeps."""
    exe = os.path.join(PKG, "build", "reinforcement_demo")
    assert os.path.exists(exe), f"{exe} missing: make -C {PKG}"
    obj = os.path.join(MODELS, "door_room.obj")
    out = str(tmp_path / "sweep.bmp")
    r = subprocess.run([exe, "sweep", obj, "1", "2", "4", out, "24", "20", "3", "2"], capture_output=True, text=True,
                       timeout=240, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("swept map") == 2 and r.stdout.count("2 casts per sector") == 3
    raw = open(out, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 4 * 24 * 20
    got = np.frombuffer(raw[54:], dtype="<u4").reshape(20, 24)
    w = worlds("door_room", None)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=24, height=20, spp=4)
    ps = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, spp=2, t_scale=20.0)
    with w.new_map(written=False) as rm:
        for k in range(3):
            casts = rm.sweep(w.sc, ps, first_sample=2 * k)
            assert f"sweep {k}: 2 casts per sector, {casts} ray casts" in r.stdout
        rm.set_td_mode(rtmi_mod.sarsa.TD_OFF)
        rm.render(w.cam, p)
        img, _ = rm.render(w.cam, p)
    assert np.array_equal(got, rtmi_mod.pack_argb(img))
    assert len(np.unique(got)) > 20


def swept(rtmi_mod, w, rm, t_scale):
    """the sampler tests' schedule: SWEEPS replace sweeps, then MEAN_SWEEPS that keep the visits, of
    SWEEP_SPP casts per sector, fresh samples each"""
    ps = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, spp=SWEEP_SPP, t_scale=t_scale)
    for k in range(SWEEPS + MEAN_SWEEPS):
        if k < SWEEPS:
            rm.forget()
        rm.sweep(w.sc, ps, first_sample=k * SWEEP_SPP)


@pytest.mark.gpu
def test_gpu_swept_map_is_a_better_unbiased_sampler(rtmi_mod, gpu_ctx, worlds):
    """door_room at the default density, 64 x 64, against rt_render at 4096 spp: at 16 spp a frozen
    render of the swept map has a lower mean squared error than that of the fresh map, and the mean
    of 16 frozen frames of the swept map lies within 4 standard errors (the frames' own spread) of
    the reference's mean (test_bake.py's unbiasedness gate)."""
    T = rtmi_mod.sarsa
    w = worlds("door_room", None)
    ref, _ = rtmi_mod.render(gpu_ctx, w.sc, w.cam, rtmi_mod.default_params(
        rtmi_mod.RT_PRESET_GPU, width=64, height=64, spp=4096, spp_split=8))
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=64, height=64, spp=16, spp_split=4)
    ref64 = ref.astype(np.float64)

    def mse(img):
        return float(np.mean((img.astype(np.float64) - ref64) ** 2))

    with w.new_map(written=False) as fresh, w.new_map(written=False) as sw:
        fresh.set_td_mode(T.TD_OFF)
        e_fresh = mse(fresh.render(w.cam, p)[0])
        swept(rtmi_mod, w, sw, 64.0)
        sw.set_td_mode(T.TD_OFF)
        frames = [sw.render(w.cam, p)[0] for _ in range(16)]
    e_swept = mse(frames[0])
    means = np.array([f.astype(np.float64).mean() for f in frames])
    se = means.std(ddof=1) / np.sqrt(len(means))
    z = (means.mean() - ref64.mean()) / se
    print(f"mse fresh {e_fresh:.6g} swept {e_swept:.6g}; mean of 16 frames {means.mean():.6g} "
          f"reference {ref64.mean():.6g} se {se:.3g} z {z:.3f}")
    assert np.isfinite(frames).all()
    assert e_swept < e_fresh, (e_swept, e_fresh)
    assert abs(z) < 4.0, (means.mean(), ref64.mean(), se, z)


@pytest.mark.gpu
def test_gpu_swept_distributions_approach_ground_truth(rtmi_mod, worlds):
    """on the small map the median total-variation distance of the volumes' sector distributions
    (Q normalised) from a 64-spp bake is smaller after the sweeps than for the fresh map"""
    P = rtmi_mod.probe
    w = worlds("door_room")
    pb = gpu_params(rtmi_mod, spp=64, spp_split=4)
    with w.new_map(written=False) as truth, w.new_map(written=False) as sw:
        truth.bake(w.sc, pb)
        qt = truth.read()[0]
        swept(rtmi_mod, w, sw, pb.t_scale)
        qs = sw.read()[0]
    tv_fresh = np.nanmedian(P.distribution_error(qt, w.fresh[0])["tv"])
    tv_swept = np.nanmedian(P.distribution_error(qt, qs)["tv"])
    print(f"median TV from the 64-spp bake: fresh {tv_fresh:.4f} swept {tv_swept:.4f}")
    assert tv_swept < tv_fresh, (tv_swept, tv_fresh)
