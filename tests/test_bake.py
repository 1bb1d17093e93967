"""Radiance maps filled from ground truth and rendered frozen: rt_sarsa_bake, rt_sarsa_write and
RT_SARSA_TD_OFF (include/rtmi.h).

  * the bake against its definition, bit for bit: the float32 numpy restatement of
    Q = max(vol_brdf * ((r + g) + b) / 3, RADIANCE_THRESHOLD) applied to rtmi.probe.radiance of the
    same volumes, on every (spp, split), hit rule, env_light and range case, with the casts;
  * the device-side finish (irradiance, CDF) against the host path of rt_sarsa_write;
  * invariance under the split of the range, its order and the cast route;
  * a frozen frame against the learning frame of the same map (image, casts, statistics), and
    that it leaves the map alone, also through the tile entry;
  * the baked map as a sampler: lower error than a fresh map's, and unbiased;
  * the warm start of training after a bake; the argument checks; the C++ facade.
The small map is door_room at area_per_sample 0.1 (344 volumes); Cornell serves the CPU hit rule's
one-word candidate table.
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
THRESHOLD = np.float32(1.0) / (np.float32(12.0) * np.float32(12.0)) * np.float32(0.8)  # RADIANCE_THRESHOLD


def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def gpu_params(rtmi_mod, **kw):
    kw.setdefault("max_bounces", 6)
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, **kw)


# ---------------------------------------------------------------- CPU ----------

def test_new_symbols_are_exported(rtmi_mod):
    lib = rtmi_mod.lib()
    for name in ("rt_sarsa_bake", "rt_sarsa_write"):
        assert hasattr(lib, name), name
        assert name in rtmi_mod._lib.EXPORTS


def header_define(name):
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    m = re.search(r"^#define\s+%s\s+(-?\d+)" % name, src, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_constants_agree(rtmi_mod):
    """include/rtmi.h, rtmi/sarsa.py and INTEGRATION.md name the same TD modes"""
    sarsa = rtmi_mod.sarsa
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, value in (("RT_SARSA_TD_FRAME", sarsa.TD_FRAME), ("RT_SARSA_TD_INFRAME", sarsa.TD_INFRAME),
                        ("RT_SARSA_TD_OFF", sarsa.TD_OFF)):
        assert header_define(name) == value
    assert sarsa.TD_OFF == 2
    m = re.search(r"`RT_SARSA_TD_OFF`\s*\(=\s*(\d+)\)", doc)
    assert m and int(m.group(1)) == sarsa.TD_OFF
    assert header_define("RT_KT_BAKE") == rtmi_mod.RT_KT_BAKE == rtmi_mod.RT_KT_COUNT - 1
    assert header_define("RT_KT_COUNT") == rtmi_mod.RT_KT_COUNT
    assert rtmi_mod.ktime_name(rtmi_mod.RT_KT_BAKE) == "k_bake"
    assert "importance_sampling_path_tracing.h" in doc and "rt_sarsa_bake" in doc and "rt_sarsa_write" in doc


def test_td_mode_3_is_refused_by_value(rtmi_mod):
    """the mode is checked before the map: 3 is refused as a mode, a valid one with no map for the map"""
    lib = rtmi_mod.lib()
    assert lib.rt_sarsa_set_td_mode(None, 3) == rtmi_mod._lib.RT_E_INVALID
    assert b"bad TD mode 3" in lib.rt_last_error()
    assert lib.rt_sarsa_set_td_mode(None, rtmi_mod.sarsa.TD_OFF) == rtmi_mod._lib.RT_E_INVALID
    assert b"NULL" in lib.rt_last_error()


def test_write_and_bake_refuse_null_map(rtmi_mod):
    lib = rtmi_mod.lib()
    q = np.zeros((1, S), np.float32)
    assert lib.rt_sarsa_write(None, 0, 1, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None) == -1
    assert b"NULL" in lib.rt_last_error()
    p = gpu_params(rtmi_mod)
    assert lib.rt_sarsa_bake(None, None, None, ctypes.byref(p), 0, 0, 0, None, None) == -1
    assert b"NULL" in lib.rt_last_error()


# ---------------------------------------------------------------- GPU ----------

class World:
    def __init__(self, rtmi_mod, ctx, scene, area=AREA):
        self.rtmi, self.ctx, self.name, self.area = rtmi_mod, ctx, scene, area
        self.g = geometry(rtmi_mod, scene)
        self.sc = rtmi_mod.Scene(ctx, self.g)
        self.cam = rtmi_mod.camera(rtmi_mod.CAMERAS[scene])
        with self.new_map() as rm:
            self.n = rm.n_volumes
            self.pos, self.nrm, self.surf, _ = rm.volumes()
            self.fresh = rm.read()
        alb = np.asarray(self.g.albedo, np.float32)[self.surf]
        lum = np.float32(0.5) * (alb.max(axis=1) + alb.min(axis=1))  # Material luminance
        self.brdf = (lum / np.float32(np.pi)).astype(np.float32)

    def new_map(self):
        return self.rtmi.sarsa.RadianceMap(self.ctx, self.sc, SEED, self.area)

    def probe(self, p, idx, first=0, scene=None):
        idx = np.asarray(idx)
        return self.rtmi.probe.radiance(self.ctx, scene or self.sc, p, self.pos[idx], self.surf[idx], idx, first,
                                        want_irr=False)

    def q_of(self, rad, idx):
        """the definition, in float32"""
        rad = np.asarray(rad, np.float32)
        lum = ((rad[..., 0] + rad[..., 1]) + rad[..., 2]) / np.float32(3.0)
        q = self.brdf[np.asarray(idx)][:, None] * lum
        assert q.dtype == np.float32
        return np.where(q > THRESHOLD, q, THRESHOLD)

    def close(self):
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(rtmi_mod, gpu_ctx):
    made = {}

    def get(scene, area=AREA):
        if (scene, area) not in made:
            made[(scene, area)] = World(rtmi_mod, gpu_ctx, scene, area)
        return made[(scene, area)]

    yield get
    for w in made.values():
        w.close()


def same_maps(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def pending(rtmi_mod, rm):
    """the map's pending TD sums and counts, copied to the host"""
    import torch
    from rtmi import dist as rdist
    s, c = rdist.td_tensors(rm, torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s.cpu().numpy().copy(), c.cpu().numpy().copy()


DEFINITION_CASES = [(scene, spp, split, rule, env)
                    for scene, rules in (("door_room", (1, 0)),)
                    for spp, split in ((1, 1), (5, 1), (8, 4))
                    for rule in rules
                    for env in (0.0, 0.75)] + [("cornell", 8, 4, 0, 0.5), ("cornell", 5, 1, 0, 0.0)]


# The instantiations of k_bake (sampler x hit rule x {table of one mask word, table of four,
# exact BVH, filter / scan}) that neither the cases above (uniform sampler; door_room's table has four
# words, cornell's one) nor test_gpu_bake_is_invariant (the BVH at rule 1) launch, once each at 8
# samples in 4 chunks over the first 5 and the last 3 volumes.
# (id, scene, rule, env, sampler, t_scale or None for the default, exact BVH)
BEYOND_T = 32768.0  # past the filter's and the tables' t_scale range: the plain scan
INSTANTIATION_CASES = [
    ("cornell-rule1-table1", "cornell", 1, 0.5, 0, None, False),
    ("cornell-rule0-bvh", "cornell", 0, 0.5, 0, None, True),
    ("cornell-rule0-filter", "cornell", 0, 0.5, 0, 128.0, False),
    ("door_room-rule1-scan", "door_room", 1, 0.75, 0, BEYOND_T, False),
    ("cornell-rule0-table1-cosine", "cornell", 0, 0.5, 1, None, False),
    ("cornell-rule1-table1-cosine", "cornell", 1, 0.5, 1, None, False),
    ("door_room-rule0-table4-cosine", "door_room", 0, 0.75, 1, None, False),
    ("door_room-rule1-table4-cosine", "door_room", 1, 0.75, 1, None, False),
    ("cornell-rule0-bvh-cosine", "cornell", 0, 0.5, 1, None, True),
    ("cornell-rule1-bvh-cosine", "cornell", 1, 0.5, 1, None, True),
    ("cornell-rule0-filter-cosine", "cornell", 0, 0.5, 1, 128.0, False),
    ("door_room-rule1-scan-cosine", "door_room", 1, 0.75, 1, BEYOND_T, False),
]
DEFINITION_PARAMS = ([c + (None,) for c in DEFINITION_CASES] +
                     [(c[1], 8, 4, c[2], c[3], c[4:]) for c in INSTANTIATION_CASES])
DEFINITION_IDS = (["-".join(str(x) for x in c) for c in DEFINITION_CASES] + [c[0] for c in INSTANTIATION_CASES])


@pytest.mark.gpu
@pytest.mark.parametrize("scene,spp,split,rule,env,inst", DEFINITION_PARAMS, ids=DEFINITION_IDS)
def test_gpu_bake_equals_its_definition(rtmi_mod, gpu_ctx, worlds, scene, spp, split, rule, env, inst):
    """Q, visits and casts of a bake == the formula on rtmi.probe.radiance of the same volumes,
    bit for bit; nothing outside the range moves.  Ranges: the whole map, one volume, and
    [7, 7 + 130) (v0 != 0, no multiple of 64); for the cases that are there for the kernel they
    launch (inst: sampler, t_scale, exact BVH), the first 5 volumes and the last 3."""
    w = worlds(scene)
    p = gpu_params(rtmi_mod, spp=spp, spp_split=split, hit_rule=rule, env_light=env)
    assert w.n > 7 + 130
    ranges = ((0, w.n), (w.n - 3, 1), (7, 130))
    sc = w.sc
    if inst is not None:
        sampler, t_scale, bvh = inst
        p.sampler = sampler
        if t_scale is not None:
            p.t_scale = t_scale
        ranges = ((0, 5), (w.n - 3, 3))
        if bvh:
            sc = rtmi_mod.Scene(gpu_ctx, w.g)
            sc.set_accel(rtmi_mod.ACCEL_BVH)
    lit = False
    try:
        for v0, n in ranges:
            idx = np.arange(v0, v0 + n)
            ref = w.probe(p, idx, scene=sc)
            want = w.q_of(ref["rad"], idx)
            with w.new_map() as rm:
                casts = rm.bake(sc, p, v0, n)
                q, cdf, vis, irr = rm.read()
                ps, pc = pending(rtmi_mod, rm)
            assert casts == ref["casts"], (v0, n)
            assert np.array_equal(q[idx], want), (v0, n, np.abs(q[idx] - want).max())
            assert (vis[idx] == spp).all()
            out = np.ones(w.n, bool)
            out[idx] = False
            for got, before in zip((q, cdf, vis, irr), w.fresh):
                assert np.array_equal(got[out], before[out]), (v0, n)
            assert not ps.any() and not pc.any()
            # a distribution over the range: a monotone CDF that ends at 1
            assert (np.diff(cdf[idx], axis=1) >= 0).all() and np.allclose(cdf[idx, -1], 1.0, atol=1e-5)
            lit = lit or bool((q[idx] > THRESHOLD).any())
    finally:
        if sc is not w.sc:
            sc.close()
    assert lit, "no sector received light: the case checks nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [6, 1])
def test_gpu_device_finish_equals_host_write(rtmi_mod, worlds, max_bounces):
    """B.write(A's Q, visits) on a fresh map of the same seed == the baked map A: irradiance, CDF and
    visits from the device finish are the host path's.  max_bounces = 1: no cast, every sector on
    the floor, the CDF that of a constant Q."""
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, spp=8, spp_split=4, max_bounces=max_bounces)
    with w.new_map() as a, w.new_map() as b, w.new_map() as c:
        casts = a.bake(w.sc, p)
        qa, cdfa, visa, irra = a.read()
        b.write(qa, visa)
        assert same_maps(b.read(), (qa, cdfa, visa, irra))
        # visits kept when not given, a sub-range written alone
        b.write(w.fresh[0][5:9], None, v0=5)
        qb, cdfb, visb, irrb = b.read()
        assert np.array_equal(qb[5:9], w.fresh[0][5:9]) and np.array_equal(visb, visa)
        # (a new map's CDF is the reference's uniform initial one, not yet the one its Q gives)
        c.write(w.fresh[0])
        assert np.array_equal(cdfb[5:9], c.read()[1][5:9]) and np.array_equal(irrb[5:9], w.fresh[3][5:9])
        keep = np.r_[0:5, 9:w.n]
        assert np.array_equal(cdfb[keep], cdfa[keep]) and np.array_equal(irrb[keep], irra[keep])
        if max_bounces == 1:
            assert casts == 0 and (qa == THRESHOLD).all()
            c.write(np.full((w.n, S), THRESHOLD, np.float32))
            qc, cdfc, _, irrc = c.read()
            assert np.array_equal(cdfc, cdfa) and np.array_equal(irrc, irra)
        else:
            assert casts > 0 and (qa > THRESHOLD).any()
        # the sampler's stored arg-max follows: a SAMPLE_MAX frame of the two maps is one image
        b.write(qa, visa)
        pr = gpu_params(rtmi_mod, width=17, height=5, spp=2)
        for m in (a, b):
            m.set_sampling(rtmi_mod.sarsa.SAMPLE_MAX)
            m.set_td_mode(rtmi_mod.sarsa.TD_OFF)
        ia, ib = a.render(w.cam, pr)[0], b.render(w.cam, pr)[0]
        assert np.array_equal(ia, ib, equal_nan=True)


@pytest.mark.gpu
def test_gpu_bake_is_invariant(rtmi_mod, gpu_ctx, worlds):
    """[0, n) in one call, in two halves, in three ranges taken backwards, and with the exact BVH
    turned on: identical maps and cast totals.  Other samples (first_sample = spp): another Q."""
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, spp=8, spp_split=4)
    with w.new_map() as one, w.new_map() as halves, w.new_map() as back, w.new_map() as bvh, w.new_map() as nxt:
        casts = one.bake(w.sc, p)
        ref = one.read()
        h = w.n // 2
        assert halves.bake(w.sc, p, 0, h) + halves.bake(w.sc, p, h) == casts
        assert same_maps(halves.read(), ref)
        cuts = [0, 65, 200, w.n]
        tot = sum(back.bake(w.sc, p, a, b - a) for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))))
        assert tot == casts and same_maps(back.read(), ref)
        assert back.bake(w.sc, p, 11, 0) == 0 and same_maps(back.read(), ref)  # n = 0
        with rtmi_mod.Scene(gpu_ctx, w.g) as sb:
            sb.set_accel(rtmi_mod.ACCEL_BVH)
            assert bvh.bake(sb, p) == casts
        assert same_maps(bvh.read(), ref)
        nxt.bake(w.sc, p, first_sample=p.spp)
        q2 = nxt.read()[0]
        assert not np.array_equal(q2, ref[0])
        idx = np.arange(w.n)
        assert np.array_equal(q2, w.q_of(w.probe(p, idx, first=p.spp)["rad"], idx))


def train_two(rtmi_mod, w, p):
    """two maps of one seed after two TD_FRAME frames"""
    a, b = w.new_map(), w.new_map()
    for m in (a, b):
        m.render(w.cam, p, 2)
    assert same_maps(a.read(), b.read()) and a.frames == b.frames == 2
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(50, 39), (1, 1)])
@pytest.mark.parametrize("split", [1, 4])
def test_gpu_frozen_frame_equals_learning_frame(rtmi_mod, worlds, width, height, split):
    """A TD_FRAME frame reads only the previous frame's table, so the third frame of map A (learning)
    and of map B (RT_SARSA_TD_OFF) are one image, cast count and statistic; B's map stays, A's moves."""
    T = rtmi_mod.sarsa
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, width=width, height=height, spp=4, spp_split=split, max_bounces=8)
    a, b = train_two(rtmi_mod, w, p)
    try:
        before = b.read()
        b.set_td_mode(T.TD_OFF)
        assert b.td_mode == T.TD_OFF and a.td_mode == T.TD_FRAME
        ia, ca = a.render(w.cam, p)
        ib, cb = b.render(w.cam, p)
        assert np.array_equal(ia, ib) and ca == cb and ca > 0
        assert a.frame_stats() == b.frame_stats()
        assert a.frames == b.frames == 3
        assert same_maps(b.read(), before)
        ps, pc = pending(rtmi_mod, b)
        assert not ps.any() and not pc.any()
        assert not np.array_equal(a.read()[2], before[2]), "the learning frame recorded no visit"
        assert not np.array_equal(a.read()[0], before[0])
        # successive frozen frames draw fresh samples
        ib2, _ = b.render(w.cam, p)
        assert b.frames == 4 and not np.array_equal(ib2, ib) and same_maps(b.read(), before)
        # back to learning: the mode round-trips and the map learns again
        b.set_td_mode(T.TD_FRAME)
        assert b.td_mode == T.TD_FRAME
        b.render(w.cam, p)
        assert not np.array_equal(b.read()[2], before[2])
        with pytest.raises(rtmi_mod.RtError):
            b.set_td_mode(3)
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(50, 39), (1, 1)])
@pytest.mark.parametrize("apply", [False, True])
def test_gpu_frozen_tiles_ignore_apply(rtmi_mod, worlds, width, height, apply):
    """the same through rt_render_sarsa_tiles_device: in RT_SARSA_TD_OFF `apply` makes no difference,
    nothing is left pending and nothing applied"""
    import torch
    from rtmi import tiles as rtiles
    T = rtmi_mod.sarsa
    w = worlds("door_room")
    p = gpu_params(rtmi_mod, width=width, height=height, spp=4, spp_split=4, max_bounces=8)
    a, b = train_two(rtmi_mod, w, p)
    try:
        before = b.read()
        b.set_td_mode(T.TD_OFF)
        origins = rtiles.tile_origins(width, height, 32)
        dev = torch.device("cuda", 0)
        outs = [torch.zeros(len(origins), 32, 32, 3, device=dev) for _ in range(2)]
        casts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2)]
        a.render_tiles_device(w.cam, p, origins, 32, outs[0].data_ptr(), casts[0].data_ptr(), True, 0)
        b.render_tiles_device(w.cam, p, origins, 32, outs[1].data_ptr(), casts[1].data_ptr(), apply, 0)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and int(casts[0]) == int(casts[1]) > 0
        assert a.frame_stats() == b.frame_stats() and a.frames == b.frames == 3
        assert same_maps(b.read(), before)
        ps, pc = pending(rtmi_mod, b)
        assert not ps.any() and not pc.any()
        assert not np.array_equal(a.read()[2], before[2])
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_gpu_baked_map_is_a_better_unbiased_sampler(rtmi_mod, gpu_ctx, worlds):
    """door_room at the default density, 64 x 64, against rt_render at 4096 spp: at 16 spp a frozen
    render of the map baked at 64 spp has a lower mean squared error than that of the fresh map, and
    the mean of 16 frozen frames of the baked map lies within 4 standard errors (the frames' own
    spread) of the reference's mean."""
    T = rtmi_mod.sarsa
    w = worlds("door_room", None)
    ref, _ = rtmi_mod.render(gpu_ctx, w.sc, w.cam, rtmi_mod.default_params(
        rtmi_mod.RT_PRESET_GPU, width=64, height=64, spp=4096, spp_split=8))
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=64, height=64, spp=16, spp_split=4)
    pb = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, spp=64, spp_split=4, t_scale=64.0)
    ref64 = ref.astype(np.float64)

    def mse(img):
        return float(np.mean((img.astype(np.float64) - ref64) ** 2))

    with w.new_map() as fresh, w.new_map() as baked:
        fresh.set_td_mode(T.TD_OFF)
        baked.set_td_mode(T.TD_OFF)
        e_fresh = mse(fresh.render(w.cam, p)[0])
        baked.bake(w.sc, pb)
        frames = [baked.render(w.cam, p)[0] for _ in range(16)]
    e_baked = mse(frames[0])
    means = np.array([f.astype(np.float64).mean() for f in frames])
    se = means.std(ddof=1) / np.sqrt(len(means))
    z = (means.mean() - ref64.mean()) / se
    print(f"mse fresh {e_fresh:.6g} baked {e_baked:.6g}; mean of 16 frames {means.mean():.6g} "
          f"reference {ref64.mean():.6g} se {se:.3g} z {z:.3f}")
    assert np.isfinite(frames).all()
    assert e_baked < e_fresh, (e_baked, e_fresh)
    assert abs(z) < 4.0, (means.mean(), ref64.mean(), se, z)


@pytest.mark.gpu
def test_gpu_training_warm_starts_from_a_bake(rtmi_mod, worlds):
    """after a bake one TD_FRAME frame moves a visited sector's Q by the spp-weighted running mean
    (q_old * spp + sum) / (spp + n), with the frame's own sums and counts (a tile render, apply = 0)"""
    import torch
    from rtmi import tiles as rtiles
    w = worlds("door_room")
    spp = 8
    with w.new_map() as rm:
        rm.bake(w.sc, gpu_params(rtmi_mod, spp=spp, spp_split=4))
        q0, _, v0, _ = rm.read()
        assert (v0 == spp).all()
        p = gpu_params(rtmi_mod, width=50, height=39, spp=4, spp_split=2, max_bounces=8)
        origins = rtiles.tile_origins(50, 39, 32)
        out = torch.zeros(len(origins), 32, 32, 3, device="cuda:0")
        casts = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        rm.render_tiles_device(w.cam, p, origins, 32, out.data_ptr(), casts.data_ptr(), False, 0)
        sums, counts = pending(rtmi_mod, rm)
        rm.apply(0)
        q1, _, v1, _ = rm.read()
    sums, counts = sums.reshape(w.n, S), counts.reshape(w.n, S).astype(np.uint32)
    hit = v1 > v0
    assert hit.sum() > 100 and np.array_equal(hit, counts > 0)
    assert np.array_equal(v1, v0 + counts)
    s32 = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32)
    want = (q0 * np.float32(spp) + s32) / (np.float32(spp) + counts.astype(np.float32)).astype(np.float32)
    want = np.where(want > THRESHOLD, want, THRESHOLD).astype(np.float32)
    assert np.array_equal(q1[hit], want[hit])
    assert np.array_equal(q1[~hit], q0[~hit])


@pytest.mark.gpu
def test_gpu_bake_and_write_refuse_bad_arguments(rtmi_mod, gpu_ctx, worlds):
    """each refusal has its code and a message, and leaves the map as it was"""
    L = rtmi_mod._lib
    lib = rtmi_mod.lib()
    w = worlds("door_room")
    good = gpu_params(rtmi_mod, spp=8, spp_split=4)
    with w.new_map() as rm:
        def call(ctx=gpu_ctx.handle, sc=w.sc.handle, m=rm.handle, p=good, v0=0, n=w.n):
            rc = lib.rt_sarsa_bake(ctx, sc, m, None if p is None else ctypes.byref(p), v0, n, 0, None, None)
            return rc, lib.rt_last_error().decode()

        cases = [
            (dict(ctx=None), L.RT_E_INVALID), (dict(sc=None), L.RT_E_INVALID), (dict(m=None), L.RT_E_INVALID),
            (dict(p=None), L.RT_E_INVALID),
            (dict(v0=w.n - 1, n=2), L.RT_E_INVALID), (dict(v0=-1, n=1), L.RT_E_INVALID),
            (dict(v0=w.n + 1, n=0), L.RT_E_INVALID), (dict(n=-1), L.RT_E_INVALID),
            (dict(v0=2 ** 31 - 1, n=2 ** 31 - 1), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=8, spp_split=3)), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=0)), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=8, max_bounces=0)), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=8, sampler=5)), L.RT_E_INVALID),
            (dict(p=gpu_params(rtmi_mod, spp=8, hit_rule=2)), L.RT_E_INVALID),
            (dict(p=rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, spp=8)), L.RT_E_UNSUPPORTED),
        ]
        for kw, code in cases:
            rc, msg = call(**kw)
            assert rc == code and msg, (kw, rc, msg)
        q = np.zeros((2, S), np.float32)
        for v0 in (w.n - 1, -1):
            with pytest.raises(rtmi_mod.RtError) as e:
                rm.write(q, v0=v0)
            assert e.value.code == L.RT_E_INVALID
        with pytest.raises(ValueError):
            rm.write(np.zeros((2, S - 1), np.float32))
        with pytest.raises(ValueError):
            rm.write(q, np.zeros((3, S), np.uint32))
        rm.write(np.zeros((0, S), np.float32), v0=w.n)  # n = 0 at the end of the map
        assert lib.rt_sarsa_write(rm.handle, 0, 1, None, None) == L.RT_E_INVALID
        assert same_maps(rm.read(), w.fresh)
        ps, pc = pending(rtmi_mod, rm)
        assert not ps.any() and not pc.any()


@pytest.mark.gpu
def test_gpu_facade_importance_sampling_equals_binding(rtmi_mod, gpu_ctx, worlds, tmp_path):
    """examples/reinforcement_main.cpp's importance mode (host/importance_sampling_path_tracing.h:
    precompute_radiance_volumes, then draw_importance_sampling_path_tracing per frame) on a 24 x 20
    screen saves the frame the binding renders from the same bake."""
    exe = os.path.join(PKG, "build", "reinforcement_demo")
    assert os.path.exists(exe), f"{exe} missing: make -C {PKG}"
    obj = os.path.join(MODELS, "door_room.obj")
    out = str(tmp_path / "importance.bmp")
    r = subprocess.run([exe, "importance", obj, "1", "2", "4", out, "24", "20", "4"], capture_output=True, text=True,
                       timeout=240, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("importance sampling") == 2 and "precomputed 4 paths per sector" in r.stdout
    raw = open(out, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 4 * 24 * 20
    got = np.frombuffer(raw[54:], dtype="<u4").reshape(20, 24)
    w = worlds("door_room", None)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=24, height=20, spp=4)
    pb = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, spp=4, spp_split=4, t_scale=20.0)
    with w.new_map() as rm:
        casts = rm.bake(w.sc, pb)
        assert f"{casts} ray casts" in r.stdout
        rm.set_td_mode(rtmi_mod.sarsa.TD_OFF)
        rm.render(w.cam, p)
        img, _ = rm.render(w.cam, p)
    assert np.array_equal(got, rtmi_mod.pack_argb(img))
    assert len(np.unique(got)) > 20
