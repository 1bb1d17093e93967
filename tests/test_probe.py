"""Ground-truth incident radiance at surface points: rt_probe_radiance[_device] and rtmi.probe.

The reference ships no code for its "true distribution" figure
(Descriptions/write_up/chapters/4_critical_evaluation.tex:92-110), so everything is pinned
against the existing restatement (oracle/):
  * the first directions against the restated DQN sampler with a one-hot Q per sector;
  * two-cast paths (max_bounces = 2) bit for bit: origin, direction and cosine restated in numpy
    float32, the hits from the pinned intersect call, the chunk sums and the fold restated, on
    every cast route but the BVH (the table, the filter, the scan);
  * at full depth, that a point's result does not depend on the list, the order, the run, the
    cast route (candidate table / BVH), the entry (host / device stream) or the batching;
  * the estimator itself against the pinned renderer: a wall pixel's radiance is
    2 * albedo * mean_k(out_irr[k]) at its hit point -- and is not with out_rad in its place;
  * the two samplers' tails agree; the argument checks; the host-side helpers.
Shapes: 1, 3 and 5 points (5 * 144 items: three workgroups, the last one ragged), chunks of 1, 5
and 2 samples, scenes of one mask word (Cornell, 38 triangles) and of two (archway, 102).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import MODELS

f32 = np.float32
SECTORS = 144
MAX_ID = (1 << 32) // SECTORS


def geometry(rtmi_mod, scene):
    if scene == "cornell":
        return rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    return rtmi_mod.obj_geometry(os.path.join(MODELS, scene + ".obj"), scene)


def surface_points(geom, surfaces):
    """One interior point per surface: v0 + 0.3 e1 + 0.4 e2 in float32."""
    t = geom.tri[np.asarray(surfaces)]
    v0, v1, v2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    return (v0 + f32(0.3) * (v1 - v0) + f32(0.4) * (v2 - v0)).astype(np.float32)


def dot3(a, b):
    """the restatement's dot3: (x + y) + z of the float32 products"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    """the restatement's normalize3: v * (1 / sqrt(dot3(v, v)))"""
    inv = f32(1.0) / np.sqrt(dot3(v, v))
    return v * inv[..., None]


def first_dirs(oracle_mod, geom, pos, tri, ids, sample, seed):
    """The directions the restated DQN sampler returns for a one-hot Q per sector: rays
    (point p, sector k) with pix = ids[p] * 144 + k, bounce 0.  -> dir (n, 144, 3), selected
    (n, 144): False where the one-hot draw returned no action (or, never, another cell)."""
    n = len(tri)
    q = np.tile(np.eye(SECTORS, dtype=np.float32), (n, 1))
    loc = np.repeat(np.asarray(pos, np.float32), SECTORS, axis=0)
    tr = np.repeat(np.asarray(tri, np.int32), SECTORS)
    pix = (np.repeat(np.asarray(ids, np.uint64), SECTORS) * SECTORS + np.tile(np.arange(SECTORS, dtype=np.uint64), n))
    assert pix.max() < 1 << 32
    _, _, d, a = oracle_mod.dqn_sample(geom.all_triangles(), q, loc, tr, pix.astype(np.uint32), int(sample), 0,
                                       int(seed), np.ones((n * SECTORS, 3), np.float32))
    k = np.tile(np.arange(SECTORS), n)
    assert np.all((a == k) | (a == -1)), "a one-hot Q selected another cell"
    return d.reshape(n, SECTORS, 3), (a == k).reshape(n, SECTORS)


CORNELL_SURF = [2, 14, 30, 7, 21]
ARCHWAY_SURF = [1, 20, 30, 47, 66]  # 1 faces a light, 30 and 66 the open side (misses)
IDS = [7, 0, MAX_ID - 1, 12345, 99]


# ---------------------------------------------------------------- CPU ----------

def test_distribution_and_error_on_hand_made_arrays(rtmi_mod):
    P = rtmi_mod.probe
    rad = np.zeros((3, SECTORS, 3), np.float32)
    rad[0, 5] = (3, 0, 0)        # luminance 1
    rad[0, 9] = (1, 1, 7)        # luminance 3
    rad[1] = 2.0                 # flat
    d = P.distribution(rad)      # point 2 received nothing
    assert d.shape == (3, SECTORS) and d.dtype == np.float64
    assert d[0, 5] == 0.25 and d[0, 9] == 0.75 and d[0].sum() == 1.0
    assert np.allclose(d[1], 1 / SECTORS, rtol=1e-15) and not d[2].any()
    with pytest.raises(ValueError):
        P.distribution(np.zeros((SECTORS, 4)))
    # total variation and KL by hand: p = (1/4, 3/4), q = (1/2, 1/2) on sectors 5 and 9
    q = np.zeros(SECTORS)
    q[[5, 9]] = 7.0              # not normalised: the function divides by the sum
    e = P.distribution_error(d[0], q)
    assert np.isclose(e["tv"], 0.25, rtol=1e-15)
    assert np.isclose(e["kl"], 0.25 * np.log(0.5) + 0.75 * np.log(1.5), rtol=1e-14)
    same = P.distribution_error(d[:2], d[:2])
    assert np.array_equal(same["tv"], [0, 0]) and np.array_equal(same["kl"], [0, 0])
    # zeros: p = 0 adds nothing; p > 0 where q = 0 is +inf; an empty row is nan
    q2 = np.zeros(SECTORS)
    q2[[5, 9, 11]] = (1, 3, 4)
    e2 = P.distribution_error(d[0], q2)
    assert np.isclose(e2["tv"], 0.5) and np.isclose(e2["kl"], np.log(2.0))
    q3 = np.zeros(SECTORS)
    q3[5] = 1
    e3 = P.distribution_error(d[0], q3)
    assert np.isclose(e3["tv"], 0.75) and np.isposinf(e3["kl"])
    e4 = P.distribution_error(d, np.ones((3, SECTORS)))
    assert np.isfinite(e4["tv"][:2]).all() and np.isnan(e4["tv"][2]) and np.isnan(e4["kl"][2])
    assert np.isnan(P.distribution_error(d[0], np.zeros(SECTORS))["kl"])
    with pytest.raises(ValueError):
        P.distribution_error(d[0], -q)
    with pytest.raises(ValueError):
        P.distribution_error(d[0], q[:10])


def test_selected_true_round_trips_through_read_selected_file(rtmi_mod, tmp_path):
    rng = np.random.default_rng(5)
    n = 4
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nrm = np.eye(3, dtype=np.float32)[[0, 1, 2, 1]] * f32(-1.0)
    rad = rng.random((n, SECTORS, 3)).astype(np.float32)
    rad[2, 10:90] = 0
    dist = rtmi_mod.probe.distribution(rad)
    path = str(tmp_path / "selected_true.txt")
    rtmi_mod.probe.write_selected_file(path, pos, nrm, dist)
    lines = open(path).read().splitlines()
    assert len(lines) == n and all(len(l.split()) == 6 + SECTORS for l in lines)
    p2, n2, d2 = rtmi_mod.sarsa.read_selected_file(path)
    assert p2.shape == (n, 3) and d2.shape == (n, SECTORS)
    assert np.array_equal(n2, nrm)
    assert np.allclose(p2, pos, rtol=5e-6, atol=0) and np.allclose(d2, dist, rtol=5e-6, atol=0)
    assert not d2[2, 10:90].any()
    # six significant digits: what was read writes the same file again
    again = str(tmp_path / "again.txt")
    rtmi_mod.probe.write_selected_file(again, p2, n2, d2)
    assert open(again).read() == open(path).read()
    with pytest.raises(ValueError):
        rtmi_mod.probe.write_selected_file(again, pos, nrm[:2], dist)


# the estimator test's pinned side (no GPU): Cornell, GPU variant, no yaw, a 2048^2 image
EST_W = 2048
EST_PIXEL = (1000, 700)  # the back wall, yellow
EST_M = 4
EST_SEEDS = tuple(range(100, 108))
EST_RENDER_SPP = 1 << 15


@functools.lru_cache(maxsize=None)
def pinned_pixel(px, py):
    """L_o of the pixel by the pinned renderer (uniform sampler, max_bounces EST_M): per seed,
    (8, 3) float64."""
    import oracle
    import rtmi
    geom = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    out = []
    for seed in EST_SEEDS:
        p = rtmi.default_params(rtmi.RT_PRESET_GPU, width=EST_W, height=EST_W, spp=EST_RENDER_SPP, spp_split=1,
                                max_bounces=EST_M, seed=seed, sampler=rtmi.RT_SAMPLER_UNIFORM)
        img, _ = oracle.render(geom, oracle.camera(rtmi.CAMERAS["cornell"]), oracle.params_from(p), (px, py, 1, 1))
        out.append(img[0, 0].astype(np.float64))
    return np.array(out)


def mean_se(a):
    a = np.asarray(a, np.float64)
    return a.mean(axis=0), a.std(axis=0, ddof=1) / np.sqrt(a.shape[0])


def test_estimator_pixel_footprint_is_below_the_error(rtmi_mod, oracle_mod):
    """The renderer's hit point moves with the pixel jitter, at most half a pixel from the centre
    ray's, where the probe sits.  Pixels 8 away in x and in y differ from the pixel by no more than
    3 standard errors of the difference, sqrt(2) se: the radiance changes by at most 6 sqrt(2) se
    over 8 pixels, so by at most 0.53 se over the half pixel -- a tenth of the test's 5."""
    px, py = EST_PIXEL
    m0, se0 = mean_se(pinned_pixel(px, py))
    assert np.all(se0 < 0.03 * m0)  # the 8 seeds resolve L_o to 3 %
    for dx, dy in ((8, 0), (0, 8)):
        m1, se1 = mean_se(pinned_pixel(px + dx, py + dy))
        assert np.all(np.abs(m1 - m0) <= 3 * np.sqrt(se0 ** 2 + se1 ** 2)), (dx, dy, m0, m1, se0, se1)


# ---------------------------------------------------------------- GPU ----------

class World:
    def __init__(self, rtmi_mod, gpu_ctx, scene):
        self.geom = geometry(rtmi_mod, scene)
        self.scene = rtmi_mod.Scene(gpu_ctx, self.geom)
        surf = CORNELL_SURF if scene == "cornell" else ARCHWAY_SURF
        self.tri = np.array(surf, np.int32)
        self.pos = surface_points(self.geom, surf)
        self.ids = np.array(IDS, np.uint32)


@pytest.fixture(scope="module")
def worlds(rtmi_mod, gpu_ctx):
    made = {}

    def get(scene):
        if scene not in made:
            made[scene] = World(rtmi_mod, gpu_ctx, scene)
        return made[scene]

    yield get
    for w in made.values():
        w.scene.close()


def gpu_params(rtmi_mod, **kw):
    kw.setdefault("spp_split", 1)
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
def test_first_directions_bit_for_bit(rtmi_mod, oracle_mod, gpu_ctx, worlds):
    w = worlds("cornell")
    tri, pos, ids = w.tri[:3], w.pos[:3], w.ids[:3]
    assert list(tri) == [2, 14, 30]
    left_out = total = 0
    for first in (0, 5):
        p = gpu_params(rtmi_mod, spp=2, max_bounces=2)
        got = rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos, tri, ids, first_sample=first, want_dir=True)
        want, sel = first_dirs(oracle_mod, w.geom, pos, tri, ids, first, p.seed)
        assert got["dir"].shape == (3, SECTORS, 3)
        assert np.array_equal(bits(got["dir"])[sel], bits(want)[sel])
        left_out += int((~sel).sum())
        total += sel.size
    assert left_out <= total // 1000  # expected 2.4e-6 of the rays


def restate_two_cast(oracle_mod, geom, pos, tri, ids, p, first):
    """rt_probe_radiance at max_bounces = 2: one cast per path.  -> rad, irr (n, 144, 3) float32
    and ok (n, 144): sectors all of whose samples' first directions could be restated."""
    n = len(tri)
    tri_all = geom.all_triangles()
    N = oracle_mod.normals(tri_all)[tri]
    split = max(1, p.spp_split)
    per = p.spp // split
    L = np.zeros((p.spp, n, SECTORS, 3), np.float32)
    Lc = np.zeros_like(L)
    ok = np.ones((n, SECTORS), bool)
    for j in range(p.spp):
        dr, sel = first_dirs(oracle_mod, geom, pos, tri, ids, first + j, p.seed)
        ok &= sel
        o = pos[:, None, :] + dr * f32(1e-5)
        d = normalize3(dr)
        c = dot3(N[:, None, :], d)
        _, hit = oracle_mod.intersect(tri_all, geom.n_surf, geom.n_light, geom.light_group, o.reshape(-1, 3),
                                      d.reshape(-1, 3), p.t_scale, p.hit_rule)
        hit = hit.reshape(n, SECTORS)
        val = np.zeros((n, SECTORS, 3), np.float32)  # a surface: depth 2 == max_bounces -> 0
        val[hit == -1] = f32(1.0) * f32(p.env_light)
        light = (hit != -1) & ((hit >> 30) & 3 == 1)
        idx = hit & 0x3FFFFFFF
        for li in np.unique(idx[light]):
            if p.hit_rule == 1:  # the light triangle's index
                e = geom.emission[li]
            else:                # the light plane's index: its triangles share one emission
                grp = geom.emission[geom.light_group == li]
                assert len(grp) and np.all(grp == grp[0])
                e = grp[0]
            val[light & (idx == li)] = f32(1.0) * e
        L[j] = val
        Lc[j] = val * c[..., None]

    def fold(v):
        tot = None
        for ch in range(split):
            acc = np.zeros((n, SECTORS, 3), np.float32)
            for j in range(ch * per, (ch + 1) * per):
                acc = acc + v[j]
            tot = acc if tot is None else tot + acc
        return tot / f32(p.spp)

    return fold(L), fold(Lc), ok


# (id, scene, hit rule, env_light, t_scale or None for the default 720, points moved off their surfaces)
TWO_CAST_CASES = [
    ("cornell-rule1", "cornell", 1, 0.0, None, False),   # the candidate table, one mask word
    ("cornell-rule0", "cornell", 0, 0.0, None, False),
    ("archway-rule1", "archway", 1, 0.25, None, False),  # two mask words; first casts that miss
    # the CPU rule's table serves t_scale >= 256: below it the casts take the two-phase filter
    ("cornell-rule0-filter", "cornell", 0, 0.0, 128.0, False),
    # points 20 behind their surfaces, outside the filter's origin bound (8 and 11): the plain scan (and
    # the table, where there is one, keeps every triangle for an origin off its surface)
    ("archway-rule0-scan", "archway", 0, 0.25, 128.0, True),
    ("cornell-rule1-far", "cornell", 1, 0.5, None, True),
]
# The instantiations of k_probe (sampler x hit rule x {table of one mask word, table of four,
# exact BVH, filter / scan}) that neither the cases above (uniform sampler) nor the other tests of
# this file launch, once each at 8 samples in 4 chunks.  One cast per path: the sampler does not
# enter the result, the kernel it selects does.
# (id, scene, hit rule, env_light, t_scale, far, sampler, exact BVH)
BEYOND_T = 32768.0  # past the filter's and the tables' t_scale range: the plain scan
INSTANTIATION_CASES = [
    ("archway-rule0-table4", "archway", 0, 0.25, None, False, 0, False),
    ("archway-rule1-scan", "archway", 1, 0.25, BEYOND_T, False, 0, False),
    ("cornell-rule0-bvh", "cornell", 0, 0.0, None, False, 0, True),
    ("cornell-rule0-cosine", "cornell", 0, 0.0, None, False, 1, False),
    ("archway-rule0-table4-cosine", "archway", 0, 0.25, None, False, 1, False),
    ("archway-rule1-table4-cosine", "archway", 1, 0.25, None, False, 1, False),
    ("cornell-rule0-bvh-cosine", "cornell", 0, 0.0, None, False, 1, True),
    ("cornell-rule1-bvh-cosine", "cornell", 1, 0.0, None, False, 1, True),
    ("cornell-rule0-filter-cosine", "cornell", 0, 0.0, 128.0, False, 1, False),
    ("archway-rule1-scan-cosine", "archway", 1, 0.25, BEYOND_T, False, 1, False),
]
TWO_CAST_PARAMS = ([c + (0, False, spp, split) for c in TWO_CAST_CASES for spp, split in [(1, 1), (5, 1), (8, 4)]] +
                   [c + (8, 4) for c in INSTANTIATION_CASES])


@pytest.mark.gpu
@pytest.mark.parametrize("scene,rule,env,t_scale,far,sampler,bvh,spp,split", [c[1:] for c in TWO_CAST_PARAMS],
                         ids=[f"{c[0]}-{c[-2]}-{c[-1]}" for c in TWO_CAST_PARAMS])
def test_two_cast_paths_bit_for_bit(rtmi_mod, oracle_mod, gpu_ctx, worlds, scene, rule, env, t_scale, far, sampler, bvh,
                                    spp, split):
    w = worlds(scene)
    first = 3
    kw = {} if t_scale is None else {"t_scale": t_scale}
    p = gpu_params(rtmi_mod, spp=spp, spp_split=split, max_bounces=2, hit_rule=rule, env_light=env, sampler=sampler, **kw)
    pos = w.pos
    if far:
        pos = (w.pos - f32(20.0) * oracle_mod.normals(w.geom.all_triangles())[w.tri]).astype(np.float32)
    rad, irr, ok = restate_two_cast(oracle_mod, w.geom, pos, w.tri, w.ids, p, first)
    assert ok.mean() >= 0.999
    if env > 0:
        assert (rad == f32(env)).all(axis=-1).any(), "no first cast missed: env_light is not exercised"
    assert rad.any()
    scene_ = w.scene
    if bvh:
        scene_ = rtmi_mod.Scene(gpu_ctx, w.geom)
        scene_.set_accel(rtmi_mod.ACCEL_BVH)
    try:
        for n in (1, 3, 5):
            got = rtmi_mod.probe.radiance(gpu_ctx, scene_, p, pos[:n], w.tri[:n], w.ids[:n], first_sample=first)
            assert got["casts"] == n * SECTORS * spp
            k = ok[:n]
            assert np.array_equal(bits(got["rad"])[k], bits(rad[:n])[k])
            assert np.array_equal(bits(got["irr"])[k], bits(irr[:n])[k])
    finally:
        if bvh:
            scene_.close()


@pytest.mark.gpu
def test_invariance_at_full_depth(rtmi_mod, gpu_ctx, worlds):
    import torch
    P = rtmi_mod.probe
    w = worlds("cornell")
    p = gpu_params(rtmi_mod, spp=8, max_bounces=80)
    ref = P.radiance(gpu_ctx, w.scene, p, w.pos, w.tri, w.ids, want_dir=True)
    assert ref["rad"].any() and ref["casts"] > 5 * SECTORS * 8
    keys = ("rad", "irr", "dir")

    def same(a, b, sel=slice(None)):
        return all(a[k].tobytes() == b[k][sel].tobytes() for k in keys)

    # a second run; one by one; in reverse order
    assert same(P.radiance(gpu_ctx, w.scene, p, w.pos, w.tri, w.ids, want_dir=True), ref)
    casts = []
    for i in range(5):
        one = P.radiance(gpu_ctx, w.scene, p, w.pos[i:i + 1], w.tri[i:i + 1], w.ids[i:i + 1], want_dir=True)
        assert same(one, ref, slice(i, i + 1)), i
        casts.append(one["casts"])
    assert sum(casts) == ref["casts"]
    rev = P.radiance(gpu_ctx, w.scene, p, w.pos[::-1], w.tri[::-1], w.ids[::-1], want_dir=True)
    assert same(rev, ref, slice(None, None, -1)) and rev["casts"] == ref["casts"]
    # the exact BVH against the default route (the candidate table)
    assert w.scene.ctab_info(1)["built"]
    with rtmi_mod.Scene(gpu_ctx, w.geom) as sb:
        sb.set_accel(rtmi_mod.ACCEL_BVH)
        bvh = P.radiance(gpu_ctx, sb, p, w.pos, w.tri, w.ids, want_dir=True)
    assert same(bvh, ref) and bvh["casts"] == ref["casts"]
    # the device entry on a stream of its own; the cast counter is accumulated into
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(w.pos).to(dev)
    d_tri = torch.from_numpy(w.tri).to(dev)
    d_ids = torch.from_numpy(w.ids.view(np.int32)).to(dev)
    d_out = [torch.full((5, SECTORS, 3), float("nan"), dtype=torch.float32, device=dev) for _ in keys]
    d_casts = torch.full((1,), 5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    P.radiance_device(gpu_ctx, w.scene, p, d_pos.data_ptr(), d_tri.data_ptr(), d_ids.data_ptr(), 5, 0,
                      d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(), d_casts.data_ptr(),
                      stream.cuda_stream)
    stream.synchronize()
    assert same({k: t.cpu().numpy() for k, t in zip(keys, d_out)}, ref)
    assert int(d_casts.item()) == 5 + ref["casts"]
    # a device list is not checked on the host: a surface or an id out of range gives that point zeros
    bad_tri, bad_ids = w.tri.copy(), w.ids.copy()
    bad_tri[1], bad_ids[3] = w.geom.n_surf, MAX_ID
    d_tri.copy_(torch.from_numpy(bad_tri))
    d_ids.copy_(torch.from_numpy(bad_ids.view(np.int32)))
    for t in d_out:
        t.fill_(float("nan"))
    d_casts.zero_()
    torch.cuda.synchronize()
    P.radiance_device(gpu_ctx, w.scene, p, d_pos.data_ptr(), d_tri.data_ptr(), d_ids.data_ptr(), 5, 0,
                      d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(), d_casts.data_ptr(),
                      stream.cuda_stream)
    stream.synchronize()
    got = {k: t.cpu().numpy() for k, t in zip(keys, d_out)}
    good = [0, 2, 4]
    assert all(got[k][good].tobytes() == ref[k][good].tobytes() for k in keys)
    assert not got["rad"][[1, 3]].any() and not got["irr"][[1, 3]].any() and np.isnan(got["dir"][[1, 3]]).all()
    assert int(d_casts.item()) == sum(casts[i] for i in good)
    # two batches of 8 samples combine into the 16-sample result of two chunks
    p1 = gpu_params(rtmi_mod, spp=8, spp_split=1, max_bounces=80)
    a = ref
    b = P.radiance(gpu_ctx, w.scene, p1, w.pos, w.tri, w.ids, first_sample=8)
    p2 = gpu_params(rtmi_mod, spp=16, spp_split=2, max_bounces=80)
    both = P.radiance(gpu_ctx, w.scene, p2, w.pos, w.tri, w.ids)
    for k in ("rad", "irr"):
        comb = (a[k] * f32(8) + b[k] * f32(8)) / f32(16)
        assert comb.dtype == np.float32 and comb.tobytes() == both[k].tobytes()
    assert both["casts"] == a["casts"] + b["casts"]
    assert a["rad"].tobytes() != b["rad"].tobytes()


def estimator_point(rtmi_mod, gpu_ctx, scene, geom):
    """The hit of the pixel's centre ray (rt_intersect): the surface and the hit point."""
    px, py = EST_PIXEL
    d = np.array([px + 0.5 - EST_W / 2, py + 0.5 - EST_W / 2, EST_W], np.float32)
    d = normalize3(d)  # no yaw: the camera's rotations are identities
    o = np.array(rtmi_mod.CAMERAS["cornell"][:3], np.float32)
    t, hit = rtmi_mod.intersect(gpu_ctx, scene, o[None], d[None], float(EST_W), rtmi_mod.RT_HIT_RULE_GPU)
    assert hit[0] != -1 and (int(hit[0]) >> 30) & 3 == rtmi_mod.RT_HIT_TYPE_SURFACE
    surf = int(hit[0]) & 0x3FFFFFFF
    D = d * f32(EST_W)
    return surf, (o + t[0] * D).astype(np.float32)


EST_PROBE_SPP = 256


@pytest.mark.gpu
def test_estimator_against_the_pinned_renderer(rtmi_mod, oracle_mod, gpu_ctx, worlds):
    """L_o = 2 albedo mean_k(out_irr[k]) per channel: the uniform sampler's first bounce weighs a
    path by brdf cos / pdf = (albedo / pi) cos 2 pi, the sectors are equal solid angles, and
    the probe's tail is the renderer's.  Both sides over 8 seeds; 256 samples per sector put
    the probe's error at the renderer's (about 2 % of L_o each), so that out_rad in place of
    out_irr -- larger by 1 / the radiance-weighted mean cosine, about 2 -- is tens of standard
    errors away and fails the same criterion."""
    w = worlds("cornell")
    surf, pos = estimator_point(rtmi_mod, gpu_ctx, w.scene, w.geom)
    albedo = w.geom.albedo[surf].astype(np.float64)
    assert albedo.min() < albedo.max(), "a coloured wall tells the channels apart"
    lo_mean, lo_se = mean_se(pinned_pixel(*EST_PIXEL))
    irr, rad = [], []
    for seed in EST_SEEDS:
        p = gpu_params(rtmi_mod, width=EST_W, height=EST_W, spp=EST_PROBE_SPP, max_bounces=EST_M, seed=seed,
                       sampler=rtmi_mod.RT_SAMPLER_UNIFORM)
        assert p.t_scale == EST_W
        got = rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos[None], [surf], [3])
        irr.append(2.0 * albedo * got["irr"][0].astype(np.float64).mean(axis=0))
        rad.append(2.0 * albedo * got["rad"][0].astype(np.float64).mean(axis=0))
    pi_mean, pi_se = mean_se(irr)
    pr_mean, pr_se = mean_se(rad)
    print("L_o", lo_mean, lo_se, "probe irr", pi_mean, pi_se, "probe rad", pr_mean, pr_se)
    assert np.all(np.abs(pi_mean - lo_mean) <= 5 * np.sqrt(pi_se ** 2 + lo_se ** 2))
    # negative control: the radiance is not the irradiance
    assert np.all(np.abs(pr_mean - lo_mean) > 5 * np.sqrt(pr_se ** 2 + lo_se ** 2))


@pytest.mark.gpu
def test_samplers_agree(rtmi_mod, gpu_ctx, worlds):
    w = worlds("cornell")
    surf, pos = estimator_point(rtmi_mod, gpu_ctx, w.scene, w.geom)
    res = {}
    for sampler in (rtmi_mod.RT_SAMPLER_UNIFORM, rtmi_mod.RT_SAMPLER_COSINE):
        vals = []
        for seed in EST_SEEDS:
            p = gpu_params(rtmi_mod, width=EST_W, height=EST_W, spp=EST_PROBE_SPP, max_bounces=EST_M, seed=seed,
                           sampler=sampler)
            got = rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos[None], [surf], [3], want_irr=False)
            vals.append(got["rad"][0].astype(np.float64).mean(axis=0))
        res[sampler] = mean_se(vals)
    (mu, su), (mc, sc) = res[rtmi_mod.RT_SAMPLER_UNIFORM], res[rtmi_mod.RT_SAMPLER_COSINE]
    print("uniform", mu, su, "cosine", mc, sc)
    assert np.all(mu > 0) and np.all(su > 0) and np.all(sc > 0)
    assert np.all(su < 0.05 * mu) and np.all(sc < 0.05 * mc)  # the agreement is a statement at 5 %
    assert not np.array_equal(mu, mc)
    assert np.all(np.abs(mu - mc) <= 5 * np.sqrt(su ** 2 + sc ** 2))


@pytest.mark.gpu
def test_arguments(rtmi_mod, oracle_mod, gpu_ctx, worlds):
    L = rtmi_mod.lib()
    w = worlds("cornell")
    n = 2
    pos, tri, ids = w.pos[:n].copy(), w.tri[:n].copy(), w.ids[:n].copy()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    up = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    sentinel = f32(-7.5)
    rad = np.full((n, SECTORS, 3), sentinel, np.float32)

    def call(ctx=gpu_ctx.handle, scene=w.scene.handle, params=None, pos_=pos, tri_=tri, ids_=ids, n_=n, out=rad,
             **kw):
        p = gpu_params(rtmi_mod, **{"spp": 4, "max_bounces": 3, **kw}) if params is None else params
        ref = ctypes.byref(p) if p is not False else None
        return L.rt_probe_radiance(ctx, scene, ref, None if pos_ is None else fp(pos_),
                                   None if tri_ is None else ip(tri_), None if ids_ is None else up(ids_), n_, 0,
                                   None if out is None else fp(out), None, None, None)

    def refused(word, **kw):
        assert call(**kw) == rtmi_mod._lib.RT_E_INVALID, word
        assert word.encode() in L.rt_last_error(), (word, L.rt_last_error())
        assert np.all(rad == sentinel), word

    refused("ctx", ctx=None)
    refused("scene", scene=None)
    refused("params", params=False)
    refused("pos", pos_=None)
    refused("tri", tri_=None)
    refused("ids", ids_=None)
    refused("out_rad", out=None)
    refused("n < 0", n_=-1)
    refused("tri[1]", tri_=np.array([0, w.geom.n_surf], np.int32))
    refused("tri[0]", tri_=np.array([-1, 0], np.int32))
    refused("ids[1]", ids_=np.array([MAX_ID - 1, MAX_ID], np.uint32))
    refused("spp", spp=0)
    refused("spp_split", spp_split=3)
    refused("max_bounces", max_bounces=0)
    # n = 0 writes nothing, whatever the pointers
    assert call(n_=0) == 0 and call(n_=0, pos_=None, tri_=None, ids_=None, out=None) == 0
    assert np.all(rad == sentinel)
    # the largest id, the last surface, optional outputs left out: accepted
    assert call(ids_=np.array([MAX_ID - 1, 0], np.uint32), tri_=np.array([w.geom.n_surf - 1, 0], np.int32)) == 0
    assert np.all(rad != sentinel)
    # max_bounces = 1: the path ends before its cast
    p = gpu_params(rtmi_mod, spp=4, max_bounces=1)
    got = rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos, tri, ids, want_dir=True)
    assert got["casts"] == 0 and not got["rad"].any() and not got["irr"].any()
    want, sel = first_dirs(oracle_mod, w.geom, pos, tri, ids, 0, p.seed)
    assert np.array_equal(bits(got["dir"])[sel], bits(want)[sel])
    with pytest.raises(ValueError):
        rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos, tri[:1], ids)
    with pytest.raises(rtmi_mod.RtError) as e:
        rtmi_mod.probe.radiance(gpu_ctx, w.scene, p, pos, [0, 99], ids)
    assert e.value.code == rtmi_mod._lib.RT_E_INVALID and "tri[1]" in str(e.value)
