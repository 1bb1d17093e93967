"""The radiance map's sampler, rebuild and TD fold on crafted Q rows, bit for bit against the
restatement (oracle/).

The learned maps of test_sarsa.py reach the corners of this code a handful of times at best:
sarsa_sample's fallback to the reference's binary search (a draw equal to a CDF entry, a NaN in
the row), plateaus and CDFs that end below 1, rows whose largest Q occurs twice, and the fold at
visit counts and sums past float32's integers.  Here both maps are loaded with rows built to sit
on those corners (RadianceMap.write on the device, Sarsa.load_q on the restatement), on Cornell
with the GPU preset's geometry, seed 1984.

A row family is assigned by volume index modulo the number of families, its special sector j
rotates with the volume index.  That a case reaches what it is meant to reach is asserted on the
restatement's own counters (Sarsa.sample_stats, Sarsa.search_stats), never on the device's.
"""
import numpy as np
import pytest

S = 144
SEED = 1984
N_VOLUMES = 24526  # Cornell, GPU preset, AREA_PER_SAMPLE 0.001
FLOOR = (np.float32(1) / np.float32(144)) * np.float32(0.8)  # RADIANCE_THRESHOLD


def _same_bits_nan_aware(a, b):
    """bit-exact, except that NaN payloads may differ between the GPU and x86"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- row families ----------

def _signed(rng, n):
    """normal deviates, a third of them negative: P(N(mu, 1) < 0) = 1/3 at mu = 0.4307"""
    return rng.normal(0.4307, 1.0, (n, S)).astype(np.float32)


def _fam_fresh(rng, fresh, j):
    return fresh.copy()


def _fam_dominant(rng, fresh, j):
    q = np.full((len(j), S), FLOOR, np.float32)
    q[np.arange(len(j)), j] = 1e6
    return q


def _fam_single(rng, fresh, j):
    q = np.zeros((len(j), S), np.float32)
    q[np.arange(len(j)), j] = 1.0
    return q


def _fam_pair(rng, fresh, j):
    q = _fam_single(rng, fresh, j)
    q[np.arange(len(j)), (j + 37) % S] = 1.0
    return q


def _fam_zero(rng, fresh, j):
    return np.zeros((len(j), S), np.float32)


def _fam_tiny(rng, fresh, j):
    return np.full((len(j), S), 1e-12, np.float32)


def _fam_signed(rng, fresh, j):
    return _signed(rng, len(j))


def _fam_nan5(rng, fresh, j):
    q = _signed(rng, len(j))
    at = np.argsort(rng.random((len(j), S)), axis=1)[:, :5]  # five distinct sectors per row
    np.put_along_axis(q, at, np.float32(np.nan), axis=1)
    return q


def _fam_inf(rng, fresh, j):
    q = np.full((len(j), S), FLOOR, np.float32)
    q[np.arange(len(j)), j] = np.inf
    return q


def _fam_twin_max(rng, fresh, j):
    """the largest Q twice, at j and (j + 37) % 144: the reference's scan keeps the first"""
    q = _signed(rng, len(j))
    top = q.max(axis=1) + np.float32(1)
    q[np.arange(len(j)), j] = top
    q[np.arange(len(j)), (j + 37) % S] = top
    return q


def _fam_nan0(rng, fresh, j):
    """NaN in sector 0: no later Q compares above it, the scan never leaves sector 0"""
    q = _signed(rng, len(j))
    q[:, 0] = np.nan
    return q


FINITE = (("fresh", _fam_fresh), ("dominant", _fam_dominant), ("single", _fam_single), ("pair", _fam_pair),
          ("zero", _fam_zero), ("tiny", _fam_tiny), ("signed", _fam_signed))
# the frozen frames add the non-finite rows and the max-direction sampler's two corner rows
FROZEN = FINITE + (("nan5", _fam_nan5), ("inf", _fam_inf), ("twin_max", _fam_twin_max), ("nan0", _fam_nan0))


def build_rows(fresh, families, shift=0):
    """(n, 144) float32: volume v gets family (v + shift) % len(families), special sector
    ((v + shift) // len(families)) % 144"""
    n, nf = fresh.shape[0], len(families)
    rows = np.empty((n, S), np.float32)
    v = np.arange(n) + shift
    for f, (_name, make) in enumerate(families):
        at = np.nonzero(v % nf == f)[0]
        rows[at] = make(np.random.default_rng([SEED, f, shift]), fresh[at], (v[at] // nf) % S)
    return rows


class World:
    """Geometry, camera, the fresh map's rows and the crafted row sets: built once, shared, never
    changed.  Everything here comes from the restatement alone."""

    def __init__(self, rtmi_mod, oracle_mod):
        self.rtmi, self.oracle = rtmi_mod, oracle_mod
        self.geom = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
        self.cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"])
        self.ocam = oracle_mod.camera(rtmi_mod.CAMERAS["cornell"])
        om = oracle_mod.Sarsa(self.geom, SEED)
        assert om.n_volumes == N_VOLUMES
        self.n = om.n_volumes
        self.fresh_state = om.read()
        fresh = self.fresh_state[0]
        self.finite = build_rows(fresh, FINITE)
        self.frozen = build_rows(fresh, FROZEN)
        self.frozen_shifted = build_rows(fresh, FROZEN, shift=5)
        self.dense = self._grid_dense(om, fresh)
        # the inputs are what their families claim
        names, nf = [f for f, _ in FROZEN], len(FROZEN)
        twin = self.frozen[names.index("twin_max")::nf]
        assert ((twin == twin.max(axis=1, keepdims=True)).sum(axis=1) == 2).all()
        assert len(np.unique(np.argmax(twin, axis=1))) > 100  # the first maximum rotates over the sectors
        assert np.isnan(self.frozen[names.index("nan0")::nf, 0]).all()
        assert (np.isnan(self.frozen[names.index("nan5")::nf]).sum(axis=1) == 5).all()
        assert 0.3 < (self.frozen[names.index("signed")::nf] < 0).mean() < 0.37
        for a in (self.finite, self.frozen, self.frozen_shifted, self.dense):
            a.setflags(write=False)

    @staticmethod
    def _grid_dense(om, fresh):
        """The floor with sector 0 raised until cdf[0] lies in [0.5, 0.6): every later entry is then a
        multiple of 2^-24, the grid of the sampler's 24-bit draws.  cdf[0] = x c / (x c + R) for
        Q[0] = x, so one reading of the odds at x gives the x of the wanted odds, per volume."""
        q = np.full(fresh.shape, FLOOR, np.float32)
        want = 0.55 / 0.45
        for _ in range(3):
            om.load_q(q)
            c0 = om.read()[1][:, 0].astype(np.float64)
            if ((c0 >= 0.5) & (c0 < 0.6)).all():
                break
            q[:, 0] = (q[:, 0].astype(np.float64) * want / (c0 / (1.0 - c0))).astype(np.float32)
        om.load_q(q)
        cdf = om.read()[1]
        assert ((cdf[:, 0] >= 0.5) & (cdf[:, 0] < 0.6)).all()
        assert (np.ldexp(cdf[:, 1:].astype(np.float64), 24) % 1.0 == 0.0).all()  # on the draws' grid
        return q

    def params(self, width, height, spp, split, hit_rule):
        return self.rtmi.default_params(self.rtmi.RT_PRESET_GPU, width=width, height=height, spp=spp,
                                        spp_split=split, hit_rule=hit_rule, env_light=0.5)

    def oracle_map(self, rows=None):
        om = self.oracle.Sarsa(self.geom, SEED)
        if rows is not None:
            om.load_q(rows)
        return om


@pytest.fixture(scope="module")
def world(rtmi_mod, oracle_mod):
    return World(rtmi_mod, oracle_mod)


@pytest.fixture(scope="module")
def gpu_scene(rtmi_mod, gpu_ctx, world):
    sc = rtmi_mod.Scene(gpu_ctx, world.geom)
    yield sc
    sc.close()


@pytest.fixture
def gpu_map(rtmi_mod, gpu_ctx, gpu_scene):
    """a fresh device map per test (a render advances its frame counter)"""
    rm = rtmi_mod.sarsa.RadianceMap(gpu_ctx, gpu_scene, SEED)
    assert rm.n_volumes == N_VOLUMES
    yield rm
    rm.close()


def assert_maps_equal(got, want, nan_aware=False, what=""):
    for name, a, b in zip(("Q", "CDF", "visits", "irradiance"), got, want):
        if a.dtype == np.float32:
            same = _same_bits_nan_aware(a, b) if nan_aware else _same_bits(a, b)
        else:
            same = np.array_equal(a, b)
        assert same, f"{what}: {name} differs in {int((a != b).sum())} entries"


# ---------------------------------------------------------------- 1. rebuild ----------

@pytest.mark.gpu
def test_gpu_rebuild_equals_oracle_on_crafted_rows(world, gpu_map):
    """rebuild_volume through rt_sarsa_write on every family, the non-finite ones included: Q, CDF,
    visits and irradiance as the restatement's load_q gives them; then a sub-range that starts and
    ends inside a 256-volume block, with visits: the rows outside it keep what they had."""
    rm, om = gpu_map, world.oracle_map()
    assert_maps_equal(rm.read(), world.fresh_state, what="fresh map")
    rm.write(world.frozen)
    om.load_q(world.frozen)
    assert_maps_equal(rm.read(), om.read(), nan_aware=True, what="all families")
    cdf = om.read()[1]
    nf = len(FROZEN)
    names = [f for f, _ in FROZEN]
    dom = cdf[names.index("dominant")::nf]
    assert (dom[:, -1] >= 1.0 - 2.0 ** -24).all() and (dom[:, -1] == 1.0).mean() > 0.5  # most end at exactly 1
    assert (dom[:, -1] == dom[:, -2]).mean() > 0.9                    # on a plateau above j
    assert (cdf[names.index("zero")::nf] == 0.0).all()
    assert (np.abs(cdf[names.index("tiny")::nf, -1] - 0.42) < 0.02).all()
    assert np.isnan(cdf[names.index("inf")::nf, -1]).all()
    v0, n = 1000, 777                                                 # blocks 3 and 6 of 256 volumes
    assert v0 % 256 and (v0 + n) % 256 and (v0 + n) // 256 > v0 // 256 + 1
    vis = np.random.default_rng(SEED).integers(0, 2 ** 32, (world.n, S), dtype=np.uint32)
    vis[:v0] = 0
    vis[v0 + n:] = 0
    rows = world.frozen.copy()
    rows[v0:v0 + n] = world.frozen_shifted[v0:v0 + n]
    rm.write(rows[v0:v0 + n], visits=vis[v0:v0 + n], v0=v0)
    om.load_q(rows)
    om.set_visits(vis)
    assert_maps_equal(rm.read(), om.read(), nan_aware=True, what="sub-range")


# ---------------------------------------------------------------- 2. learning ----------

def _learn_and_compare(world, rm, om, p, frames):
    op = world.oracle.params_from(p)
    for frame in range(frames):
        img_o, casts_o = om.render(world.ocam, op, 1)
        img_g, casts_g = rm.render(world.cam, p, 1)
        assert casts_g == casts_o, (frame, casts_g, casts_o)
        assert _same_bits(img_g, img_o), f"frame {frame}: image differs in {int((img_g != img_o).sum())} values"
        assert_maps_equal(rm.read(), om.read(), what=f"frame {frame}")
        assert rm.frame_stats() == om.stats(), frame


@pytest.mark.gpu
@pytest.mark.parametrize("split", (1, 4))
@pytest.mark.parametrize("hit_rule", (0, 1))
def test_gpu_learning_on_finite_rows_equals_oracle(world, gpu_map, split, hit_rule):
    """Two learning frames of 64 x 64 x 16 from the finite families: image, casts, Q, CDF, visits,
    irradiance and the frame statistics after each.  Frame 1 samples the written rows (plateaus,
    CDFs that end below 1, failed searches), frame 2 the cdf_top the apply rebuilt, and a third
    frame in max-direction mode its qmax."""
    rm, om = gpu_map, world.oracle_map(world.finite)
    rm.write(world.finite)
    p = world.params(64, 64, 16, split, hit_rule)
    # what frame 1 reaches, on the restatement alone (a second map: om stays at frame 0)
    probe = world.oracle_map(world.finite)
    probe.render(world.ocam, world.oracle.params_from(p), 1)
    samples, failed, _ = probe.sample_stats()
    events = {name: int(probe.read()[2][f::len(FINITE)].sum()) for f, (name, _) in enumerate(FINITE)}
    print(f"split {split} rule {hit_rule}: {samples} CDF samples, {failed} failed searches, events {events}")
    assert failed > 0
    assert events.pop("zero") == 0  # no search of a zero row succeeds: nothing to learn from
    assert min(events.values()) >= 1000, events
    _learn_and_compare(world, rm, om, p, 2)
    # a third frame through the max-direction sampler: it takes the qmax the apply rebuilt (the zero
    # rows are still all equal: sector 0, whose pdf is 0, so pixels may be non-finite)
    rm.set_sampling(world.rtmi.sarsa.SAMPLE_MAX)
    om.set_sampling(1)
    img_o, casts_o = om.render(world.ocam, world.oracle.params_from(p), 1)
    img_g, casts_g = rm.render(world.cam, p, 1)
    assert casts_g == casts_o
    assert _same_bits_nan_aware(img_g, img_o)
    assert_maps_equal(rm.read(), om.read(), what="max-direction frame")
    assert rm.frame_stats() == om.stats()
    assert rm.frames == 3


# ---------------------------------------------------------------- 3. frozen ----------

@pytest.fixture(scope="module")
def frozen_oracle(world):
    """the restatement's map with every family loaded; render_rect leaves it as it is"""
    return world.oracle_map(world.frozen)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1), ids=("cdf", "max"))
@pytest.mark.parametrize("hit_rule", (0, 1))
def test_gpu_frozen_frame_on_all_rows_equals_oracle(world, gpu_map, frozen_oracle, mode, hit_rule):
    """RT_SARSA_TD_OFF on every family, NaN and inf rows included, in both sampling modes: the image
    (NaN-aware) and the casts of the restatement's render_rect, and the map untouched.  In max
    mode the twin_max rows hold their largest Q twice (the first counts) and the nan0 rows a NaN in
    sector 0 (the scan stays there)."""
    T = world.rtmi.sarsa
    rm, om = gpu_map, frozen_oracle
    rm.write(world.frozen)
    rm.set_td_mode(T.TD_OFF)
    rm.set_sampling(T.SAMPLE_MAX if mode else T.SAMPLE_CDF)
    om.set_sampling(mode)
    before = rm.read()
    p = world.params(64, 64, 16, 4, hit_rule)
    img_o, casts_o = om.render_rect(world.ocam, world.oracle.params_from(p), (0, 0, 64, 64))
    if not mode:
        samples, failed, _ = om.sample_stats()
        assert failed > 0 and samples > failed
    img_g, casts_g = rm.render(world.cam, p, 1)
    assert casts_g == casts_o, (casts_g, casts_o)
    assert _same_bits_nan_aware(img_g, img_o), f"image differs in {int((img_g != img_o).sum())} values"
    assert np.isfinite(img_o).any()
    assert_maps_equal(rm.read(), before, nan_aware=True, what="frozen map")


# ---------------------------------------------------------------- 4. in-frame ----------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1), ids=("cdf", "max"))
def test_gpu_in_frame_single_lane_on_finite_rows(world, gpu_map, mode):
    """RT_SARSA_TD_INFRAME with one lane (a 1 x 1 image, one chunk of 64 samples): the events run one
    at a time in sample order, the restatement's sequential rule, here from the finite families."""
    T = world.rtmi.sarsa
    rm, om = gpu_map, world.oracle_map(world.finite)
    rm.write(world.finite)
    rm.set_td_mode(T.TD_INFRAME)
    om.set_td_mode(1)
    rm.set_sampling(T.SAMPLE_MAX if mode else T.SAMPLE_CDF)
    om.set_sampling(mode)
    p = world.params(1, 1, 64, 1, 1)
    op = world.oracle.params_from(p)
    for frame in range(2):
        img_o, casts_o = om.render(world.ocam, op, 1)
        img_g, casts_g = rm.render(world.cam, p, 1)
        assert casts_g == casts_o, (frame, casts_g, casts_o)
        assert _same_bits_nan_aware(img_g, img_o), frame
        assert_maps_equal(rm.read(), om.read(), nan_aware=True, what=f"frame {frame}")
    assert om.read()[2].sum() > 20  # the rule ran


# ---------------------------------------------------------------- 5. ties ----------

@pytest.mark.gpu
def test_gpu_ties_between_draw_and_cdf_equal_oracle(world, gpu_map):
    """Grid-dense rows in every volume: 143 of a row's 144 CDF entries are multiples of 2^-24 in
    [0.5, 1], so a 24-bit draw meets one often enough to count.  One learning frame of
    64 x 64 x 64, compared like the finite rows' frames; the restatement's counters say that draws
    tied with entries and that searches probed an equal entry (sarsa_sample's fallback)."""
    rm, om = gpu_map, world.oracle_map(world.dense)
    rm.write(world.dense)
    p = world.params(64, 64, 64, 4, 1)
    probe = world.oracle_map(world.dense)
    probe.render(world.ocam, world.oracle.params_from(p), 1)
    samples, failed, _ = probe.sample_stats()
    ties, equal_probes = probe.search_stats()
    print(f"{samples} CDF samples, {failed} failed, {ties} ties, {equal_probes} searches with an equal probe")
    assert ties >= 8 and equal_probes >= 4, (ties, equal_probes)
    _learn_and_compare(world, rm, om, p, 1)


# ---------------------------------------------------------------- 6. fold ----------

FOLD_VISITS = (0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31)
FOLD_COUNTS = (0, 1, 3, 2 ** 24 + 1)
FOLD_SUMS = (0, 1, -1, 2 ** 53 + 1, 2 ** 61, -2 ** 61)
FOLD_Q = (FLOOR, np.float32(1e6), np.float32(1e-40))  # the floor, a large value, a denormal


@pytest.mark.gpu
def test_gpu_fold_equals_oracle_on_crafted_pending_sums(world, gpu_map):
    """k_sarsa_apply on given Q, visits, pending sums and counts: every combination of visits around
    2^24 and at 2^31, counts 0 / 1 / 3 / 2^24 + 1, sums 0, +-1, 2^53 + 1 and +-2^61 (fixed point
    2^-32) and Q at the floor, 1e6 and a denormal.  Q, CDF, visits and irradiance as the
    restatement folds them; sectors with count 0 keep Q and visits; then one frozen frame from
    both applied maps."""
    import torch

    T = world.rtmi.sarsa
    rm, om = gpu_map, world.oracle_map()
    rng = np.random.default_rng([SEED, 6])
    shape = (world.n, S)
    pick = [rng.integers(0, len(t), shape) for t in (FOLD_VISITS, FOLD_COUNTS, FOLD_SUMS, FOLD_Q)]
    combos = ((pick[0] * len(FOLD_COUNTS) + pick[1]) * len(FOLD_SUMS) + pick[2]) * len(FOLD_Q) + pick[3]
    n_combos = len(FOLD_VISITS) * len(FOLD_COUNTS) * len(FOLD_SUMS) * len(FOLD_Q)
    assert len(np.unique(combos)) == n_combos  # every combination occurs
    vis = np.array(FOLD_VISITS, np.uint32)[pick[0]]
    cnt = np.array(FOLD_COUNTS, np.uint32)[pick[1]]
    sums = np.array(FOLD_SUMS, np.int64)[pick[2]]
    q = np.array(FOLD_Q, np.float32)[pick[3]]
    assert int(vis.astype(np.uint64).max() + cnt.max()) < 2 ** 32
    assert (q[q == FOLD_Q[2]] > 0).all() and FOLD_Q[2] < np.finfo(np.float32).tiny

    rm.write(q, visits=vis)
    om.load_q(q)
    om.set_visits(vis)
    assert_maps_equal(rm.read(), om.read(), what="before the fold")
    ts, tc = world.rtmi.dist.td_tensors(rm, torch.device("cuda", 0))
    ts.copy_(torch.from_numpy(sums.ravel()))
    tc.copy_(torch.from_numpy(cnt.ravel().view(np.int32)))
    torch.cuda.synchronize()
    rm.apply()
    torch.cuda.synchronize()
    om.apply_pending(sums, cnt)
    got, want = rm.read(), om.read()
    assert_maps_equal(got, want, what="after the fold")
    idle = cnt == 0
    assert _same_bits(got[0][idle], q[idle]) and np.array_equal(got[2][idle], vis[idle])
    assert np.array_equal(got[2], vis + cnt)
    assert not _same_bits(got[0][~idle], q[~idle])
    assert int(tc.abs().sum().item()) == 0  # the applied counts are cleared

    rm.set_td_mode(T.TD_OFF)
    p = world.params(64, 64, 16, 4, 1)
    img_o, casts_o = om.render_rect(world.ocam, world.oracle.params_from(p), (0, 0, 64, 64))
    img_g, casts_g = rm.render(world.cam, p, 1)
    assert casts_g == casts_o
    assert _same_bits_nan_aware(img_g, img_o)
