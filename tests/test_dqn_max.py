"""The Q-network's max-direction render (RT_DQN_SAMPLE_MAX, rtmi.h): the reference's
sample_max_direction (nn_rendering_helpers.cu:491-553) in rt_render_dqn[_tiles_device], the
sampler alone (rt_dqn_sample_max) and the frame statistics (rt_dqn_render_stats).

Everything compared is bit for bit.  The restatement (restate below) is built from pieces the
suite already pins and takes nothing from the device:
  action      the scalar scan `max_idx = 0, max_q = 0; if Q[k] > max_q: take k` in numpy (scan_rows);
  direction   oracle.dqn_sample on the one-hot row of that action with the same (pix, sample,
              bounce, seed): the two samplers share Philox counter 73 and grid_dir, and the oracle
              must return the action for every row (asserted for every row used, on the CPU);
  throughput  float32 numpy: c = (N.x d.x + N.y d.y) + N.z d.z, pdf = float32(RHO) * 2, (tp * c) / pdf;
  trace       oracle.intersect from pos + dir * 1e-5f along normalize3(dir) under hit rule 1,
              loc = o + t * (d * t_scale), tp times albedo / pi, the emission, or env_light;
  Q           numpy: the selection network's Q is its folded layer 0 (np_layer0 of
              tests/test_dqn_forward_exact.py) at any position, a bias-only network's is ReLU(b4);
              for the shipped cornell_12_12.model, rt_dqn_forward.
The same loop in CDF mode (oracle.dqn_sample on the bf16 Q) equals oracle.render_dqn_wave without
a GPU, which checks the loop's camera, trace, order and fold; its per-path throughputs give the
CDF frame's statistics.

Which crafted row catches which wrong sampler: an argmax on Q x cos -- ROWS "raw-not-cos" (the
larger Q in a corner cell of small cosine) and the bias network "first"; a scan from -inf -- ROWS
"all-negative" (it would return the largest negative cell, not 0); a last-wins tie rule -- ROWS
"tie-in-block", "tie-across-blocks", "inf-twice" and the bias network "tie"; a bf16 Q row -- ROWS
"bf16-close" and the bias network "close" (two cells that round to one bf16, the larger second).
"""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from conftest import MODELS, ROOT
from test_dqn_forward_exact import bf16_round, np_layer0
from test_probe import dot3, normalize3

F = np.float32
SEED = 1984
ENV = 0.25
PI_F = F(3.14159265358979323846)
RHO = F(1) / (F(2) * PI_F)
PDF_MAX = RHO * F(2)                 # the reference's constant pdf (nn_rendering_helpers.cu:547)
THRESHOLD = F(0.0001)                # THROUGHPUT_THRESHOLD
END_MISS, END_LIGHT, END_CAP, END_NONE = 0, 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def header_define(name):
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(-?\d+)", src, flags=re.M)
    assert m, name
    return int(m.group(1))


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


# ---- the restatement ---------------------------------------------------------------------

def scan_rows(q):
    """The reference's scan per row of q (n, 144): max_idx = 0, max_q = 0.0f; for k in order:
    if Q[k] > max_q take k.  A NaN compares false, so it never wins."""
    q = np.ascontiguousarray(q, F).reshape(-1, 144)
    best = np.zeros(len(q), F)
    act = np.zeros(len(q), np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(144):
            m = q[:, k] > best
            best = np.where(m, q[:, k], best)
            act = np.where(m, np.int32(k), act)
    return act


def one_hot(act):
    q = np.zeros((len(act), 144), F)
    q[np.arange(len(act)), act] = 1
    return q


def max_step(O, tri_all, N_all, act, loc, tri, pix, sample, bounce, seed, tp):
    """direction and throughput of the max sampler for rows of one sample index; asserts the
    one-hot precondition for every row"""
    _, _, d, a = O.dqn_sample(tri_all, one_hot(act), loc, tri, pix, int(sample), int(bounce), int(seed),
                              np.ones((len(act), 3), F))
    assert np.array_equal(a, act), "oracle.dqn_sample did not return the one-hot row's cell"
    c = dot3(N_all[tri], d)
    tp = (tp * c[:, None]) / PDF_MAX
    assert d.dtype == F and tp.dtype == F
    return d, tp


def restate(O, g, ocam, p, q_of, mode="max"):
    """rt_render_dqn's frame in wavefront order, rays r = sample * n_pix + pixel (row-major).
    -> dict(img (H, W, 3), casts, tp (spp * n_pix, 3) final throughputs, end (spp * n_pix,) END_*)."""
    W_, H, spp = p.width, p.height, p.spp
    n_pix = W_ * H
    n = n_pix * spp
    tri_all = g.all_triangles()
    N_all = O.normals(tri_all)
    op = O.params_from(p)
    hit0 = O.primary_hits(tri_all, g.n_surf, g.n_light, ocam, op, (0, 0, W_, H), 0, spp)
    hit0 = np.moveaxis(hit0, 2, 0).reshape(n)
    op2 = O.params_from(p)
    op2.max_bounces = 2
    locs = []

    def grab(loc):
        locs.append(loc.copy())
        return np.ones((len(loc), 144), F)

    O.render_dqn_wave(g, ocam, op2, grab)
    surf0 = (hit0 >= 0) & (hit0 < g.n_surf)
    tp = np.ones((n, 3), F)
    end = np.full(n, END_CAP, np.int32)
    miss0, light0 = hit0 < 0, hit0 >= g.n_surf
    tp[miss0] = tp[miss0] * F(p.env_light)
    tp[light0] = tp[light0] * g.emission[hit0[light0] - g.n_surf]
    tp[surf0] = tp[surf0] * (g.albedo[hit0[surf0]] / PI_F)
    end[miss0], end[light0] = END_MISS, END_LIGHT
    loc = np.zeros((n, 3), F)
    if surf0.any():
        assert len(locs[0]) == int(surf0.sum())
        loc[surf0] = locs[0]
    tri = np.where(surf0, hit0, 0).astype(np.int32)
    live = np.flatnonzero(surf0)
    casts = n
    pi = np.arange(n) % n_pix
    pix = ((pi // W_) * p.width + pi % W_).astype(np.uint32)
    for b in range(1, p.max_bounces):
        if live.size == 0:
            break
        Q = np.ascontiguousarray(q_of(loc[live]), F)
        act = scan_rows(Q) if mode == "max" else np.full(live.size, -1, np.int32)
        d = np.zeros((live.size, 3), F)
        ntp = tp[live].copy()
        smp = live // n_pix
        for s in np.unique(smp):
            m = smp == s
            r = live[m]
            if mode == "max":
                d[m], ntp[m] = max_step(O, tri_all, N_all, act[m], loc[r], tri[r], pix[r], s, b, p.seed, tp[r])
            else:
                _, ntp[m], d[m], act[m] = O.dqn_sample(tri_all, bf16_round(Q[m]), loc[r], tri[r], pix[r], int(s), b,
                                                       int(p.seed), tp[r])
        casts += live.size
        none = act < 0                      # (CDF only: the reference then traces a zero direction)
        ntp[none] = ntp[none] * F(p.env_light)
        end[live[none]] = END_NONE
        o = loc[live] + d * F(1e-5)
        dn = normalize3(np.where(none[:, None], F(1), d))
        t, hit = O.intersect(tri_all, g.n_surf, g.n_light, g.light_group, o, dn, p.t_scale, 1)
        kind = np.where(hit == -1, 3, (hit >> 30) & 3)
        idx = hit & 0x3FFFFFFF
        miss, light, surf = ~none & (kind == 3), ~none & (kind == 1), ~none & (kind == 2)
        ntp[miss] = ntp[miss] * F(p.env_light)
        ntp[light] = ntp[light] * g.emission[idx[light]]
        ntp[surf] = ntp[surf] * (g.albedo[idx[surf]] / PI_F)
        end[live[miss]], end[live[light]] = END_MISS, END_LIGHT
        nloc = o + t[:, None] * (dn * F(p.t_scale))
        assert ntp.dtype == F and nloc.dtype == F
        tp[live] = ntp
        loc[live[surf]] = nloc[surf]
        tri[live[surf]] = idx[surf]
        live = live[surf]
    acc = np.zeros((n_pix, 3), F)
    for s in range(spp):
        acc = acc + tp[s * n_pix:(s + 1) * n_pix]
    img = (acc / F(spp)).reshape(H, W_, 3)
    with np.errstate(invalid="ignore"):
        zero = int(np.all(tp < THRESHOLD, axis=1).sum())
    return {"img": img, "casts": casts, "tp": tp, "end": end, "paths": n, "zero": zero}


# ---- the crafted rows of the sampler test ---------------------------------------------------

UNIQUE_K = (0, 1, 35, 36, 71, 72, 107, 108, 143)
SUBNORMAL = np.array([1], np.uint32).view(F)[0]


def crafted_rows():
    """(names, q (m, 144), expected action) -- the expectation written down per row, not computed"""
    rng = np.random.default_rng(SEED)
    rows, names, want = [], [], []

    def add(name, row, a):
        names.append(name)
        rows.append(np.asarray(row, F))
        want.append(a)

    for k in UNIQUE_K:
        r = rng.uniform(0.0, 1.0, 144).astype(F)
        r[k] = F(1.5)
        add(f"unique-{k}", r, k)
    r = np.full(144, 0.25, F)
    r[[40, 50, 60]] = 2.0
    add("tie-in-block", r, 40)
    r = np.full(144, 0.25, F)
    r[[50, 110]] = 2.0
    add("tie-across-blocks", r, 50)
    add("all-zeros", np.zeros(144, F), 0)
    r = -rng.uniform(1.0, 2.0, 144).astype(F)
    r[50] = F(-0.5)
    add("all-negative", r, 0)
    add("all-nan", np.full(144, np.nan, F), 0)
    r = rng.uniform(0.0, 1.0, 144).astype(F)
    r[20] = np.nan
    r[90] = F(3.0)
    add("nan-above-finite", r, 90)
    r = rng.uniform(0.0, 1.0, 144).astype(F)
    r[[30, 100]] = np.inf
    add("inf-twice", r, 30)
    r = np.full(144, -0.0, F)
    r[10] = 0.0
    add("negzero-with-zero", r, 0)
    r = np.zeros(144, F)
    r[77] = SUBNORMAL
    add("subnormal-max", r, 77)
    # cell 0 is a corner of the grid (cosine 1 - (11/12)^2 = 0.16), cell 66 next to the pole
    r = np.full(144, 0.25, F)
    r[0], r[66] = 3.0, 2.9
    add("raw-not-cos", r, 0)
    # 1 and 1 + 2^-10 are one bf16; the larger is the later cell
    r = np.full(144, 0.25, F)
    r[5], r[100] = 1.0, F(1.0) + F(2.0 ** -10)
    add("bf16-close", r, 100)
    return names, np.stack(rows), np.array(want, np.int32)


SAMPLER_N = 300            # one full and one partial workgroup of the sampler kernel
SAMPLER_SURF = (2, 30)     # two Cornell surfaces with different shading frames
SAMPLER_CASES = [(1, SEED), (7, SEED), (1, 77), (7, 77)]   # (bounce, seed)


def sampler_inputs():
    names, rows, want = crafted_rows()
    rng = np.random.default_rng(SEED + 1)
    idx = np.arange(SAMPLER_N) % len(rows)
    q = rows[idx].copy()
    extra = np.arange(SAMPLER_N) >= 2 * len(rows)              # beyond two copies: random rows
    q[extra] = rng.normal(size=(int(extra.sum()), 144)).astype(F)
    tri = np.where((np.arange(SAMPLER_N) // len(rows)) % 2 == 0, SAMPLER_SURF[0], SAMPLER_SURF[1]).astype(np.int32)
    pix = rng.integers(0, 1 << 20, SAMPLER_N).astype(np.uint32)
    tp = rng.uniform(0.1, 2.0, (SAMPLER_N, 3)).astype(F)
    return names, rows, want, idx, extra, q, tri, pix, tp


def surface_points(g, tri):
    t = g.tri[np.asarray(tri)]
    v0, v1, v2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    return (v0 + F(0.3) * (v1 - v0) + F(0.4) * (v2 - v0)).astype(F)


def sampler_expectation(O, g, bounce, seed, sample=2):
    names, rows, want, idx, extra, q, tri, pix, tp = sampler_inputs()
    act = scan_rows(q)
    assert np.array_equal(act[~extra], want[idx[~extra]]), "scan_rows disagrees with the written expectation"
    loc = surface_points(g, tri)
    d, tp2 = max_step(O, g.all_triangles(), O.normals(g.all_triangles()), act, loc, tri, pix, sample, bounce, seed, tp)
    return q, loc, tri, pix, tp, act, d, tp2


# ---- networks -------------------------------------------------------------------------------

SEL = np.arange(56, 200)


@functools.lru_cache(maxsize=None)
def selection_net():
    """(W, b, verts, q_of): Q[a] = h1[56 + a] of a random layer 0 over 12 inputs, exactly, at any
    position (rtmi.dqn.selection_weights); q_of is numpy's"""
    import rtmi
    rng = np.random.default_rng(SEED + 2)
    W0 = rng.standard_normal((200, 12)).astype(F)
    b0 = rng.uniform(0.0, 2.0, 200).astype(F)
    verts = rng.uniform(-1.0, 1.0, 12).astype(F)
    W, b = rtmi.dqn.selection_weights(W0, b0, SEL)
    return W, b, verts, lambda loc: np_layer0(W0, b0, verts, np.ascontiguousarray(loc, F).reshape(-1, 3))[:, SEL]


BIAS_ROWS = ("first", "last", "tie", "close")


@functools.lru_cache(maxsize=None)
def bias_net(kind):
    """(W, b, verts, q_of): W4 = 0 and b4 a crafted row, so Q = ReLU(b4) at every hit:
    first -- action 0, the corner cell, against a cell near the pole almost as large (raw Q, not
    Q x cos); last -- action 143; tie -- equal maxima in blocks 1 and 3, the first wins;
    close -- two cells that are one bf16, the larger second (fp32 Q, not bf16)."""
    import rtmi
    W, b = rtmi.dqn.synthetic_weights(12, seed=SEED + 3)
    W[3][:] = 0
    row = np.full(144, 0.25, F)
    row[3] = -1.0                              # (ReLU: a 0 among the cells)
    if kind == "first":
        row[0], row[66] = 3.0, 2.9
    elif kind == "last":
        row[143], row[66] = 3.0, 2.9
    elif kind == "tie":
        row[[40, 110]] = 2.0
    else:
        row[5], row[100] = 1.0, F(1.0) + F(2.0 ** -10)
    b[3][:] = row
    verts = np.random.default_rng(SEED + 4).uniform(-1.0, 1.0, 12).astype(F)
    qrow = np.maximum(row, F(0))
    return W, b, verts, lambda loc: np.tile(qrow, (len(loc), 1))


BIAS_ACTION = {"first": 0, "last": 143, "tie": 40, "close": 100}

# the frame of the restatement test: Cornell 20 x 17 (four 16 x 16 blocks, three of them partial),
# spp 3, 6 bounces, seen from the opening and pitched up: surfaces, the ceiling light and the outside
FRAME = dict(width=20, height=17, spp=3, max_bounces=6)
VIEW = ((0.0, 0.0, -2.0, 1.0), {"yaw_x": -0.35})
INSIDE = ((0.0, 0.2, -0.9, 1.0), {"yaw_x": 0.3})   # inside the box: the table / filter cast routes


def frame_params(R, **kw):
    return R.default_params(R.RT_PRESET_GPU, env_light=ENV, **{**FRAME, **kw})


def net_of(name):
    return selection_net() if name == "selection" else bias_net(name)


@functools.lru_cache(maxsize=None)
def expected(name, view="view", mode="max"):
    import oracle
    import rtmi
    g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
    pos, yaws = VIEW if view == "view" else INSIDE
    return restate(oracle, g, oracle.camera(pos, **yaws), frame_params(rtmi), net_of(name)[3], mode)


# ---------------------------------------------------------------- CPU ----------

def test_symbols_prototypes_and_constants(rtmi_mod):
    R, L = rtmi_mod, rtmi_mod.lib()
    for s, n_args in (("rt_dqn_set_sampling", 2), ("rt_dqn_get_sampling", 2), ("rt_dqn_sample_max", 13),
                      ("rt_dqn_render_stats", 3), ("rt_dqn_enable_stats", 2)):
        assert s in R._lib.EXPORTS and hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == n_args, s
    assert L.rt_dqn_sample_max.argtypes == L.rt_dqn_sample.argtypes      # rt_dqn_sample's argument list
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for proto in (r"int rt_dqn_set_sampling\(rt_dqn\* dqn, int mode\);",
                  r"int rt_dqn_get_sampling\(const rt_dqn\* dqn, int\* mode\);",
                  r"int rt_dqn_sample_max\(rt_ctx\* ctx, const rt_scene\* scene, uint64_t seed, const float\* q,",
                  r"int rt_dqn_enable_stats\(rt_ctx\* ctx, int on\);",
                  r"int rt_dqn_render_stats\(const rt_ctx\* ctx, uint64_t\* paths, uint64_t\* zero_paths\);"):
        assert re.search(proto, src), proto
    assert "nn_rendering_helpers.cu:491-553" in src and "biased" in src
    assert header_define("RT_DQN_SAMPLE_CDF") == 0 == R.dqn.SAMPLE_CDF == R.dqn.Dqn.SAMPLE_CDF == R._lib.RT_DQN_SAMPLE_CDF
    assert header_define("RT_DQN_SAMPLE_MAX") == 1 == R.dqn.SAMPLE_MAX == R.dqn.Dqn.SAMPLE_MAX == R._lib.RT_DQN_SAMPLE_MAX
    facade = open(os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd", "host",
                               "reinforcement_path_tracing.h")).read()
    assert "rt_dqn_set_sampling(net_, on ? RT_DQN_SAMPLE_MAX : RT_DQN_SAMPLE_CDF)" in facade
    assert "zero_contribution_paths()" in facade and "rt_dqn_render_stats(" in facade
    assert callable(R.dqn.sample_max) and callable(R.dqn.render_stats)


def test_null_handles_are_refused_without_a_gpu(rtmi_mod):
    R, L = rtmi_mod, rtmi_mod.lib()
    m = ctypes.c_int(5)
    for mode in (R.dqn.SAMPLE_CDF, R.dqn.SAMPLE_MAX, 7):
        assert L.rt_dqn_set_sampling(None, mode) == R._lib.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    assert L.rt_dqn_get_sampling(None, ctypes.byref(m)) == R._lib.RT_E_INVALID and m.value == 5
    assert L.rt_dqn_render_stats(None, None, None) == R._lib.RT_E_INVALID
    assert L.rt_dqn_enable_stats(None, 1) == R._lib.RT_E_INVALID
    fp = np.zeros(144, F).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.rt_dqn_sample_max(None, None, 1, fp, fp, None, None, 1, 0, 1, fp, fp, None) == R._lib.RT_E_INVALID


def test_scan_and_crafted_rows():
    """The numpy scan against a scalar loop, and against the expectation written per crafted row."""
    names, rows, want = crafted_rows()
    assert len(set(names)) == len(names) == 20
    got = scan_rows(rows)
    for name, row, a, w in zip(names, rows, got, want):
        mi, mq = 0, F(0)
        for k in range(144):
            if row[k] > mq:
                mi, mq = k, row[k]
        assert a == mi == w, (name, a, mi, w)
    # what a wrong sampler would answer on the rows that are there to catch it
    by = dict(zip(names, rows))
    c = np.array([1 - max(abs(2 * ((k // 12 + 0.5) / 12) - 1), abs(2 * ((k % 12 + 0.5) / 12) - 1)) ** 2 for k in range(144)])
    assert int(np.argmax(by["raw-not-cos"] * c)) == 66                         # Q x cos
    assert int(np.argmax(by["all-negative"])) == 50                            # a scan from -inf
    assert 143 - int(np.argmax(by["tie-across-blocks"][::-1])) == 110          # last wins
    assert 143 - int(np.argmax(by["tie-in-block"][::-1])) == 60
    assert int(np.argmax(bf16_round(by["bf16-close"]))) == 5                   # a bf16 row
    assert SUBNORMAL > 0 and SUBNORMAL == F(2.0 ** -149)


@pytest.mark.parametrize("bounce,seed", SAMPLER_CASES)
def test_one_hot_precondition_of_the_sampler_rows(rtmi_mod, oracle_mod, bounce, seed):
    """The oracle returns the row's action for each of the 300 rows (max_step asserts it: no
    row is dropped), and the directions leave the surface."""
    g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU)
    q, loc, tri, pix, tp, act, d, tp2 = sampler_expectation(oracle_mod, g, bounce, seed)
    N = oracle_mod.normals(g.all_triangles())[tri]
    assert len(act) == SAMPLER_N and set(np.unique(tri)) == set(SAMPLER_SURF)
    assert len(np.unique(N, axis=0)) == 2
    assert np.all(dot3(N, d) > 0) and np.all(np.isfinite(tp2))
    assert len(np.unique(act)) > 20


def test_restatement_in_cdf_mode_is_the_oracle_render(rtmi_mod, oracle_mod):
    """restate(mode="cdf") against orc_render_dqn_wave with the same Q: the loop's camera hits,
    trace, throughput products, ray order, cast count and per-pixel fold."""
    R, O = rtmi_mod, oracle_mod
    g = R.cornell_geometry(R.RT_PRESET_GPU)
    for name in ("selection", "first"):
        q_of = net_of(name)[3]
        for view in ("view", "inside"):
            pos, yaws = VIEW if view == "view" else INSIDE
            want, casts, _ = O.render_dqn_wave(g, O.camera(pos, **yaws), O.params_from(frame_params(R)), q_of)
            got = expected(name, view, "cdf")
            assert got["casts"] == casts, (name, view)
            assert np.array_equal(bits(got["img"]), bits(want)), (name, view)


def test_restated_frames_cover_every_kind_of_path(rtmi_mod, oracle_mod):
    """The max-mode frames of the render test, without a GPU: the one-hot precondition at every
    bounce of every path (asserted inside restate), paths that end on a light, on the bounce cap
    and on a miss, and zero-contribution counts that are neither 0 nor all."""
    for name in ("selection",) + BIAS_ROWS:
        e = expected(name)
        counts = {k: int((e["end"] == k).sum()) for k in (END_MISS, END_LIGHT, END_CAP)}
        print(name, counts, "zero", e["zero"], "of", e["paths"], "casts", e["casts"])
        assert e["paths"] == 20 * 17 * 3 and (e["end"] != END_NONE).all()
        assert counts[END_MISS] > 0 and counts[END_LIGHT] > 0 and counts[END_CAP] > 0, (name, counts)
        if name in ("tie", "close"):   # cells 40 and 100 keep every path's throughput above the threshold:
            assert e["zero"] == 0      # the count's other edge
        else:
            assert 0 < e["zero"] < e["paths"], name
        assert e["casts"] > e["paths"]
    # the bias networks take their row's action at every hit; the selection network's action varies
    for name in BIAS_ROWS:
        assert scan_rows(bias_net(name)[3](np.zeros((3, 3), F))).tolist() == [BIAS_ACTION[name]] * 3
    pts = np.random.default_rng(SEED).uniform(-1, 1, (200, 3)).astype(F)
    assert len(np.unique(scan_rows(selection_net()[3](pts)))) > 3
    # the CDF frames of the mode test
    e = expected("selection", "view", "cdf")
    assert 0 < e["zero"] < e["paths"]


# ---------------------------------------------------------------- GPU ----------

class World:
    def __init__(self, R, ctx):
        self.R, self.ctx = R, ctx
        self.g = R.cornell_geometry(R.RT_PRESET_GPU)
        self.sc = R.Scene(ctx, self.g)
        self.nets = {}

    def net(self, name):
        if name not in self.nets:
            if name == "model":
                W, b = self.R.dqn.split_layers(self.R.dqn.read_dynet(os.path.join(MODELS, "cornell_12_12.model")))
                verts = self.g.nn_vertices
            else:
                W, b, verts, _ = net_of(name)
            self.nets[name] = self.R.dqn.Dqn(self.ctx, verts, W, b)
        return self.nets[name]

    def close(self):
        for n in self.nets.values():
            n.close()
        self.sc.close()


@pytest.fixture(scope="module")
def world(rtmi_mod, gpu_ctx):
    w = World(rtmi_mod, gpu_ctx)
    rtmi_mod.dqn.enable_stats(gpu_ctx, True)
    yield w
    rtmi_mod.dqn.enable_stats(gpu_ctx, False)
    w.close()


@contextlib.contextmanager
def max_mode(net):
    net.set_sampling(net.SAMPLE_MAX)
    try:
        yield net
    finally:
        net.set_sampling(net.SAMPLE_CDF)


def render_max(w, net, cam, p, sc=None):
    """(image, casts, paths, zero_paths) of a max-mode frame"""
    with max_mode(net):
        img, casts = w.R.dqn.render(w.ctx, sc or w.sc, net, cam, p)
    return (img, casts) + w.R.dqn.render_stats(w.ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("bounce,seed", SAMPLER_CASES)
def test_gpu_sampler_on_crafted_rows(rtmi_mod, oracle_mod, world, bounce, seed):
    """rt_dqn_sample_max on 300 rows (one full and one partial workgroup): action, direction and
    throughput bit for bit, q untouched.  The rows and what each catches: the module docstring."""
    R = rtmi_mod
    q, loc, tri, pix, tp, act, d, tp2 = sampler_expectation(oracle_mod, world.g, bounce, seed)
    q_in = q.copy()
    got_tp, got_d, got_a = R.dqn.sample_max(world.ctx, world.sc, seed, q_in, loc, tri, pix, 2, bounce, tp)
    assert np.array_equal(q_in.view(np.uint32), q.view(np.uint32)), "q was modified"
    names, _, want, idx, extra, *_ = sampler_inputs()
    bad = np.flatnonzero(got_a != act)
    assert bad.size == 0, [(int(i), names[idx[i]] if not extra[i] else "random", int(got_a[i]), int(act[i])) for i in bad[:8]]
    assert np.array_equal(bits(got_d), bits(d))
    assert np.array_equal(bits(got_tp), bits(tp2))


RENDER_NETS = ("selection",) + BIAS_ROWS + ("model",)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RENDER_NETS)
def test_gpu_render_equals_restatement(rtmi_mod, oracle_mod, world, name):
    """Cornell 20 x 17 x 3 spp, 6 bounces, a pass holding one sample slot and all three: image, cast
    count, paths and zero_paths against the restatement (Q from numpy; for cornell_12_12.model
    from rt_dqn_forward)."""
    R = rtmi_mod
    net = world.net(name)
    pos, yaws = VIEW
    cam, p = R.camera(pos, **yaws), frame_params(R)
    if name == "model":
        e = restate(oracle_mod, world.g, oracle_mod.camera(pos, **yaws), p, net.forward)
    else:
        e = expected(name)
    n_pix = 4 * 256
    for rays in (n_pix, 3 * n_pix):
        with env(RTMI_DQN_RAYS_IN_FLIGHT=rays):
            img, casts, paths, zero = render_max(world, net, cam, p)
        print(f"{name}: casts {casts} (restated {e['casts']}), zero paths {zero} of {paths} (restated {e['zero']})")
        assert casts == e["casts"] and (paths, zero) == (e["paths"], e["zero"])
        assert np.array_equal(bits(img), bits(e["img"]))


def tile_render(w, net, cam, p, tiles, T):
    import torch
    out = torch.full((len(tiles), T, T, 3), -7.0, dtype=torch.float32, device=torch.device("cuda", 0))
    casts = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", 0))
    w.R.dqn.render_tiles_device(w.ctx, w.sc, net, cam, p, tiles, T, out.data_ptr(), casts.data_ptr(), 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(casts.item())


def assemble(got, tiles, T, W_, H):
    img = np.zeros((H, W_, 3), F)
    for i, (x, y) in enumerate(tiles):
        vw, vh = min(T, W_ - x), min(T, H - y)
        img[y:y + vh, x:x + vw] = got[i, :vh, :vw]
        assert np.all(got[i, vh:] == F(-7)) and np.all(got[i, :, vw:] == F(-7))
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("selection", "model"))
def test_gpu_route_invariance(rtmi_mod, world, name):
    """One frame from inside the box (the table route) by every route: the action fused and
    written out, both forward kernels, the matrix-core filter (a scene whose table upload fails)
    and the BVH, one rectangle and a shuffled tile list; and from the opening, where the casts
    are the plain scan's, against the BVH.  Images, casts and statistics bit-identical."""
    R, w = rtmi_mod, world
    net = w.net(name)
    p = frame_params(R)
    for view in (INSIDE, VIEW):
        cam = R.camera(view[0], **view[1])
        ref = render_max(w, net, cam, p)
        assert ref[0].mean() > 0 and ref[2] == p.width * p.height * p.spp and ref[3] <= ref[2]

        def same(other, what):
            assert other[1:] == ref[1:], (what, other[1:], ref[1:])
            assert np.array_equal(bits(other[0]), bits(ref[0])), what

        with env(RTMI_DQN_MAX_FUSED="0"):
            same(render_max(w, net, cam, p), "written out")
        with env(RTMI_DQN_MAX_FUSED="1"):
            same(render_max(w, net, cam, p), "fused")
        try:
            net.set_mlp(net.MLP_STATIONARY)
            same(render_max(w, net, cam, p), "stationary")
            net.set_mlp(net.MLP_STREAM)
            same(render_max(w, net, cam, p), "stream")
        finally:
            net.set_mlp(net.MLP_AUTO)
        with R.Scene(w.ctx, w.g) as sc:
            sc.set_accel(R.ACCEL_BVH)
            same(render_max(w, net, cam, p, sc), "bvh")
            sc.set_accel(R.ACCEL_SCAN)
            same(render_max(w, net, cam, p, sc), "scan")
        with env(RT_CTAB_TEST_FAIL="1"), R.Scene(w.ctx, w.g) as sc:
            same(render_max(w, net, cam, p, sc), "no table")
            assert not sc.ctab_info(R.RT_HIT_RULE_GPU)["built"]
        if view is INSIDE:
            assert w.sc.ctab_info(R.RT_HIT_RULE_GPU)["built"]
        T = 16
        tiles = R.tiles.tile_origins(p.width, p.height, T)
        tiles = tiles[np.random.default_rng(SEED).permutation(len(tiles))]
        for fused in ("1", "0"):
            with env(RTMI_DQN_MAX_FUSED=fused), max_mode(net):
                got, casts = tile_render(w, net, cam, p, tiles, T)
            same((assemble(got, tiles, T, p.width, p.height), casts) + R.dqn.render_stats(w.ctx), f"tiles fused={fused}")


FLOOR = ((0.0, 0.0, -0.5, 1.0), {"yaw_x": 0.9})   # inside the box, pitched at the floor: every camera ray lands on a surface


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("selection", "model"))
def test_gpu_ray_counts_around_the_forward_tile(rtmi_mod, oracle_mod, world, name):
    """W x 1 frames through a tile list with W = 1, 95, 96, 97, 193 rays at bounce 1 (the forward's
    96-row tile edges; the count asserted from the camera hits): fused against written out."""
    R, w = rtmi_mod, world
    net = w.net(name)
    assert R.dqn.mlp_rows() == 96
    cam, ocam = R.camera(FLOOR[0], **FLOOR[1]), oracle_mod.camera(FLOOR[0], **FLOOR[1])
    for W_ in (1, 95, 96, 97, 193):
        p = frame_params(R, width=W_, height=1, spp=1)
        hits = oracle_mod.primary_hits(w.g.all_triangles(), w.g.n_surf, w.g.n_light, ocam, oracle_mod.params_from(p),
                                       (0, 0, W_, 1), 0, 1)
        assert int(((hits >= 0) & (hits < w.g.n_surf)).sum()) == W_
        tiles = R.tiles.tile_origins(W_, 1, 16)
        out = []
        for fused in ("1", "0"):
            with env(RTMI_DQN_MAX_FUSED=fused), max_mode(net):
                got, casts = tile_render(w, net, cam, p, tiles, 16)
            out.append((assemble(got, tiles, 16, W_, 1), casts) + R.dqn.render_stats(w.ctx))
        rect = render_max(w, net, cam, p)
        for o in out:
            assert o[1:] == rect[1:] and o[2] == W_, (W_, o[1:], rect[1:])
            assert np.array_equal(bits(o[0]), bits(rect[0])), W_
        if name == "selection":
            e = restate(oracle_mod, w.g, ocam, p, net_of(name)[3])
            assert rect[1:] == (e["casts"], e["paths"], e["zero"]) and np.array_equal(bits(rect[0]), bits(e["img"])), W_


@pytest.mark.gpu
def test_gpu_mode_is_a_property_of_the_handle(rtmi_mod, oracle_mod, world):
    """CDF -> MAX -> CDF on one handle: the CDF frames equal each other and a fresh handle's, the
    max frame differs, and rt_dqn_render_stats after a CDF frame equals the recount on the
    restatement run in CDF mode (oracle.render_dqn_wave does not expose its paths' throughputs)."""
    R, w = rtmi_mod, world
    W, b, verts, q_of = net_of("selection")
    pos, yaws = VIEW
    cam, p = R.camera(pos, **yaws), frame_params(R)
    e = expected("selection", "view", "cdf")
    with R.dqn.Dqn(w.ctx, verts, W, b) as net:
        assert net.sampling == net.SAMPLE_CDF
        a = R.dqn.render(w.ctx, w.sc, net, cam, p) + R.dqn.render_stats(w.ctx)
        net.set_sampling(net.SAMPLE_MAX)
        assert net.sampling == net.SAMPLE_MAX
        m = R.dqn.render(w.ctx, w.sc, net, cam, p) + R.dqn.render_stats(w.ctx)
        net.set_sampling(net.SAMPLE_CDF)
        c = R.dqn.render(w.ctx, w.sc, net, cam, p) + R.dqn.render_stats(w.ctx)
    with R.dqn.Dqn(w.ctx, verts, W, b) as fresh:
        f = R.dqn.render(w.ctx, w.sc, fresh, cam, p) + R.dqn.render_stats(w.ctx)
    for other in (c, f):
        assert other[1:] == a[1:] and np.array_equal(bits(other[0]), bits(a[0]))
    assert a[1:] == (e["casts"], e["paths"], e["zero"]), (a[1:], e["casts"], e["paths"], e["zero"])
    assert np.array_equal(bits(a[0]), bits(e["img"]))
    em = expected("selection")
    assert m[1:] == (em["casts"], em["paths"], em["zero"]) and np.array_equal(bits(m[0]), bits(em["img"]))
    assert not np.array_equal(bits(m[0]), bits(a[0]))


@pytest.mark.gpu
def test_gpu_refusals(rtmi_mod, world):
    R, w, L = rtmi_mod, world, rtmi_mod.lib()
    net = w.net("selection")
    for bad in (-1, 2, 7):
        with pytest.raises(R.RtError):
            net.set_sampling(bad)
        assert L.rt_dqn_set_sampling(net.handle, bad) == R._lib.RT_E_INVALID and b"mode" in L.rt_last_error()
    assert net.sampling == net.SAMPLE_CDF
    assert L.rt_dqn_set_sampling(None, 1) == R._lib.RT_E_INVALID
    assert L.rt_dqn_get_sampling(net.handle, None) == R._lib.RT_E_INVALID
    with R.Context(0) as fresh:   # no render on this context yet
        with pytest.raises(R.RtError):
            R.dqn.render_stats(fresh)
        a = ctypes.c_uint64(9)
        assert L.rt_dqn_render_stats(fresh.handle, ctypes.byref(a), None) == R._lib.RT_E_INVALID and a.value == 9
        # the statistics are counted on request: off by default, per context, render by render
        W, b, verts, _ = net_of("first")
        cam, p = R.camera(VIEW[0], **VIEW[1]), frame_params(R, width=8, height=8, spp=1)
        with R.Scene(fresh, w.g) as sc, R.dqn.Dqn(fresh, verts, W, b) as net2:
            img0, casts0 = R.dqn.render(fresh, sc, net2, cam, p)
            with pytest.raises(R.RtError):
                R.dqn.render_stats(fresh)
            R.dqn.enable_stats(fresh, True)
            img1, casts1 = R.dqn.render(fresh, sc, net2, cam, p)
            paths, zero = R.dqn.render_stats(fresh)
            assert paths == 64 and 0 <= zero <= 64
            assert casts1 == casts0 and np.array_equal(bits(img1), bits(img0))   # counting changes nothing
            R.dqn.enable_stats(fresh, False)
            R.dqn.render(fresh, sc, net2, cam, p)
            with pytest.raises(R.RtError):
                R.dqn.render_stats(fresh)
    # rt_dqn_sample_max: rt_dqn_sample's checks
    q = np.ones((2, 144), F)
    loc = surface_points(w.g, [2, 30])
    tri = np.array([2, 30], np.int32)
    pix = np.array([1, 2], np.uint32)
    tp = np.ones((2, 3), F)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    up = ctypes.POINTER(ctypes.c_uint32)
    d, a = np.zeros((2, 3), F), np.zeros(2, np.int32)

    def call(sampler, ctx=w.ctx.handle, scene=w.sc.handle, q_=q, tri_=tri, n=2, act=a):
        return sampler(ctx, scene, SEED, None if q_ is None else q_.ctypes.data_as(fp), loc.ctypes.data_as(fp),
                       tri_.ctypes.data_as(ip), pix.ctypes.data_as(up), n, 0, 1, tp.ctypes.data_as(fp),
                       d.ctypes.data_as(fp), None if act is None else act.ctypes.data_as(ip))

    for kw in (dict(ctx=None), dict(scene=None), dict(q_=None), dict(act=None), dict(n=-1),
               dict(tri_=np.array([2, w.g.n_surf], np.int32)), dict(tri_=np.array([-1, 2], np.int32))):
        assert call(L.rt_dqn_sample_max, **kw) == call(L.rt_dqn_sample, **kw) == R._lib.RT_E_INVALID, kw
    assert call(L.rt_dqn_sample_max, n=0) == R._lib.RT_OK
    assert call(L.rt_dqn_sample_max) == R._lib.RT_OK and a.tolist() == [0, 0]   # equal cells: the first
