"""The dense shared exact phase of the one-word table route (rt_trace.hpp cand_exact_dense:
closest_hit_cand<0, 1, 96>, behind k_intersect_cand<0, 1, 96> and the table-route instances of
k_render_ps): the wave's (lane, candidate) pairs past each lane's own three are numbered
lane-major and tested 64 to a round; a pair's owner comes from a byte row and a maximum scan, and
an owner folds only the pairs of its range that passed.  The hit must stay the scan's bit for bit.

Mask-driven cases (rt_intersect_cand on given masks, the harness of test_cand_route.py): 256
rays a launch, four adjacent waves with four different patterns, each wave's LDS block exactly
the render kernels', so a write past one block shows as a wrong hit in its neighbour.  (t, hit)
against the restatement's masked scan (orc_intersect_masked), bit for bit.  The patterns are
built from each ray's own passing triangles (their t from one-bit masked scans), so what a
pattern is meant to hold -- pair totals, a range across a round boundary with a pass on each
side, ties inside the window, an own-lane winner kept or replaced -- is asserted on the CPU
from the masks by a restatement of the window (fold) before the GPU sees them.

Render cases: image words and casts against oracle.render on the clipped 40 x 24 and 17 x 33
frames, per_chunk 1, 4 and 5 (the wide layout), from the bench camera and from a camera a few
hundredths off the left wall looking along it, where the bounce rays' candidate lists are long.
"""
import numpy as np
import pytest

from ray_sets import bounce_rays
from test_cand_route import _bits, _mask_of, hit_triangles
from test_mf_filter import edge_rays, surface_rays

OWN = 3           # RT_CTAB_OWN: candidates a lane tests itself, in index order
CAP = 96          # the table route's pair cap (selects k_intersect_cand<0, 1, 96>)
TS = 512.0
EPS = np.float32(1e-5)
FLT_MAX = np.float32(3.4028234663852886e38)


# ---------------------------------------------------------------- scenes and ray pools ----------

def box64_geometry(rtmi):
    """A closed box [-1, 1]^3 of 62 surface triangles (five faces of 3 x 2 quads, one of a single
    quad) and a two-triangle light under its ceiling: 64 triangles, the lights at bits 62, 63."""
    tris = []
    faces = [(ax, side) for ax in range(3) for side in (-1.0, 1.0)]
    for n_face, (ax, side) in enumerate(faces):
        ku, kv = (3, 2) if n_face < 5 else (1, 1)
        gu, gv = np.linspace(-1.0, 1.0, ku + 1), np.linspace(-1.0, 1.0, kv + 1)
        for i in range(ku):
            for j in range(kv):
                def p(a, b):
                    v = np.zeros(3)
                    v[ax], v[(ax + 1) % 3], v[(ax + 2) % 3] = side, a, b
                    return v
                a, b, c, d = p(gu[i], gv[j]), p(gu[i + 1], gv[j]), p(gu[i + 1], gv[j + 1]), p(gu[i], gv[j + 1])
                tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
    tri = np.asarray(tris, np.float32)
    assert tri.shape[0] == 62
    q = [np.array(v) for v in ((-0.4, 0.9, -0.4), (0.4, 0.9, -0.4), (0.4, 0.9, 0.4), (-0.4, 0.9, 0.4))]
    light = np.asarray([np.concatenate([q[0], q[1], q[2]]), np.concatenate([q[0], q[2], q[3]])], np.float32)
    return rtmi.Geometry(tri, np.full((62, 3), 0.75, np.float32), light, np.full((2, 3), 10.0, np.float32),
                         np.zeros(2, np.int32))


_GEOM, _POOL = {}, {}


def _geom(rtmi, kind):
    if kind not in _GEOM:
        _GEOM[kind] = rtmi.cornell_geometry(0) if kind == "cornell" else box64_geometry(rtmi)
    return _GEOM[kind]


def pool(rtmi, oracle, kind):
    """(geom, tri, o, d, T): the scene's pool of rays -- surface rays, rays at edges and vertices,
    rays from vertices (every triangle of the vertex at t = +-0) -- and T[i, k], the t of triangle
    k for ray i where it passes the exact test (CPU rule, t_scale 512), else +inf: the t of the
    masked scan on the one-bit mask.  Read-only, computed once."""
    if kind in _POOL:
        return _POOL[kind]
    geom = _geom(rtmi, kind)
    tri = np.ascontiguousarray(geom.all_triangles(), np.float32)
    n_tri = tri.shape[0]
    o1, d1 = surface_rays(tri, 1500, seed=31)
    o2, d2 = edge_rays(tri, 3000, seed=32)
    rng = np.random.default_rng(33)
    allv = tri.reshape(-1, 3)
    o3 = allv[rng.integers(0, allv.shape[0], 300)].copy()
    d3 = allv[rng.integers(0, allv.shape[0], 300)] + rng.normal(size=(300, 3)).astype(np.float32) * np.float32(0.05) - o3
    d3[np.linalg.norm(d3, axis=1) < 1e-3] = (0.0, 0.0, 1.0)
    d3 = (d3 / np.linalg.norm(d3, axis=1, keepdims=True)).astype(np.float32)
    o = np.ascontiguousarray(np.concatenate([o1, o2, o3]), np.float32)
    d = np.ascontiguousarray(np.concatenate([d1, d2, d3]), np.float32)
    P = oracle.pass_masks(tri, o, d, TS, 0)
    T = np.full((o.shape[0], n_tri), np.inf, np.float32)
    for k in range(n_tri):
        one = np.zeros_like(P)
        one[:, 0] = P[:, 0] & (np.uint64(1) << np.uint64(k))
        T[:, k] = oracle.intersect_masked(tri, geom.n_surf, geom.n_light, geom.light_group, o, d, one, TS, 0)[0]
    for a in (o, d, T):
        a.setflags(write=False)
    _POOL[kind] = (geom, tri, o, d, T)
    return _POOL[kind]


def fold(t_row, ids, best=FLT_MAX, tri=-1):
    """The CPU rule's window over candidates `ids` in index order from (best, tri): a candidate
    takes the hit when it passes with t < best + eps (float32)."""
    for k in sorted(ids):
        if t_row[k] < np.float32(best + EPS):
            best, tri = t_row[k], int(k)
    return best, tri


# ---------------------------------------------------------------- patterns ----------
# A pattern gives a wave its 64 (ray of the pool, candidate set) lanes.

def _with_passes(rng, T, i, size):
    """`size` candidates for ray i: its passing triangles first, then others at random"""
    n_tri = T.shape[1]
    ps = np.nonzero(np.isfinite(T[i]))[0]
    rest = np.setdiff1d(np.arange(n_tri), ps)
    ids = np.concatenate([rng.permutation(ps), rng.permutation(rest)])[:size]
    return set(int(k) for k in ids)


def _placed(rng, T, i, own_pass, extra_pass, n_more=0):
    """Candidates for ray i with the passing triangles `own_pass` among the lane's own three, and
    `extra_pass` past them; the other own candidates and `n_more` further extras do not pass.
    None if the indices leave no room."""
    n_tri = T.shape[1]
    fail = [k for k in range(n_tri) if not np.isfinite(T[i, k])]
    lo = [k for k in fail if k < min(extra_pass)]
    if len(lo) < OWN - len(own_pass) or (own_pass and max(own_pass) > min(extra_pass)):
        return None
    own = list(own_pass) + [int(k) for k in rng.permutation(lo)[:OWN - len(own_pass)]]
    if max(own) > min(extra_pass):
        return None
    hi = [k for k in fail if k > min(extra_pass)]  # (the first passing extra is the lane's first pair)
    more = [int(k) for k in rng.permutation(hi)[:n_more]]
    return set(own) | set(int(k) for k in extra_pass) | set(more)


def _counts(rng, total, room, lanes=64):
    """extras per lane, `total` in all, at most `room` each"""
    q = np.zeros(lanes, int)
    for _ in range(total):
        q[rng.choice(np.nonzero(q < room)[0])] += 1
    return q


def _near_ties(T, i, at_least):
    """the passing triangles of ray i within eps above its smallest t, if there are at least
    `at_least`, the first not among the scene's first three, and a later one has the larger t"""
    ps = np.nonzero(np.isfinite(T[i]))[0]
    if ps.size < at_least:
        return None
    near = ps[T[i, ps] < np.float32(T[i, ps].min() + EPS)]
    if near.size < at_least or near[0] < OWN or not T[i, near[-1]] > T[i, near[0]]:
        return None
    return [int(k) for k in near[:max(at_least, 2)]] if at_least == 2 else [int(k) for k in near]


def wave_patterns(T, n_surf):
    n, n_tri = T.shape
    room = n_tri - OWN
    ps = np.isfinite(T)
    everything = set(range(n_tri))

    def any_ray(rng):
        return int(rng.integers(0, n))

    def light_lanes(rng):  # every lane 0..3 candidates: the shared phase is skipped
        return [(i, _with_passes(rng, T, i, int(rng.integers(0, OWN + 1)))) for i in (any_ray(rng) for _ in range(64))]

    def heavy(lane):
        def f(rng):
            w = light_lanes(rng)
            w[lane] = (w[lane][0], set(everything))
            return w
        return f

    def each_four(rng):
        return [(i, _with_passes(rng, T, i, OWN + 1)) for i in (any_ray(rng) for _ in range(64))]

    def total(t):
        def f(rng):
            q = _counts(rng, t, room)
            return [(i, _with_passes(rng, T, i, OWN + int(q[l]))) for l, i in enumerate(any_ray(rng) for _ in range(64))]
        return f

    def straddle(rng):
        """lanes 20 and 40 own the pairs around positions 64 and 128: the first passing extra of
        each at the last position of a round, another in the next round"""
        two = [i for i in range(n) if ps[i, OWN:].sum() >= 2]
        w = []
        for edge, lane in ((64, 20), (128, 40)):
            q = _counts(rng, edge - 1 - sum(max(len(c) - OWN, 0) for _, c in w), room, lane - len(w))
            w += [(i, _with_passes(rng, T, i, OWN + int(q[l]))) for l, i in enumerate(any_ray(rng) for _ in range(q.size))]
            while True:
                i = int(rng.choice(two))
                p = [int(k) for k in np.nonzero(ps[i])[0] if k >= OWN][:2]
                c = _placed(rng, T, i, [], p, n_more=4)
                if c is not None and len(c) == OWN + 6:
                    break
            w.append((i, c))
        w += [(i, _with_passes(rng, T, i, OWN + int(rng.integers(0, 3)))) for i in (any_ray(rng) for _ in range(64 - len(w)))]
        return w

    def interleaved(rng):
        return [(i, _with_passes(rng, T, i, OWN + int(rng.integers(0, 7))) if l % 2 == 0 else set())
                for l, i in enumerate(any_ray(rng) for _ in range(64))]

    def own_against_shared(replaced):
        """one passing candidate among the own three, one past them that is nearer (it takes the
        hit) or farther by more than eps (the own-lane winner stays)"""
        def f(rng):
            w = []
            while len(w) < 64:
                i = any_ray(rng)
                p = np.nonzero(ps[i])[0]
                if p.size < 2:
                    continue
                a, b = int(p[0]), int(p[-1])
                later_wins = T[i, b] < np.float32(T[i, a] + EPS)
                if later_wins != replaced or (not replaced and not T[i, b] > T[i, a] + np.float32(1e-3)):
                    continue
                c = _placed(rng, T, i, [a], [b], n_more=int(rng.integers(0, 4)))
                if c is not None:
                    w.append((i, c))
            return w
        return f

    def ties(k):
        """k passing extras within eps of each other, a later one the farther: it takes the hit"""
        def f(rng):
            good = [i for i in range(n) if _near_ties(T, i, k) is not None]
            w = []
            while len(w) < 64:
                i = int(rng.choice(good))
                c = _placed(rng, T, i, [], _near_ties(T, i, k), n_more=int(rng.integers(0, 3)))
                if c is not None:
                    w.append((i, c))
            return w
        return f

    def from_vertices(rng):  # the pool's last 300 rays: their vertex's triangles at t = +-0, never a pass
        return [(i, _with_passes(rng, T, i, OWN + int(rng.integers(1, 6))) | set(int(k) for k in rng.integers(0, n_tri, 4)))
                for i in (int(rng.integers(n - 300, n)) for _ in range(64))]

    def high_bits(rng):
        """(64 triangles) candidates 31, 32 and 63 in every lane past its own three; each passes in some lane"""
        w = []
        want = [31, 32, 63]
        while len(w) < 64:
            k = want[len(w) % 3]
            i = int(rng.choice(np.nonzero(ps[:, k])[0]))
            # (the own three below every pass and below 31: placed like passing extras)
            c = _placed(rng, T, i, [], sorted(set(int(x) for x in np.nonzero(ps[i])[0]) | {31, 32, 63}), n_more=0)
            if c is not None:
                w.append((i, c))
        return w

    pats = [("skipped", light_lanes), ("one lane all", heavy(17)), ("lane 0 heavy", heavy(0)), ("lane 63 heavy", heavy(63)),
            ("each lane four", each_four), ("total 63", total(63)), ("total 64", total(64)), ("total 65", total(65)),
            ("total 96", total(96)), ("total 97", total(97)), ("total 129", total(129)), ("straddle", straddle),
            ("interleaved", interleaved), ("own kept", own_against_shared(False)), ("own replaced", own_against_shared(True)),
            ("ties of two", ties(2)), ("ties of three", ties(3)), ("from vertices", from_vertices),
            ("total 129", total(129)), ("skipped", light_lanes)]
    if n_tri == 64:
        pats = [("high bits", high_bits), ("one lane all", heavy(17)), ("total 129", total(129)), ("each lane four", each_four),
                ("lane 63 heavy", heavy(63)), ("high bits", high_bits), ("straddle", straddle), ("total 65", total(65))]
    return pats


_WAVES = {}


def waves(rtmi, oracle, kind):
    """(names, ray index per lane (n_waves, 64), candidate rows (n_waves * 64, n_tri) bool)"""
    if kind not in _WAVES:
        geom, tri, o, d, T = pool(rtmi, oracle, kind)
        rng = np.random.default_rng(7 + T.shape[1])
        pats = wave_patterns(T, geom.n_surf)
        assert len(pats) % 4 == 0
        idx = np.zeros((len(pats), 64), int)
        rows = np.zeros((len(pats) * 64, T.shape[1]), bool)
        for wv, (_, f) in enumerate(pats):
            for l, (i, c) in enumerate(f(rng)):
                idx[wv, l] = i
                rows[64 * wv + l, sorted(c)] = True
        _WAVES[kind] = ([p[0] for p in pats], idx, rows)
    return _WAVES[kind]


def _layout(rows):
    """per lane of a wave: candidates, extras past the own three, first pair number"""
    cand = [np.nonzero(r)[0] for r in rows]
    cnt = np.asarray([max(c.size - OWN, 0) for c in cand])
    return cand, cnt, np.concatenate([[0], np.cumsum(cnt)[:-1]])


# ---------------------------------------------------------------- CPU ----------

@pytest.mark.parametrize("kind", ["cornell", "box64"])
def test_patterns_hold_what_they_name(rtmi_mod, oracle_mod, kind):
    geom, tri, o, d, T = pool(rtmi_mod, oracle_mod, kind)
    names, idx, rows = waves(rtmi_mod, oracle_mod, kind)
    n_tri = T.shape[1]
    assert n_tri == (38 if kind == "cornell" else 64)
    seen = {}
    for wv, name in enumerate(names):
        cand, cnt, excl = _layout(rows[64 * wv:64 * wv + 64])
        tot = int(cnt.sum())
        # per lane: the own-lane fold, the whole fold, and the passing extras with their pair numbers
        own, full, pos = [], [], []
        for l in range(64):
            t_row = T[idx[wv, l]]
            own.append(fold(t_row, cand[l][:OWN]))
            full.append(fold(t_row, cand[l][OWN:], *own[l]))
            assert full[l] == fold(t_row, cand[l])
            pos.append([excl[l] + j for j, k in enumerate(cand[l][OWN:]) if np.isfinite(t_row[k])])
        most = max(len(p) for p in pos)
        print(f"{kind} wave {wv} '{name}': {tot} pairs, {sum(len(p) for p in pos)} pass, at most {most} in a lane, "
              f"busiest lane {int(cnt.max())}")
        seen[name] = seen.get(name, 0) + 1
        if name == "skipped":
            assert tot == 0 and any(c.size for c in cand)
        elif name == "one lane all":
            assert cand[17].size == n_tri and cnt[17] == tot == n_tri - OWN
        elif name in ("lane 0 heavy", "lane 63 heavy"):
            l = 0 if name == "lane 0 heavy" else 63
            assert cand[l].size == n_tri and tot == n_tri - OWN
        elif name == "each lane four":
            assert np.all(cnt == 1) and tot == 64
        elif name.startswith("total"):
            assert tot == int(name.split()[1])
        elif name == "straddle":
            for edge, l in ((64, 20), (128, 40)):
                assert excl[l] < edge < excl[l] + cnt[l]
                assert any(p < edge for p in pos[l]) and any(p >= edge for p in pos[l]), (edge, pos[l])
            assert most >= 2
        elif name == "interleaved":
            assert all(cand[l].size == 0 for l in range(1, 64, 2)) and tot > 64
        elif name == "own kept":
            assert all(pos[l] and full[l][1] == own[l][1] >= 0 for l in range(64))
        elif name == "own replaced":
            assert all(own[l][1] >= 0 and full[l][1] in cand[l][OWN:] for l in range(64))
        elif name in ("ties of two", "ties of three"):
            k = 2 if name.endswith("two") else 3
            late = 0
            for l in range(64):
                t_row, ex = T[idx[wv, l]], [c for c in cand[l][OWN:] if np.isfinite(T[idx[wv, l], c])]
                assert len(ex) >= k and own[l][1] == -1
                assert np.all(t_row[ex] < np.float32(t_row[ex].min() + EPS))
                # the window keeps moving: the last of them takes the hit, though an earlier one is nearer
                assert full[l][1] == ex[-1]
                late += bool(t_row[ex[-1]] > t_row[ex].min())
            assert late >= 32 and most >= k
        elif name == "from vertices":
            zero = 0
            for l in range(64):  # (under the GPU rule the vertex's triangles pass at t = +-0)
                m = _mask_of(rows[64 * wv + l][None, :], n_tri)
                tz = oracle_mod.intersect_masked(tri, geom.n_surf, geom.n_light, geom.light_group,
                                                 o[idx[wv, l]][None, :], d[idx[wv, l]][None, :], m, TS, 1)[0]
                zero += bool(tz[0] == 0.0)
            assert zero >= 8 and tot > 64
        elif name == "high bits":
            hits = [full[l][1] for l in range(64)]
            assert all(k in cand[l][OWN:] for l in range(64) for k in (31, 32, 63))
            assert all(any(np.isfinite(T[idx[wv, l], k]) for l in range(64)) for k in (31, 32, 63))
            assert {31, 32, 63} & set(hits) and tot > 128
    want = ({"skipped", "one lane all", "lane 0 heavy", "lane 63 heavy", "each lane four", "total 63", "total 64",
             "total 65", "total 96", "total 97", "total 129", "straddle", "interleaved", "own kept", "own replaced",
             "ties of two", "ties of three", "from vertices"} if kind == "cornell" else
            {"high bits", "one lane all", "total 129", "straddle"})
    assert want <= set(seen), want - set(seen)
    # four different patterns in every launch
    assert all(len(set(names[a:a + 4])) == 4 for a in range(0, len(names), 4))


GRAZING_CAM = ((-0.93, 0.0, -0.9, 1.0), 0.0)  # 0.07 off the left wall (x = -1), looking along it


def test_grazing_bounce_rays_have_long_lists(rtmi_mod):
    """(CPU) The table's candidate lists for bounce rays nearly in a plane, as they leave the wall
    the grazing camera looks along: some ray has a dozen candidates and some group of 64 more
    than 64 pairs past the lanes' own three -- more than one round."""
    geom = _geom(rtmi_mod, "cornell")
    tri = np.ascontiguousarray(geom.all_triangles(), np.float32)
    surf, o, d, kind = bounce_rays(tri, geom.n_surf, 6000, seed=17)
    v = tri[:geom.n_surf].reshape(-1, 3, 3)
    left = np.nonzero(np.all(v[:, :, 0] == -1.0, axis=1))[0]
    assert left.size >= 2
    pick = np.nonzero(np.isin(surf, left) & (kind >= 2))[0]
    assert pick.size >= 128
    masks = rtmi_mod.ctab_candidates(tri, geom.n_surf, surf[pick], o[pick], d[pick], hit_rule=0)[0]
    pc = np.unpackbits(masks.view(np.uint8), axis=1).sum(axis=1)
    extras = np.maximum(pc - OWN, 0)
    groups = [int(extras[a:a + 64].sum()) for a in range(0, pick.size - 63, 64)]
    print(f"{pick.size} grazing rays off the left wall: up to {pc.max()} candidates, mean {pc.mean():.2f}; "
          f"pairs per group of 64: {groups}")
    assert pc.max() >= 12 and max(groups) > 64


# ---------------------------------------------------------------- GPU ----------

@pytest.fixture(scope="module")
def scenes(rtmi_mod, gpu_ctx):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = rtmi_mod.Scene(gpu_ctx, _geom(rtmi_mod, kind))
        return made[kind]
    yield get
    for sc in made.values():
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cornell", "box64"])
def test_gpu_dense_phase_on_given_masks(rtmi_mod, oracle_mod, gpu_ctx, scenes, kind):
    geom, tri, o, d, T = pool(rtmi_mod, oracle_mod, kind)
    names, idx, rows = waves(rtmi_mod, oracle_mod, kind)
    flat = idx.reshape(-1)
    ro, rd = np.ascontiguousarray(o[flat]), np.ascontiguousarray(d[flat])
    masks = _mask_of(rows, T.shape[1])
    tm, hm = oracle_mod.intersect_masked(tri, geom.n_surf, geom.n_light, geom.light_group, ro, rd, masks, TS, 0)
    # (the restatement of the window above is the masked scan's)
    hit = hit_triangles(oracle_mod, geom, ro, rd, TS, 0, masks)
    for r in range(0, flat.size, 37):
        assert fold(T[flat[r]], np.nonzero(rows[r])[0])[1] == hit[r]
    sc = scenes(kind)
    for a in range(0, flat.size, 256):  # four adjacent waves a launch
        t, h = rtmi_mod.intersect_cand(gpu_ctx, sc, ro[a:a + 256], rd[a:a + 256], TS, 0, masks=masks[a:a + 256],
                                       pair_cap=CAP, guard=96)
        assert np.all(_bits(t[256:]) == 0xA5A5A5A5) and np.all(_bits(h[256:]) == 0xA5A5A5A5)
        bad = np.nonzero((h[:256] != hm[a:a + 256]) | (_bits(t[:256]) != _bits(tm[a:a + 256])))[0]
        assert bad.size == 0, (f"launch at {a} ({names[a // 64:a // 64 + 4]}): {bad.size} rays differ from the masked "
                               f"scan, e.g. lane {bad[0] % 64} of '{names[(a + bad[0]) // 64]}': ({t[bad[0]]}, {h[bad[0]]}) "
                               f"for ({tm[a + bad[0]]}, {hm[a + bad[0]]}); waves {sorted({names[(a + b) // 64] for b in bad})}")


T_SCALE = 256.0
RENDER_CASES = [(view, w, h, spp) for view in ("bench", "grazing") for (w, h) in ((40, 24), (17, 33))
                for spp in (64, 256, 320)]
_REF = {}


def _render_args(rtmi, view, w, h, spp):
    pos, yaw_y = (rtmi.CAMERAS["cornell"], 0.0) if view == "bench" else GRAZING_CAM
    return pos, yaw_y, rtmi.default_params(rtmi.RT_PRESET_CPU, t_scale=T_SCALE, width=w, height=h, spp=spp, spp_split=64)


def _ref(rtmi, oracle, case):
    if case not in _REF:
        pos, yaw_y, p = _render_args(rtmi, *case)
        img, casts = oracle.render(_geom(rtmi, "cornell"), oracle.camera(pos, yaw_y=yaw_y), oracle.params_from(p))
        img.setflags(write=False)
        _REF[case] = (img, int(casts))
    return _REF[case]


def test_grazing_view_sees_the_wall_and_the_light(rtmi_mod, oracle_mod):
    """(CPU) the grazing view's paths bounce (casts beyond the camera rays) and carry light"""
    case = ("grazing", 40, 24, 64)
    img, casts = _ref(rtmi_mod, oracle_mod, case)
    assert casts > 2 * 40 * 24 * 64 and np.count_nonzero(img) > img.size // 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", RENDER_CASES, ids=["-".join(str(x) for x in c) for c in RENDER_CASES])
def test_gpu_image_and_casts(rtmi_mod, oracle_mod, gpu_ctx, scenes, case):
    pos, yaw_y, p = _render_args(rtmi_mod, *case)
    sc = scenes("cornell")
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(p.hit_rule)["built"]  # the table route was taken
    ref, ref_casts = _ref(rtmi_mod, oracle_mod, case)
    print(f"{case}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
