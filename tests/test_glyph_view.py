"""Radiance-volume glyphs (rtmi.h "radiance-volume glyphs"): rt_selected_read, rt_glyph_mesh,
rt_glyph_colours, rt_glyphs_*, rt_render_glyph_view[_tiles_device].

CPU (no GPU): the reader against rtmi.sarsa.read_selected_file; the mesh bit for bit against
chiu_map restated in numpy float32 (oracle.sincos_turn for the polynomial) at axis-aligned
normals, where the frame is exact, and by its properties in float64 at an oblique normal; the
colours against a numpy float32 restatement; every refusal.

GPU: the view's winner, t and colour of every pixel against oracle.primary_hits over the soup
[scene surfaces, rt_glyph_mesh's triangles, lights], rtmi.intersect on a scene of that soup, and
the tables the AOVs select; the chunk fold, the two routes of the glyph cast, tile renders, the
empty set, set_colours, and that a view leaves the scene and the glyph set as it found them.
The shapes (50x39, 17x5, 1x1, 80x72 with 32-pixel tiles) leave most waves partly filled.

One property is asserted in another form than its issue words it.  "|V - P| = D |N| within 1e-5"
cannot hold for the issue's un-normalised normal (0.3, -0.8, 0.52), |N| = 1.0002: by the issue's
own vertex formula V - P = T xs + N ys + B zs with (T, B) = normal_frame(N), T has length 1 and N,
B = N x T length |N|, so |V - P| runs from D (along T) to D |N| around the rim, 2e-4 apart.  The
test asserts what the formula gives -- the frame coordinates (xs, ys, zs) have length D within
1e-5 relative and |V - P|^2 = xs^2 + |N|^2 (ys^2 + zs^2) -- and the issue's own wording, to the
letter, at the same direction normalised (|N| = 1), where it is true.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, MODELS

F = np.float32
SEED = 1984
SELECTED = os.path.join(GOLDEN, "selected_sarsa_ref.txt")
VALUE_WORD = 0x476C7968  # counter word 3 of the value table's Philox blocks ("Glyh"): apart from every render draw
_FP = ctypes.POINTER(ctypes.c_float)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def value_table(oracle_mod, n):
    """The fixed test distributions: glyph g, sectors 4 j .. 4 j + 3 = u of the four words of the
    Philox block (g, j, 0, VALUE_WORD) under key (SEED, 0); u = (x >> 8) 2^-24."""
    out = np.zeros((n, 144), F)
    for g in range(n):
        for j in range(36):
            w = oracle_mod.philox([g, j, 0, VALUE_WORD], [SEED, 0])
            out[g, 4 * j:4 * j + 4] = (w >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    return out


# ------------------------------------------------------------ restatements ----------

def chiu_f32(oracle_mod, x, y):
    """rt_math.hpp chiu_map in its host form, numpy float32 operation by operation."""
    x = F(2) * F(x) - F(1)
    y = F(2) * F(y) - F(1)
    if y > -x:
        if y < x:
            xx = x
            off, yy = (F(0), y) if y > 0 else (F(0.875), x + y)
        else:
            xx = y
            off, yy = (F(0.125), y - x) if x > 0 else (F(0.25), -x)
    else:
        if y > x:
            xx = -x
            off, yy = (F(0.375), -x - y) if y > 0 else (F(0.5), -y)
        else:
            xx = -y
            if x > 0:
                off, yy = F(0.75), x
            elif y != 0:
                off, yy = F(0.625), x - y
            else:
                return F(0), F(1), F(0)
    c = F(1) - xx * xx
    s = xx * np.sqrt(F(2) - xx * xx)
    phi = off + F(0.125) * (yy / xx)
    sp, cp = oracle_mod.sincos_turn(float(phi))
    out = s * F(cp), c, s * F(sp)
    assert all(type(v) is np.float32 for v in out)
    return out


def normalize_f32(v):
    inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def frame_f32(n):
    """create_normal_coordinate_system (rt_math.hpp normal_frame): T, B = cross(n, T) in glm's order."""
    T = normalize_f32([n[2], F(0), -n[0]]) if abs(n[0]) > abs(n[1]) else normalize_f32([F(0), -n[2], n[1]])
    B = [n[1] * T[2] - T[1] * n[2], n[2] * T[0] - T[2] * n[0], n[0] * T[1] - T[0] * n[1]]
    return T, B


def mesh_f32(oracle_mod, P, N, D):
    """rt_glyph_mesh of one glyph as rtmi.h states it: (288, 9) float32."""
    P, N, D = [F(v) for v in P], [F(v) for v in N], F(D)
    T, B = frame_f32(N)
    V = np.zeros((13, 13, 3), F)
    for x in range(13):
        for y in range(13):
            xh, yh, zh = chiu_f32(oracle_mod, F(x) / F(12), F(y) / F(12))
            xs, ys, zs = xh * D, yh * D, zh * D
            for c in range(3):
                V[x, y, c] = (T[c] * xs + N[c] * ys) + (B[c] * zs + P[c])
    return triangles_of_grid(V)


def triangles_of_grid(V):
    """Quad k = x * 12 + y: triangle 2k = (V[x][y], V[x][y+1], V[x+1][y]), 2k + 1 = (V[x+1][y], V[x][y+1], V[x+1][y+1])."""
    tri = np.zeros((288, 9), V.dtype)
    for x in range(12):
        for y in range(12):
            k = x * 12 + y
            tri[2 * k] = np.concatenate([V[x, y], V[x, y + 1], V[x + 1, y]])
            tri[2 * k + 1] = np.concatenate([V[x + 1, y], V[x, y + 1], V[x + 1, y + 1]])
    return tri


def chiu_f64(u, v):
    """Shirley and Chiu's concentric map of the unit square, lifted to the hemisphere as the
    reference lifts it: cos(theta) = 1 - r^2.  Returns (along T, along N, along B)."""
    a, b = 2.0 * u - 1.0, 2.0 * v - 1.0
    if a == 0.0 and b == 0.0:
        return np.array([0.0, 1.0, 0.0])
    if a > -b:
        r, phi = (a, (math.pi / 4) * (b / a)) if a > b else (b, (math.pi / 4) * (2.0 - a / b))
    else:
        r, phi = (-a, (math.pi / 4) * (4.0 + b / a)) if a < b else (-b, (math.pi / 4) * (6.0 - a / b))
    st = r * math.sqrt(2.0 - r * r)
    return np.array([st * math.cos(phi), 1.0 - r * r, st * math.sin(phi)])


def colours_f32(values, mode):
    v = np.ascontiguousarray(values, F).reshape(-1, 144)
    out = np.zeros((v.shape[0], 144, 3), F)
    for g, row in enumerate(v):
        if mode == 0:
            m = F(0)
            for x in row:
                if m < x:
                    m = x
            ratio = np.zeros(144, F) if m == 0 else row / m
            out[g, :, 0], out[g, :, 1] = ratio, F(1) - ratio
        else:
            m = F(0.0001)
            for x in row:
                if abs(x) > m:
                    m = abs(x)
            out[g] = (F(1) - np.abs(row) / m)[:, None]
    assert out.dtype == F
    return out


# ---------------------------------------------------------------- CPU: reader ----------

def test_reader_equals_python_reader(rtmi_mod):
    pos, nrm, val = rtmi_mod.read_selected(SELECTED)
    want = rtmi_mod.sarsa.read_selected_file(SELECTED)
    assert pos.shape == (3, 3) and nrm.shape == (3, 3) and val.shape == (3, 144)
    for a, b in zip((pos, nrm, val), want):
        assert a.dtype == F and np.array_equal(bits(a), bits(b))
    assert rtmi_mod.glyphs.read_selected is rtmi_mod.read_selected


def row_text(k, n_values=150):
    return " ".join(repr(0.25 * k + 0.001 * j) for j in range(n_values))


def test_reader_skips_blank_lines_and_names_the_bad_line(rtmi_mod, tmp_path):
    L = rtmi_mod.lib()
    good = tmp_path / "good.txt"
    good.write_text("\n" + row_text(1) + "\n   \t\n" + row_text(2) + "\n\n")
    pos, nrm, val = rtmi_mod.read_selected(str(good))
    assert pos.shape == (2, 3) and val.shape == (2, 144)
    want = np.array([[F(0.25 * k + 0.001 * j) for j in range(150)] for k in (1, 2)], F)
    assert np.array_equal(bits(np.concatenate([pos, nrm, val], axis=1)), bits(want))
    # the second pass refuses a file whose row count is not the sizing pass's
    n = ctypes.c_int32(3)
    buf = [np.zeros((3, c), F) for c in (3, 3, 144)]
    assert L.rt_selected_read(os.fsencode(str(good)), ctypes.byref(n), *[b.ctypes.data_as(_FP) for b in buf]) == -4
    for name, text, line in (("short", row_text(1) + "\n" + row_text(2, 149) + "\n", 2),
                             ("long", row_text(1) + "\n\n" + row_text(2, 151) + "\n", 3),
                             ("word", row_text(1, 149) + " abc\n", 1),
                             ("tail", row_text(1) + "\n" + row_text(2) + "\n" + row_text(3, 6) + "\n", 3)):
        bad = tmp_path / (name + ".txt")
        bad.write_text(text)
        with pytest.raises(rtmi_mod.RtError) as e:
            rtmi_mod.read_selected(str(bad))
        assert e.value.code == -4 and f"line {line}:" in str(e.value), (name, str(e.value))
    with pytest.raises(rtmi_mod.RtError) as e:
        rtmi_mod.read_selected(str(tmp_path / "missing.txt"))
    assert e.value.code == -4
    n = ctypes.c_int32(0)
    assert L.rt_selected_read(None, ctypes.byref(n), None, None, None) == -1
    assert L.rt_selected_read(os.fsencode(str(good)), None, None, None, None) == -1
    assert L.rt_selected_read(os.fsencode(str(good)), ctypes.byref(n), buf[0].ctypes.data_as(_FP), None, None) == -1
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n")
    assert rtmi_mod.read_selected(str(empty))[2].shape == (0, 144)


# ---------------------------------------------------------------- CPU: mesh ----------

AXIS_GLYPHS = (((0.0, 1.0, -0.5), (0.0, -1.0, 0.0)), ((0.5, 0.2, 1.0), (0.0, 0.0, -1.0)), ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)))


@pytest.mark.parametrize("diameter", (0.15, 0.4))
def test_mesh_equals_float32_restatement_at_axis_normals(rtmi_mod, oracle_mod, diameter):
    pos = np.array([g[0] for g in AXIS_GLYPHS], F)
    nrm = np.array([g[1] for g in AXIS_GLYPHS], F)
    tri, qn = rtmi_mod.glyph_mesh(pos, nrm, diameter)
    assert tri.shape == (3, 288, 9) and qn.shape == (3, 144, 3) and tri.dtype == F
    for g in range(3):
        want = mesh_f32(oracle_mod, pos[g], nrm[g], diameter)
        assert np.array_equal(bits(tri[g]), bits(want)), g
    # a glyph's mesh is its own: alone, and without the optional normals
    alone = np.zeros((1, 288, 9), F)
    assert rtmi_mod.lib().rt_glyph_mesh(pos[1:2].ctypes.data_as(_FP), nrm[1:2].ctypes.data_as(_FP), 1, diameter,
                                        alone.ctypes.data_as(_FP), None) == 0
    assert np.array_equal(bits(alone[0]), bits(tri[1]))


def grid_of_triangles(tri):
    """The 13 x 13 vertices back out of (288, 9) triangles, checking that every triangle is the
    one its place in the list says and that neighbouring quads share their vertices bit for bit."""
    V = np.zeros((13, 13, 3), tri.dtype)
    for x in range(12):
        for y in range(12):
            V[x, y] = tri[2 * (x * 12 + y), 0:3]
        V[x, 12] = tri[2 * (x * 12 + 11), 3:6]
    for y in range(12):
        V[12, y] = tri[2 * (11 * 12 + y), 6:9]
    V[12, 12] = tri[2 * (11 * 12 + 11) + 1, 6:9]
    assert np.array_equal(bits(tri), bits(triangles_of_grid(V)))
    return V


@pytest.mark.parametrize("diameter", (0.15, 0.4))
def test_mesh_properties_at_an_oblique_normal(rtmi_mod, diameter):
    N32 = np.array([0.3, -0.8, 0.52], F)
    P32 = np.array([0.2, -0.1, 0.3], F)
    unit32 = (N32.astype(np.float64) / np.linalg.norm(N32.astype(np.float64))).astype(F)
    for nrm32 in (N32, unit32):
        tri, qn = rtmi_mod.glyph_mesh(P32[None], nrm32[None], diameter)
        V = grid_of_triangles(tri[0]).astype(np.float64)  # order, winding and shared vertices
        P, N, D = P32.astype(np.float64), nrm32.astype(np.float64), float(F(diameter))
        T = np.array([0.0, -N[2], N[1]]) / math.hypot(N[2], N[1])  # |N.x| <= |N.y|: the frame's second branch
        assert abs(N[0]) <= abs(N[1])
        B = np.cross(N, T)
        nn = np.linalg.norm(N)
        R = V - P
        a, b, c = R @ T, (R @ N) / nn ** 2, (R @ B) / nn ** 2  # R = a T + b N + c B, the frame being orthogonal
        coords = np.stack([a, b, c], axis=2)
        # the direction of every vertex in (T, N, B) is the closed-form Chiu map
        want = np.array([[chiu_f64(x / 12.0, y / 12.0) for y in range(13)] for x in range(13)])
        assert np.max(np.abs(coords / D - want)) <= 1e-5
        # its length: D in frame coordinates; in space what the frame's lengths (1, |N|, |N|) make of it
        assert np.max(np.abs(np.linalg.norm(coords, axis=2) / D - 1.0)) <= 1e-5
        dist = np.linalg.norm(R, axis=2)
        assert np.max(np.abs(dist / np.sqrt(a * a + nn ** 2 * (b * b + c * c)) - 1.0)) <= 1e-5
        if nrm32 is unit32:  # |V - P| = D |N|, to the letter, where |N| = 1
            assert abs(nn - 1.0) < 1e-7
            assert np.max(np.abs(dist / (D * nn) - 1.0)) <= 1e-5
        # rim vertices lie on the base plane, (6, 6) is the pole
        rim = np.zeros((13, 13), bool)
        rim[[0, 12], :] = rim[:, [0, 12]] = True
        assert np.max(np.abs((R @ N)[rim])) / nn <= 1e-5 * D
        assert np.min((R @ N)[~rim]) > 0
        assert np.max(np.abs(V[6, 6] - (P + N * D))) <= 1e-5 * D
        # the quad normals: unit length, along centroid - P
        q = qn[0].astype(np.float64)
        assert np.max(np.abs(np.linalg.norm(q, axis=1) - 1.0)) <= 1e-6
        for x in range(12):
            for y in range(12):
                mid = (V[x, y] + V[x + 1, y] + V[x, y + 1] + V[x + 1, y + 1]) / 4.0 - P
                assert np.linalg.norm(q[x * 12 + y] - mid / np.linalg.norm(mid)) <= 1e-5, (x, y)


# ---------------------------------------------------------------- CPU: colours ----------

def test_colours_equal_float32_restatement(rtmi_mod, oracle_mod):
    G = rtmi_mod.glyphs
    v = np.concatenate([value_table(oracle_mod, 3), rtmi_mod.read_selected(SELECTED)[2]])
    v[1] -= F(0.5)                     # signed values
    zero = np.zeros((1, 144), F)       # the zero row
    peak = np.zeros((1, 144), F)       # a row with one maximum
    peak[0, 77] = 3.5
    neg = -value_table(oracle_mod, 1) - F(1)  # RATIO: m stays 0
    allv = np.concatenate([v, zero, peak, neg])
    for mode in (G.RATIO, G.MAGNITUDE):
        got = rtmi_mod.glyph_colours(allv, mode)
        assert got.shape == (len(allv), 144, 3) and got.dtype == F
        assert np.array_equal(bits(got), bits(colours_f32(allv, mode))), mode
    ratio = rtmi_mod.glyph_colours(allv, G.RATIO)
    iz, ip, ineg = len(v), len(v) + 1, len(v) + 2
    assert np.array_equal(ratio[iz], np.tile(np.array([0, 1, 0], F), (144, 1)))
    assert np.array_equal(ratio[ineg], ratio[iz])
    assert np.array_equal(ratio[ip, 77], [1, 0, 0]) and np.array_equal(np.delete(ratio[ip], 77, 0), ratio[iz][:143])
    grey = rtmi_mod.glyph_colours(allv, G.MAGNITUDE)
    assert np.all(grey[iz] == 1) and np.all(grey[ip, 77] == 0) and np.all(np.delete(grey[ip], 77, 0) == 1)
    assert np.all(grey[..., 0] == grey[..., 1]) and np.all(grey[..., 1] == grey[..., 2])


# ---------------------------------------------------------------- CPU: refusals ----------

def test_host_entries_refuse_bad_arguments(rtmi_mod):
    L = rtmi_mod.lib()
    G = rtmi_mod.glyphs
    pos, nrm = np.array([[0.1, 0.2, 0.3]], F), np.array([[0, 1, 0]], F)
    for bad_pos, bad_nrm, d in ((np.array([[np.nan, 0, 0]], F), nrm, 0.15), (pos, np.array([[0, np.inf, 0]], F), 0.15),
                                (pos, np.zeros((1, 3), F), 0.15), (pos, nrm, 0.0), (pos, nrm, -0.15),
                                (pos, nrm, float("nan")), (pos, nrm, float("inf"))):
        with pytest.raises(rtmi_mod.RtError) as e:
            rtmi_mod.glyph_mesh(bad_pos, bad_nrm, d)
        assert e.value.code == -1
    for bad in (np.nan, np.inf, -np.inf):
        v = np.zeros((2, 144), F)
        v[1, 143] = bad
        for mode in (G.RATIO, G.MAGNITUDE):
            with pytest.raises(rtmi_mod.RtError) as e:
                rtmi_mod.glyph_colours(v, mode)
            assert e.value.code == -1
    with pytest.raises(rtmi_mod.RtError) as e:
        rtmi_mod.glyph_colours(np.zeros((1, 144), F), 2)
    assert e.value.code == -1
    # nothing to do is not an error
    assert rtmi_mod.glyph_mesh(np.zeros((0, 3), F), np.zeros((0, 3), F))[0].shape == (0, 288, 9)
    assert rtmi_mod.glyph_colours(np.zeros((0, 144), F)).shape == (0, 144, 3)
    assert L.rt_glyph_mesh(None, None, 1, 0.15, None, None) == -1
    assert L.rt_glyph_colours(None, 1, 0, None) == -1


def test_device_entries_refuse_before_any_device_work(rtmi_mod):
    """No GPU here: every one of these returns before a device is touched."""
    L = rtmi_mod.lib()
    G = rtmi_mod.glyphs
    n = G.MAX + 1
    pos, nrm, val = np.zeros((n, 3), F), np.tile(np.array([0, 1, 0], F), (n, 1)), np.ones((n, 144), F)
    h = ctypes.c_void_p()
    fp = lambda a: a.ctypes.data_as(_FP)  # noqa: E731
    assert G.MAX == rtmi_mod.RT_GLYPH_MAX == 256
    assert L.rt_glyphs_create(None, fp(pos), fp(nrm), fp(val), n, 0.15, 0, ctypes.byref(h)) == -1
    assert b"257" in L.rt_last_error()
    assert L.rt_glyphs_create(None, fp(pos), fp(nrm), fp(val), -1, 0.15, 0, ctypes.byref(h)) == -1
    assert L.rt_glyphs_create(None, fp(pos), fp(nrm), fp(val), 1, 0.15, 0, ctypes.byref(h)) == -1  # no context
    assert L.rt_glyphs_create(None, None, None, None, 0, 0.15, 0, ctypes.byref(h)) == -1            # no context
    assert L.rt_glyphs_create_sized(None, fp(pos), fp(nrm), fp(val), None, 2, 0, ctypes.byref(h)) == -1
    assert L.rt_glyphs_create_sized(None, fp(pos), fp(nrm), fp(val), fp(val), n, 0, ctypes.byref(h)) == -1
    assert not h
    assert L.rt_glyphs_set_colours(None, None) == -1 and L.rt_glyphs_info(None, None, None, None) == -1
    assert L.rt_glyphs_destroy(None) == 0
    cam = rtmi_mod.camera()
    out = np.zeros((8, 8, 3), F)
    opts = rtmi_mod.RtGlyphViewOpts(0)
    tiles = np.zeros((1, 2), np.int32)

    def both(p):
        a = L.rt_render_glyph_view(None, None, None, ctypes.byref(cam), p, ctypes.byref(opts), 0, None, fp(out),
                                   None, None, None, None)
        b = L.rt_render_glyph_view_tiles_device(None, None, None, ctypes.byref(cam), p, ctypes.byref(opts), 0, None,
                                                tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 16, None, None)
        assert a == b
        return a

    def params(**kw):
        p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, width=8, height=8, spp=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)

    assert both(None) == -1
    for bad in ({"spp": 0}, {"spp": -3}, {"width": 0}, {"height": -1}, {"spp": 6, "spp_split": 4}, {"spp": 9, "spp_split": 3},
                {"spp": 128, "spp_split": 128}):
        assert both(params(**bad)) == -1, bad
    assert both(params(preset=rtmi_mod.RT_PRESET_CPU)) == -5
    assert both(params(hit_rule=rtmi_mod.RT_HIT_RULE_CPU)) == -5
    assert both(params()) == -1 and b"NULL" in L.rt_last_error()  # good params, no handles


# ---------------------------------------------------------------- GPU ----------

CORNELL_SET = (  # position, normal, diameter
    ((0.0, 1.0, -0.5), (0.0, -1.0, 0.0), 0.4),    # floor
    ((-0.6, 1.0, -0.8), (0.0, -1.0, 0.0), 0.4),   # floor
    ((0.5, 0.2, 1.0), (0.0, 0.0, -1.0), 0.4),     # back wall
    ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.4),     # side wall
    ((0.6, 1.0, 0.6), (0.0, -1.0, 0.0), 0.4),     # behind the tall block, wholly hidden
    ((0.0, 0.0, -2.0), (0.0, 0.0, -1.0), 0.15),   # floating, facing the camera
    ((0.3, -1.0, 0.0), (0.0, 1.0, 0.0), 0.4),     # on the ceiling, in front of the light
)
ENV = 0.25  # env_light of every view: a miss is visible


def glyph_set(rtmi_mod, name):
    """(scene, positions, normals, one diameter per glyph)"""
    if name == "cornell7":
        return ("cornell", np.array([g[0] for g in CORNELL_SET], F), np.array([g[1] for g in CORNELL_SET], F),
                np.array([g[2] for g in CORNELL_SET], F))
    if name == "inside":  # the camera (0, 0, -3) is inside the glyph
        return "cornell", np.array([[0, 0, -3.05]], F), np.array([[0, 0, 1]], F), np.array([0.4], F)
    pos, nrm, _ = rtmi_mod.read_selected(SELECTED)
    return "door_room", pos, nrm, np.full(len(pos), {"door015": 0.15, "door04": 0.4}[name], F)


class Stage:
    """One glyph set over its scene: the device scene and set, the mesh, the soup [scene surfaces,
    glyph triangles, lights] as a scene of its own, and per (shape, first sample) the restated
    rays and hits -- computed once, shared by the tests and left unchanged."""

    def __init__(self, rtmi_mod, oracle_mod, ctx, scenes, name):
        self.rtmi, self.oracle, self.ctx, self.name = rtmi_mod, oracle_mod, ctx, name
        self.scene_name, self.pos, self.nrm, self.diam = glyph_set(rtmi_mod, name)
        self.g, self.sc = scenes(self.scene_name)
        self.values = value_table(oracle_mod, len(self.pos))
        self.table = rtmi_mod.glyph_colours(self.values)
        meshes = [rtmi_mod.glyph_mesh(self.pos[i:i + 1], self.nrm[i:i + 1], float(self.diam[i])) for i in range(len(self.pos))]
        self.tri = np.concatenate([m[0] for m in meshes]).reshape(-1, 9)
        self.qn = np.concatenate([m[1] for m in meshes])
        same = bool(np.all(self.diam == self.diam[0]))
        self.gl = rtmi_mod.Glyphs(ctx, self.pos, self.nrm, self.values, float(self.diam[0]) if same else self.diam)
        self.n_g = self.tri.shape[0]
        self.soup = np.concatenate([self.g.tri, self.tri, self.g.light])
        self._soup_scene = None
        self.cam = rtmi_mod.camera(rtmi_mod.CAMERAS[self.scene_name])
        self.ocam = oracle_mod.camera(rtmi_mod.CAMERAS[self.scene_name])
        self._ref = {}

    @property
    def soup_scene(self):
        if self._soup_scene is None:
            geom = self.rtmi.Geometry(np.concatenate([self.g.tri, self.tri]),
                                      np.concatenate([self.g.albedo, np.zeros((self.n_g, 3), F)]), self.g.light,
                                      self.g.emission, self.g.light_group)
            self._soup_scene = self.rtmi.Scene(self.ctx, geom)
        return self._soup_scene

    def params(self, W, H, spp=1, split=1, **kw):
        p = self.rtmi.default_params(self.rtmi.RT_PRESET_GPU, width=W, height=H, spp=spp, spp_split=split, env_light=ENV)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def ref(self, W, H, first):
        """Sample `first` of every pixel: rays, the soup's hit decoded, the scene's own hit."""
        key = (W, H, first)
        if key not in self._ref:
            p = self.params(W, H)
            op = self.oracle.params_from(p)
            ns, nl, ng = self.g.n_surf, self.g.n_light, self.n_g
            hit = self.oracle.primary_hits(self.soup, ns + ng, nl, self.ocam, op, (0, 0, W, H), first, first + 1)[:, :, 0]
            own = self.oracle.primary_hits(self.g.all_triangles(), ns, nl, self.ocam, op, (0, 0, W, H), first,
                                           first + 1)[:, :, 0]
            is_g = (hit >= ns) & (hit < ns + ng)
            j = np.where(is_g, hit - ns, 0)
            self._ref[key] = {
                "d": camera_dirs(self.oracle, p, self.cam, first), "hit": hit, "own": own, "is_g": is_g,
                "glyph": np.where(is_g, j // 288, -1).astype(np.int32),
                "sector": np.where(is_g, (j % 288) // 2, -1).astype(np.int32),
                # the soup's hit as a triangle of the scene (-1: a miss; meaningless on glyph pixels)
                "as_scene": np.where(hit >= ns + ng, hit - ng, hit),
            }
        return self._ref[key]

    def expected_rgb(self, r, tri, base, table=None, shade_d=None):
        """What the AOVs select: the glyph's sector colour (times the shading factor), else the base, else
        the scene's albedo / emission / env_light."""
        table = self.table if table is None else table
        ns = self.g.n_surf
        if base is None:
            base = np.full(tri.shape + (3,), F(ENV), F)
            surf, light = (tri >= 0) & (tri < ns), tri >= ns
            base[surf] = self.g.albedo[tri[surf]]
            base[light] = self.g.emission[tri[light] - ns]
        col = table[np.maximum(r["glyph"], 0), np.maximum(r["sector"], 0)]
        if shade_d is not None:
            nq = self.qn[np.maximum(r["glyph"], 0), np.maximum(r["sector"], 0)]
            dot = (nq[..., 0] * shade_d[..., 0] + nq[..., 1] * shade_d[..., 1]) + nq[..., 2] * shade_d[..., 2]
            f = F(0.25) + F(0.75) * np.maximum(-dot, F(0))
            assert f.dtype == F
            col = col * f[..., None]
        return np.where(r["is_g"][..., None], col, base).astype(F)

    def close(self):
        self.gl.close()
        if self._soup_scene is not None:
            self._soup_scene.close()


def camera_dirs(oracle_mod, p, cam, s):
    """rt_oracle.c's camera_ray (GPU preset) for sample s of every pixel, in numpy float32:
    direction (H, W, 3) -- as tests/test_volume_view.py restates it."""
    f = np.float32
    W, H = p.width, p.height
    key = [p.seed & 0xFFFFFFFF, (p.seed >> 32) & 0xFFFFFFFF]
    r1, r2 = np.zeros((H, W), f), np.zeros((H, W), f)
    for y in range(H):
        for x in range(W):
            w = oracle_mod.philox([y * W + x, s, 0, 0], key)
            u = (w[:2] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
            r1[y, x], r2[y, x] = u[0], u[1]
    px, py = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    dx = (px + r1) - f(W) / f(2)
    dy = (py + r2) - f(H) / f(2)
    dz = np.full((H, W), f(H), f)
    inv = f(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx * inv, dy * inv, dz * inv
    cy, sy = f(math.cos(float(f(cam.yaw_y)))), f(math.sin(float(f(cam.yaw_y))))
    cx, sx = f(math.cos(float(f(cam.yaw_x)))), f(math.sin(float(f(cam.yaw_x))))
    z, one = f(0), f(1)
    rx = (cy * dx + z * dy) + (-sy * dz + z * one)
    ry = (z * dx + one * dy) + (z * dz + z * one)
    rz = (sy * dx + z * dy) + (cy * dz + z * one)
    rw = (z * dx + z * dy) + (z * dz + one * one)
    qx = (one * rx + z * ry) + (z * rz + z * rw)
    qy = (z * rx + cx * ry) + (sx * rz + z * rw)
    qz = (z * rx + -sx * ry) + (cx * rz + z * rw)
    d = np.stack([qx, qy, qz], axis=2)
    assert d.dtype == f
    return d


@pytest.fixture(scope="module")
def stages(rtmi_mod, oracle_mod, gpu_ctx):
    scenes, made = {}, {}

    def scene(name):
        if name not in scenes:
            g = (rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_GPU) if name == "cornell"
                 else rtmi_mod.obj_geometry(os.path.join(MODELS, name + ".obj"), name))
            scenes[name] = (g, rtmi_mod.Scene(gpu_ctx, g))
        return scenes[name]

    def get(name):
        if name not in made:
            made[name] = Stage(rtmi_mod, oracle_mod, gpu_ctx, scene, name)
        return made[name]

    yield get
    for s in made.values():
        s.close()
    for _, sc in scenes.values():
        sc.close()


# (glyph set, width, height)
CASES = [("cornell7", 50, 39), ("door04", 80, 72), ("door015", 80, 72), ("door04", 17, 5), ("door04", 1, 1),
         ("inside", 50, 39)]
CASE_IDS = [f"{c[0]}-{c[1]}x{c[2]}" for c in CASES]
FIRST = (0, 5)


def base_image(W, H):
    return np.random.default_rng(W * 1000 + H).random((H, W, 3), dtype=F)


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_winner_equals_scan_of_the_soup(stages, case, first):
    name, W, H = case
    st = stages(name)
    r = st.ref(W, H, first)
    _, tri, glyph, sector, _ = st.gl.view(st.sc, st.cam, st.params(W, H), first, aov=True)
    assert np.array_equal(glyph, r["glyph"]) and np.array_equal(sector, r["sector"])
    assert np.array_equal(tri, r["own"])  # the scene's own hit, glyph in front or not
    assert np.array_equal(tri[~r["is_g"]], r["as_scene"][~r["is_g"]])  # the winner's class where no glyph won
    # the conditions that make the case worth running
    n_glyph = np.count_nonzero(r["is_g"])
    print(f"{name} {W}x{H} sample {first}: {n_glyph} glyph pixels of {W * H}, per glyph "
          f"{np.bincount(glyph[glyph >= 0], minlength=st.gl.n_glyphs).tolist()}, "
          f"{len(set(zip(glyph[glyph >= 0].tolist(), sector[glyph >= 0].tolist())))} (glyph, sector) pairs, "
          f"{np.count_nonzero(r['hit'] >= st.g.n_surf + st.n_g)} light pixels, {np.count_nonzero(r['hit'] < 0)} misses")
    if (name, W, H) == ("cornell7", 50, 39):
        per = np.bincount(glyph[glyph >= 0], minlength=7)
        assert n_glyph >= 300 and np.all(np.delete(per, 4) >= 10) and per[4] == 0
        assert len(set(zip(glyph[glyph >= 0].tolist(), sector[glyph >= 0].tolist()))) >= 150
        assert np.count_nonzero(r["hit"] >= st.g.n_surf + st.n_g) >= 5 and np.count_nonzero(r["hit"] < 0) >= 100
        hidden = r["is_g"] & (r["own"] >= st.g.n_surf)  # the ceiling glyph in front of the light
        assert hidden.any()
    elif (name, W, H) == ("door04", 80, 72):
        assert n_glyph >= 1000
    elif (name, W, H) == ("door015", 80, 72):
        assert n_glyph >= 100 and not np.any(glyph == 2)  # the third glyph is off screen
    elif name == "inside":
        assert r["is_g"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", (CASES[0], CASES[1]), ids=(CASE_IDS[0], CASE_IDS[1]))
def test_gpu_scene_hit_equals_volume_view(rtmi_mod, gpu_ctx, stages, case):
    name, W, H = case
    st = stages(name)
    with rtmi_mod.sarsa.RadianceMap(gpu_ctx, st.sc, SEED, 0.1) as rm:
        for first in FIRST:
            p = st.params(W, H)
            tri = st.gl.view(st.sc, st.cam, p, first, aov=True)[1]
            assert np.array_equal(tri, rm.view(st.cam, p, first, aov=True)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_t_equals_intersect_on_the_soup(rtmi_mod, gpu_ctx, stages, case, first):
    name, W, H = case
    st = stages(name)
    r = st.ref(W, H, first)
    p = st.params(W, H)
    t = st.gl.view(st.sc, st.cam, p, first, aov=True)[4]
    o = np.broadcast_to(np.array(rtmi_mod.CAMERAS[st.scene_name][:3], F), r["d"].shape)
    sc = st.soup_scene
    assert sc.geom.n_tri > 256  # the BVH path; then the scan
    modes = (rtmi_mod.ACCEL_AUTO, rtmi_mod.ACCEL_SCAN) if (case, first) == (CASES[0], 0) else (rtmi_mod.ACCEL_AUTO,)
    for mode in modes:
        sc.set_accel(mode)
        want_t, codes = rtmi_mod.intersect(gpu_ctx, sc, o.reshape(-1, 3), r["d"].reshape(-1, 3), p.t_scale, 1)
        assert np.array_equal(bits(t), bits(want_t.reshape(H, W))), mode
        c = codes.reshape(H, W).astype(np.int64) & 0xFFFFFFFF
        tri = np.where(codes.reshape(H, W) == -1, -1,
                       np.where((c >> 30) == 2, c & 0x3FFFFFFF, st.g.n_surf + st.n_g + (c & 0x3FFFFFFF)))
        assert np.array_equal(tri, r["hit"]), mode
    sc.set_accel(rtmi_mod.ACCEL_AUTO)
    assert np.all(np.isinf(t[r["hit"] < 0])) and np.all(np.isfinite(t[r["hit"] >= 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_colour_is_what_the_aovs_select(stages, case, first):
    name, W, H = case
    st = stages(name)
    r = st.ref(W, H, first)
    p = st.params(W, H)
    base = base_image(W, H)
    rgb, tri, *_ = st.gl.view(st.sc, st.cam, p, first, aov=True)
    assert np.array_equal(bits(rgb), bits(st.expected_rgb(r, tri, None)))
    assert np.array_equal(rgb, st.gl.view(st.sc, st.cam, p, first))  # the same image without the AOVs
    over = st.gl.view(st.sc, st.cam, p, first, base=base)
    assert np.array_equal(bits(over), bits(st.expected_rgb(r, tri, base)))
    shaded = st.gl.view(st.sc, st.cam, p, first, base=base, shade=True)
    assert np.array_equal(bits(shaded), bits(st.expected_rgb(r, tri, base, shade_d=r["d"])))
    if r["is_g"].any():
        assert not np.array_equal(shaded, over)
    # max_bounces and sampler are ignored
    q = st.params(W, H, max_bounces=1, sampler=st.rtmi.RT_SAMPLER_COSINE)
    assert np.array_equal(over, st.gl.view(st.sc, st.cam, q, first, base=base))


def fold(samples, split):
    """each chunk's samples added in order, the chunk sums added in order, / spp."""
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
    assert tot.dtype == np.float32
    return tot / np.float32(spp)


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", (CASES[0], CASES[3], CASES[4]), ids=(CASE_IDS[0], CASE_IDS[3], CASE_IDS[4]))
def test_gpu_fold_equals_single_sample_views(stages, case, first):
    name, W, H = case
    st = stages(name)
    for base, shade in ((None, False), (base_image(W, H), True)):
        singles = [st.gl.view(st.sc, st.cam, st.params(W, H), first + s, base=base, shade=shade) for s in range(8)]
        if W * H > 1:
            assert not np.array_equal(singles[0], singles[1])  # each sample re-jitters
        for split in (1, 2, 8):
            got = st.gl.view(st.sc, st.cam, st.params(W, H, spp=8, split=split), first, base=base, shade=shade)
            assert np.array_equal(bits(got), bits(fold(singles, split))), split


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_routes_give_the_same_bytes(stages, case, first):
    name, W, H = case
    st = stages(name)
    base = base_image(W, H)
    assert "RTMI_GLYPH_BVH" not in os.environ and st.gl.info()["bvh_nodes"] > 0
    got = {}
    try:
        for route in ("bvh", "scan"):
            if route == "scan":
                os.environ["RTMI_GLYPH_BVH"] = "0"
            got[route] = st.gl.view(st.sc, st.cam, st.params(W, H), first, base=base, shade=True, aov=True) + \
                (st.gl.view(st.sc, st.cam, st.params(W, H, spp=4, split=2), first),)
    finally:
        os.environ.pop("RTMI_GLYPH_BVH", None)
    for a, b in zip(got["bvh"], got["scan"]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("yaws", ({}, {"yaw_y": 0.3}, {"yaw_x": 0.2}), ids=("straight", "yaw_y", "pitched"))
def test_gpu_scene_routes_give_the_same_hits(rtmi_mod, oracle_mod, gpu_ctx, stages, yaws):
    """The scene's own cast: the rectangle cull (pitch 0), the plain scan (a pitched camera has no
    cull) and the scene's BVH where its accel mode turns it on -- against the scan of the soup."""
    st = stages("cornell7")
    W, H, first = 50, 39, 5
    p = st.params(W, H)
    cam = rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"], **yaws)
    ocam = oracle_mod.camera(rtmi_mod.CAMERAS["cornell"], **yaws)
    ns, ng = st.g.n_surf, st.n_g
    hit = oracle_mod.primary_hits(st.soup, ns + ng, st.g.n_light, ocam, oracle_mod.params_from(p), (0, 0, W, H), first,
                                  first + 1)[:, :, 0]
    is_g = (hit >= ns) & (hit < ns + ng)
    assert np.count_nonzero(is_g) >= 100 and np.count_nonzero(~is_g) >= 100
    base = base_image(W, H)
    got = st.gl.view(st.sc, cam, p, first, base=base, shade=True, aov=True)
    assert np.array_equal(got[2], np.where(is_g, (hit - ns) // 288, -1))
    assert np.array_equal(got[3], np.where(is_g, ((hit - ns) % 288) // 2, -1))
    assert np.array_equal(got[1][~is_g], np.where(hit >= ns + ng, hit - ng, hit)[~is_g])
    with rtmi_mod.Scene(gpu_ctx, st.g) as sc:
        sc.set_accel(rtmi_mod.ACCEL_BVH)
        assert sc.accel_info()["nodes"] > 0
        for a, b in zip(got, st.gl.view(sc, cam, p, first, base=base, shade=True, aov=True)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRST)
def test_gpu_tiles_equal_rectangle_render(rtmi_mod, stages, first):
    import torch
    st = stages("door04")
    W, H, T = 80, 72, 32
    p = st.params(W, H, spp=4, split=2)
    base = base_image(W, H)
    origins = rtmi_mod.tiles.tile_origins(W, H, T)
    assert len(origins) == 9
    pick = origins[[8, 2, 4, 0, 7, 5, 1, 6, 3]]  # every tile, shuffled
    dev = torch.device("cuda", 0)
    d_base = torch.from_numpy(base).to(dev)
    fill = -7.0
    for b, bp, shade in ((None, 0, False), (base, d_base.data_ptr(), True)):
        full = st.gl.view(st.sc, st.cam, p, first, base=b, shade=shade)
        out = torch.full((len(pick), T, T, 3), fill, dtype=torch.float32, device=dev)
        st.gl.view_tiles_device(st.sc, st.cam, p, pick, T, out.data_ptr(), 0, first, base_ptr=bp, shade=shade)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, (x, y) in enumerate(pick):
            vw, vh = min(T, W - x), min(T, H - y)
            assert np.array_equal(bits(got[k, :vh, :vw]), bits(full[y:y + vh, x:x + vw])), (x, y)
            # the overhang of an edge tile is not written
            assert np.all(got[k, vh:] == fill) and np.all(got[k, :, vw:] == fill), (x, y)
    st.gl.view_tiles_device(st.sc, st.cam, p, pick[:0], T, 0, 0, first)  # an empty tile list is a no-op


@pytest.mark.gpu
def test_gpu_empty_set_returns_the_base(rtmi_mod, gpu_ctx, stages):
    st = stages("cornell7")
    W, H = 50, 39
    p = st.params(W, H)
    base = base_image(W, H)
    with rtmi_mod.Glyphs(gpu_ctx, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 144), F)) as none:
        assert none.info() == {"glyphs": 0, "triangles": 0, "bvh_nodes": 0}
        none.set_colours(np.zeros((0, 144, 3), F))
        for first in FIRST:
            assert np.array_equal(bits(none.view(st.sc, st.cam, p, first, base=base, shade=True)), bits(base))
            rgb, tri, glyph, sector, t = none.view(st.sc, st.cam, p, first, aov=True)
            r = st.ref(W, H, first)
            assert np.array_equal(tri, r["own"]) and np.all(glyph == -1) and np.all(sector == -1)
            empty = {"glyph": glyph, "sector": sector, "is_g": np.zeros((H, W), bool)}
            assert np.array_equal(bits(rgb), bits(st.expected_rgb(empty, tri, None)))  # the albedo view
            assert np.array_equal(np.isinf(t), tri < 0)


@pytest.mark.gpu
def test_gpu_set_colours_changes_the_colour_only(rtmi_mod, gpu_ctx, stages):
    src = stages("cornell7")
    W, H, first = 50, 39, 0
    p = src.params(W, H)
    r = src.ref(W, H, first)
    with rtmi_mod.Glyphs(gpu_ctx, src.pos, src.nrm, src.values, src.diam) as gl:
        before = gl.view(src.sc, src.cam, p, first, aov=True)
        table = np.random.default_rng(7).random((gl.n_glyphs, 144, 3), dtype=F)
        gl.set_colours(table)
        after = gl.view(src.sc, src.cam, p, first, aov=True)
        for a, b in zip(before[1:], after[1:]):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(bits(after[0]), bits(src.expected_rgb(r, after[1], None, table=table)))
        assert not np.array_equal(before[0], after[0])
        with pytest.raises(ValueError):
            gl.set_colours(table[:3])
        # the CPU engine's colouring
        with rtmi_mod.Glyphs(gpu_ctx, src.pos, src.nrm, src.values, src.diam, rtmi_mod.glyphs.MAGNITUDE) as grey:
            got = grey.view(src.sc, src.cam, p, first)
            want = src.expected_rgb(r, after[1], None, table=rtmi_mod.glyph_colours(src.values, rtmi_mod.glyphs.MAGNITUDE))
            assert np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell7", "door04"))
def test_gpu_view_reads_only(rtmi_mod, gpu_ctx, stages, name):
    st = stages(name)
    W, H = 50, 39
    p = st.params(W, H, spp=4, split=2)
    # a render first, so that the scene has whatever tables its renders build
    rtmi_mod.render(gpu_ctx, st.sc, st.cam, st.params(16, 16, max_bounces=3))
    state = lambda: (st.sc.ctab_info(0), st.sc.ctab_info(1), st.sc.accel_info(), st.gl.info())  # noqa: E731
    before = state()
    first = st.gl.view(st.sc, st.cam, p, 3, base=base_image(W, H), shade=True, aov=True)
    assert state() == before
    again = st.gl.view(st.sc, st.cam, p, 3, base=base_image(W, H), shade=True, aov=True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert state() == before


@pytest.mark.gpu
def test_gpu_view_refuses_bad_arguments(rtmi_mod, stages):
    st = stages("door04")
    for bad, code in (({"spp": 0}, -1), ({"spp": 6, "split": 4}, -1), ({"W": 0}, -1),
                      ({"preset": rtmi_mod.RT_PRESET_CPU}, -5), ({"hit_rule": rtmi_mod.RT_HIT_RULE_CPU}, -5)):
        kw = {"W": 8, "H": 8}
        kw.update(bad)
        with pytest.raises(rtmi_mod.RtError) as e:
            st.gl.view(st.sc, st.cam, st.params(**kw))
        assert e.value.code == code, bad
    with pytest.raises(ValueError):
        st.gl.view(st.sc, st.cam, st.params(8, 8), base=np.zeros((4, 4, 3), F))
    L = rtmi_mod.lib()
    p = st.params(8, 8)
    assert L.rt_render_glyph_view(st.ctx.handle, st.sc.handle, st.gl.handle, ctypes.byref(st.cam), ctypes.byref(p), None, 0,
                                  None, None, None, None, None, None) == -1  # out_rgb is required
    out = np.zeros((8, 8, 3), F)  # opts may be NULL: no shading
    assert L.rt_render_glyph_view(st.ctx.handle, st.sc.handle, st.gl.handle, ctypes.byref(st.cam), ctypes.byref(p), None, 0,
                                  None, out.ctypes.data_as(_FP), None, None, None, None) == 0
    assert np.array_equal(out, st.gl.view(st.sc, st.cam, p))
