"""k_render_ps's pending list (rt_kernels.hip: ps_body's pipelined loop): a sample whose cast
ends on a surface with one bounce left is parked -- its hit point in its own slot, its entry in
the wave's pending list -- and a light pre-test pass runs inside the loop only on 64 pending
samples, lane l on the l-th oldest; what is left runs after the loop, the last pass partial.

The specification does not change, so the yardstick is test_ps_pipeline.py's: CPU preset,
t_scale 256, the table route asserted, the uint32 view of the image and the ray casts against
the CPU restatement (oracle.render).  The cases pin image and casts at the shapes where the
list's bookkeeping can go wrong, not the mechanism:

  spp 64, split 64    per_chunk 1: at most 64 pending samples, every pass runs after the loop
  spp 128             per_chunk 2: one pass inside the loop, or none
  spp 192, 256        per_chunk 3 and 4 (the bench's wave): more than 128 samples go through the
                      list, so entries move from its second register to its first
  (64, 16), (16, 4)   several pixels per wave: the narrow layout with per-lane pixel words
  spp 320, 512        per_chunk 5 and 8: the wide layout
  closed corner       every bounce cast ends on a surface: 64 new pending samples per trip, a full
                      pass in every trip but the first and one after the loop, nothing left over
  all miss            the queue and the list are both empty
  crowded views       test_ps_settle.py's, 32 x 32 x 256: passes settled inside full passes and
                      in the passes after the loop; on the sheet scene the window's tie rule decides

Every case but the all-miss view and max_bounces 0 and 1 must have a terminal cast that ends on
a light (test_cases_reach_the_light, on the CPU): the restatement's image at max_bounces 2
differs from its image at max_bounces 1, which draws the same first two casts of every path.
"""
import dataclasses

import numpy as np
import pytest

from test_ps_pipeline import AWAY_CAM, CROWDED_CAM
from test_ps_settle import sheet_geometry

T_SCALE = 256.0
# Cornell turned a quarter about x, (x, y, z) -> (x, z, -y), and closed with a front wall: the
# ceiling with the light in its plane becomes the wall at z = +1, which a camera at yaw 0 faces.
# From (0.7, 0.7, 0.9), a tenth in front of it, a 40 x 24 frame sees that wall near its corner,
# away from the light: every camera ray ends on it, and no ray leaving it can reach the light (it
# starts in the light's plane) or leave the closed room.
CORNER_CAM = ((0.7, 0.7, 0.9, 1.0), 0.0)


def corner_geometry(g):
    def turn(t):
        v = t.reshape(-1, 3, 3)
        return np.stack([v[..., 0], v[..., 2], -v[..., 1]], axis=-1).reshape(-1, 9).astype(np.float32)

    # the front wall: the back wall (triangles 14, 15: z = 1) mirrored to z = -1, two vertices
    # swapped so that it still faces the room
    back = g.tri[14:16].reshape(-1, 3, 3).copy()
    assert np.all(back[..., 2] == 1.0)
    back[..., 2] = -1.0
    front = back[:, [0, 2, 1], :].reshape(-1, 9)
    tri = np.concatenate([g.tri, front]).astype(np.float32)
    alb = np.concatenate([g.albedo, g.albedo[14:16]]).astype(np.float32)
    return dataclasses.replace(g, tri=turn(tri), albedo=alb, light=turn(g.light))


def _case(id_, scene="cornell", cam=None, light=True, **params):
    return dict(id=id_, scene=scene, cam=cam, light=light, params=params)


F = dict(width=40, height=24)  # (the right-hand column of workgroups is clipped)
SEED_HI = (0x1234ABCD << 32) | 1984
CASES = [
    _case("pc1", spp=64, spp_split=64, **F),
    _case("pc2", spp=128, spp_split=64, **F),
    _case("pc3", spp=192, spp_split=64, **F),
    _case("pc4-bench-wave", spp=256, spp_split=64, **F),
    _case("pc4-17x33", width=17, height=33, spp=256, spp_split=64),
    _case("narrow-4px", spp=64, spp_split=16, **F),
    _case("narrow-16px", spp=16, spp_split=4, **F),
    _case("wide-pc5", spp=320, spp_split=64, **F),
    _case("wide-pc8", spp=512, spp_split=64, **F),
    _case("corner-pc4", scene="corner", cam=CORNER_CAM, spp=256, spp_split=64, **F),
    _case("corner-pc2", scene="corner", cam=CORNER_CAM, spp=128, spp_split=64, **F),
    _case("all-miss", cam=AWAY_CAM, light=False, spp=256, spp_split=64, **F),
    _case("crowded", cam=CROWDED_CAM, width=32, height=32, spp=256, spp_split=64),
    _case("crowded-sheet", scene="sheet", cam=CROWDED_CAM, width=32, height=32, spp=256, spp_split=64),
    _case("bounces0", light=False, max_bounces=0, spp=256, spp_split=64, **F),
    _case("bounces1", light=False, max_bounces=1, spp=256, spp_split=64, **F),
    _case("cosine", sampler="RT_SAMPLER_COSINE", spp=256, spp_split=64, **F),
    _case("cosine-narrow", sampler="RT_SAMPLER_COSINE", spp=64, spp_split=16, **F),
    _case("gpu-rule", hit_rule="RT_HIT_RULE_GPU", spp=256, spp_split=64, **F),
    _case("gpu-rule-cosine-pc3", hit_rule="RT_HIT_RULE_GPU", sampler="RT_SAMPLER_COSINE", spp=192, spp_split=64, **F),
    _case("seed-high-word", seed=SEED_HI, spp=256, spp_split=64, **F),
    _case("seed-high-word-narrow", seed=SEED_HI, spp=16, spp_split=4, **F),
]
IDS = [c["id"] for c in CASES]

_GEOM, _REF = {}, {}


def _geom(rtmi_mod, scene):
    if scene not in _GEOM:
        g = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
        _GEOM[scene] = {"cornell": lambda: g, "sheet": lambda: sheet_geometry(g), "corner": lambda: corner_geometry(g)}[scene]()
    return _GEOM[scene]


def _params(rtmi_mod, case, **over):
    kw = dict(case["params"])
    for name in ("sampler", "hit_rule"):
        if name in kw:
            kw[name] = getattr(rtmi_mod, kw[name])
    kw.update(over)
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, t_scale=T_SCALE, **kw)


def _cam(rtmi_mod, case):
    return case["cam"] if case["cam"] is not None else (rtmi_mod.CAMERAS["cornell"], 0.0)


def _ref(rtmi_mod, oracle_mod, case, **over):
    """The restatement's (image, casts) of a case, computed once and shared (read-only)."""
    key = (case["id"], tuple(sorted(over.items())))
    if key not in _REF:
        pos, yaw_y = _cam(rtmi_mod, case)
        img, casts = oracle_mod.render(_geom(rtmi_mod, case["scene"]), oracle_mod.camera(pos, yaw_y=yaw_y),
                                       oracle_mod.params_from(_params(rtmi_mod, case, **over)))
        img.setflags(write=False)
        _REF[key] = (img, int(casts))
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_reach_the_light(rtmi_mod, oracle_mod, case):
    """(CPU) What the restatement says of each case: a terminal cast ends on a light wherever the
    list is exercised; the corner view's paths all take three casts (every camera ray and every
    bounce cast ends on a surface); the all-miss view casts camera rays only."""
    p = _params(rtmi_mod, case)
    n = p.width * p.height * p.spp
    img, casts = _ref(rtmi_mod, oracle_mod, case)
    if case["light"]:
        assert p.max_bounces == 2
        one, casts_one = _ref(rtmi_mod, oracle_mod, case, max_bounces=1)
        changed = int(np.count_nonzero(np.any(img.view(np.uint32) != one.view(np.uint32), axis=2)))
        print(f"{case['id']}: casts {casts} ({casts_one} at one bounce), {changed} pixels take light from a terminal cast")
        assert changed > 0 and casts > casts_one
    if case["scene"] == "corner":
        assert casts == 3 * n
    if case["id"] == "all-miss":
        assert casts == n and not np.any(img)


@pytest.fixture(scope="module")
def scenes(rtmi_mod, gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = rtmi_mod.Scene(gpu_ctx, _geom(rtmi_mod, name))
        return made[name]

    yield get
    for sc in made.values():
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_and_casts(rtmi_mod, oracle_mod, gpu_ctx, scenes, case):
    p = _params(rtmi_mod, case)
    pos, yaw_y = _cam(rtmi_mod, case)
    sc = scenes(case["scene"])
    img, casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(pos, yaw_y=yaw_y), p)
    assert sc.ctab_info(p.hit_rule)["built"]  # the table route was taken
    ref, ref_casts = _ref(rtmi_mod, oracle_mod, case)
    print(f"{case['id']}: casts {casts} (oracle {ref_casts}), "
          f"{int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))} differing words")
    assert casts == ref_casts
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
