"""The Neural-Q training frame (rt_neuralq_render_frame) bit for bit against its restatement.

The pieces of the frame are pinned one by one elsewhere (the sampler, the TD targets, the
training step, the hit rule); what joins them -- which array offsets a batch reads, the Philox
event ids, whether the next-state Q is taken before or after the previous batch's update, the
restart's y/z exchange, the early exit, the sample index across frames, the epsilon decay, the
tail batch -- is pinned here.  oracle.NeuralQ (rt_oracle.c orc_neuralq_frame) restates the frame
in the reference's per-ray arrays without evaluating a network: it calls q_fn and step_fn where
the renderer evaluates and updates its own.

Lockstep: two DqnTrainers start from the same weights.  A renders with NeuralQ.render_frame; B
serves the restatement's callbacks (q_fn = rt_dqn_trainer_forward_device, step_fn =
rt_dqn_train_step_device).  If the frame is the restatement, B sees A's batches in A's order and
every number agrees bit for bit: the image, the stats rows, the cast count, epsilon, every
per-ray array (rt_neuralq_read_rays) and the eight parameter arrays.  Every comparison is
equality of the uint32 views; nothing here has a tolerance.

The lockstep rests on one assumption: a row of the trainer's forward does not depend on how many
rows are launched with it, nor on where the rows start (the frame passes r.loc + 3 * b0).
test_forward_rows_do_not_depend_on_the_launch checks that on its own.

Coverage is asserted on the restatement's branch counters (_check_coverage), never on the device's, and
the cases were tuned without a GPU on an fp64 network (oracle.AdamRef as q_fn / step_fn): the
branch structure does not hang on the last bits of Q.  Negative controls live on the restatement's
side only (oracle.NQ_VARIANTS): each must make a compared array differ from the device's.

The state the update trains on is the position before the trace for every ray, terminating or
not: the reference (TRAIN_ON_POSITION false) updates on prev_ray_vertices, converted from every
ray's position at the top of the bounce.  prev_ray_locations, which its trace_ray writes on
surface hits only, belongs to the build it does not ship; the prev_surface_only control restates
that array and must differ from the device (rt_oracle.c, the comment of orc_neuralq_frame).

No GPU: the restatement alone with the fp64 network -- the counters of every case, the callback
order, determinism, and that every variant changes its output.
"""
import functools
import os

import numpy as np
import pytest

from conftest import MODELS

HIDDEN = (65, 130, 63)  # test_dqn_train.py's net B: one off the 64-wide tiles on either side

# eps: (start, min, decay).  mixed: 91 rays (less than a workgroup, a tail wave), batches 37/37/17.
# greedy2: 340 rays (two workgroups, the second partial), one batch larger than n, two frames.
CASES = {
    "mixed": dict(scene="cornell", w=13, h=7, spp=2, max_bounces=6, batch=37, eps=(0.5, 0.2, 0.2), frames=1),
    "greedy2": dict(scene="cornell", w=20, h=17, spp=1, max_bounces=6, batch=512, eps=(0.0, 0.0, 0.0), frames=2),
    "dead": dict(scene="cornell", w=13, h=7, spp=2, max_bounces=5, batch=40, eps=(0.0, 0.0, 0.0), frames=1,
                 dead=True),
    "open": dict(scene="door_room", w=9, h=5, spp=2, max_bounces=6, batch=16, eps=(1.0, 1.0, 0.0), frames=1,
                 env_light=0.5),
    "cap2": dict(scene="cornell", w=13, h=7, spp=2, max_bounces=2, batch=64, eps=(0.5, 0.2, 0.2), frames=1),
    "bvh": dict(scene="cornell", w=13, h=7, spp=2, max_bounces=6, batch=37, eps=(0.5, 0.2, 0.2), frames=1,
                bvh=True),
}
VARIANTS = ("target_event", "restart_no_swap", "tp_state2", "q_before_step", "prev_surface_only")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(geometry, camera position, nn_vertices)"""
    import rtmi
    if name == "cornell":
        g = rtmi.cornell_geometry(rtmi.RT_PRESET_GPU)
        # the Cornell box has no OBJ vertex list: its triangles' vertices stand in
        return g, rtmi.CAMERAS["cornell"], g.all_triangles().reshape(-1).astype(np.float32)
    g = rtmi.obj_geometry(os.path.join(MODELS, f"{name}.obj"), name)
    return g, rtmi.CAMERAS[name], np.ascontiguousarray(g.nn_vertices, np.float32).ravel()


@functools.lru_cache(maxsize=None)
def _weights(scene, dead=False):
    import rtmi
    nn = _scene(scene)[2]
    W, b = rtmi.dqn.synthetic_weights(nn.size, seed=1984, hidden=HIDDEN)
    if dead:  # an output bias below every pre-activation: the rectifier leaves Q = 0 everywhere
        b = b[:3] + [np.full(144, -1e6, np.float32)]
    return W, b


def _params(rtmi_mod, case):
    c = CASES[case]
    kw = dict(width=c["w"], height=c["h"], spp=c["spp"], max_bounces=c["max_bounces"])
    if "env_light" in c:
        kw["env_light"] = c["env_light"]
    return rtmi_mod.default_params(rtmi_mod.RT_PRESET_GPU, **kw)


def _run_oracle(oracle_mod, rtmi_mod, case, q_fn, step_fn, variant="none"):
    """(frames [dict], the oracle.NeuralQ) of the case on the restatement"""
    c = CASES[case]
    g, cam_pos, _ = _scene(c["scene"])
    nq = oracle_mod.NeuralQ(g, q_fn, step_fn, batch_size=c["batch"], epsilon_start=c["eps"][0],
                            epsilon_min=c["eps"][1], epsilon_decay=c["eps"][2], variant=variant)
    ocam, op = oracle_mod.camera(cam_pos), oracle_mod.params_from(_params(rtmi_mod, case))
    return [nq.render_frame(ocam, op) for _ in range(c["frames"])], nq


def _fp64_net(oracle_mod, case):
    """the CPU stand-in for the trainer: (q_fn, step_fn) on an fp64 AdamRef"""
    c = CASES[case]
    ref = oracle_mod.AdamRef(_scene(c["scene"])[2], *_weights(c["scene"], c.get("dead", False)))
    return (lambda loc: ref.forward(loc)[4].astype(np.float32)), (lambda loc, act, tgt: ref.step(loc, act, tgt)[0])


def _check_coverage(case, frames):
    """the branches the case exists for, on the restatement's own counters (summed over frames)"""
    c = CASES[case]
    k = {name: sum(f["counters"][name] for f in frames) for name in frames[0]["counters"]}
    n = c["w"] * c["h"]
    rows = k["greedy"] + k["explore"]
    print(f"{case}: {k}, casts {[f['casts'] for f in frames]}")
    assert k["miss"] + k["light"] == k["restart"]  # every terminated ray restarts in its bounce
    assert rows % n == 0 and sum(f["casts"] for f in frames) == rows + n * c["spp"] * c["frames"]
    if case in ("mixed", "bvh"):
        assert k["greedy"] >= 0.2 * rows and k["explore"] >= 0.2 * rows
        assert k["restart"] >= 1 and k["second_restart"] >= 1 and k["light"] >= 1
    if case == "greedy2":
        assert k["explore"] == 0 and k["greedy"] > k["no_cell"]
    if case == "dead":
        assert k["explore"] == 0 and k["greedy"] > 0 and k["no_cell"] == k["greedy"]
        # the early exit: some sample left the bounce loop before max_bounces
        assert rows < n * c["spp"] * c["frames"] * (c["max_bounces"] - 1)
    if case == "open":
        assert k["miss"] >= 1 and k["greedy"] == 0
    if case == "cap2":
        assert k["live_at_cap"] >= 1
        assert rows == n * c["spp"]  # no early exit: both bounces ran in every sample
        for f in frames:
            live = f["rays"]["state"] == 0
            assert live.any() and np.all(f["rays"]["bounces"][live] == c["max_bounces"])
    return k


def _first_difference(got, want, names=("device", "restatement")):
    """None, or "array[ray]: <got> vs <want>" of the first array that differs in a bit"""
    for name in want:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape:
            return f"{name}: shape {a.shape} vs {b.shape}"
        if a.dtype != b.dtype:
            return f"{name}: dtype {a.dtype} vs {b.dtype}"
        av, bv = a.view(np.uint32) if a.dtype.itemsize == 4 else a, b.view(np.uint32) if b.dtype.itemsize == 4 else b
        if not np.array_equal(av, bv):
            flat = np.flatnonzero((av != bv).reshape(av.shape[0], -1).any(axis=1)) if av.ndim else np.array([0])
            i = int(flat[0])
            return f"{name}[{i}]: {names[0]} {a[i] if a.ndim else a} vs {names[1]} {b[i] if b.ndim else b} " \
                   f"({flat.size} of {av.shape[0] if av.ndim else 1} rows differ)"
    return None


def _flatten(frames, eps, params=None):
    """one dict of named arrays for _first_difference: per frame the image (a row per ray), the
    stats, the casts, the per-ray arrays; epsilon; the parameters"""
    import oracle
    out = {}
    for i, f in enumerate(frames):
        out[f"frame{i}.img"] = f["img"].reshape(-1, 3)
        out[f"frame{i}.stats"] = f["stats"]
        out[f"frame{i}.casts"] = np.array([f["casts"]], np.uint64)
        assert set(f["rays"]) == {name for name, _, _ in oracle.NQ_RAYS}
        for name, _, _ in oracle.NQ_RAYS:
            out[f"frame{i}.{name}"] = f["rays"][name]
    out["epsilon"] = np.array([eps], np.float32)
    if params is not None:
        W, b = params
        for l in range(4):
            out[f"W{l}"], out[f"b{l}"] = W[l], b[l]
    return out


# --- no GPU: the restatement alone ----------------------------------------------

@functools.lru_cache(maxsize=None)
def _cpu_run(case, variant="none"):
    import oracle
    import rtmi
    frames, nq = _run_oracle(oracle, rtmi, case, *_fp64_net(oracle, case), variant=variant)
    return frames, nq.epsilon, tuple(nq.calls)


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_branch_counters(oracle_mod, rtmi_mod, case):
    """Every case reaches the branches it exists for, on the restatement driven by the fp64
    network; the callbacks come in the renderer's order (per bounce b > 0 one q over all rays,
    then per batch q and step on the batch, the tail batch n % batch last)."""
    c = CASES[case]
    frames, eps, calls = _cpu_run(case)
    _check_coverage(case, frames)
    n = c["w"] * c["h"]
    sizes = [min(c["batch"], n - b0) for b0 in range(0, n, c["batch"])]
    per_bounce = [("q", n)] + [x for nb in sizes for x in (("q", nb), ("step", nb))]
    assert len(calls) % len(per_bounce) == 0 and len(calls) > 0
    assert list(calls) == per_bounce * (len(calls) // len(per_bounce))
    if case == "mixed":
        assert sizes == [37, 37, 17]
    # epsilon: start, then max(eps - decay, min) after every sample, in float
    e = np.float32(c["eps"][0])
    for _ in range(c["spp"] * c["frames"]):
        e = max(np.float32(e - np.float32(c["eps"][2])), np.float32(c["eps"][1]))
    assert np.float32(eps) == e
    for f in frames:
        assert np.isfinite(f["img"]).all() and np.isfinite(f["stats"]).all()
        assert np.array_equal(f["img"].reshape(-1, 3), f["rays"]["total"] / np.float32(c["spp"]))
        assert set(np.unique(f["rays"]["state"])) <= {0, 2}  # every terminal ray was restarted


def test_ray_array_lists_agree(oracle_mod, rtmi_mod):
    """The per-ray arrays are positional arguments of both C entry points: the binding's list
    and the restatement's are the same names, types and widths in the same order."""
    assert tuple(rtmi_mod.dqn.NeuralQ.RAY_ARRAYS) == tuple(oracle_mod.NQ_RAYS)


def test_restatement_is_deterministic_and_frames_continue(oracle_mod, rtmi_mod):
    """The same inputs give the same bits; the second frame of greedy2 continues the sample
    sequence (it is not the first frame again)."""
    for case in ("mixed", "greedy2"):
        frames, eps, _ = _cpu_run(case)
        again, nq = _run_oracle(oracle_mod, rtmi_mod, case, *_fp64_net(oracle_mod, case))
        assert _first_difference(_flatten(again, nq.epsilon), _flatten(frames, eps)) is None
    f0, f1 = _cpu_run("greedy2")[0]
    assert not np.array_equal(f0["img"], f1["img"]) and not np.array_equal(f0["rays"]["loc"], f1["rays"]["loc"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_changes_the_restatement(oracle_mod, rtmi_mod, variant):
    """Each negative control is a different computation on the mixed case: some output array
    differs from the unmodified restatement's."""
    frames, eps, _ = _cpu_run("mixed")
    alt, alt_eps, _ = _cpu_run("mixed", variant)
    d = _first_difference(_flatten(alt, alt_eps), _flatten(frames, eps), (variant, "the algorithm"))
    print(f"{variant}: {d}")
    assert d is not None


# --- GPU ---------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _twin_callbacks(tr):
    """(q_fn, step_fn) on the twin trainer: its forward and its training step"""
    import torch

    def q_fn(loc):
        x = _dev(loc)
        q = torch.empty((loc.shape[0], 144), dtype=torch.float32, device="cuda")
        tr.forward_device(x.data_ptr(), loc.shape[0], q.data_ptr())
        return q.cpu().numpy()

    def step_fn(prev, act, tgt):
        x, a, t = _dev(prev), _dev(act), _dev(tgt)
        return tr.step_device(x.data_ptr(), a.data_ptr(), t.data_ptr(), prev.shape[0])[0]

    return q_fn, step_fn


def _trainer(rtmi_mod, ctx, case):
    c = CASES[case]
    return rtmi_mod.dqn.DqnTrainer(ctx, _scene(c["scene"])[2], *_weights(c["scene"], c.get("dead", False)))


def _device_run(rtmi_mod, ctx, case):
    """the case on the device: (_flatten'ed arrays with the trained parameters)"""
    c = CASES[case]
    g, cam_pos, _ = _scene(c["scene"])
    p = _params(rtmi_mod, case)
    frames = []
    with rtmi_mod.Scene(ctx, g) as sc, _trainer(rtmi_mod, ctx, case) as tr:
        if c.get("bvh"):
            sc.set_accel(rtmi_mod.ACCEL_BVH)
        with rtmi_mod.dqn.NeuralQ(ctx, sc, tr, batch_size=c["batch"], epsilon_start=c["eps"][0],
                                  epsilon_min=c["eps"][1], epsilon_decay=c["eps"][2]) as nq:
            with pytest.raises(rtmi_mod.RtError):
                nq.read_rays()  # refused before the first frame
            for _ in range(c["frames"]):
                img, stats, casts = nq.render_frame(rtmi_mod.camera(cam_pos), p)
                frames.append({"img": img, "stats": stats, "casts": casts, "rays": nq.read_rays()})
            eps = nq.epsilon
        return _flatten(frames, eps, tr.params())


_DEVICE = {}


def _device_cached(rtmi_mod, ctx, case):
    if case not in _DEVICE:
        _DEVICE[case] = _device_run(rtmi_mod, ctx, case)
    return _DEVICE[case]


def _lockstep(rtmi_mod, oracle_mod, ctx, case, variant="none"):
    """the restatement of the case in lockstep with a fresh twin trainer: (frames, flattened)"""
    with _trainer(rtmi_mod, ctx, case) as twin:
        frames, nq = _run_oracle(oracle_mod, rtmi_mod, case, *_twin_callbacks(twin), variant=variant)
        return frames, _flatten(frames, nq.epsilon, twin.params())


@pytest.mark.gpu
def test_forward_rows_do_not_depend_on_the_launch(rtmi_mod, gpu_ctx):
    """What the lockstep assumes: Q of a row is the same bits whether the row is launched with
    all n rows or in a slice, at an offset pointer (as the frame passes r.loc + 3 * b0) or in a
    buffer of its own; slices off a multiple of 64, a one-row slice, the tail.  The forward is
    read-only: the parameters are unchanged after it."""
    import torch
    n = 340
    loc = np.random.default_rng(7).uniform(-1, 1, (n, 3)).astype(np.float32)
    with _trainer(rtmi_mod, gpu_ctx, "mixed") as tr:
        W0, b0 = tr.params()
        x = _dev(loc)
        q_all = torch.empty((n, 144), dtype=torch.float32, device="cuda")
        tr.forward_device(x.data_ptr(), n, q_all.data_ptr())
        full = q_all.cpu().numpy()
        assert np.isfinite(full).all() and (full > 0).any()
        for lo, hi in ((0, 37), (37, 74), (74, 91), (65, 66), (3, 259), (257, 340), (339, 340)):
            m = hi - lo
            q = torch.empty((m, 144), dtype=torch.float32, device="cuda")
            tr.forward_device(x.data_ptr() + 12 * lo, m, q.data_ptr())
            assert np.array_equal(q.cpu().numpy().view(np.uint32), full[lo:hi].view(np.uint32)), (lo, hi, "offset")
            own = _dev(loc[lo:hi])
            tr.forward_device(own.data_ptr(), m, q.data_ptr())
            assert np.array_equal(q.cpu().numpy().view(np.uint32), full[lo:hi].view(np.uint32)), (lo, hi, "own")
        W1, b1 = tr.params()
        assert all(np.array_equal(a, c) for a, c in zip(W0 + b0, W1 + b1))
        # one step, then the forward sees the new parameters
        a, t = _dev(np.arange(n, dtype=np.int32) % 144), _dev(np.ones(n, np.float32))
        tr.step_device(x.data_ptr(), a.data_ptr(), t.data_ptr(), n)
        tr.forward_device(x.data_ptr(), n, q_all.data_ptr())
        assert not np.array_equal(q_all.cpu().numpy(), full)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_frame_is_the_restatement_bit_for_bit(rtmi_mod, oracle_mod, gpu_ctx, case):
    """The device frame(s) of the case against the restatement in lockstep with the twin
    trainer: image, stats rows, casts, epsilon, every per-ray array, all eight parameter arrays.
    The restatement's counters show the case reached its branches."""
    got = _device_cached(rtmi_mod, gpu_ctx, case)
    frames, want = _lockstep(rtmi_mod, oracle_mod, gpu_ctx, case)
    _check_coverage(case, frames)
    d = _first_difference(got, want)
    assert d is None, f"{case}: first difference at {d}"
    W0, b0 = _weights(CASES[case]["scene"], CASES[case].get("dead", False))
    trained = not all(np.array_equal(got[f"W{l}"], W0[l]) and np.array_equal(got[f"b{l}"], b0[l]) for l in range(4))
    assert trained != bool(CASES[case].get("dead"))  # (a dead network passes no gradient)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_negative_controls_differ_from_the_device(rtmi_mod, oracle_mod, gpu_ctx, variant):
    """A restatement that is wrong in one joint -- the targets' Philox event, the restart's y/z
    exchange, throughput on restarted rays, next-state Q before the batch's step, the update's
    state from prev_ray_locations (surface hits only; the reference's TRAIN_ON_POSITION build)
    instead of the position before the trace -- no longer equals the device on the mixed case:
    the comparison resolves each of them."""
    got = _device_cached(rtmi_mod, gpu_ctx, "mixed")
    _, want = _lockstep(rtmi_mod, oracle_mod, gpu_ctx, "mixed", variant)
    d = _first_difference(got, want)
    print(f"{variant}: {d}")
    assert d is not None, f"the {variant} control equals the device: the mixed case is too weak"
