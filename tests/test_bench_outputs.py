"""bench.py's --dump-outputs and --full: the dump's budget and fixed sample (CPU), and on the
GPU one small plain run whose dumped frame is the frame rtmi.render returns, with nothing of
--full in its line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench as b  # noqa: E402  (imports torch and rtmi; no GPU call)

    return b


def test_dump_keeps_small_arrays_whole(bench, tmp_path):
    img = np.arange(5 * 7 * 3, dtype=np.float32).reshape(5, 7, 3)
    info = bench.dump_outputs(str(tmp_path / "d"), {"image": img, "ray_casts": np.array([2 ** 40 + 1], np.float64),
                                                    "visits": np.arange(4, dtype=np.uint32)})
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    casts = np.load(tmp_path / "d" / "ray_casts.npy")
    assert casts.dtype == np.float64 and casts[0] == 2 ** 40 + 1
    assert np.load(tmp_path / "d" / "visits.npy").dtype == np.float32
    assert info["image"] == {"shape": [5, 7, 3], "dtype": "float32"}


def test_dump_samples_a_large_array_the_same_way_every_time(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = np.random.default_rng(3).random((40, 50, 3)).astype(np.float32)  # 24 kB
    small = np.arange(16, dtype=np.float64)  # 128 B, taken whole first
    a = bench.dump_outputs(str(tmp_path / "a"), {"image": big, "ray_casts": small})
    b = bench.dump_outputs(str(tmp_path / "b"), {"ray_casts": small, "image": big})
    assert a == b and a["image"]["sampled"] == (4096 - 128) // 4
    ia, ib = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    assert np.array_equal(ia, ib) and ia.shape == (a["image"]["sampled"],)
    assert np.array_equal(np.load(tmp_path / "a" / "ray_casts.npy"), small)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096 + 2 * 128  # (the .npy headers)
    # the sample is elements of the array in flat order
    idx = np.sort(np.random.default_rng(1984).choice(big.size, size=ia.size, replace=False))
    assert np.array_equal(ia, big.reshape(-1)[idx])


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_and_leaves_the_rest_to_full(rtmi_mod, gpu_ctx, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--width", "64", "--height", "64", "--spp", "8", "--spp-split", "2", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "Mrays/s"
    for key in ("roofline", "parity", "cpu_baseline"):
        assert key not in line
    assert sorted(os.listdir(out)) == ["image.npy", "ray_casts.npy"]
    geom = rtmi_mod.cornell_geometry(rtmi_mod.RT_PRESET_CPU)
    p = rtmi_mod.default_params(rtmi_mod.RT_PRESET_CPU, width=64, height=64, spp=8, spp_split=2)
    with rtmi_mod.Scene(gpu_ctx, geom) as sc:
        ref, ref_casts = rtmi_mod.render(gpu_ctx, sc, rtmi_mod.camera(rtmi_mod.CAMERAS["cornell"]), p)
    img = np.load(out / "image.npy")
    assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.load(out / "ray_casts.npy")[0] == 3 * ref_casts == 3 * line["ray_casts_per_step"]
