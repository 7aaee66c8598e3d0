"""bench.py helpers that need no GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pmc_traffic_picks_the_newest_profile_numerically(tmp_path, monkeypatch):
    """roofline.traffic comes from the committed PMC summaries; 'v12' must win over 'v9' (a plain string sort says otherwise)"""
    b = _bench()
    d = tmp_path / "profiles" / "r01"
    d.mkdir(parents=True)
    for tag, val in (("v9_split", 9.0), ("v12_final", 12.0), ("v3_linear", 3.0)):
        (d / ("pmc_c3_%s.json" % tag)).write_text(json.dumps({"kernels": {"sweep_tiled<2, 32, true, true>": {"hbm_bytes_per_launch": val}}}))
    d2 = tmp_path / "profiles" / "r02"
    d2.mkdir()
    (d2 / "pmc_c3_v1_first.json").write_text(json.dumps({"kernels": {"sweep_tiled<2, 32, true, true>": {"hbm_bytes_per_launch": 101.0}}}))
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    got = b.pmc_traffic("sweep_tiled", "c3")
    assert got["bytes"] == 101.0 and got["source"].endswith("pmc_c3_v1_first.json")   # a later round beats any version of an earlier one
    (d2 / "pmc_c3_v1_first.json").unlink()
    assert b.pmc_traffic("sweep_tiled", "c3")["bytes"] == 12.0
    assert b.pmc_traffic("sweep_tiled", "c9") is None


def test_committed_profiles_resolve():
    """every sweep kernel resolves to the newest committed summary that names it -- "newest" is read off the directory listing, not
    pinned to a round number (a literal here broke HEAD at the end of round 3)"""
    import glob
    import re
    b = _bench()

    def key(path):
        m = re.search(r"profiles[/\\]r(\d+)[/\\]pmc_[^_]+_v(\d+)", path)
        return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)
    for kernel in ("sweep_tiled", "sweep_fx_tiled", "sweep_fx_rect"):       # exact sampler, fixed sampler general / rectified
        got = b.pmc_traffic(kernel, "c3")
        assert got is not None and got["bytes"] > 1.0e9 and "pmc_c3_v" in got["source"], kernel
        naming = []
        for path in glob.glob(os.path.join(ROOT, "profiles", "*", "pmc_c3_*.json")):
            rec = json.load(open(path))
            if any(n.startswith(kernel) and "hbm_bytes_per_launch" in c for n, c in rec.get("kernels", {}).items()):
                naming.append(path)
        assert os.path.join(ROOT, got["source"]) == max(naming, key=key), kernel
        assert 0.3 < got["valu_utilisation"] < 1.05


def test_gpus_without_a_launcher_starts_the_launcher_as_a_child():
    """`python bench.py --gpus 2` without torch.distributed.run: one process drives one GPU, so bench.py starts the launcher itself --
    as a child process, before torch is imported or a GPU touched -- and relays its output and exit code (the first 8-GPU
    node must yield a curve, not a usage error).  Here there is no GPU: both ranks come up under the launcher, say so, and the launcher's
    non-zero exit code is what this process returns."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c1", "--steps", "1", "--warmup", "0"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert "--nproc-per-node 2" in out.stderr and "starting" in out.stderr            # the launcher was started by bench.py itself ...
    assert out.stderr.count("bench.py needs a GPU") >= 1 or "ProcessGroupNCCL" in out.stderr or "NCCL" in out.stderr   # ... its ranks ran bench.py (and found no GPU)
    assert out.returncode != 0                                                         # ... and its exit code came back
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_via_comm_refuses_a_launcher():
    """--via-comm is ONE process driving N GPUs through mvs_comm_*: under torch.distributed.run it must refuse before touching anything"""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--via-comm"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "ONE process" in out.stderr


def test_scene_views_are_synths_views_bit_for_bit():
    """bench.py renders the scene's views on host threads: the same arrays as synth.make_views, so the inputs do not depend on it"""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
    from mvs_amd import synth
    b = _bench()
    got = b.scene_views(200, 120, 5, 0.15, synth.SEED_SCENE + 1)
    want = synth.make_views(200, 120, 5, radius=0.15, seed=synth.SEED_SCENE + 1)
    for g, w in zip(got[:3] + (got[4],), want[:3] + (want[4],)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert len(got[3]) == 5 and all(np.array_equal(g, w) for g, w in zip(got[3], want[3]))


def test_dumped_outputs_are_float_within_budget_and_repeatable(tmp_path):
    """--dump-outputs: float32 / float64 files only, at most 64 MB in all, the same sample of a large output in every run"""
    import numpy as np
    import torch
    b = _bench()
    W, H, D = 3840, 2160, 64   # c4's frame: the per-pixel maps no longer fit whole
    rng = np.random.default_rng(1)
    maps = {"depth": rng.random((H, W), np.float32), "cost": rng.random((H, W), np.float32), "plane_index": rng.integers(0, D, (H, W)).astype(np.int32)}
    vol = torch.arange(D * 1000, dtype=torch.int32)
    for d in ("a", "b"):
        b.write_outputs(str(tmp_path / d), maps, vol)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["cost.npy", "depth.npy", "pixel_index.npy", "plane_index.npy", "volume_index.npy", "volume_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
    pix = np.load(tmp_path / "a" / "pixel_index.npy").astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "depth.npy"), maps["depth"].reshape(-1)[pix])
    cells = np.load(tmp_path / "a" / "volume_index.npy").astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "volume_sample.npy"), cells.astype(np.float64))
