"""CPU: `bench.py --gpus N` launches N workers itself (torch.distributed.run as a child, gloo for
the self-test) and refuses a world size that does not match --gpus."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _run(args, env=None, timeout=300):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True,
                          env=e, timeout=timeout, cwd=str(ROOT))


def test_self_launch_two_workers_cover_every_chunk_once():
    r = _run(["--gpus", "2", "--launcher-selftest"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["world"] == 2 and line["max_rank"] == 1.0
    ranks = sorted(line["ranks"])
    assert [p[0] for p in ranks] == [0, 1] and all(p[1] == 2 for p in ranks)
    # C3: the fixed 256-chunk table and C5: the 92 lineitem chunks, each split contiguously
    assert ranks[0][2] == 0 and ranks[0][3] == ranks[1][2] and ranks[1][3] == 256
    assert ranks[0][4] == 0 and ranks[0][5] == ranks[1][4] and ranks[1][5] == 92
    assert ranks[0][3] == 128  # equal chunks -> an even split


def test_extras_need_full():
    """A plain run measures the headline alone: options that add work are refused without --full."""
    for extra in (["--workloads", "c5"], ["--e2e"]):
        r = _run(["--gpus", "1"] + extra, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-500:]


def test_dump_outputs_is_exact_sampled_and_repeatable(tmp_path):
    """--dump-outputs' writer on host tensors: float32/float64 files that hold the values exactly,
    a buffer over its share of the budget as the same sorted sample every time."""
    import numpy as np
    import torch
    import bench
    import vortex_amd.arrays as A
    rng = np.random.default_rng(3)
    u64 = rng.integers(0, 2 ** 63, 1000, dtype=np.uint64)
    f64 = rng.standard_normal(3 * bench.DUMP_BUDGET // (8 * 6))  # 3x its share (6 buffers below)
    as_t = lambda a: torch.from_numpy(a.view(np.uint8).copy())
    res = [A.Canonical("primitive", u64.size, "u64", values=as_t(u64)),
           A.Canonical("primitive", f64.size, "f64", values=as_t(f64), validity=torch.full((8,), 255, dtype=torch.uint8)),
           A.Canonical("varbinview", 4, "u8", views=torch.arange(64, dtype=torch.uint8),
                       data=torch.arange(40, dtype=torch.uint8), data_buffers=[(0, 10), (16, 20)])]
    sizes = bench.dump_outputs(res, "T", tmp_path / "a")
    assert sorted(sizes) == ["T_0_values", "T_1_validity", "T_1_values", "T_2_data0", "T_2_data1", "T_2_views"]
    files = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in sizes}
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert sum((tmp_path / "a" / f"{k}.npy").stat().st_size for k in sizes) <= 64_000_000
    assert np.array_equal(files["T_0_values"].astype(np.uint32).view(np.uint64), u64)
    assert np.array_equal(files["T_2_data1"], np.arange(16, 36, dtype=np.float32))
    cap = bench.DUMP_BUDGET // (8 * 6)
    idx = np.sort(np.random.default_rng(7 + 1).integers(0, f64.size, cap))
    assert np.array_equal(files["T_1_values"], f64[idx])
    bench.dump_outputs(res, "T", tmp_path / "b")
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")) for k, v in files.items())


def test_world_mismatch_exits_nonzero():
    r = _run(["--gpus", "1", "--launcher-selftest"], env={"WORLD_SIZE": "2", "RANK": "0"}, timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=2" in r.stderr
