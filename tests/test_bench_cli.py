"""bench.py's command line: a plain run measures only the headline figure, --dump-outputs writes
what the last timed step decoded, everything else waits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib as O

BENCH = os.path.join(O.ROOT, "bench.py")
FULL_ONLY = ("roofline", "stages_ms_per_step", "parity_timed_output", "call_shapes", "extra_workloads",
             "cpu_baseline", "cpu_oracle_1core", "host_input_images_per_s_per_gpu", "parse_images_per_s")


def test_bench_options():
    """--full and --dump-outputs exist beside the contract's --gpus / --steps / --warmup."""
    out = subprocess.run([sys.executable, BENCH, "--help"], check=True, capture_output=True, text=True).stdout
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs DIR"):
        assert opt in out


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """Three 1080p images, 2 timed steps: the line holds the headline fields and nothing that
    --full measures; the dump is float32, within 64 MB, and holds the CPU oracle's RGB bytes at the
    seeded positions of the destination arena (3 x 1080 x 5760 values are more than a dump holds,
    so this is the sampled form)."""
    env = dict(os.environ, RJ_BENCH_DATA=str(tmp_path / "data"))
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "3",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["runs"]["count"] == 1
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 3e3 / line["ms_per_step"]) <= 0.01 * line["value"]  # 3 images per step
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(dump)) == ["decoded.npy"]
    got = np.load(dump / "decoded.npy")
    assert got.dtype == np.float32 and got.shape == (bench_mod().DUMP_ELEMS,) and got.nbytes <= 64 << 20

    import rocjpeg_amd as R
    B = bench_mod()
    base = os.path.join(env["RJ_BENCH_DATA"], f"c2_v{B.GEN_VERSION}_p0_n3")
    idx = np.load(base + ".idx.npy")
    with open(base + ".bin", "rb") as f:
        raw = f.read()  # the run's dataset
    arena = []
    for o, s in zip(idx[0], idx[1]):
        st, want = O.oracle_decode(raw[int(o):int(o) + int(s)], int(R.OutputFormat.RGB), [(1080, 3 * 1920)])
        assert st == 0
        arena.append(want[0].reshape(-1))
    arena = np.concatenate(arena)
    pos = np.random.default_rng(B.SEED0).integers(0, arena.size, B.DUMP_ELEMS)
    assert np.array_equal(got, arena[pos].astype(np.float32))


def bench_mod():
    import bench
    return bench
