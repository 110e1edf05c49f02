"""bench.py's plain run and its --dump-outputs files: the result line's headline fields, the
outputs of the last timed step as float64 .npy files (capped at 64 MB by a fixed seeded row
sample), and -- on the GPU -- those files against a direct solve of the same seeded batch."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    import torch
    B = 300
    t = {"u_star": torch.arange(B * 40, dtype=torch.float64).reshape(B, 20, 2),
         "status": torch.arange(B, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "whole"), t)
    assert sorted(os.listdir(tmp_path / "whole")) == ["status.npy", "u_star.npy"]
    for k, v in t.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, v.numpy().astype(np.float64))
    # above the cap: the same sorted, seeded rows of every array, the same from call to call
    row = 40 * 8 + 8 + 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * row + 5)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), t)
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 100 and (np.diff(rows) > 0).all() and rows.max() < B
    total = 0
    for k in ("u_star", "status", "rows"):
        a, b = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 100 * row + 5
    assert np.array_equal(np.load(tmp_path / "s1" / "u_star.npy"), t["u_star"].numpy()[rows.astype(int)])
    assert np.array_equal(np.load(tmp_path / "s1" / "status.npy"), rows)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`: one JSON line with the headline
    fields and none of --full's legs; the dumped arrays equal a direct solve of the C2 batch."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "MPC solves/sec (batched, N=20)" and d["unit"] == "solves/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["solver"]["solved_frac"] == 1.0
    assert not {"roofline", "cpu_baseline", "c3", "c4", "c5", "cascaded", "latency"} & set(d)

    from vcmpc import Context
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    b = kinematic_batch(1024, N=20, seed=31)
    with Context(N=20, max_batch=1024, device=0, kin_car=load_config("kinematic_car"),
                 kin_mpc=load_config("kinematic_mpc")) as ctx:
        u0, xbar, ustar, status, iters = ctx.solve(b["x0"], b["kappa"], b["ds"], b["ubar"].copy())
    ref = {"u_star": ustar, "xbar": xbar, "u0": u0, "status": status, "iters": iters}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in ref)
    for k, v in ref.items():
        a = np.load(out / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == np.asarray(v).shape
        assert np.array_equal(a, np.asarray(v, dtype=np.float64)), k
