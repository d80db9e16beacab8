"""bench.py's plain run and --dump-outputs: the plain line is the headline
only (everything else needs --full), the dump is float64 .npy within the
64 MB budget, and what the timed steps compute depends on the arguments
alone — not on how many steady-state warm-up steps the clock asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Ctx:
    def get_clock(self):
        return 0.125, 25


class _Prob:
    ctx = _Ctx()

    def __init__(self, shape):
        r = np.random.default_rng(7)
        self.sol = r.standard_normal(shape) + 1j * r.standard_normal(shape)


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_small_state_is_written_whole(tmp_path):
    p = _Prob((3, 16, 9))
    rec = bench.dump_outputs(str(tmp_path / "d"), p, 0, 1)
    a = np.load(tmp_path / "d" / "sol.npy")
    assert a.dtype == np.float64 and a.shape == (3, 16, 9, 2) and not rec["sampled"]
    assert np.array_equal(a[..., 0], p.sol.real) and np.array_equal(a[..., 1], p.sol.imag)
    assert np.array_equal(np.load(tmp_path / "d" / "clock.npy"), [0.125, 25.0])
    assert sorted(rec["files"]) == sorted(os.listdir(tmp_path / "d"))


def test_dump_large_state_is_a_fixed_sample_within_budget(tmp_path, monkeypatch):
    # the budget scaled down (the sampling code is the same): 3·32·17 entries
    # of 16 B = 26112 B against 16 kB
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 16000)
    p = _Prob((3, 32, 17))
    rec = bench.dump_outputs(str(tmp_path / "a"), p, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), p, 0, 1)
    a, b = np.load(tmp_path / "a" / "sol.npy"), np.load(tmp_path / "b" / "sol.npy")
    assert rec["sampled"] and a.dtype == np.float64 and a.shape == (rec["sol_entries_written"], 2)
    assert _dir_bytes(tmp_path / "a") <= 16000 and a.shape[0] >= (16000 - 4096) // 16
    assert np.array_equal(a, b)  # the same entries in every run
    flat = p.sol.reshape(-1)
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(flat.size, a.shape[0], replace=False))
    assert np.array_equal(a[:, 0], flat[idx].real) and np.array_equal(a[:, 1], flat[idx].imag)
    # every rank of an N-rank run gets its share of the budget and its own files
    rec2 = bench.dump_outputs(str(tmp_path / "c"), p, 1, 2)
    assert rec2["files"] == ["sol_rank1.npy", "clock_rank1.npy"] and _dir_bytes(tmp_path / "c") <= 8000


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "qg2",
                        "--stepper", "IFMAB3", "--grid", "256", "--steps", "6", "--warmup", "2", *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_outputs_repeat(tmp_path):
    from juliaraytracingsw_amd import drivers

    a = _bench("--min-warmup-s", "0", "--dump-outputs", str(tmp_path / "a"))
    b = _bench("--min-warmup-s", "0.02", "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["steps"] == 6 and line["warmup"] == 2 and line["full"] is False
        assert line["unit"] == "timesteps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
        # what --full measures is not on the plain line
        assert not {"kernels", "kernels_cold", "roofline", "cpu_baseline", "config4", "config5", "box",
                    "host_boundary"} & set(line)
    assert a["warmup_extra_steps"] == 0 and b["warmup_extra_steps"] > 0
    sa, sb = np.load(tmp_path / "a" / "sol.npy"), np.load(tmp_path / "b" / "sol.npy")
    assert sa.dtype == np.float64 and np.isfinite(sa).all() and np.abs(sa).max() > 0
    assert np.array_equal(sa, sb)
    assert np.array_equal(np.load(tmp_path / "a" / "clock.npy"), np.load(tmp_path / "b" / "clock.npy"))
    # … and equal to warmup + steps uninterrupted steps of the same seeded problem
    prob, _ = drivers.qg2_problem(256, "IFMAB3")
    prob.stepforward(8)
    sol, clock = prob.sol, prob.ctx.get_clock()
    prob.close()
    assert np.array_equal(sa[..., 0], sol.real) and np.array_equal(sa[..., 1], sol.imag)
    assert np.array_equal(np.load(tmp_path / "a" / "clock.npy"), np.array(clock, float))
