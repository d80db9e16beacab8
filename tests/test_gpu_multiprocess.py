"""One process per slab on the GPU box: torch.distributed.run starts `world`
ranks, each with its own libsw context holding one slab, exchanging through
the host-staged transport (gloo).  The gathered results must equal the
undecomposed run bitwise, the device-recorded energy diagnostics and the CFL
reduction included."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("case,world,steps,freq,aliased", [("rsw_fab3", 2, 6, 2, False), ("qg2_ifmrk4", 2, 6, 2, False),
                                                           ("rsw_ifmab3", 4, 6, 2, False),
                                                           # more records than one host-staged gather holds
                                                           # before the chunked, incremental gather
                                                           ("rsw_fab3", 2, 240, 1, False),
                                                           # aliased_state on one slab per process: the aliased
                                                           # columns' x-spectra all-gathered per calcN, the
                                                           # full-array state/calcN/energies gathered
                                                           ("qg2_ifmrk4", 2, 6, 2, True), ("qg2_ifmab3", 4, 6, 2, True),
                                                           ("rsw_fab3", 2, 6, 2, True),
                                                           # MultiLayerQG (aliased_fraction = 0: the Nyquist
                                                           # column on slab 0, the Nyquist row of each slab)
                                                           ("mlqg_frk4", 2, 6, 2, True), ("mlqg_frk4", 2, 6, 2, False)])
def test_one_process_per_slab(case, world, steps, freq, aliased, tmp_path):
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
           os.path.join(HERE, "mp_slab_worker.py"), "--case", case, "--out", str(out),
           "--steps", str(steps), "--freq", str(freq)] + (["--aliased"] if aliased else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["world"] == world
    assert res["state_equal"] and res["calcN_equal"] and res["physical_equal"], res
    assert res["ke_rel"] == 0 and res["pe_rel"] == 0, res
    assert res["records_equal"] and res["cfl_equal"], res
    assert (res["aliased_max"] > 0) == aliased, res
    # the link probe of sw_create ran on the host-staged transport (round 6,
    # VERDICT r05 #4b): α ≥ 0, β > 0, the message size of this decomposition;
    # the host-staged transport keeps the sequential schedule
    lk = res["link"]
    assert lk["probed"] and lk["transport"] == "host-staged", lk
    assert lk["GBps_per_peer_direction"] > 0 and lk["latency_us"] >= 0 and lk["msg_bytes"] > 0, lk
    assert not lk["pipelined"] and lk["row_chunks"] == 1 and lk["peer_GBps"] == [0.0] * 8, lk


def test_bench_line_explains_the_exchange():
    """The N-rank bench line rehearsed on one GPU (SW_BENCH_BACKEND=gloo: two
    ranks, the host-staged transport): `comm` carries the transport, the RCCL
    rank count, the schedule and every rank's exposed transpose time and
    bytes per step (the driver's 8-GPU node runs it over RCCL)."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, SW_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--grid", "256",
           "--steps", "20", "--warmup", "5", "--min-warmup-s", "0", "--profile-steps", "3", "--no-cpu-baseline", "--no-config5",
           "--no-config4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "slab2" and line["scaling"] == "strong"
    c = line["comm"]
    assert c["transport"] == "host-staged" and c["rccl_ranks"] == 0 and c["nranks"] == 2
    assert c["schedule"] == "sequential" and c["row_chunks"] == 1
    assert [p["rank"] for p in c["per_rank"]] == [0, 1]
    assert c["link"]["probed"] and c["link"]["transport"] == "host-staged" and c["link"]["GBps_per_peer_direction"] > 0
    assert c["link"]["msg_bytes"] == 48 * 128 * 16  # kcl · nyl · 16 B per (peer, field)
    for p in c["per_rank"]:
        # RSW 256²: 9 mixed fields of kcl·nyl·16 B per step, half of each
        # slab's blocks go to the other rank
        assert p["sent_MB_per_step"] == pytest.approx(9 * 48 * 128 * 16 / 1e6, rel=1e-12)  # kcl = 48, nyl = 128
        assert 0 < p["exposed_transpose_us_per_step"] < p["step_us"]
