"""bench.py's entry points on the CPU (`--rehearsal`: no engine, a stand-in CPU step): the N > 1 paths the
driver uses -- a plain `python bench.py --gpus 2` that starts its own ranks as a child process, and the
same file launched under `torch.distributed.run` -- must rendezvous on 127.0.0.1 (gloo here), time between
barriers, reduce MAX over ranks and print exactly ONE JSON line from rank 0."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _json_lines(text):
    out = []
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            try:
                out.append(json.loads(line))
            except ValueError:
                pass
    return out


def _env():
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    return e


def test_plain_invocation_with_gpus_2_starts_its_own_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearsal", "--steps", "20", "--warmup", "5",
                        "--envs", "512"], capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    j = lines[0]
    assert j["n_gpus"] == 2 and j["steps"] == 20 and j["warmup"] == 5 and j["timed_steps"] == 20
    assert j["rehearsal"] is True and j["value"] is None and j["roofline"] is None
    assert j["scaling"] == "weak" and j["ms_per_step"] > 0


def test_driver_style_torchrun_launch():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2",
                        "--rehearsal", "--steps", "7", "--warmup", "2", "--envs", "64"],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2 and lines[0]["steps"] == 7


def test_a_failing_rank_fails_the_launcher():
    """A rank that dies AFTER the rendezvous (ACAS2D_BENCH_FAIL_RANK, a test hook inside the ranks) takes the job down:
    torchrun reports it, `python bench.py --gpus 2` hands the non-zero code back and prints no result line; the same
    command without the hook succeeds (test_plain_invocation_with_gpus_2_starts_its_own_ranks)."""
    env = dict(_env(), ACAS2D_BENCH_FAIL_RANK="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearsal", "--steps", "5", "--warmup", "1", "--envs", "64"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode != 0 and not _json_lines(r.stdout)
    # an argument the parent itself rejects never starts any rank
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearsal", "--dtype", "f16"],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert r.returncode == 2


def test_pick_chunk_and_repeats():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.pick_chunk(20, 200) == 20 and bench.pick_chunk(2000, 200) == 200
    assert bench.pick_chunk(1000, 200) == 200 and bench.pick_chunk(7, 200) == 7
    assert bench.pick_chunk(1009, 200) == 200            # a prime: whole replays + an eager remainder
    a = bench.parse(["--steps", "20"])
    assert a.steps == 20 and a.gpus == 1 and a.dump_outputs is None and not hasattr(a, "repeats")
    # --steps is the number of timed steps: graphs of an even multiple of the action rows that divides it, else the
    # largest even one and an eager rest (a prime K included)
    assert bench.pick_graph_steps(20, 20, 200) == 20 and bench.pick_graph_steps(2000, 25, 200) == 200
    assert bench.pick_graph_steps(7, 7, 200) == 7 and bench.pick_graph_steps(1009, 25, 200) == 200
    assert bench.pick_graph_steps(201, 1, 200) == 200 and bench.pick_graph_steps(600, 30, 200) == 150


def test_counter_traffic_names_the_kernel_sources_it_was_taken_on():
    """profiles/traffic.json carries a digest of the kernel sources its rocprofv3 counter passes ran on; bench.py
    recomputes it and says in the line whether the timed sources are the same (`kernel_sources_match`)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    rec = b.load_traffic(65536, 8, "f32", detail=True)
    assert rec is not None and len(rec["kernel_sources_sha256"]) == 64 and isinstance(rec["kernel_sources_match"], bool)
    assert len(b.kernel_sources_sha256()) == 64 and rec["build"] != "unlabelled"


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    """bench.dump_outputs: one float32 / float64 .npy per output, the infos zeroed where the env did not finish (the
    engine leaves them stale there), and above the limit the same seeded sample of env rows in every array."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    E, D = 1000, 29
    g = torch.Generator().manual_seed(0)
    done = torch.rand(E, generator=g) < 0.1
    outs = {"obs": torch.rand(E, D, generator=g), "reward": torch.rand(E, generator=g, dtype=torch.float64),
            "done": done, "outcome": torch.randint(1, 4, (E,), generator=g, dtype=torch.uint8),
            "terminal_observation": torch.rand(E, D, generator=g), "episode_return": torch.rand(E, generator=g),
            "episode_steps": torch.randint(1, 1000, (E,), generator=g, dtype=torch.int32), "absent": None}
    names = bench.dump_outputs(outs, str(tmp_path / "all"))
    assert names == sorted(n for n in outs if n != "absent")
    a = {n: np.load(tmp_path / "all" / (n + ".npy")) for n in names}
    assert a["obs"].dtype == np.float32 and a["reward"].dtype == np.float64 and a["done"].dtype == np.float32
    assert np.array_equal(a["obs"], outs["obs"].numpy()) and np.array_equal(a["done"], done.numpy().astype(np.float32))
    m = done.numpy()
    assert np.array_equal(a["episode_steps"][m], outs["episode_steps"].numpy()[m]) and not a["episode_steps"][~m].any()
    assert np.array_equal(a["terminal_observation"][m], outs["terminal_observation"].numpy()[m])
    assert not a["terminal_observation"][~m].any() and not a["outcome"][~m].any()
    limit = 100_000
    for d in ("s1", "s2"):
        bench.dump_outputs(outs, str(tmp_path / d), limit=limit)
    s1 = {f.name: np.load(f) for f in (tmp_path / "s1").iterdir()}
    s2 = {f.name: np.load(f) for f in (tmp_path / "s2").iterdir()}
    assert sorted(s1) == sorted(s2) and all(np.array_equal(s1[n], s2[n]) for n in s1)
    assert sum(v.nbytes for v in s1.values()) <= limit
    idx = s1["sample_index.npy"].astype(np.int64)
    assert 0 < len(idx) < E and np.all(np.diff(idx) > 0)
    assert np.array_equal(s1["obs.npy"], a["obs"][idx]) and np.array_equal(s1["done.npy"], a["done"][idx])


def test_dump_outputs_from_the_command_line(tmp_path):
    """`--dump-outputs DIR` through the whole command (--rehearsal: the stand-in step's output): exactly --steps timed
    steps, and the same arguments write the same arrays."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rehearsal", "--steps", "30", "--warmup", "4",
                            "--envs", "256", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        j = _json_lines(r.stdout)
        assert len(j) == 1 and j[0]["steps"] == 30 and j[0]["timed_steps"] == 30 and j[0]["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / d)) == ["acc.npy"]
        got.append(np.load(tmp_path / d / "acc.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (256,) and np.array_equal(got[0], got[1])


import pytest  # noqa: E402


@pytest.mark.gpu
def test_two_real_ranks_on_one_gpu():
    """The N > 1 path on hardware, as far as one GPU goes: `python bench.py --gpus 2` starts two ranks that both use
    GPU 0 (--device 0, gloo for the barrier / MAX: RCCL wants one device per rank), each steps its own shard of
    65 536 envs with its own global env offset, rank 0 prints the one line.  (The 8-GPU curve is the driver's.)"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--device", "0", "--steps", "100",
                        "--warmup", "20", "--no-rollout"], capture_output=True, text=True, timeout=900, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    j = lines[0]
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["envs_per_gpu"] == 65536
    # two ranks time-share one GPU: the whole-job rate is about the single-rank rate, never twice it
    assert 4e9 < j["value"] < 2.4e10 and j["config"]["episodes_finished"] > 1000
    assert "x2" in j["config"]["parallelism"] and j["roofline"]["frac"] > 0.15


@pytest.mark.gpu
def test_dump_outputs_are_the_same_on_every_run(tmp_path):
    """Two runs with the same arguments but different spin lengths (the replays before the timed region) write the same
    outputs bit for bit: the timed steps start from the state after the warm-up and the settling steps every time."""
    import numpy as np
    got = []
    for d, spin in (("a", "0.05"), ("b", "0.3")):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--envs", "4096", "--dtype", "f64", "--steps", "50",
                            "--warmup", "10", "--spin-seconds", spin, "--no-extra", "--no-rollout", "--no-cpu-baseline",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=900, env=_env(),
                           cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        j = _json_lines(r.stdout)
        assert len(j) == 1 and j[0]["timed_steps"] == 50 and j[0]["ms_per_step"] > 0
        got.append({n[:-4]: np.load(tmp_path / d / n) for n in os.listdir(tmp_path / d)})
    a, b = got
    assert sorted(a) == ["done", "episode_return", "episode_steps", "obs", "outcome", "reward", "terminal_observation"]
    assert a["obs"].shape == (4096, 29) and a["obs"].dtype == np.float64 and a["done"].dtype == np.float32
    assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a)
    assert set(np.unique(a["done"])) <= {0.0, 1.0} and a["done"].any()
    assert np.all((a["episode_steps"] > 0) == (a["done"] > 0))
