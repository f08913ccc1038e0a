"""`python bench.py --gpus N` typed as it stands must start its own ranks: the parent makes no GPU
call, spawns torch.distributed.run as a child, forwards rank 0's JSON line and returns non-zero when a rank fails.
Rehearsed here on the CPU with the gloo backend and the stub workload (no library, no GPU)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True, timeout=300)


def test_self_launch_world2_gloo():
    p = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "stub", "--backend", "gloo"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout          # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["backend"] == "gloo"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0
    assert out["comparable"] is False


def test_self_launch_propagates_failure():
    # a rank that dies (unknown backend) must make the parent exit non-zero
    p = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "stub", "--backend", "no_such_backend"])
    assert p.returncode != 0


def test_parent_makes_no_gpu_call():
    """the launcher branch runs before torch / the library are imported: with both made un-importable in the PARENT only
    (a sitecustomize that poisons them unless RANK is set) the launch still succeeds"""
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "sitecustomize.py"), "w") as f:
            f.write("import os, sys\n"
                    "if 'RANK' not in os.environ and any(a.endswith('bench.py') for a in sys.argv[:1]):\n"
                    "    sys.modules['torch'] = None\n"
                    "    sys.modules['paillier_halo2_amd'] = None\n")
        pp = d + os.pathsep + os.environ.get("PYTHONPATH", "")
        p = _run(["--gpus", "2", "--steps", "2", "--warmup", "0", "--workload", "stub", "--backend", "gloo"], {"PYTHONPATH": pp})
        assert p.returncode == 0, p.stderr[-2000:]
        assert json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])["rccl_ranks"] == 2


def test_single_rank_without_launcher():
    p = _run(["--gpus", "1", "--steps", "2", "--warmup", "0", "--workload", "stub"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1


def test_force_dist_single_rank_creates_the_group():
    """--gpus 1 --force-dist: one rank, still through the launcher and a process group (what the GPU test runs with backend nccl)"""
    p = _run(["--gpus", "1", "--force-dist", "--steps", "2", "--warmup", "0", "--workload", "stub", "--backend", "gloo"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1 and out["backend"] == "gloo"


def test_steps_default_and_refusals():
    """--steps sets the timed steps (10 when it is not given); --dump-outputs is refused where there is no connected proof to write"""
    p = _run(["--gpus", "1", "--warmup", "0", "--workload", "stub"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])["steps"] == 10
    assert _run(["--gpus", "1", "--steps", "0", "--workload", "stub"]).returncode == 2
    for extra in (["--workload", "stub"], ["--workload", "msm22"], ["--hot-path-headline"]):
        p = _run(["--gpus", "1", "--steps", "1", "--dump-outputs", "unused"] + extra)
        assert p.returncode == 2 and "--dump-outputs" in p.stderr, (extra, p.stderr[-2000:])


def test_dump_proof_words_exact_and_capped(tmp_path):
    """the dumped arrays are the proof's Montgomery words, exactly (float64 of 32-bit halves); over the cap, a fixed sample of rows"""
    import numpy as np

    import bench

    rng = np.random.default_rng(7)
    words = lambda *shape: rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    pr = type("Proof", (), {})()
    pr.commitments = {"advice": words(40, 8), "h": words(3, 8)}
    pr.evals = {"advice": words(40, 4, 4), "random": words(1, 1, 4)}
    n = bench.dump_proof(str(tmp_path / "all"), pr)
    got = {f[:-4]: np.load(str(tmp_path / "all" / f)) for f in os.listdir(tmp_path / "all")}
    assert set(got) == {"commitments_advice", "commitments_h", "evals_advice", "evals_random"}
    assert n == sum(a.nbytes for a in got.values())
    for fam, d in (("commitments", pr.commitments), ("evals", pr.evals)):
        for k, v in d.items():
            a = got[fam + "_" + k]
            assert a.dtype == np.float64 and a.shape == v.shape[:-1] + (2 * v.shape[-1],)
            assert np.array_equal(a.astype(np.uint32).view(np.uint64), v)
    cap = n // 4
    m1 = bench.dump_proof(str(tmp_path / "s1"), pr, cap_bytes=cap)
    m2 = bench.dump_proof(str(tmp_path / "s2"), pr, cap_bytes=cap)
    assert m1 == m2 <= cap
    a1, a2 = np.load(str(tmp_path / "s1" / "evals_advice.npy")), np.load(str(tmp_path / "s2" / "evals_advice.npy"))
    assert 0 < a1.shape[0] < 40 and np.array_equal(a1, a2)
    rows = a1.astype(np.uint32).view(np.uint64)
    assert all(any(np.array_equal(r, v) for v in pr.evals["advice"]) for r in rows)
