"""The path bench.py TIMES, checked (VERDICT r03 item 1 / ADVICE r03 #2).

bench.py's timed loop is a two-slot, three-stream, three-context pipeline ordered by events (ProofWorkload.run); the at-size
parity tests run the same kernels serially on one stream.  Here the pipeline itself is the thing under test, at the c2 size
(2048-bit n, k = 17: 3033 + 84 columns, the headline's launch shapes):
  * ProofWorkload.verify_pipelined -- four pipelined steps over three messages of one circuit shape, every commitment and
    sampled coefficient / extended columns against a serial one-context recomputation -- passes, and its serial reference
    agrees with the oracle chain (bench.oracle_check: cells, commitment, coefficients, extended values of sampled columns);
  * with an event edge REMOVED (consumer not waiting for the witness; producer not waiting for the previous readers of its
    slot) the same check FAILS -- i.e. it would notice a missing edge in the timed loop;
  * host/prove_c2.cpp (the plain C++ caller over the C ABI, three contexts ordered by pz_ctx_wait) runs the same check on its
    own pipeline, prints per-message commitment hashes equal to the Python path's, and fails with an edge removed; a small
    job (256-bit key, k = 12) runs the same binary in seconds.
"""
import argparse
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _workload(enc_bits, k, seed=0x5043, pool=256):
    import torch

    import bench
    import paillier_halo2_amd as pz

    eng = pz.Engine(0)
    eng.bind_torch_stream()
    wl = bench.ProofWorkload(eng, torch, enc_bits, k, seed=seed, scale=1.0, pool=pool)
    return bench, eng, wl


@pytest.fixture(scope="module")
def c2():
    bench, eng, wl = _workload(2048, 17)
    wl.run(1)      # warm: tables, workspaces
    yield bench, eng, wl
    eng.close()


def test_messages_share_the_circuit_shape(c2):
    _, _, wl = c2
    (nn, g, m0, r0) = wl.variants[0]["ints"]
    assert len(wl.variants) == 3
    for var in wl.variants[1:]:
        n2, g2, m, r = var["ints"]
        assert (n2, g2) == (nn, g) and m != m0 and r != r0
        assert m.bit_length() == m0.bit_length() and bin(m).count("1") == bin(m0).count("1")   # paillier.rs:50-55: same steps, same columns
        assert not np.array_equal(var["circ_inputs"], wl.variants[0]["circ_inputs"])


def test_pipelined_step_equals_serial_and_oracle(c2, cref):
    bench, _, wl = c2
    v = wl.verify_pipelined()
    assert v["verified"] is True, v
    assert v["pipelined_steps_checked"] == 4 and v["messages"] == 3
    # the tester's row budget (layout.RowBudget): calculate_params(Some(20)) configures 3034 advice columns, the cells fill 3033 of them
    assert (wl.adv_cols, wl.lk_cols, wl.rows, wl.row_budget.minimum_rows) == (3034, 84, (1 << 17) - 9, 20)
    assert v["commitments_compared"] == 4 * (3034 + 84 + wl.counts["msm_full"]) and v["transforms_compared"] == 4 * 5 * 2
    assert len(set(v["commitment_hash_by_message"].values())) == 3     # three different witnesses went through the two slots
    # ... and they are the commitments every box and every caller has produced for this seed (tests/golden/c2_commitment_hashes.json)
    import json

    with open(os.path.join(ROOT, "tests", "golden", "c2_commitment_hashes.json")) as f:
        gold = json.load(f)
    assert gold["seed"] == "0x5043" and (gold["advice_cols"], gold["lookup_cols"], gold["minimum_rows"]) == (3034, 84, 20)
    assert v["commitment_hash_by_message"] == gold["commitment_hash_by_message"]
    vo = bench.oracle_check(wl, lambda s: None)
    assert vo["ok"] is True, vo


def _one_queue(torch, a, b):
    """True when work on stream b waits behind stream a's: the two share a hardware queue, which runs its work in order"""
    busy, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        torch.cuda._sleep(100_000_000)
        busy.record(a)
    with torch.cuda.stream(b):
        torch.cuda._sleep(1000)
        done.record(b)
    done.synchronize()
    shared = busy.query()
    busy.synchronize()
    return shared


def _place_streams(wl, edge):
    """A process opens few hardware queues (GPU_MAX_HW_QUEUES), so its streams share them, and a queue runs its work in order: a
    removed edge can only show where the stream that no longer waits is on another queue than the work it should wait for.
    ready / free: the witness stream is placed beside the commitment (main) stream and the transform stream.  ntt_ready: the
    transform stream beside both (its reads would otherwise queue behind the commitment stream's own wait for K4)."""
    import torch

    main = torch.cuda.current_stream()

    def pick(ok):
        for _ in range(16):
            s = torch.cuda.Stream()
            if s.cuda_stream != main.cuda_stream and ok(s):
                return s
        pytest.fail("no placement of this process's streams lets the removed edge %r show" % edge)

    if edge == "ntt_ready":
        sw = pick(lambda s: _one_queue(torch, main, s))
        sn = pick(lambda s: not _one_queue(torch, main, s) and not _one_queue(torch, sw, s))
    else:
        sw = pick(lambda s: not _one_queue(torch, main, s))
        sn = pick(lambda s: not _one_queue(torch, sw, s))
    wl.stream_w, wl.stream_n = sw, sn
    wl.engw.set_stream(sw.cuda_stream)
    wl.engn.set_stream(sn.cuda_stream)


@pytest.mark.parametrize("edge", ["ready", "free", "ntt_ready"])
def test_a_removed_event_edge_is_noticed(c2, edge):
    """ready: the commitment stream does not wait for K4; free: the witness stream overwrites a slot its readers still use;
    ntt_ready: the transform stream does not wait for K4.  Every kernel stays inside its buffers whatever it reads (the sort's
    position checks), so these runs are safe; what they must not be is `verified`."""
    _, _, wl = c2
    assert wl.stream_w is not None and wl.stream_n is not None
    _place_streams(wl, edge)
    wl.drop_edge = edge
    try:
        v = wl.verify_pipelined()
    finally:
        wl.drop_edge = ""
    assert v["verified"] is False, (edge, v)
    assert v["mismatches"] or v["async_error"]
    # and the pipeline is sound again afterwards
    v2 = wl.verify_pipelined()
    assert v2["verified"] is True, v2


def _args(steps, warmup, seed):
    return argparse.Namespace(steps=steps, warmup=warmup, seed=seed)


def test_prove_c2_at_size_verifies_and_matches_the_python_path(c2):
    bench, _, wl = c2
    mine = wl.verify_pipelined()
    assert mine["verified"] is True
    out = bench.dropin_device_resident(wl, _args(2, 1, 0x5043), lambda s: None)
    assert "error" not in out, out
    assert out["verified"] is True, out
    assert out["advice_cols"] == 3034 and out["lookup_cols"] == 84 and out["messages"] == 3
    theirs = out["commitment_hash_by_message"]
    assert set(theirs) == {"0", "1", "2"}
    for k_, h_ in theirs.items():
        assert mine["commitment_hash_by_message"][k_] == h_, (k_, mine["commitment_hash_by_message"], theirs)


@pytest.mark.parametrize("edge", ["ready", "free"])
def test_prove_c2_notices_a_removed_wait(c2, edge):
    bench, _, wl = c2
    out = bench.dropin_device_resident(wl, _args(1, 1, 0x5043), lambda s: None, env_extra={"PZ_PROVE_DROP_EDGE": edge})
    assert "error" not in out, out
    assert out["verified"] is False and out["mismatch"], out


def test_prove_c2_small_job():
    """the same binary on a job that takes seconds: 256-bit key, k = 12, 32-column pools"""
    bench, eng, wl = _workload(256, 12, seed=0x77, pool=32)
    try:
        wl.run(1)
        mine = wl.verify_pipelined()
        assert mine["verified"] is True, mine
        out = bench.dropin_device_resident(wl, _args(3, 1, 0x77), lambda s: None)
        assert "error" not in out, out
        assert out["verified"] is True and out["mul_mod_steps"] == wl.n_steps
        for k_, h_ in out["commitment_hash_by_message"].items():
            assert mine["commitment_hash_by_message"][k_] == h_
    finally:
        eng.close()
