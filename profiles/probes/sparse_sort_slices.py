"""probe: the digit sort of the proof's own advice columns (config c2: 2048-bit n, k = 17) under the density hint, per slice size.
PZ_MSM_SPARSE_SLICE (read once per process) sets the largest slice of a SPARSE launch: run once per value, e.g. 8192, 32768, 131072.
Prints the library's own event timers per launch of all advice columns: sort (hist .. scatter), accumulate, tree, whole MSM; AUTO
(no hint: the parent's launches) beside SPARSE in the same process, and checks that both give the same points.  For a counter run
(rocprofv3 --pmc FETCH_SIZE, then WRITE_SIZE; profiles/pmc_summary.py) take one mode per process: MODES=sparse REPS=1."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import paillier_halo2_amd as pz
import bench

eng = pz.Engine(0)
os.environ["PZ_BENCH_PIPELINE"] = "0"
wl = bench.ProofWorkload(eng, torch, 2048, 17, seed=0x5043, scale=1.0)
wl.produce(0)
torch.cuda.synchronize()
eng.timing_enable(True)
reps = int(os.environ.get("REPS", "5"))
nc, n = wl.adv_cols, wl.n
outs = {}
modes = os.environ.get("MODES", "auto,sparse,auto,sparse").split(",")   # MODES=sparse: one mode only (counter runs)
for name in modes:
    hint = {"auto": None, "sparse": pz.MSM_SPARSE}[name]
    fn = lambda: eng.msm_dev(wl.bases, wl.d_adv[0].data_ptr(), nc, n, 4 * n, wl.d_out_adv.data_ptr(), density=hint)
    fn(); eng.sync()
    outs[name] = wl.d_out_adv.cpu().numpy().copy()
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.sync()
    dt = (time.perf_counter() - t0) / reps
    sort, acc, tree, whole = (eng.timing_get(w)[0] / reps for w in (5, 0, 6, 4))
    print("slice=%s %-6s cols=%d  sort %.2f ms  accumulate %.2f ms  tree %.2f ms  msm %.2f ms  wall %.2f ms" % (
        os.environ.get("PZ_MSM_SPARSE_SLICE", "default"), name, nc, sort, acc, tree, whole, dt * 1e3), flush=True)
if len(outs) == 2:
    a, s = (eng.g1_normalize(outs[k].view(np.uint64)) for k in ("auto", "sparse"))
    print("same points:", bool(np.array_equal(a, s)), flush=True)
