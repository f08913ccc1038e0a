"""GPU: pz_msm_g1_dev_ex's density hint (include/pz.h PZ_MSM_AUTO / PZ_MSM_SPARSE / PZ_MSM_DENSE; Engine.msm_dev(density=...)).

The hint chooses which scatter kernels a column batch queues and how large a sort slice is; it must never change a group
element.  Everything here compares affine-normalised commitments column by column, EXACTLY:
  * SPARSE and DENSE against AUTO (the device-side choice, what pz_msm_g1_dev does) on short, full-width, mixed, all-zero, all-one
    and small negative scalars and on a window sub-range -- both wrong-hint directions are among them;
  * the column-sized slices of a SPARSE batch: column lengths below, at and above one slice, in launches wide enough for the
    512-workgroup rule to leave the slices large (one slice per column: no k_msm_totals, cursors from the bucket offsets alone)
    and in a narrower one that cuts a column into two larger-than-8192 slices; no position check may fire;
  * one case against the C oracle's MSM;
  * create_proof with the prover's hints and with every choice left to the device: the same proof, byte for byte.
Bases are loaded with window_bits = 16, so the small lengths run the production c == 16 code."""
import numpy as np
import pytest

from oracle import pyref as P
from tests.test_gpu_connected_proof import world  # noqa: F401  (the k = 14 connected-proof fixture: the smallest shape those tests use)
from tests.util import canon_rand_scalars, ints_to_u64x4, witness_like_canon

pytestmark = pytest.mark.gpu

R = P.FR_R
N_MAX = 1 << 15
NC = 12           # more than 8 columns: the column-batch path


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


@pytest.fixture(scope="module")
def bases(eng):
    """2^15 walk bases P_i = (s + i t) G made on the device, their table at window_bits = 16; shorter columns use a prefix"""
    import torch

    s, t = (0x2B7 << 236) + 0x4321, 0xFEEDC0DE1234567
    ks = ints_to_u64x4([s + i * t for i in range(N_MAX)])
    d_k = torch.from_numpy(ks.view(np.int64)).cuda()
    eng.fr_convert_dev(d_k.data_ptr(), N_MAX, True)
    d_b = torch.zeros((N_MAX, 8), dtype=torch.int64, device="cuda")
    eng.g1_fixed_base_mul_dev(d_k.data_ptr(), N_MAX, d_b.data_ptr())
    eng.sync()
    tb = eng.load_bases_dev(d_b.data_ptr(), N_MAX, window_bits=16)
    assert (tb.window_bits, tb.n_windows) == (16, 16)
    yield tb, d_b
    tb.free()


def _short(n, seed):
    a = canon_rand_scalars(n, seed)
    a[:, 1:] = 0          # < 2^64
    return a


def _neg(n, seed):
    """r - k for small k (canonical): the sign folds into the point, the digits are those of k"""
    ks = np.random.default_rng(seed).integers(1, 1 << 20, size=n)
    return ints_to_u64x4([R - int(k) for k in ks])


def _const(n, v):
    return np.tile(ints_to_u64x4([v]), (n, 1))


def _batches(n):
    """name -> (NC, n, 4) canonical scalars"""
    short = [_short(n, 100 + j) for j in range(NC)]
    full = [canon_rand_scalars(n, 200 + j) for j in range(NC)]
    edge = [_const(n, 0), _const(n, 1), _neg(n, 300), witness_like_canon(n, 301)]
    return {
        "short": np.stack(short),
        "full": np.stack(full),
        "mixed": np.stack([short[j] if j % 2 else full[j] for j in range(NC)]),
        # an all-zero column, a column of ones (one bucket holds every entry), small negatives, the witness mix -- among short and full ones
        "edge": np.stack(edge + short[:4] + full[:4]),
    }


def _upload(eng, cols):
    import torch

    d_s = torch.from_numpy(np.ascontiguousarray(cols).view(np.int64)).cuda()
    eng.fr_convert_dev(d_s.data_ptr(), cols.shape[0] * cols.shape[1], True)
    return d_s


def _commit(eng, tb, d_s, nc, n, stride_rows, density, lo=0, hi=None):
    """-> (nc, 8) affine points; eng.sync() raises PZ_ERR_ASYNC if a position check fired"""
    import torch

    d_o = torch.zeros((nc, 12), dtype=torch.int64, device="cuda")
    eng.msm_dev(tb, d_s.data_ptr(), nc, n, 4 * stride_rows, d_o.data_ptr(), lo, hi, density=density)
    eng.sync()
    return eng.g1_normalize(d_o.cpu().numpy().view(np.uint64))


def _same_under_every_hint(eng, tb, cols, n, lo=0, hi=None, what=""):
    import paillier_halo2_amd as pz

    nc, rows = cols.shape[0], cols.shape[1]
    d_s = _upload(eng, cols)
    auto = _commit(eng, tb, d_s, nc, n, rows, None, lo, hi)
    assert np.array_equal(auto, _commit(eng, tb, d_s, nc, n, rows, pz.MSM_AUTO, lo, hi)), (what, "AUTO by name")
    for name, hint in (("SPARSE", pz.MSM_SPARSE), ("DENSE", pz.MSM_DENSE)):
        got = _commit(eng, tb, d_s, nc, n, rows, hint, lo, hi)
        for j in range(nc):
            assert np.array_equal(got[j], auto[j]), (what, name, "column", j)
    return auto


@pytest.mark.parametrize("n", [1 << 12, (1 << 15) - 37])
@pytest.mark.parametrize("kind", ["short", "full", "mixed", "edge"])
def test_hints_do_not_change_the_commitments(eng, bases, n, kind):
    """SPARSE and DENSE against AUTO, 12 columns: a right hint, a wrong hint in either direction, and the edge columns"""
    tb, _ = bases
    _same_under_every_hint(eng, tb, _batches(n)[kind], n, what=(kind, n))


@pytest.mark.parametrize("n", [1 << 12, (1 << 15) - 37])
def test_hints_with_a_window_range(eng, bases, n):
    """win_lo = 3, win_hi = 9: the digits of six windows only"""
    tb, _ = bases
    _same_under_every_hint(eng, tb, _batches(n)["mixed"], n, lo=3, hi=9, what=("windows 3..9", n))


# (columns, length): what msm_spt_sparse makes of them at the shipped slice limit (a whole column of 2^17 at most)
#   512 x 8192   one slice of 8192 per column          1024 x 8193   one slice of 16384, 8191 of it beyond the column
#   512 x 2^15   one slice of 2^15 per column          300 x 2^15    two slices of 16384 (512 workgroups wanted): k_msm_totals runs
@pytest.mark.parametrize("nc,n", [(512, 8192), (1024, 8193), (512, 1 << 15), (300, 1 << 15)])
def test_sparse_slices_below_at_and_above_one_slice(eng, bases, nc, n):
    """witness-like columns (every fourth one full-width: a wrong hint inside the batch) in launches wide enough for large slices"""
    import torch

    import paillier_halo2_amd as pz

    tb, _ = bases
    gen = torch.Generator(device="cuda")
    gen.manual_seed(nc * 31 + n)
    d_s = torch.randint(-(1 << 63), (1 << 63) - 1, (nc, n, 4), dtype=torch.int64, device="cuda", generator=gen)
    d_s[:, :, 3] &= 0x0FFFFFFFFFFFFFFF
    keep = torch.rand((nc, n), device="cuda", generator=gen)
    short = torch.ones(nc, dtype=torch.bool, device="cuda")
    short[3::4] = False
    d_s[short, :, 1:] = 0                                           # < 2^64 ...
    d_s[:, :, 0] = torch.where((keep < 0.6) & short[:, None], d_s[:, :, 0] & 0xFFFF, d_s[:, :, 0])    # ... most of them < 2^16
    d_s[:, :, 0] = torch.where((keep < 0.2) & short[:, None], torch.zeros_like(d_s[:, :, 0]), d_s[:, :, 0])   # and a fifth zero
    eng.fr_convert_dev(d_s.data_ptr(), nc * n, True)
    auto = _commit(eng, tb, d_s, nc, n, n, None)
    got = _commit(eng, tb, d_s, nc, n, n, pz.MSM_SPARSE)     # its eng.sync(): no position check fired
    bad = [j for j in range(nc) if not np.array_equal(got[j], auto[j])]
    assert not bad, (nc, n, bad[:8])
    eng.sync()


def test_hinted_batch_against_the_oracle(eng, bases, cref):
    """n = 2^10, 12 mixed columns: every hint against the C oracle's best_multiexp"""
    import paillier_halo2_amd as pz

    tb, d_b = bases
    n = 1 << 10
    cols = _batches(n)["mixed"]
    b_host = d_b[:n].cpu().numpy().view(np.uint64)
    want = np.stack([cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont([int.from_bytes(r.tobytes(), "little") for r in cols[j]]), b_host))
                     for j in range(NC)])
    d_s = _upload(eng, cols)
    for hint in (None, pz.MSM_SPARSE, pz.MSM_DENSE):
        got = _commit(eng, tb, d_s, NC, n, n, hint)
        for j in range(NC):
            assert np.array_equal(got[j], want[j]), (hint, "column", j)


def test_proof_with_hints_is_the_proof_without(eng, cref, world):  # noqa: F811
    """create_proof at k = 14 (34 advice + lookup columns), the same seed: the prover's hints against every choice left to the device"""
    from paillier_halo2_amd import prover

    hinted = prover.create_proof(world["pk"], world["witness"](), world["ch"], seed=41, tile=8)
    plain = prover.create_proof(world["pk"], world["witness"](), world["ch"], seed=41, tile=8, hooks={"density_hints": False})
    assert set(hinted.commitments) == set(plain.commitments) and set(hinted.evals) == set(plain.evals)
    for name in hinted.commitments:
        assert np.asarray(hinted.commitments[name]).tobytes() == np.asarray(plain.commitments[name]).tobytes(), name
    for name in hinted.evals:
        assert np.asarray(hinted.evals[name]).tobytes() == np.asarray(plain.evals[name]).tobytes(), name
    assert hinted.h_degree_ok and plain.h_degree_ok
