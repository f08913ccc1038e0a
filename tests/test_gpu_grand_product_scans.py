"""GPU: pz_permutation_product_sets_dev built from a prefix scan of the numerators, a suffix scan of the denominators and one inversion
per set (pz_quotient.hip, the k_gp_* kernels), against Python integers written here:

    ratio_i = num_i * den_i^-1   with 0^-1 = 0        num_i = prod_c (v_c[i] + beta delta^c w^i + gamma)
    z_j[0]  = z_{j-1}[u],  z_0[0] = 1                 den_i = prod_c (v_c[i] + beta sigma_c[i] + gamma)
    z_j[i+1] = z_j[i] * ratio_i

All n rows of every set are compared.  The shapes are the smallest at which each mechanism can go wrong: a few threads of one workgroup
(k = 5, 8), several workgroups per column (k = 13: the block totals' scans, the suffix direction across blocks, the partial products at
row u), zero denominators and a zero numerator, the product carried across workspace batches (PZ_PERM_SET_BATCH), strides beyond 4n."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests.test_gpu_next_rows import _dev, _ints, _m, eng  # noqa: F401  (module-scoped engine)

pytestmark = pytest.mark.gpu

R = P.FR_R
DELTA = pow(P.FR_GENERATOR, 1 << P.FR_S, R)
RUN = 16          # a multiple of every run length a thread of the scan kernels may own (8 or 16 rows)
BLOCK = 256 * 16  # ... and of every workgroup's share of a column


def _ratios(val, sig, chunk, k, beta, gamma):
    """per set: the n ratios num_i / den_i (zero where den_i = 0)"""
    n, m, w = 1 << k, len(val), P.fr_omega(k)
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * w % R
    out = []
    for c0 in range(0, m, chunk):
        num, den = [1] * n, [1] * n
        for c in range(c0, min(c0 + chunk, m)):
            bd, v, s = beta * pow(DELTA, c, R) % R, val[c], sig[c]
            for i in range(n):
                num[i] = num[i] * ((v[i] + bd * wp[i] + gamma) % R) % R
                den[i] = den[i] * ((v[i] + beta * s[i] + gamma) % R) % R
        out.append([a * (pow(d, -1, R) if d else 0) % R for a, d in zip(num, den)])
    return out


def _chained(ratios, u):
    sets, z0 = [], 1
    for rt in ratios:
        z = [z0]
        for r in rt[:-1]:
            z.append(z[-1] * r % R)
        sets.append(z)
        z0 = z[u]
    return sets


def _gpu(eng, cref, val, sig, chunk, k, u, beta, gamma, pad=(0, 0, 0)):
    """the library's sets, as lists of ints; pad = extra rows of the column, sigma and z strides (checked to stay untouched in z)"""
    import torch

    n, m = 1 << k, len(val)
    nsets = -(-m // chunk)

    def padded(rows, extra):
        t = _dev(cref, rows)
        if not extra:
            return t
        p = torch.full((m, n + extra, 4), -1, dtype=torch.int64, device="cuda")
        p[:, :n] = t
        return p

    d_val, d_sig = padded(val, pad[0]), padded(sig, pad[1])
    d_z = torch.full((nsets, n + pad[2], 4), 0x5a5a5a5a, dtype=torch.int64, device="cuda")
    eng.permutation_product_sets_dev(d_val.data_ptr(), 4 * (n + pad[0]), d_sig.data_ptr(), 4 * (n + pad[1]), m, chunk, k, u,
                                     _m(cref, P.fr_omega(k)), _m(cref, beta), _m(cref, gamma), _m(cref, DELTA), d_z.data_ptr(),
                                     4 * (n + pad[2]))
    eng.sync()
    assert bool((d_z[:, n:] == 0x5a5a5a5a).all()), "rows between the sets were written"
    return [_ints(cref, d_z[j, :n]) for j in range(nsets)]


def _world(k, m, seed):
    rng = random.Random(seed)
    n = 1 << k
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    val = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    sig = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    return val, sig, beta, gamma


def _check(eng, cref, val, sig, chunk, k, u, beta, gamma, **kw):
    want = _chained(_ratios(val, sig, chunk, k, beta, gamma), u)
    got = _gpu(eng, cref, val, sig, chunk, k, u, beta, gamma, **kw)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, "set %d, first differing row %d" % (j, next(i for i in range(len(w)) if g[i] != w[i]))
    return want


@pytest.mark.parametrize("chunk", [1, 2, 3])
@pytest.mark.parametrize("m", [1, 2, 3, 7])
@pytest.mark.parametrize("k", [5, 8])
def test_one_block(eng, cref, k, m, chunk):
    """one workgroup, a few threads: the short last set (m = 7 by 2 or 3, 3 by 2) and the single-set call (m <= chunk: no chaining)"""
    val, sig, beta, gamma = _world(k, m, 0x6770 + 64 * k + 8 * m + chunk)
    _check(eng, cref, val, sig, chunk, k, (1 << k) - 6, beta, gamma)


@pytest.fixture(scope="module")
def big():
    """k = 13, five columns in sets of two: every column spans several workgroups.  The ratios are computed once and left unchanged."""
    k, m = 13, 5
    val, sig, beta, gamma = _world(k, m, 0x6771)
    return dict(k=k, val=val, sig=sig, beta=beta, gamma=gamma, ratios=_ratios(val, sig, 2, k, beta, gamma))


@pytest.mark.parametrize("u", [19 * RUN - 1, 19 * RUN, BLOCK, (1 << 13) - 7], ids=["run_end", "run_start", "block_start", "n-7"])
def test_several_blocks(eng, cref, big, u):
    """row u at the last row of a thread's run, at the first row of the next run, at the first row of a workgroup's share, at n - 7"""
    assert BLOCK < (1 << big["k"])
    want = _chained(big["ratios"], u)
    got = _gpu(eng, cref, big["val"], big["sig"], 2, big["k"], u, big["beta"], big["gamma"])
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, "set %d, first differing row %d" % (j, next(i for i in range(len(w)) if g[i] != w[i]))


def _zero_den(val, sig, beta, gamma, c, i):
    val[c][i] = -(beta * sig[c][i] + gamma) % R


@pytest.mark.parametrize("where", ["row0", "run_boundary", "run_end", "row_u", "last_set"])
def test_zero_denominator(eng, cref, where):
    """a = -(beta sigma + gamma) makes den = 0: the ratio of that row is 0 (the inverse of zero is zero), the set is 0 from the next row on,
    and -- when that row lies before u -- every later set starts from 0 and is 0 throughout"""
    k, m, chunk = 8, 5, 2
    n, u = 1 << k, (1 << k) - 6
    val, sig, beta, gamma = _world(k, m, 0x6772)
    c, i = {"row0": (1, 0), "run_boundary": (0, 4 * RUN), "run_end": (2, 4 * RUN - 1), "row_u": (0, u), "last_set": (4, 5 * RUN + 3)}[where]
    _zero_den(val, sig, beta, gamma, c, i)
    want = _check(eng, cref, val, sig, chunk, k, u, beta, gamma)
    j = c // chunk
    assert all(x != 0 for x in want[j][:i + 1]) and all(x == 0 for x in want[j][i + 1:])
    for later in want[j + 1:]:
        assert all(x == 0 for x in later) if i < u else all(x != 0 for x in later)


def test_zero_denominator_across_blocks(eng, cref, big):
    """the same at k = 13, the zero at the last row of the first workgroup's share of the middle set, u beyond it"""
    k, u = big["k"], (1 << big["k"]) - 7
    val = [list(v) for v in big["val"]]
    _zero_den(val, big["sig"], big["beta"], big["gamma"], 3, BLOCK - 1)
    want = _check(eng, cref, val, big["sig"], 2, k, u, big["beta"], big["gamma"])
    assert want[1][BLOCK - 1] != 0 and not any(want[1][BLOCK:]) and not any(want[2])


def test_zero_numerator(eng, cref):
    """a = -(beta delta^c w^i + gamma) makes num = 0 with den != 0: a true zero product, not the inverse's convention"""
    k, m, chunk = 8, 5, 2
    n, u = 1 << k, (1 << k) - 6
    val, sig, beta, gamma = _world(k, m, 0x6773)
    c, i = 2, 3 * RUN + 5
    val[c][i] = -(beta * pow(DELTA, c, R) * pow(P.fr_omega(k), i, R) + gamma) % R
    want = _check(eng, cref, val, sig, chunk, k, u, beta, gamma)
    assert want[1][i] != 0 and not any(want[1][i + 1:]) and not any(want[2]) and all(want[0])


def test_chain_across_workspace_batches(eng, cref, monkeypatch):
    """PZ_PERM_SET_BATCH = 2 splits five sets into three workspace batches: the running product is carried from batch to batch, and
    the result is the uncapped call's"""
    k, m, chunk = 8, 9, 2
    u = (1 << k) - 6
    val, sig, beta, gamma = _world(k, m, 0x6774)
    monkeypatch.delenv("PZ_PERM_SET_BATCH", raising=False)
    whole = _check(eng, cref, val, sig, chunk, k, u, beta, gamma)
    monkeypatch.setenv("PZ_PERM_SET_BATCH", "2")
    assert _gpu(eng, cref, val, sig, chunk, k, u, beta, gamma) == whole
    monkeypatch.setenv("PZ_PERM_SET_BATCH", "1")
    assert _gpu(eng, cref, val, sig, chunk, k, u, beta, gamma) == whole


def test_strides_beyond_4n(eng, cref):
    """col_stride, sigma_stride and z_stride larger than 4n, each its own: the rows between the sets of z stay as they were"""
    k, m, chunk = 8, 5, 2
    val, sig, beta, gamma = _world(k, m, 0x6775)
    _check(eng, cref, val, sig, chunk, k, (1 << k) - 6, beta, gamma, pad=(5, 2, 3))
