"""GPU: the witness expansion (K4, csrc/pz_witness.hip) held to Python integers on structured steps.
The catalogue and what it visits are in tests/witness_operands.py and pinned by tests/test_witness_operands.py; here the device
expands every step of it -- honest or not -- and every advice and lookup cell must equal oracle/pyref.py's, as canonical integers.
Then whole circuits (kinds 0, 1, 2) under structured keys, the plain column cut and the break-point layout at column heights that
put a boundary inside every kind of segment, and the lookup sort on the structured lookup streams.  One Engine, no subprocess."""
import numpy as np
import pytest

from oracle import pyref as P
from tests import witness_operands as WO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _zeros(*shape):
    import torch

    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def _same(got, want, what):
    if got != want:
        bad = [k for k in range(min(len(got), len(want))) if got[k] != want[k]]
        raise AssertionError("%s: %d of %d cells differ, first at %s (lengths %d, %d)" % (what, len(bad), len(want), bad[:1], len(got), len(want)))


# ------------------------------------------------------------------------------------------ the catalogue, step by step
HOST_FORM = {((4, 64, 15), "all_ones"), ((33, 64, 14), "alt"), ((65, 17, 8), "top2"), ((97, 64, 9), "all_ones")}    # one shape per PER
ADVICE_ONLY = ((8, 90, 32), "zero_mid")
LOOKUP_ONLY = ((32, 63, 9), "pow2_plus1")
CASES = [(s, m) for s in WO.SHAPES for m in WO.MODULI] + [(WO.WIDEST, "all_ones")]


@pytest.mark.parametrize("shape,name", CASES, ids=["%d-%d-%d-%s" % (s + (m,)) for s, m in CASES])
def test_witness_expand_on_the_catalogue(eng, cref, shape, name):
    """all steps of a shape under one modulus in one launch (one workgroup per step): every advice and every lookup cell equals the
    reference expansion's.  On chosen cases the same records go through the host-pointer form, and through the forms that write the
    advice or the lookup cells alone, which must give the same words."""
    L, W, lb = shape
    L64 = -(-L * W // 64)
    n = WO.modulus(name, L, W)
    steps = WO.steps(name, L, W, WO.step_cap(L))
    recs = np.stack([np.stack([cref.int_to_limbs(v, L64) for v in s[1:5]]) for s in steps])
    mod = cref.int_to_limbs(n, L64)
    adv_n, lk_n = eng.witness_cells_per_step(L, W, lb)
    d_steps, d_mod = _dev(recs), _dev(mod)
    d_adv, d_lk = _zeros(len(steps), adv_n, 4), _zeros(len(steps), lk_n, 4)
    eng.witness_expand_dev(L, W, lb, d_steps.data_ptr(), len(steps), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    adv, lk = _host(d_adv), _host(d_lk)
    for i, s in enumerate(steps):
        want_adv, want_lk = P.expand_mul_mod_cells(s.a, s.b, s.q, s.r, n, L, lb, W)
        _same(cref.fr_mont_to_ints(adv[i]), want_adv, "step %d (%s) advice" % (i, s.name))
        _same(cref.fr_mont_to_ints(lk[i]), want_lk, "step %d (%s) lookup" % (i, s.name))
    if (shape, name) in HOST_FORM:
        h_adv, h_lk = eng.witness_expand(L, W, lb, recs, mod)
        assert np.array_equal(h_adv, adv) and np.array_equal(h_lk, lk)
    if (shape, name) == ADVICE_ONLY:
        d_a2 = _zeros(len(steps), adv_n, 4)
        eng.witness_expand_dev(L, W, lb, d_steps.data_ptr(), len(steps), d_mod.data_ptr(), d_a2.data_ptr(), 0)
        eng.sync()
        assert np.array_equal(_host(d_a2), adv)
    if (shape, name) == LOOKUP_ONLY:
        d_l2 = _zeros(len(steps), lk_n, 4)
        eng.witness_expand_dev(L, W, lb, d_steps.data_ptr(), len(steps), d_mod.data_ptr(), 0, d_l2.data_ptr())
        eng.sync()
        assert np.array_equal(_host(d_l2), lk)


# ------------------------------------------------------------------------------------------ whole circuits under structured keys
CONFIGS = {"128/64": (128, 64, 15), "96/32": (96, 32, 9), "264/88": (264, 88, 15)}
KIND_ID = {"encrypt": 0, "add": 1, "uniform": 2}


def _inputs(cref, n, g, x, y, res, Ln, W):
    wn, wr = -(-Ln * W // 64), -(-2 * Ln * W // 64)
    return np.concatenate([cref.int_to_limbs(v, wn) for v in (n, g, x, y)] + [cref.int_to_limbs(res, wr)])


def _g(n, bits):
    return n + 1 if (n + 1) >> bits == 0 else n - 1


class Circuit:
    """one circuit's records (from the K3 entry points where the limbs are 64-bit words), the model's streams and the gate positions"""

    def __init__(self, eng, cref, kind, cfg, n, x, y):
        self.kind, self.n, self.x, self.y = kind, n, x, y
        self.bits, self.W, self.lb = bits, W, lb = CONFIGS[cfg]
        self.Ln, self.L = Ln, L = bits // W, 2 * (bits // W)
        self.g = g = _g(n, bits)
        wn, wr = -(-Ln * W // 64), -(-L * W // 64)
        self.wr = wr
        arr = lambda v: cref.int_to_limbs(v, wn)
        if kind == "add":
            self.res, fin = P.add_trace(n, x, y)
            steps_int, self.ng, self.nr = [fin], 0, 0
        elif kind == "encrypt":
            self.res, sg, sr, fin = P.encrypt_trace(n, g, x, y)
            steps_int, self.ng, self.nr = sg + sr + [fin], len(sg), len(sr)
        else:
            self.res, sg, sr, fin = P.encrypt_uniform_trace(n, g, x, y, bits)
            steps_int, self.ng, self.nr = sg + sr + [fin], len(sg), len(sr)
        want = np.stack([np.stack([cref.int_to_limbs(v, wr) for v in st]) for st in steps_int])
        if W == 64:       # the records the device's own big-integer kernels leave
            if kind == "add":
                q, rem = eng.mul_mod(wr, cref.int_to_limbs(x, wr), cref.int_to_limbs(y, wr), cref.int_to_limbs(n * n, wr))
                steps = np.stack([cref.int_to_limbs(x, wr), cref.int_to_limbs(y, wr), q.reshape(-1), rem.reshape(-1)]).reshape(1, 4, wr)
            elif kind == "encrypt":
                c, steps, ngd, nrd = eng.paillier_encrypt(Ln, arr(n), arr(g), arr(x), arr(y))
                assert (int(ngd[0]), int(nrd[0])) == (self.ng, self.nr) and cref.limbs_to_int(c[0]) == self.res
                steps = steps[0, : len(steps_int)]
            else:
                one = lambda v: arr(v).reshape(1, -1)
                c, steps, ngd, nrd = eng.paillier_encrypt_uniform(Ln, bits, one(n), one(g), one(x), one(y))
                assert cref.limbs_to_int(c[0]) == self.res
                steps = steps[0, : len(steps_int)]
            assert np.array_equal(np.ascontiguousarray(steps, dtype=np.uint64), want), "K3 records"
        self.d_steps = _dev(want)
        self.d_mod = _dev(cref.int_to_limbs(n * n, wr))
        self.adv_n, self.lk_n = eng.circuit_cells(KIND_ID[kind], Ln, W, lb, self.ng, self.nr)
        if kind == "uniform":
            self.want_adv, self.want_lk, self.seg = P.expand_uniform_circuit_cells(n, g, x, y, self.res, bits, W, lb)
            self.gates, end = P.gate_offsets_uniform_circuit(bits, W, lb, self.nr)
        else:
            self.want_adv, self.want_lk, self.seg = P.expand_circuit_cells(kind, n, g, x, y, self.res, bits, W, lb)
            self.gates, end = P.gate_offsets_circuit(kind, bits, W, lb, self.ng, self.nr)
        assert (len(self.want_adv), len(self.want_lk)) == (self.adv_n, self.lk_n) == (end, self.lk_n) and self.seg["satisfied"]

    def want_with(self, res):
        """the model's streams with another `res`: only assign_integer(res) and assert_equal_fresh read it"""
        a0, l0 = self.seg["assign_res"]
        ta, tl = P.expand_assign_cells(res, self.L, self.W, self.lb)
        ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(self.res, self.L, self.W), P.decompose_biguint(res, self.L, self.W))
        adv = self.want_adv[:a0] + [v % P.FR_R for v in ta + ae]
        assert len(adv) == self.adv_n and bit == int(res == self.res)
        return adv, self.want_lk[:l0] + [v % P.FR_R for v in tl]

    def expand(self, eng, cref, res, rows=0, stride=0, d_adv=None, d_lk=None):
        d_adv = _zeros(self.adv_n, 4) if d_adv is None else d_adv
        d_lk = _zeros(self.lk_n, 4) if d_lk is None else d_lk
        eng.circuit_expand_dev(KIND_ID[self.kind], self.Ln, self.W, self.lb, _inputs(cref, self.n, self.g, self.x, self.y, res, self.Ln, self.W),
                               self.d_steps.data_ptr(), self.ng, self.nr, self.d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr(), rows, stride)
        eng.sync()
        return d_adv, d_lk

    def check(self, eng, cref):
        top = 1 << (self.L * self.W - 1)
        for res in (self.res, self.res ^ 1, self.res ^ top):
            d_adv, d_lk = self.expand(eng, cref, res)
            got_adv, got_lk = cref.fr_mont_to_ints(_host(d_adv)), cref.fr_mont_to_ints(_host(d_lk))
            want_adv, want_lk = self.want_with(res)
            _same(got_adv, want_adv, "advice")
            _same(got_lk, want_lk, "lookup")
            assert P.check_gates(got_adv, self.gates) == [] and max(got_lk) < 1 << self.lb
            assert got_adv[-1] == int(res == self.res)


def _operand_pairs(n, bits, width):
    """(x, y) over {0, 1, all ones of `width` bits, n - 1}: each value once in either place"""
    ones = (1 << width) - 1
    return [(0, 1), (1, n - 1), (ones, 0), (n - 1, ones)]


# which of the four operand pairs a case runs: an encryption one per case, an addition (one step) all four, the uniform-shape circuit
# (2 bits + |r^n| + 1 steps whatever the message is) two per key size, so that every one of the four goes through it under every key kind
CIRCUIT_CASES = [(kind, cfg, key, pair) for kind, cfgs in (("encrypt", ("128/64", "96/32")), ("add", ("128/64", "96/32", "264/88")),
                                                           ("uniform", ("128/64", "96/32")))
                 for cfg in cfgs for key in WO.circuit_keys(CONFIGS[cfg][0])
                 for pair in {"encrypt": (0, 1, 2, 3), "add": ("all",), "uniform": (0, 1) if cfg == "128/64" else (2, 3)}[kind]]


@pytest.mark.parametrize("kind,cfg,key,pair", CIRCUIT_CASES, ids=["%s-%s-%s-%s" % c for c in CIRCUIT_CASES])
def test_whole_circuits_under_structured_keys(eng, cref, kind, cfg, key, pair):
    """kinds 0, 1 and 2 under all-ones, 2^(bits-1) + 1, alternating and Mersenne-product keys, operands from {0, 1, all ones, n - 1}:
    every cell of the device's stream equals the model's, with the right `res` and with one wrong in its lowest and in its highest
    limb; the gate identity holds on every enabled window and the last cell says whether the circuit is satisfied.  The square of n
    and the refresh chain see limbs of all ones here; refresh spills by two limbs and by none in every one of these shapes."""
    bits, W, lb = CONFIGS[cfg]
    n = WO.circuit_keys(bits)[key]
    assert n & 1 and n >> bits == 0
    inc = P.refresh_aux(W, bits // W, bits // W)
    assert 2 in inc and 0 in inc and len(inc) == 2 * (bits // W)
    pairs = _operand_pairs(n, bits, bits if kind == "add" else 16)
    for x, y in pairs if pair == "all" else pairs[pair: pair + 1]:
        Circuit(eng, cref, kind, cfg, n, x, y).check(eng, cref)


def test_plain_column_cut(eng, cref):
    """the dense stream cut into columns of `rows` cells stored `stride` apart, at heights 8 and 9 (a boundary every few cells) and
    1000: every cell at its place, the rows above the usable ones and the columns' unused ends untouched"""
    bits = 264
    c = Circuit(eng, cref, "add", "264/88", WO.circuit_keys(bits)["mersenne"], (1 << bits) - 1, WO.circuit_keys(bits)["mersenne"] - 1)
    wants = (cref.fr_ints_to_mont(c.want_adv), cref.fr_ints_to_mont(c.want_lk))
    for rows, stride in ((8, 16), (9, 9), (1000, 1024)):
        bufs = [_zeros(-(-len(w) // rows) * stride, 4) for w in wants]
        c.expand(eng, cref, c.res, rows, stride, bufs[0], bufs[1])
        for d_buf, want in zip(bufs, wants):
            nc = -(-len(want) // rows)
            exp = np.zeros((nc * rows, 4), dtype=np.uint64)
            exp[: len(want)] = want
            got = _host(d_buf).reshape(nc, stride, 4)
            assert not got[:, rows:].any(), "rows above the usable ones stay zero"
            assert np.array_equal(got[:, :rows].reshape(-1, 4), exp), (rows, stride)


# ------------------------------------------------------------------------------------------ break-point columns
def _where(c, idx):
    """the kind of segment the stream cell `idx` of circuit `c` lies in (inside a mul_mod block only)"""
    from paillier_halo2_amd import layout

    sc = layout.mul_mod_cells(c.L, c.W, c.lb)
    rc_adv, _ = layout.range_check_cells(c.W, c.lb)
    cb_adv, _ = layout.range_check_cells(WO.carry_bits(c.L, c.W), c.lb)
    # one iteration of is_equal_muled as oracle/pyref.py::expand_mul_mod_cells lays it out (and gate_offsets_mul_mod enables it): a sub
    # gate (4 cells), a sum of three (7), div_mod, an add gate (4), div_mod, is_equal, an and gate (4), then the carry's range check;
    # div_mod ends with an is_equal of its own.  The last iteration has an is_equal and an and gate in the range check's place.
    n_eq, n_dm = len(P._is_equal_cells(0, 0)[0]), len(P._div_mod_cells(0, c.W)[0])
    dm1, dm2 = 4 + 7, 4 + 7 + n_dm + 4
    iteration = dm2 + n_dm + n_eq + 4
    is_eq = ((dm1 + n_dm - n_eq, dm1 + n_dm), (dm2 + n_dm - n_eq, dm2 + n_dm), (dm2 + n_dm, dm2 + n_dm + n_eq))
    assert sc.seg["lt"] - sc.seg["eq"] == 2 + (2 * c.L - 1) * iteration + (2 * c.L - 2) * cb_adv + n_eq + 4
    blocks = [(c.seg[nm][0] + 2, cnt) for nm, cnt in (("pow_g", c.ng), ("pow_r", c.nr))] if c.kind == "encrypt" else []
    blocks.append((c.seg["final"][0], 1))
    for base, cnt in blocks:
        if base <= idx < base + cnt * sc.advice:
            rel = (idx - base) % sc.advice
            if rel < sc.seg["mul_ab"]:
                return "range_check" if rel % (c.L + c.L * rc_adv) >= c.L else "assign"
            if rel < sc.seg["add_r"]:
                return "convolution"
            if rel < sc.seg["eq"]:
                return "add_r"
            if rel < sc.seg["lt"]:
                p = (rel - sc.seg["eq"] - 2) % (iteration + cb_adv) if rel >= sc.seg["eq"] + 2 else -1
                last = rel >= sc.seg["lt"] - (n_eq + 4)
                if last or any(lo <= p < hi for lo, hi in is_eq):
                    return "is_equal"
                return "range_check" if p >= iteration else "eq_other"
            return "r<n"
    return "outside"


@pytest.mark.parametrize("kind,cfg,key", [("add", "264/88", "mersenne"), ("encrypt", "128/64", "pow2_plus1")])
def test_break_point_columns(eng, cref, kind, cfg, key):
    """the advice stream in halo2-lib's break-point layout at column heights 8 .. 11 and 64: the starts are the restatement's; every
    column holds its cells from row 0 on and ends with the cell the next one begins with (the shared cell is stored twice);
    everything else stays zero.  The small heights put a boundary inside a convolution row, an is_equal block, a range-check body
    and the r < n segment."""
    import paillier_halo2_amd as pz
    from oracle import circuit as CQ
    from paillier_halo2_amd import layout

    bits, W, lb = CONFIGS[cfg]
    n = WO.circuit_keys(bits)[key]
    c = Circuit(eng, cref, kind, cfg, n, 1 if kind == "encrypt" else (1 << bits) - 1, n - 1)
    mask, n_cells = P.gate_mask_circuit(kind, bits, W, lb, c.ng, c.nr)
    assert n_cells == c.adv_n
    want = cref.fr_ints_to_mont(c.want_adv)
    want_lk = cref.fr_ints_to_mont(c.want_lk)
    seen, skipped = set(), 0
    for max_rows in (8, 9, 10, 11, 64):
        mine = WO.break_points(mask.tolist(), max_rows)
        if mine is None:
            skipped += 1
            with pytest.raises(pz.PzError) as e:
                layout.break_points(mask, max_rows)
            assert e.value.status == pz._lib.PZ_ERR_UNSUPPORTED
            continue
        starts = layout.break_points(mask, max_rows)
        assert starts.tolist() == CQ.break_points(mask, max_rows) == mine
        # the lookup stream keeps the plain cut, lr rows per column, under the same stride
        ncols, stride = len(starts) - 1, max_rows + 3
        lr = stride - 1
        nlc = -(-c.lk_n // lr)
        d_cols, d_lk, d_starts = _zeros(ncols * stride, 4), _zeros(nlc * stride, 4), _dev(starts)
        eng.circuit_expand_cols_dev(KIND_ID[kind], c.Ln, W, lb, _inputs(cref, n, c.g, c.x, c.y, c.res, c.Ln, W), c.d_steps.data_ptr(), c.ng, c.nr,
                                    c.d_mod.data_ptr(), d_cols.data_ptr(), d_lk.data_ptr(), d_starts.data_ptr(), ncols, max_rows, lr, stride)
        eng.sync()
        got = _host(d_cols).reshape(-1, stride, 4)
        exp = np.zeros_like(got)
        st = starts.astype(np.int64)
        for j in range(ncols):
            hi = min(int(st[j + 1]) + 1, n_cells)
            assert hi - st[j] <= max_rows
            exp[j, : hi - st[j]] = want[st[j]: hi]
        assert np.array_equal(got, exp), max_rows
        got_lk = _host(d_lk).reshape(nlc, stride, 4)
        exp_lk = np.zeros((nlc * lr, 4), dtype=np.uint64)
        exp_lk[: c.lk_n] = want_lk
        assert np.array_equal(got_lk[:, :lr].reshape(-1, 4), exp_lk) and not got_lk[:, lr:].any()
        seen |= {_where(c, int(s)) for s in st[1:-1]}
    assert skipped <= 1
    assert {"convolution", "is_equal", "range_check", "r<n"} <= seen, seen


# ------------------------------------------------------------------------------------------ the lookup sort on these streams
def _permute(eng, cref, cols, rows, lb):
    table = [i if i < (1 << lb) else 0 for i in range(rows)]
    d_in = _dev(np.stack([cref.fr_ints_to_mont(col) for col in cols]))
    d_tab = _dev(cref.fr_ints_to_mont(table))
    d_pi, d_pt = _zeros(len(cols), rows, 4), _zeros(len(cols), rows, 4)
    eng.lookup_permute_dev(d_in.data_ptr(), len(cols), 4 * rows, d_tab.data_ptr(), rows, lb, d_pi.data_ptr(), d_pt.data_ptr(), 4 * rows)
    eng.sync()
    for j, col in enumerate(cols):
        Ap, Sp = P.permute_expression_pair(col, table)
        _same(cref.fr_mont_to_ints(_host(d_pi[j])), Ap, "A' of column %d" % j)
        _same(cref.fr_mont_to_ints(_host(d_pt[j])), Sp, "S' of column %d" % j)


@pytest.mark.parametrize("shape", [(2, 16, 4), (32, 63, 9)], ids=lambda s: "lb%d" % s[2])
def test_lookup_permute_on_structured_streams(eng, cref, shape):
    """the counting sort behind the lookup argument at M = 16 (one value per thread of the scan) and M = 512 (two): a catalogue step's
    lookup stream, and columns made by hand -- all zero, all M - 1, every value once, values only at the first or only at the last
    entry of a thread's slice of the scan -- at rows = M, M + 1 and 1000"""
    L, W, lb = shape
    M = 1 << lb
    n = WO.modulus("all_ones", L, W)
    stream = []
    for s in WO.steps("all_ones", L, W, 12):
        stream += P.expand_mul_mod_cells(s.a, s.b, s.q, s.r, n, L, lb, W)[1]
    assert max(stream) == M - 1 and min(stream) == 0
    for rows in (M, M + 1, 1000):
        pad = lambda col: (list(col) + [0] * rows)[:rows]
        per = -(-M // 256)
        cols = [pad(stream), pad(stream[::-1]), [0] * rows, [M - 1] * rows, pad(range(M)), pad(range(M - 1, -1, -1)),
                pad([v - v % per for v in stream]), pad([v - v % per + per - 1 for v in stream]), pad([0, M - 1] * (rows // 2))]
        _permute(eng, cref, cols, rows, lb)
