// pz_witness.hip -- K4: expansion of a mul_mod step trace into the advice / lookup cell stream
// (Fr Montgomery, 32 B per cell) that halo2-lib's Context holds after BigUintChip::mul_mod emitted
// its constraints.  Replaces the per-cell CPU pushes behind the dependency call sites
// /root/reference/src/paillier.rs:39-57 and src/bench.rs:44-74.
//
// Layout = paillier_halo2_amd/layout.py::mul_mod_cells (segments: assign q/n/r with range-check
// digit splits | limb convolution a*b | limb convolution q*n | qn + r | carry chain of
// is_equal_muled | r < n); the value semantics are restated in oracle/pyref.py::expand_mul_mod_cells.
//
// Step records are 64-bit words; limbs of any width 16..90 bits are cut out of them into LDS.
// One workgroup (4 waves) per step.  The two convolutions are 76 % of the cells: a wave owns a
// product limb (row), lanes own the terms, partial sums come from a 192-bit wave prefix scan, every
// lane writes a contiguous 96/192-byte run -> fully coalesced streaming stores.  Operand limbs are
// converted to Montgomery form once per step into LDS.  The short serial carry / borrow chains run
// on one lane between two barriers.  Bound: HBM write bandwidth, 32 B per cell.
#include <array>
#include <vector>

#include "fp.cuh"
#include "pz_internal.h"

struct U192 {
    u64 w[3];
};
__device__ __forceinline__ U192 u_make(u64 a, u64 b = 0, u64 c = 0) {
    U192 r;
    r.w[0] = a; r.w[1] = b; r.w[2] = c;
    return r;
}
__device__ __forceinline__ U192 u_add(const U192& a, const U192& b) {
    U192 r;
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u64 t = a.w[i] + b.w[i];
        u64 c1 = t < a.w[i];
        u64 t2 = t + c;
        c = c1 | (t2 < t);
        r.w[i] = t2;
    }
    return r;
}
__device__ __forceinline__ U192 u_sub(const U192& a, const U192& b, bool& borrow) {
    U192 r;
    u64 br = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u64 t = a.w[i] - b.w[i];
        u64 b1 = a.w[i] < b.w[i];
        u64 t2 = t - br;
        br = b1 | (t < br);
        r.w[i] = t2;
    }
    borrow = br != 0;
    return r;
}
__device__ __forceinline__ bool u_eq(const U192& a, const U192& b) {
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2];
}
__device__ __forceinline__ U192 u_shr(const U192& a, unsigned s) {  // s < 192
    U192 r = a;
    while (s >= 64) {
        r.w[0] = r.w[1]; r.w[1] = r.w[2]; r.w[2] = 0;
        s -= 64;
    }
    if (s) {
        r.w[0] = (r.w[0] >> s) | (r.w[1] << (64 - s));
        r.w[1] = (r.w[1] >> s) | (r.w[2] << (64 - s));
        r.w[2] >>= s;
    }
    return r;
}
__device__ __forceinline__ U192 u_shl(const U192& a, unsigned s) {  // s < 192
    U192 r = a;
    while (s >= 64) {
        r.w[2] = r.w[1]; r.w[1] = r.w[0]; r.w[0] = 0;
        s -= 64;
    }
    if (s) {
        r.w[2] = (r.w[2] << s) | (r.w[1] >> (64 - s));
        r.w[1] = (r.w[1] << s) | (r.w[0] >> (64 - s));
        r.w[0] <<= s;
    }
    return r;
}
__device__ __forceinline__ U192 u_lowbits(const U192& a, unsigned bits) {  // a mod 2^bits, bits <= 192
    U192 r = a;
    if (bits < 64) { r.w[0] &= (1ull << bits) - 1; r.w[1] = 0; r.w[2] = 0; }
    else if (bits < 128) { if (bits > 64) r.w[1] &= (1ull << (bits - 64)) - 1; else r.w[1] = 0; r.w[2] = 0; }
    else if (bits < 192) { if (bits > 128) r.w[2] &= (1ull << (bits - 128)) - 1; else r.w[2] = 0; }
    return r;
}
struct S192 {
    U192 m;
    bool neg;
};
__device__ __forceinline__ S192 s_sub(const U192& a, const U192& b) {  // a - b
    S192 r;
    bool br;
    r.m = u_sub(a, b, br);
    r.neg = br;
    if (br) {
        bool d;
        r.m = u_sub(b, a, d);
    }
    return r;
}
__device__ __forceinline__ S192 s_addu(const S192& a, const U192& b) {  // a + b, b >= 0
    if (!a.neg) {
        S192 r;
        r.m = u_add(a.m, b);
        r.neg = false;
        return r;
    }
    return s_sub(b, a.m);
}
__device__ __forceinline__ Fr fr_from_u(const U192& v) {
    Fr x;
    x.v[0] = (u32)v.w[0]; x.v[1] = (u32)(v.w[0] >> 32);
    x.v[2] = (u32)v.w[1]; x.v[3] = (u32)(v.w[1] >> 32);
    x.v[4] = (u32)v.w[2]; x.v[5] = (u32)(v.w[2] >> 32);
    x.v[6] = 0; x.v[7] = 0;
    if ((v.w[0] | v.w[1] | v.w[2]) == 0) return x;
    return fp_to_mont(x);
}
__device__ __forceinline__ Fr fr_from_s(const S192& v) {
    Fr x = fr_from_u(v.m);
    return v.neg ? fp_neg(x) : x;
}
__device__ __forceinline__ void mul64w(u64 a, u64 b, u64& hi, u64& lo) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p00 = (u64)a0 * b0;
    const u64 t = (u64)a0 * b1 + (p00 >> 32);
    const u64 u = (u64)a1 * b0 + (u32)t;
    lo = (u << 32) | (u32)p00;
    hi = (u64)a1 * b1 + (t >> 32) + (u >> 32);
}

// product of two limbs of at most 96 bits (x = x0 + x1 2^64, x1 < 2^32): < 2^192.  `wide` is kernel-uniform
// (limb_bits > 64); the 64-bit-limb configuration pays one 64x64 product as before.
__device__ __forceinline__ U192 u_mul_limb(const U192& x, const U192& y, bool wide) {
    u64 hi, lo;
    mul64w(x.w[0], y.w[0], hi, lo);
    U192 r = u_make(lo, hi, 0);
    if (wide) {
        u64 h1, l1, h2, l2;
        mul64w(x.w[0], y.w[1], h1, l1);
        mul64w(x.w[1], y.w[0], h2, l2);
        r = u_add(r, u_make(0, l1, h1));
        r = u_add(r, u_make(0, l2, h2));
        r = u_add(r, u_make(0, 0, x.w[1] * y.w[1]));
    }
    return r;
}
// limb i (W bits) of the little-endian 64-bit-word integer `words[0..nw)`
__device__ __forceinline__ void limb_extract(const u64* __restrict__ words, unsigned nw, unsigned i, unsigned W, u64 out[2]) {
    const unsigned o = i * W, wi = o >> 6, sh = o & 63;
    const u64 w0 = wi < nw ? words[wi] : 0, w1 = wi + 1 < nw ? words[wi + 1] : 0, w2 = wi + 2 < nw ? words[wi + 2] : 0;
    U192 v = u_lowbits(u_shr(u_make(w0, w1, w2), sh), W);
    out[0] = v.w[0];
    out[1] = v.w[1];
}

// Where a cell of the stream lives: the stream is cut into the circuit's columns of `rows` usable rows, and a column
// may be stored with a larger stride (2^k: room for the blinding rows) -- cell c sits at c + (c / rows) * pad.
// rows == 0: the stream is dense.
// starts != nullptr: halo2-lib's BREAK-POINT layout of the advice stream (assign_with_constraints of the dependency, SURVEY tag [D]):
// column j holds the cells starts[j] .. starts[j + 1] from row 0 on -- the cell a column ends with is ALSO row 0 of the next one
// (a gate must not straddle two columns: the column breaks where a 4-cell gate would, and the shared cell carries the value
// across, tied by a copy constraint).  starts[0] = 0, starts[n_cols] = the stream's length; a column takes at most rows + 1 cells
// (rows = max_rows - 1 new ones), so c / rows never overshoots the column and the search walks forward from there.  pad = the
// column stride in this mode.
struct CellPtr {
    Fr* base;
    size_t idx, rows, pad;
    const u64* starts;
    unsigned ncols;
    __device__ __forceinline__ CellPtr operator+(size_t o) const {
        CellPtr r = *this;
        r.idx += o;
        return r;
    }
    __device__ __forceinline__ explicit operator bool() const { return base != nullptr; }
    __device__ __forceinline__ size_t plain_col() const {
        // one division per cell: 32-bit whenever the stream has fewer than 2^32 cells (a 64-bit division is ~100 instructions)
        return ((idx | rows) >> 32) == 0 ? (size_t)((u32)idx / (u32)rows) : idx / rows;
    }
    __device__ __forceinline__ Fr* addr() const {   // (dense / plain cut only)
        if (!rows) return base + idx;
        return base + idx + plain_col() * pad;
    }
};
__device__ __forceinline__ void fp_store(const CellPtr& p, const Fr& v) {
    if (!p.starts) {
        fp_store(p.addr(), v);
        return;
    }
    size_t col = p.plain_col();
    if (col >= p.ncols) col = p.ncols - 1;
    while (col + 1 < p.ncols && p.starts[col + 1] <= p.idx) ++col;
    const size_t row = p.idx - p.starts[col];
    if (row < p.pad) fp_store(p.base + col * p.pad + row, v);            // (row < stride always for a table built by pz_circuit_break_points)
    if (row == 0 && col > 0) {                                         // the previous column's last cell is this one too
        const size_t prow = p.idx - p.starts[col - 1];
        if (prow < p.pad) fp_store(p.base + (col - 1) * p.pad + prow, v);
    }
}

struct ExpP {
    unsigned L, D, lb;
    unsigned W, L64;                          // circuit limb width; 64-bit words per big integer of a step record
    unsigned k64, rem64, rc64_adv, rc64_lk;   // range_check(limb, W)   (names from the 64-bit-limb first version)
    unsigned cb, kcb, remcb, rccb_adv, rccb_lk;  // range_check(carry, cb)
    size_t off_assign, off_ab, off_qn, off_add, off_eq, off_lt, cells;
    size_t lk_assign, lk_eq, lk_lt, lookups;
    u64 max_w[3];  // L*(2^W-1)^2 + (2^W-1)
    size_t cell0, lk0;        // stream index of this launch's first advice / lookup cell
    size_t rows, pad;         // column cut of the stream (CellPtr); 0, 0 = dense
    const u64* bp_starts;     // != nullptr: the advice stream in break-point layout (CellPtr::starts); the lookup stream keeps the plain cut
    size_t bp_div, bp_stride; // max_rows - 1, column stride
    unsigned bp_ncols;
    size_t pair_stride, odd_off;   // != 0: steps come in pairs (uniform-shape circuit): step s sits at
                                   // cell0 + (s / 2) * pair_stride + (s & 1) * odd_off instead of cell0 + s * cells
    size_t chain_steps, chain_stride;   // != 0 (with pair_stride): the pairs come in chains of chain_steps steps, chain_stride cells apart
                                        // (weighted tally): step s is step s % chain_steps of the chain at cell0 + (s / chain_steps) * chain_stride
    size_t chain_recs, rec0;            // chain_recs != 0 (with chain_steps; ballot): a chain's records lie chain_recs apart in `steps` and this
                                        // launch expands those from rec0 on: step s reads (and numbers its lookups by) record
                                        // (s / chain_steps) * chain_recs + rec0 + s % chain_steps instead of record s
};

__device__ __forceinline__ CellPtr adv_ptr(const ExpP& P, Fr* advice, size_t idx) {
    if (P.bp_starts) return CellPtr{advice, idx, P.bp_div, P.bp_stride, P.bp_starts, P.bp_ncols};
    return CellPtr{advice, idx, P.rows, P.pad, nullptr, 0};
}

// A cell's value as an integer: +-m, or the field inverse of that.  The helpers below pick the VALUE of a cell (cheap integer
// selects, even when the lanes of a wave sit at different positions of a pattern) and the caller converts it to Montgomery
// form ONCE (cv_to_fr): with the conversion inside every switch arm a wave paid one Montgomery product per arm.
struct CV {
    U192 m;
    bool neg, inv;
};
__device__ __forceinline__ CV cv_u(const U192& m) { return CV{m, false, false}; }
__device__ __forceinline__ CV cv_s(const S192& v) { return CV{v.m, v.neg, false}; }
__device__ __forceinline__ CV cv_inv(const S192& v) { return CV{v.m, v.neg, true}; }
__device__ __forceinline__ CV cv_one() { return CV{u_make(1), false, false}; }
__device__ __forceinline__ CV cv_zero() { return CV{u_make(0), false, false}; }
__device__ __forceinline__ Fr cv_to_fr(const CV& c) {
    Fr x = fr_from_u(c.m);
    if (c.neg) x = fp_neg(x);
    if (c.inv) x = fp_inv(x);   // is_zero's inverse cell of a non-zero difference: rare
    return x;
}


// position p of RangeChip::range_check(x, bits): advice pattern
__device__ __forceinline__ CV rc_adv_cell(const U192& x, unsigned bits, unsigned lb, unsigned p) {
    const unsigned k = (bits + lb - 1) / lb, rem = bits % lb;
    const unsigned body = k > 1 ? 1 + 3 * (k - 1) : 0;
    if (p < body) {
        if (p == 0) return cv_u(u_lowbits(x, lb));
        const unsigned g = (p - 1) / 3 + 1, w = (p - 1) % 3;
        if (w == 0) return cv_u(u_lowbits(u_shr(x, lb * g), lb));
        if (w == 1) return cv_u(u_shl(u_make(1), lb * g));
        return cv_u(u_lowbits(x, lb * (g + 1)));
    }
    const unsigned t = p - body;  // tail gate
    const U192 last = u_lowbits(u_shr(x, lb * (k - 1)), lb);
    if (t == 0) return cv_zero();
    if (rem == 1) return cv_u(last);
    if (t == 1) return cv_u(last);
    if (t == 2) return cv_u(u_make(1ull << (lb - rem)));
    return cv_u(u_shl(last, lb - rem));
}
__device__ __forceinline__ CV rc_lk_cell(const U192& x, unsigned bits, unsigned lb, unsigned p) {
    const unsigned k = (bits + lb - 1) / lb, rem = bits % lb;
    if (p < k) return cv_u(u_lowbits(u_shr(x, lb * p), lb));
    return cv_u(u_shl(u_lowbits(u_shr(x, lb * (k - 1)), lb), lb - rem));
}

// 8-cell is_zero pattern on the (signed) difference d, then positions 0..11 of is_equal(x, y)
__device__ __forceinline__ CV is_equal_cell(const U192& x, const U192& y, unsigned p) {
    S192 d = s_sub(x, y);
    const bool z = !d.neg && (d.m.w[0] | d.m.w[1] | d.m.w[2]) == 0;
    switch (p) {
        case 0: return cv_s(d);
        case 1: return cv_u(y);
        case 2: return cv_one();
        case 3: return cv_u(x);
        case 4: return z ? cv_one() : cv_zero();
        case 5: return cv_s(d);
        case 6: return z ? cv_one() : cv_inv(d);
        case 7: return cv_one();
        case 8: return cv_zero();
        case 9: return cv_s(d);
        case 10: return z ? cv_one() : cv_zero();
        default: return cv_zero();
    }
}
// 22 cells of div_mod_unsafe(v, 2^W)
__device__ __forceinline__ CV div_mod_cell(const U192& v, unsigned p, unsigned W) {
    const U192 qd = u_shr(v, W);
    const U192 rd = u_lowbits(v, W);
    const U192 prod = u_shl(qd, W);
    switch (p) {
        case 0: return cv_u(qd);
        case 1: return cv_u(rd);
        case 2: return cv_zero();
        case 3: return cv_u(qd);
        case 4: return cv_u(u_shl(u_make(1), W));
        case 5: return cv_u(prod);
        case 6: return cv_u(rd);  // v - prod
        case 7: return cv_u(prod);
        case 8: return cv_one();
        case 9: return cv_u(v);
        default: return is_equal_cell(rd, rd, p - 10);
    }
}

#define EXP_THREADS 256
#define EXP_MAXL 128

__global__ __launch_bounds__(EXP_THREADS) void k_witness_expand(ExpP P, const u64* __restrict__ steps,
                                                                const u64* __restrict__ modulus,
                                                                Fr* __restrict__ advice, Fr* __restrict__ lookup) {
    __shared__ u64 s_a[EXP_MAXL][2], s_b[EXP_MAXL][2], s_q[EXP_MAXL][2], s_r[EXP_MAXL][2], s_n[EXP_MAXL][2];
    __shared__ Fr s_am[EXP_MAXL], s_bm[EXP_MAXL], s_qm[EXP_MAXL], s_nm[EXP_MAXL];
    __shared__ u64 s_pab[2 * EXP_MAXL][3], s_pqn[2 * EXP_MAXL][3];
    __shared__ u64 s_carry[2 * EXP_MAXL + 1][2], s_accx[2 * EXP_MAXL + 1][2];
    __shared__ unsigned char s_eqbit[2 * EXP_MAXL + 2], s_borrow[EXP_MAXL + 1];
    const unsigned L = P.L, D = P.D, lb = P.lb, W = P.W;
    const bool wide = W > 64;
    const size_t step = blockIdx.x;
    const size_t cstep = P.chain_steps ? step % P.chain_steps : step;
    const size_t recno = P.chain_recs ? step / P.chain_steps * P.chain_recs + P.rec0 + cstep : step;
    const u64* st = steps + recno * 4 * (size_t)P.L64;
    const CellPtr adv = adv_ptr(P, advice, P.cell0 + (P.chain_steps ? step / P.chain_steps * P.chain_stride : 0) +
                                               (P.pair_stride ? (cstep >> 1) * P.pair_stride + (cstep & 1) * P.odd_off : cstep * P.cells));
    const CellPtr lk{lookup, P.lk0 + recno * P.lookups, P.rows, P.pad, nullptr, 0};
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const U192 MAXV = u_make(P.max_w[0], P.max_w[1], P.max_w[2]);
    const U192 BASE = u_shl(u_make(1), W);
#define LIMB(X, i) u_make((X)[i][0], (X)[i][1])

    for (unsigned i = tid; i < L; i += EXP_THREADS) {
        limb_extract(st, P.L64, i, W, s_a[i]);
        limb_extract(st + P.L64, P.L64, i, W, s_b[i]);
        limb_extract(st + 2 * (size_t)P.L64, P.L64, i, W, s_q[i]);
        limb_extract(st + 3 * (size_t)P.L64, P.L64, i, W, s_r[i]);
        limb_extract(modulus, P.L64, i, W, s_n[i]);
        s_am[i] = fr_from_u(LIMB(s_a, i));
        s_bm[i] = fr_from_u(LIMB(s_b, i));
        s_qm[i] = fr_from_u(LIMB(s_q, i));
        s_nm[i] = fr_from_u(LIMB(s_n, i));
    }
    __syncthreads();

    // ---- the two limb convolutions: wave per product limb (row), lanes own terms
    const unsigned PER = (D + 63) / 64;
    for (int which = 0; which < 2; ++which) {
        const u64(*xs)[2] = which ? s_q : s_a;
        const u64(*ys)[2] = which ? s_n : s_b;
        const Fr* xm = which ? s_qm : s_am;
        const Fr* ym = which ? s_nm : s_bm;
        u64(*pout)[3] = which ? s_pqn : s_pab;
        const CellPtr seg = adv + (which ? P.off_qn : P.off_ab);
        if (seg && tid == 0) fp_store(seg, fp_zero<FrTag>());  // load_zero
        for (unsigned i = wave; i < D; i += EXP_THREADS / 64) {
            const size_t row = 1 + (size_t)i + 3 * ((size_t)i * (i + 1) / 2);
            // local inclusive prefix over this lane's PER terms
            U192 pre[4];      // PER <= 4 (D <= 2 * EXP_MAXL - 1): unrolled so that pre[] stays in registers
            U192 run = u_make(0);
#pragma unroll
            for (unsigned t = 0; t < 4; ++t) {
                if (t < PER) {
                    const unsigned j = lane * PER + t;
                    U192 p = u_make(0);
                    if (j <= i && j < L && (i - j) < L) p = u_mul_limb(LIMB(xs, j), LIMB(ys, i - j), wide);
                    run = u_add(run, p);
                }
                pre[t] = run;
            }
            // wave inclusive scan of lane totals
            U192 tot = run;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                U192 o;
                o.w[0] = __shfl_up(tot.w[0], off, 64);
                o.w[1] = __shfl_up(tot.w[1], off, 64);
                o.w[2] = __shfl_up(tot.w[2], off, 64);
                if (lane >= (unsigned)off) tot = u_add(tot, o);
            }
            bool dummy;
            const U192 excl = u_sub(tot, run, dummy);
            if (seg && lane == 0) fp_store(seg + row, fp_zero<FrTag>());
#pragma unroll
            for (unsigned t = 0; t < 4; ++t) {
                const unsigned j = lane * PER + t;
                if (t < PER && j <= i) {
                    const U192 s = u_add(excl, pre[t]);
                    if (seg) {
                        const CellPtr c = seg + row + 1 + 3 * (size_t)j;
                        fp_store(c, j < L ? xm[j] : fp_zero<FrTag>());
                        fp_store(c + 1, (i - j) < L ? ym[i - j] : fp_zero<FrTag>());
                        fp_store(c + 2, fr_from_u(s));
                    }
                    if (j == i) {
                        pout[i][0] = s.w[0]; pout[i][1] = s.w[1]; pout[i][2] = s.w[2];
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- serial chains (one lane): carries of is_equal_muled, borrows of r < n
    if (tid == 0) {
        U192 carry = u_make(0), accx = u_make(0);
        unsigned eq = 1;
        s_eqbit[0] = 1;
        for (unsigned i = 0; i < D; ++i) {
            s_carry[i][0] = carry.w[0]; s_carry[i][1] = carry.w[1];
            s_accx[i][0] = accx.w[0]; s_accx[i][1] = accx.w[1];
            const U192 A = u_make(s_pab[i][0], s_pab[i][1], s_pab[i][2]);
            U192 Bq = u_make(s_pqn[i][0], s_pqn[i][1], s_pqn[i][2]);
            if (i < L) Bq = u_add(Bq, LIMB(s_r, i));
            S192 s = s_addu(s_addu(s_sub(A, Bq), carry), MAXV);  // >= 0 for a consistent step
            const U192 t = u_add(accx, MAXV);
            const unsigned e = (!s.neg && u_eq(u_lowbits(s.m, W), u_lowbits(t, W))) ? 1u : 0u;
            eq &= e;
            s_eqbit[i + 1] = (unsigned char)eq;
            carry = u_shr(s.m, W);
            accx = u_shr(t, W);
        }
        s_carry[D][0] = carry.w[0]; s_carry[D][1] = carry.w[1];
        s_accx[D][0] = accx.w[0]; s_accx[D][1] = accx.w[1];
        s_eqbit[D + 1] = (unsigned char)(eq & (u_eq(carry, accx) ? 1u : 0u));
        unsigned borrow = 0;
        for (unsigned i = 0; i < L; ++i) {
            s_borrow[i] = (unsigned char)borrow;
            // r_i < n_i + borrow  (n_i + borrow may be 2^W)
            bool lt;
            (void)u_sub(LIMB(s_r, i), u_add(LIMB(s_n, i), u_make(borrow)), lt);
            borrow = lt ? 1u : 0u;
        }
        s_borrow[L] = (unsigned char)borrow;
    }
    __syncthreads();

    // ---- segment: assign_integer(q), (n), (r)
    {
        const unsigned per_int = L + L * P.rc64_adv;
        for (unsigned t = tid; t < 3 * per_int; t += EXP_THREADS) {
            const unsigned which = t / per_int, u = t % per_int;
            const u64(*X)[2] = which == 0 ? s_q : (which == 1 ? s_n : s_r);
            CV v;
            if (u < L) v = cv_u(LIMB(X, u));
            else {
                const unsigned i = (u - L) / P.rc64_adv, p = (u - L) % P.rc64_adv;
                v = rc_adv_cell(LIMB(X, i), W, lb, p);
            }
            if (adv) fp_store(adv + P.off_assign + t, cv_to_fr(v));
        }
        if (lk)
            for (unsigned t = tid; t < 3 * L * P.rc64_lk; t += EXP_THREADS) {
                const unsigned which = t / (L * P.rc64_lk), u = t % (L * P.rc64_lk);
                const u64(*X)[2] = which == 0 ? s_q : (which == 1 ? s_n : s_r);
                fp_store(lk + P.lk_assign + t, cv_to_fr(rc_lk_cell(LIMB(X, u / P.rc64_lk), W, lb, u % P.rc64_lk)));
            }
    }
    // ---- segment: qn + r
    if (adv)
        for (unsigned t = tid; t < 4 * L; t += EXP_THREADS) {
            const unsigned i = t / 4, p = t % 4;
            const U192 qn = u_make(s_pqn[i][0], s_pqn[i][1], s_pqn[i][2]);
            CV v;
            if (p == 0) v = cv_u(qn);
            else if (p == 1) v = cv_one();
            else if (p == 2) v = cv_u(LIMB(s_r, i));
            else v = cv_u(u_add(qn, LIMB(s_r, i)));
            fp_store(adv + P.off_add + t, cv_to_fr(v));
        }
    // ---- segment: is_equal_muled
    {
        const unsigned per = 75 + P.rccb_adv;  // limbs 0..D-2; the last limb has 75 + 16
        if (adv && tid == 0) {
            fp_store(adv + P.off_eq, fp_zero<FrTag>());
            fp_store(adv + P.off_eq + 1, fp_one<FrTag>());
        }
        const unsigned total = (D - 1) * per + 75 + 16;
        for (unsigned t = tid; t < total; t += EXP_THREADS) {
            unsigned i, p;
            if (t < (D - 1) * per) { i = t / per; p = t % per; }
            else { i = D - 1; p = t - (D - 1) * per; }
            const U192 A = u_make(s_pab[i][0], s_pab[i][1], s_pab[i][2]);
            U192 Bq = u_make(s_pqn[i][0], s_pqn[i][1], s_pqn[i][2]);
            if (i < L) Bq = u_add(Bq, LIMB(s_r, i));
            const U192 carry = u_make(s_carry[i][0], s_carry[i][1]);
            const U192 accx = u_make(s_accx[i][0], s_accx[i][1]);
            const S192 diff = s_sub(A, Bq);
            const S192 dc = s_addu(diff, carry);
            const S192 ssum = s_addu(dc, MAXV);
            const U192 tt = u_add(accx, MAXV);
            const U192 ncarry = u_make(s_carry[i + 1][0], s_carry[i + 1][1]);
            CV v;
            if (p < 4) {
                v = p == 0 ? cv_s(diff) : p == 1 ? cv_u(Bq) : p == 2 ? cv_one() : cv_u(A);
            } else if (p < 11) {
                switch (p - 4) {
                    case 0: v = cv_s(diff); break;
                    case 1: v = cv_u(carry); break;
                    case 2: v = cv_one(); break;
                    case 3: v = cv_s(dc); break;
                    case 4: v = cv_u(MAXV); break;
                    case 5: v = cv_one(); break;
                    default: v = cv_s(ssum); break;
                }
            } else if (p < 33) {
                v = div_mod_cell(ssum.m, p - 11, W);
            } else if (p < 37) {
                v = p == 33 ? cv_u(accx) : p == 34 ? cv_one() : p == 35 ? cv_u(MAXV) : cv_u(tt);
            } else if (p < 59) {
                v = div_mod_cell(tt, p - 37, W);
            } else if (p < 71) {
                v = is_equal_cell(u_lowbits(ssum.m, W), u_lowbits(tt, W), p - 59);
            } else if (p < 75) {
                const unsigned e = u_eq(u_lowbits(ssum.m, W), u_lowbits(tt, W)) ? 1u : 0u;
                const unsigned in = s_eqbit[i], out = s_eqbit[i + 1];
                v = p == 71 ? cv_zero() : p == 72 ? (in ? cv_one() : cv_zero())
                    : p == 73 ? (e ? cv_one() : cv_zero()) : (out ? cv_one() : cv_zero());
            } else if (i < D - 1) {
                v = rc_adv_cell(ncarry, P.cb, lb, p - 75);
            } else {
                const U192 qacc = u_make(s_accx[D][0], s_accx[D][1]);
                if (p < 75 + 12) v = is_equal_cell(ncarry, qacc, p - 75);
                else {
                    const unsigned e = u_eq(ncarry, qacc) ? 1u : 0u;
                    const unsigned in = s_eqbit[D], out = s_eqbit[D + 1];
                    const unsigned pp = p - 87;
                    v = pp == 0 ? cv_zero() : pp == 1 ? (in ? cv_one() : cv_zero())
                        : pp == 2 ? (e ? cv_one() : cv_zero()) : (out ? cv_one() : cv_zero());
                }
            }
            if (adv) fp_store(adv + P.off_eq + 2 + t, cv_to_fr(v));
        }
        if (lk)
            for (unsigned t = tid; t < (D - 1) * P.rccb_lk; t += EXP_THREADS) {
                const unsigned i = t / P.rccb_lk, p = t % P.rccb_lk;
                fp_store(lk + P.lk_eq + t, cv_to_fr(rc_lk_cell(u_make(s_carry[i + 1][0], s_carry[i + 1][1]), P.cb, lb, p)));
            }
    }
    // ---- segment: r < n
    {
        const unsigned per = 11 + P.rc64_adv;
        for (unsigned t = tid; t < L * per; t += EXP_THREADS) {
            const unsigned i = t / per, p = t % per;
            const unsigned borrow = s_borrow[i], lt = s_borrow[i + 1];
            const U192 nb = u_add(LIMB(s_n, i), u_make(borrow));
            bool br;
            const U192 shift = u_sub(u_add(LIMB(s_r, i), BASE), nb, br);  // r_i - nb + 2^W
            const U192 outv = u_lowbits(shift, W);
            CV v;
            switch (p) {
                case 0: v = cv_u(LIMB(s_n, i)); break;
                case 1: v = cv_one(); break;
                case 2: v = borrow ? cv_one() : cv_zero(); break;
                case 3: v = cv_u(nb); break;
                case 4: v = cv_u(shift); break;
                case 5: v = lt ? cv_one() : cv_zero(); break;
                case 6: v = cv_u(outv); break;
                case 7: v = cv_u(LIMB(s_r, i)); break;
                case 8: v = lt ? cv_one() : cv_zero(); break;
                case 9: v = cv_u(BASE); break;
                case 10: v = cv_u(lt ? u_add(LIMB(s_r, i), BASE) : LIMB(s_r, i)); break;
                default: v = rc_adv_cell(outv, W, lb, p - 11); break;
            }
            if (adv) fp_store(adv + P.off_lt + t, cv_to_fr(v));
        }
        if (adv && tid == 0) fp_store(adv + P.off_lt + (size_t)L * per, s_borrow[L] ? fp_one<FrTag>() : fp_zero<FrTag>());
        if (lk)
            for (unsigned t = tid; t < L * P.rc64_lk; t += EXP_THREADS) {
                const unsigned i = t / P.rc64_lk, p = t % P.rc64_lk;
                bool br;
                const U192 shift = u_sub(u_add(LIMB(s_r, i), BASE), u_add(LIMB(s_n, i), u_make(s_borrow[i])), br);
                fp_store(lk + P.lk_lt + t, cv_to_fr(rc_lk_cell(u_lowbits(shift, W), W, lb, p)));
            }
    }
}

#undef LIMB

// ------------------------------------------------------------------------------------------------
// host: layout arithmetic (mirrors paillier_halo2_amd/layout.py::mul_mod_cells)
// ------------------------------------------------------------------------------------------------
static void rc_counts(unsigned bits, unsigned lb, unsigned& k, unsigned& rem, unsigned& adv, unsigned& lk) {
    k = (bits + lb - 1) / lb;
    rem = bits % lb;
    adv = k == 1 ? 0 : 1 + 3 * (k - 1);
    lk = k;
    if (rem == 1) adv += 4;
    else if (rem > 1) { adv += 4; lk += 1; }
}

// 192-bit host helpers for MAX = L*(2^W-1)^2 + (2^W-1) = (L << 2W) - (L << (W+1)) + L + (1 << W) - 1
static void h_shl(const uint64_t a[3], unsigned s, uint64_t r[3]) {
    uint64_t t[3] = {a[0], a[1], a[2]};
    while (s >= 64) { t[2] = t[1]; t[1] = t[0]; t[0] = 0; s -= 64; }
    if (s) { t[2] = (t[2] << s) | (t[1] >> (64 - s)); t[1] = (t[1] << s) | (t[0] >> (64 - s)); t[0] <<= s; }
    r[0] = t[0]; r[1] = t[1]; r[2] = t[2];
}
static void h_add(uint64_t a[3], const uint64_t b[3]) {
    unsigned __int128 c = 0;
    for (int i = 0; i < 3; ++i) { c += (unsigned __int128)a[i] + b[i]; a[i] = (uint64_t)c; c >>= 64; }
}
static void h_sub(uint64_t a[3], const uint64_t b[3]) {
    uint64_t br = 0;
    for (int i = 0; i < 3; ++i) {
        const uint64_t t = a[i] - b[i], b1 = a[i] < b[i], t2 = t - br;
        br = b1 | (t < br);
        a[i] = t2;
    }
}
static unsigned h_bits(const uint64_t a[3]) {
    for (int i = 2; i >= 0; --i)
        if (a[i]) return 64 * i + (64 - __builtin_clzll(a[i]));
    return 0;
}

static int make_params(uint32_t L, uint32_t limb_bits, uint32_t lb, ExpP& P) {
    // limb_bits = 64 is the reference bench's choice (bench.rs:140, paillier.rs:116); its add test runs 88-bit limbs
    // (paillier.rs:186-187).  A limb travels as two 64-bit words and a product limb as three: 2W + log2(L) + 3 <= 192.
    if (limb_bits < 16 || limb_bits > 90) return PZ_ERR_UNSUPPORTED;
    if (L < 2 || L > EXP_MAXL) return PZ_ERR_UNSUPPORTED;
    if (lb < 4 || lb > 32) return PZ_ERR_INVALID;
    {
        unsigned lg = 0;
        while ((1u << lg) < L) ++lg;
        if (2 * limb_bits + lg + 3 > 192) return PZ_ERR_UNSUPPORTED;
    }
    memset(&P, 0, sizeof P);
    P.L = L;
    P.D = 2 * L - 1;
    P.lb = lb;
    P.W = limb_bits;
    P.L64 = (L * limb_bits + 63) / 64;
    rc_counts(limb_bits, lb, P.k64, P.rem64, P.rc64_adv, P.rc64_lk);
    if (P.k64 < 2) return PZ_ERR_INVALID;
    const uint64_t Lw[3] = {L, 0, 0}, one[3] = {1, 0, 0};
    uint64_t mx[3], t[3];
    h_shl(Lw, 2 * limb_bits, mx);
    h_shl(Lw, limb_bits + 1, t);
    h_sub(mx, t);
    h_add(mx, Lw);
    h_shl(one, limb_bits, t);
    h_add(mx, t);
    h_sub(mx, one);
    P.max_w[0] = mx[0]; P.max_w[1] = mx[1]; P.max_w[2] = mx[2];
    h_shl(mx, 1, t);  // 2*MAX
    const unsigned bits = h_bits(t);
    P.cb = bits - limb_bits;
    rc_counts(P.cb, lb, P.kcb, P.remcb, P.rccb_adv, P.rccb_lk);
    size_t off = 0;
    P.off_assign = off;
    off += 3 * ((size_t)L + (size_t)L * P.rc64_adv);
    size_t per_mul = 1;
    for (unsigned i = 0; i < P.D; ++i) per_mul += 1 + 3 * ((size_t)i + 1);
    P.off_ab = off; off += per_mul;
    P.off_qn = off; off += per_mul;
    P.off_add = off; off += 4 * (size_t)L;
    P.off_eq = off; off += 2 + (size_t)P.D * 75 + (size_t)(P.D - 1) * P.rccb_adv + 16;
    P.off_lt = off; off += (size_t)L * (11 + P.rc64_adv) + 1;
    P.cells = off;
    P.lk_assign = 0;
    P.lk_eq = 3 * (size_t)L * P.rc64_lk;
    P.lk_lt = P.lk_eq + (size_t)(P.D - 1) * P.rccb_lk;
    P.lookups = P.lk_lt + (size_t)L * P.rc64_lk;
    return PZ_OK;
}

// the tail of every cell-count entry point: the builder's refusal, or the two counts to whoever asked for them
static int put_cells(int rc, const size_t& a, const size_t& l, size_t* advice_cells, size_t* lookup_cells) {
    PZCHK(rc);
    if (advice_cells) *advice_cells = a;
    if (lookup_cells) *lookup_cells = l;
    return PZ_OK;
}

extern "C" int pz_witness_cells_per_step(uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits,
                                         size_t* advice_cells, size_t* lookup_cells) {
    ExpP P;
    const int rc = make_params(limbs, limb_bits, lookup_bits, P);
    return put_cells(rc, P.cells, P.lookups, advice_cells, lookup_cells);
}

extern "C" int pz_witness_expand_dev(pz_ctx* ctx, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits,
                                     const uint64_t* d_steps, size_t n_steps, const uint64_t* d_modulus,
                                     uint64_t* d_advice, uint64_t* d_lookup) {
    if (!ctx || (n_steps && (!d_steps || !d_modulus))) return PZ_ERR_INVALID;
    ExpP P;
    PZCHK(make_params(limbs, limb_bits, lookup_bits, P));
    if (!n_steps || (!d_advice && !d_lookup)) return PZ_OK;
    PZ_ENTER(ctx);
    pz_timer tm(ctx, PZ_T_EXPAND);
    hipLaunchKernelGGL(k_witness_expand, dim3((unsigned)n_steps), dim3(EXP_THREADS), 0, ctx->stream, P, d_steps,
                       d_modulus, (Fr*)d_advice, (Fr*)d_lookup);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

// ------------------------------------------------------------------------------------------------
// The rest of the circuit: every cell the drivers bench.rs:33-75 / :77-117 push that is
// NOT inside a mul_mod -- the input assignments, square + refresh of n, load_zero, the constant cells of
// pow_mod_fixed_exp, the assignment of res and assert_equal_fresh -- in the layout of
// paillier_halo2_amd/layout.py::circuit_cells (values: oracle/pyref.py::expand_circuit_cells).  A few thousand to a few
// hundred thousand cells per proof: one workgroup, the serial carry chain of refresh on one lane.
//
// Every kind's stream is put together from the same pieces, described here once; the block comment above a kind names only what is
// its own.
//   * k_circuit_misc (one workgroup): assign_integer of the Ln-limb inputs that head the stream, square(n) + refresh, the single
//     constant cells, and -- for the kinds with ONE result -- the result block.
//   * k_circuit_assign_many: a run of equally wide assign_integer blocks, one workgroup each.
//   * the result block (result_block): assign_integer(res) followed by assert_equal_fresh(c, res), c the value the records computed.
//     Kinds with a result per entry write them with k_circuit_results, one workgroup each, together with the [1, 0] head of the
//     entry's pow_mod_fixed_exp.
//   * an exponent chain [1, 0 | num_to_bits | bits x (mul_mod, select, square_mod)]: k_circuit_bits[_many] for the head,
//     k_circuit_select[_many] for the selects, launch_chains for the record pairs; runs of whole mul_mod blocks go through
//     launch_runs.  nbits_cells and bit_stride name the chain's geometry.
//   * host: circ_base and square_refresh_cells open every parameter builder, expand_enter and expand_stage every expansion.
// ------------------------------------------------------------------------------------------------
#define CIRC_MAXF 256   // fresh limbs of n^2 (2 Ln)
#define CIRC_MAXJ 3     // pieces a product limb is cut into (2W + log2(Ln) bits -> at most 3 limbs)
#define LIMB(X, i) u_make((X)[i][0], (X)[i][1])

struct CircP {
    ExpP e;                         // shape of the mul_mod steps (L = 2 Ln): range-check parameters, limb width
    unsigned Ln, nf, words_n, kind;
    unsigned n_in;                  // Ln-limb inputs assigned here: n | g | x | y (kinds 0..2), n | g (ballot) or n alone
    bool no_res;                    // no result block in k_circuit_misc: the kind has one per entry (k_circuit_results)
    bool has_zero;                  // load_zero behind refresh (the tallies extend nothing: none)
    size_t res_off;                 // word offset of res inside `inputs` (unless no_res)
    size_t a_cts, l_cts;            // kinds 3, 4: the count assign_integer(c_i, 2 Ln limbs) blocks (k_circuit_assign_many)
    size_t n_cts;                   // kinds 3, 4: the number of ciphertexts
    unsigned w_bits;                // kind 4: bits per weight
    size_t a_wts;                   // kind 4: the count load_witness(w_i) cells
    unsigned rc_adv, rc_lk;         // range_check(limb, W)
    size_t a_assign[4], a_square, a_refresh, a_zero, a_pow[2], a_res;   // advice offsets of the segments
    size_t l_assign[4], l_refresh, l_res;                               // lookup offsets
    unsigned char inc[CIRC_MAXF];
};

// assign_integer of the nl limbs X: the limbs, then per limb the cells of its range check; the lookup cells likewise.  Every thread of
// the block calls it.
__device__ __forceinline__ void assign_integer_cells(const CircP& C, const u64 (*X)[2], unsigned nl, const CellPtr& a, const CellPtr& l) {
    const unsigned W = C.e.W, lb = C.e.lb;
    for (unsigned t = threadIdx.x; t < nl * (1 + C.rc_adv); t += blockDim.x) {
        Fr v;
        if (t < nl) v = fr_from_u(LIMB(X, t));
        else v = cv_to_fr(rc_adv_cell(LIMB(X, (t - nl) / C.rc_adv), W, lb, (t - nl) % C.rc_adv));
        fp_store(a + t, v);
    }
    if (l)
        for (unsigned t = threadIdx.x; t < nl * C.rc_lk; t += blockDim.x) fp_store(l + t, cv_to_fr(rc_lk_cell(LIMB(X, t / C.rc_lk), W, lb, t % C.rc_lk)));
}

// The result block at advice cell a / lookup cell l: assign_integer(res), then assert_equal_fresh(c, res) = [0, 1] and per limb the 12
// cells of is_equal and [0, running bit, this limb's bit, running bit].  res, cval: L64 words each; s_res, s_c, s_eq: the block's shared
// limb arrays (CIRC_MAXF limbs; CIRC_MAXF + 1 bytes).  Every thread of the block calls it (two barriers inside).
__device__ __forceinline__ void result_block(const CircP& C, const u64* __restrict__ res, const u64* __restrict__ cval, u64 (*s_res)[2],
                                             u64 (*s_c)[2], unsigned char* s_eq, const CellPtr& a, const CellPtr& l) {
    const unsigned nf = C.nf, tid = threadIdx.x;
    for (unsigned t = tid; t < nf; t += blockDim.x) {
        limb_extract(res, C.e.L64, t, C.e.W, s_res[t]);
        limb_extract(cval, C.e.L64, t, C.e.W, s_c[t]);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned eq = 1;
        s_eq[0] = 1;
        for (unsigned i = 0; i < nf; ++i) {
            eq &= u_eq(LIMB(s_c, i), LIMB(s_res, i)) ? 1u : 0u;
            s_eq[i + 1] = (unsigned char)eq;
        }
    }
    __syncthreads();
    assign_integer_cells(C, s_res, nf, a, l);
    const CellPtr e = a + (size_t)nf * (1 + C.rc_adv);
    if (tid == 0) {
        fp_store(e, fp_zero<FrTag>());
        fp_store(e + 1, fp_one<FrTag>());
    }
    for (unsigned t = tid; t < 16 * nf; t += blockDim.x) {
        const unsigned i = t / 16, p = t % 16;
        Fr v;
        if (p < 12) v = cv_to_fr(is_equal_cell(LIMB(s_c, i), LIMB(s_res, i), p));
        else {
            const unsigned eq = u_eq(LIMB(s_c, i), LIMB(s_res, i)) ? 1u : 0u, in = s_eq[i], out = s_eq[i + 1];
            v = p == 12 ? fp_zero<FrTag>() : p == 13 ? (in ? fp_one<FrTag>() : fp_zero<FrTag>())
                : p == 14 ? (eq ? fp_one<FrTag>() : fp_zero<FrTag>()) : (out ? fp_one<FrTag>() : fp_zero<FrTag>());
        }
        fp_store(e + 2 + t, v);
    }
}

__global__ __launch_bounds__(256) void k_circuit_misc(CircP C, const u64* __restrict__ inputs /* n | g | x | y | res; kind 3: n | c_1 .. c_B | res; kind 4: n | c_1 .. c_B | w_1 .. w_B | res */,
                                                      const u64* __restrict__ cval /* the circuit's result, L64 words (unless C.no_res) */,
                                                      Fr* __restrict__ advice, Fr* __restrict__ lookup) {
    const CellPtr adv = adv_ptr(C.e, advice, 0), lk{lookup, 0, C.e.rows, C.e.pad, nullptr, 0};
    __shared__ u64 s_in[4][EXP_MAXL / 2 + 1][2];       // limbs of n, g, x, y
    __shared__ u64 s_res[CIRC_MAXF][2], s_c[CIRC_MAXF][2], s_fresh[CIRC_MAXF][2];
    __shared__ u64 s_sq[CIRC_MAXF][3];                 // limbs of n * n (unreduced convolution sums)
    __shared__ u64 s_dm[CIRC_MAXF][CIRC_MAXJ][3];      // refresh: the value each div_mod_unsafe divides
    __shared__ u64 s_ad[CIRC_MAXF][CIRC_MAXJ][3];      // refresh: limb i + j before the j-th remainder is added
    __shared__ unsigned s_roff[CIRC_MAXF + 1];
    __shared__ unsigned char s_eq[CIRC_MAXF + 1];
    const unsigned Ln = C.Ln, nf = C.nf, W = C.e.W, lb = C.e.lb, tid = threadIdx.x;
    const bool wide = W > 64;
    const unsigned D = 2 * Ln - 1;
    for (unsigned t = tid; t < C.n_in * Ln; t += blockDim.x) limb_extract(inputs + (size_t)(t / Ln) * C.words_n, C.words_n, t % Ln, W, s_in[t / Ln][t % Ln]);
    __syncthreads();
    // ---- square(n): one lane per product limb, cells written as the row is summed
    if (tid == 0) fp_store(adv + C.a_square, fp_zero<FrTag>());
    for (unsigned i = tid; i < D; i += blockDim.x) {
        const size_t row = 1 + (size_t)i + 3 * ((size_t)i * (i + 1) / 2);
        const CellPtr c = adv + C.a_square + row;
        fp_store(c, fp_zero<FrTag>());
        U192 sum = u_make(0);
        for (unsigned j = 0; j <= i; ++j) {
            const bool in = j < Ln && (i - j) < Ln;
            if (in) sum = u_add(sum, u_mul_limb(LIMB(s_in[0], j), LIMB(s_in[0], i - j), wide));
            fp_store(c + 1 + 3 * (size_t)j, j < Ln ? fr_from_u(LIMB(s_in[0], j)) : fp_zero<FrTag>());
            fp_store(c + 2 + 3 * (size_t)j, (i - j) < Ln ? fr_from_u(LIMB(s_in[0], i - j)) : fp_zero<FrTag>());
            fp_store(c + 3 + 3 * (size_t)j, fr_from_u(sum));
        }
        s_sq[i][0] = sum.w[0]; s_sq[i][1] = sum.w[1]; s_sq[i][2] = sum.w[2];
    }
    for (unsigned i = D + tid; i < nf; i += blockDim.x) { s_sq[i][0] = 0; s_sq[i][1] = 0; s_sq[i][2] = 0; }
    __syncthreads();
    // ---- serial chain: refresh's carries
    if (tid == 0) {
        unsigned off = 1;
        for (unsigned i = 0; i < nf; ++i) {
            s_roff[i] = off;
            U192 limb = u_make(s_sq[i][0], s_sq[i][1], s_sq[i][2]);
            for (unsigned j = 0; j <= C.inc[i]; ++j) {
                s_dm[i][j][0] = limb.w[0]; s_dm[i][j][1] = limb.w[1]; s_dm[i][j][2] = limb.w[2];
                const U192 nrem = u_lowbits(limb, W);
                if (j == 0) {
                    s_sq[i][0] = nrem.w[0]; s_sq[i][1] = nrem.w[1]; s_sq[i][2] = 0;
                } else if (i + j < nf) {
                    s_ad[i][j][0] = s_sq[i + j][0]; s_ad[i][j][1] = s_sq[i + j][1]; s_ad[i][j][2] = s_sq[i + j][2];
                    const U192 nv = u_add(u_make(s_sq[i + j][0], s_sq[i + j][1], s_sq[i + j][2]), nrem);
                    s_sq[i + j][0] = nv.w[0]; s_sq[i + j][1] = nv.w[1]; s_sq[i + j][2] = nv.w[2];
                }
                limb = u_shr(limb, W);
                off += 22 + (j ? 4 : 0);
            }
            s_fresh[i][0] = s_sq[i][0]; s_fresh[i][1] = s_sq[i][1];
        }
        s_roff[nf] = off;
    }
    __syncthreads();
    // ---- assign_integer of n, g, x, y (Ln limbs)
    for (unsigned which = 0; which < C.n_in; ++which) assign_integer_cells(C, s_in[which], Ln, adv + C.a_assign[which], lk + C.l_assign[which]);
    // ---- refresh
    if (tid == 0) fp_store(adv + C.a_refresh, fp_zero<FrTag>());
    for (unsigned i = 0; i < nf; ++i) {
        const unsigned len = s_roff[i + 1] - s_roff[i];
        for (unsigned t = tid; t < len; t += blockDim.x) {
            // blocks: j = 0: 22 cells; j > 0: 22 + 4 cells
            unsigned j = 0, p = t;
            if (p >= 22) { j = 1 + (p - 22) / 26; p = (p - 22) % 26; }
            const U192 v = u_make(s_dm[i][j][0], s_dm[i][j][1], s_dm[i][j][2]);
            Fr x;
            if (p < 22) x = cv_to_fr(div_mod_cell(v, p, W));
            else {
                const U192 before = u_make(s_ad[i][j][0], s_ad[i][j][1], s_ad[i][j][2]), nrem = u_lowbits(v, W);
                x = p == 22 ? fr_from_u(before) : p == 23 ? fp_one<FrTag>() : p == 24 ? fr_from_u(nrem) : fr_from_u(u_add(before, nrem));
            }
            fp_store(adv + C.a_refresh + s_roff[i] + t, x);
        }
    }
    for (unsigned t = tid; t < nf * C.rc_adv; t += blockDim.x)
        fp_store(adv + C.a_refresh + s_roff[nf] + t, cv_to_fr(rc_adv_cell(LIMB(s_fresh, t / C.rc_adv), W, lb, t % C.rc_adv)));
    if (lk)
        for (unsigned t = tid; t < nf * C.rc_lk; t += blockDim.x)
            fp_store(lk + C.l_refresh + t, cv_to_fr(rc_lk_cell(LIMB(s_fresh, t / C.rc_lk), W, lb, t % C.rc_lk)));
    // ---- load_zero; assign_constant(1) + load_zero of both pow_mod_fixed_exp
    if (tid == 0) {
        if (C.has_zero) fp_store(adv + C.a_zero, fp_zero<FrTag>());
        if (C.kind == 0 || C.kind == 2)
            for (int k = 0; k < 2; ++k) {
                fp_store(adv + C.a_pow[k], fp_one<FrTag>());
                fp_store(adv + C.a_pow[k] + 1, fp_zero<FrTag>());
            }
    }
    // ---- assign_integer(res) (2 Ln limbs), assert_equal_fresh(c, res)
    if (!C.no_res) result_block(C, inputs + C.res_off, cval, s_res, s_c, s_eq, adv + C.a_res, lk + C.l_res);
}

// ---- a run of assign_integer blocks, grid.x = integer: the nl limbs of integer i (words words each inside `vals`) at advice cell
// a0 + i * nl * (1 + rc_adv) / lookup cell l0 + i * nl * rc_lk; the shared array holds ONE integer, however many there are
__global__ __launch_bounds__(256) void k_circuit_assign_many(CircP C, unsigned nl, unsigned words, const u64* __restrict__ vals, size_t a0, size_t l0,
                                                             Fr* __restrict__ advice, Fr* __restrict__ lookup) {
    __shared__ u64 s_x[CIRC_MAXF][2];
    const CellPtr a = adv_ptr(C.e, advice, a0 + (size_t)blockIdx.x * nl * (1 + C.rc_adv));
    const CellPtr l{lookup, l0 + (size_t)blockIdx.x * nl * C.rc_lk, C.e.rows, C.e.pad, nullptr, 0};
    for (unsigned t = threadIdx.x; t < nl; t += blockDim.x) limb_extract(vals + (size_t)blockIdx.x * words, words, t, C.e.W, s_x[t]);
    __syncthreads();
    assign_integer_cells(C, s_x, nl, a, l);
}

// ---- the result blocks of a kind with one result per entry, and the [1, 0] heads that go with them: block i of k_circuit_results
struct ResP {
    size_t in_res, in_stride;        // res_i: L64 words at word in_res + i * in_stride of `inputs`
    size_t rec0, rec_stride;         // the value computed for it: field `field` of record rec0 + i * rec_stride
    unsigned field;                  // 3: the record's remainder; 0: its first operand
    size_t a_head, head_stride;      // the [1, 0] of a pow_mod_fixed_exp at advice cell a_head + i * head_stride
    size_t a_res, l_res, res_stride; // block i at advice cell a_res + i * res_stride / lookup cell l_res + i * nf * rc_lk
    size_t sum_n, in_ms, a_sum;      // ballot, sum_n >= 2: block 0 also writes FlexGate::sum of the sum_n one-word messages at in_ms
};
// FlexGate::sum's cells m_1 | 1 | m_2 | s_2 | 1 | m_3 | s_3 | .. ; s_pre: n prefix sums (below 2^74).  Every thread of the block calls it.
__device__ __forceinline__ void flex_sum_cells(const u64* __restrict__ ms, size_t n, u64 (*s_pre)[2], const CellPtr& a) {
    if (threadIdx.x == 0) {
        U192 s = u_make(0);
        for (size_t t = 0; t < n; ++t) {
            s = u_add(s, u_make(ms[t]));
            s_pre[t][0] = s.w[0]; s_pre[t][1] = s.w[1];
        }
    }
    __syncthreads();
    for (size_t t = threadIdx.x; t < 1 + 3 * (n - 1); t += blockDim.x) {
        Fr v;
        if (t == 0) v = fr_from_u(u_make(ms[0]));
        else {
            const size_t m = (t - 1) / 3 + 1, w = (t - 1) % 3;
            v = w == 0 ? fp_one<FrTag>() : w == 1 ? fr_from_u(u_make(ms[m])) : fr_from_u(LIMB(s_pre, m));
        }
        fp_store(a + t, v);
    }
}
// grid.x = entry.  Dynamic shared memory: 16 bytes per message of the ballot's sum (R.sum_n >= 2), none otherwise.
__global__ __launch_bounds__(256) void k_circuit_results(CircP C, ResP R, const u64* __restrict__ inputs, const u64* __restrict__ steps,
                                                         Fr* __restrict__ advice, Fr* __restrict__ lookup) {
    __shared__ u64 s_res[CIRC_MAXF][2], s_c[CIRC_MAXF][2];
    __shared__ unsigned char s_eq[CIRC_MAXF + 1];
    extern __shared__ u64 s_pre[][2];
    const size_t i = blockIdx.x;
    if (threadIdx.x == 0) {
        const CellPtr p = adv_ptr(C.e, advice, R.a_head + i * R.head_stride);
        fp_store(p, fp_one<FrTag>());
        fp_store(p + 1, fp_zero<FrTag>());
    }
    if (i == 0 && R.sum_n >= 2) flex_sum_cells(inputs + R.in_ms, R.sum_n, s_pre, adv_ptr(C.e, advice, R.a_sum));
    result_block(C, inputs + R.in_res + i * R.in_stride, steps + ((R.rec0 + i * R.rec_stride) * 4 + R.field) * (size_t)C.e.L64, s_res, s_c, s_eq,
                 adv_ptr(C.e, advice, R.a_res + i * R.res_stride), CellPtr{lookup, R.l_res + i * C.nf * C.rc_lk, C.e.rows, C.e.pad, nullptr, 0});
}

// ---- uniform-shape circuit: FlexGate::num_to_bits of the message's limbs and the limb-wise select after
// every mul_mod(acc, sq) of pow_mod.  grid.x = limb of m (num_to_bits) / exponent bit (select).
// cell t of num_to_bits(x, nbits): the inner product of the bits with the powers of two (1 + 3 (nbits - 1) cells), then assert_bit
// of every bit ([0, b, b, b]) -- 7 nbits - 2 cells
__host__ __device__ static inline size_t nbits_cells(size_t nbits) { return 7 * nbits - 2; }
__device__ __forceinline__ Fr num_to_bits_cell(const U192& x, unsigned nbits, unsigned t) {
    const unsigned nip = 1 + 3 * (nbits - 1);
    if (t == 0) return fr_from_u(u_lowbits(x, 1));
    if (t < nip) {
        const unsigned i = (t - 1) / 3 + 1, w = (t - 1) % 3;
        return w == 0 ? fr_from_u(u_lowbits(u_shr(x, i), 1)) : w == 1 ? fr_from_u(u_shl(u_make(1), i)) : fr_from_u(u_lowbits(x, i + 1));
    }
    const unsigned i = (t - nip) / 4, w = (t - nip) % 4;
    return w == 0 ? fp_zero<FrTag>() : fr_from_u(u_lowbits(u_shr(x, i), 1));
}
__global__ __launch_bounds__(256) void k_circuit_bits(ExpP P, unsigned Ln, unsigned words_n, const u64* __restrict__ m_words,
                                                      size_t cell_base, size_t limb_stride, Fr* __restrict__ advice) {
    const unsigned li = blockIdx.x, W = P.W;
    u64 lw[2];
    limb_extract(m_words, words_n, li, W, lw);
    const U192 x = u_make(lw[0], lw[1]);
    const CellPtr a = adv_ptr(P, advice, cell_base + (size_t)li * limb_stride);
    for (unsigned t = threadIdx.x; t < nbits_cells(W); t += blockDim.x) fp_store(a + t, num_to_bits_cell(x, W, t));
}
// the many-chain form (weighted tally, kind 4): grid.x = chain.  Chain i's exponent is the ONE word weights[i]; the block writes the
// load_witness cell of w_i (a_wts + i) and, at cell_base + i * chain_stride, the chain's head: assign_constant(1), load_zero, then
// num_to_bits(w_i, nbits)
__global__ __launch_bounds__(256) void k_circuit_bits_many(ExpP P, unsigned nbits, const u64* __restrict__ weights, size_t a_wts, size_t cell_base,
                                                           size_t chain_stride, Fr* __restrict__ advice) {
    const size_t i = blockIdx.x;
    const U192 x = u_make(weights[i]);
    const CellPtr a = adv_ptr(P, advice, cell_base + i * chain_stride);
    if (threadIdx.x == 0) {
        fp_store(adv_ptr(P, advice, a_wts + i), fr_from_u(x));
        fp_store(a, fp_one<FrTag>());
        fp_store(a + 1, fp_zero<FrTag>());
    }
    for (unsigned t = threadIdx.x; t < nbits_cells(nbits); t += blockDim.x) fp_store(a + 2 + t, num_to_bits_cell(x, nbits, t));
}
// the limb-wise select(bit, muled, acc) after the mul_mod(acc, sq) step `st` (a = acc, r = muled): 8 cells per limb
// [d | 1 | acc | muled | acc | bit | d | out], d = muled - acc
__device__ __forceinline__ void select_cells(const ExpP& P, const u64* __restrict__ st, unsigned bit, const CellPtr& a) {
    const unsigned W = P.W, L = P.L;
    for (unsigned t = threadIdx.x; t < 8 * L; t += blockDim.x) {
        const unsigned limb = t / 8, p = t % 8;
        u64 aw[2], mw[2];
        limb_extract(st, P.L64, limb, W, aw);                           // acc
        limb_extract(st + 3 * (size_t)P.L64, P.L64, limb, W, mw);       // muled
        const U192 acc = u_make(aw[0], aw[1]), mul = u_make(mw[0], mw[1]);
        const S192 d = s_sub(mul, acc);
        Fr v;
        switch (p) {
            case 0: case 6: v = fr_from_s(d); break;
            case 1: v = fp_one<FrTag>(); break;
            case 2: case 4: v = fr_from_u(acc); break;
            case 3: v = fr_from_u(mul); break;
            case 5: v = bit ? fp_one<FrTag>() : fp_zero<FrTag>(); break;
            default: v = fr_from_u(bit ? mul : acc); break;
        }
        fp_store(a + t, v);
    }
}
__global__ __launch_bounds__(256) void k_circuit_select(ExpP P, unsigned Ln, unsigned words_n, const u64* __restrict__ m_words,
                                                        const u64* __restrict__ steps, size_t cell_base, size_t limb_stride,
                                                        size_t bit_stride, size_t nbits_cells, Fr* __restrict__ advice) {
    const unsigned i = blockIdx.x, W = P.W;                 // exponent bit i = limb li, bit bi
    const unsigned li = i / W, bi = i % W;
    u64 lw[2];
    limb_extract(m_words, words_n, li, W, lw);
    const unsigned bit = (unsigned)(u_lowbits(u_shr(u_make(lw[0], lw[1]), bi), 1).w[0]);
    const u64* st = steps + (size_t)(2 * i) * 4 * P.L64;    // the mul_mod(acc, sq) step: a = acc, r = muled
    // cells of this bit: after its limb's num_to_bits block and its mul_mod step
    const CellPtr a = adv_ptr(P, advice, cell_base + (size_t)li * limb_stride + nbits_cells + (size_t)bi * bit_stride + P.cells);
    select_cells(P, st, bit, a);
}
// the many-chain form (weighted tally, kind 4; ballot): grid.x = chain * nbits + bit.  `steps` holds the chains' records chain-major,
// chain_recs apart (2 nbits where nothing else lies between them); chain i sits at cell_base + i * chain_stride, its bit blocks
// head_cells (= [1, 0] + num_to_bits) further on
__global__ __launch_bounds__(256) void k_circuit_select_many(ExpP P, unsigned nbits, const u64* __restrict__ weights, const u64* __restrict__ steps,
                                                             size_t chain_recs, size_t cell_base, size_t chain_stride, size_t bit_stride,
                                                             size_t head_cells, Fr* __restrict__ advice) {
    const size_t i = blockIdx.x / nbits;
    const unsigned bi = blockIdx.x % nbits;
    const unsigned bit = (unsigned)((weights[i] >> bi) & 1);
    const u64* st = steps + (i * chain_recs + 2 * (size_t)bi) * 4 * P.L64;
    select_cells(P, st, bit, adv_ptr(P, advice, cell_base + i * chain_stride + head_cells + (size_t)bi * bit_stride + P.cells));
}

// RefreshAux::new(limb_bits, l, r).increased_limbs_vec with the maximal limb values tracked as bit lengths + exact
// small big-integers (3 x 64-bit words are enough: a product limb is below 2^(2W + 8))
static int refresh_aux_host(unsigned W, unsigned nl, unsigned nr, unsigned char* inc, unsigned* n_out) {
    const unsigned d = nl + nr - 1;
    std::vector<std::array<uint64_t, 3>> muled;
    uint64_t mx2[3], one[3] = {1, 0, 0}, t[3];
    // (2^W - 1)^2 = 2^(2W) - 2^(W+1) + 1
    h_shl(one, 2 * W, mx2);
    h_shl(one, W + 1, t);
    h_sub(mx2, t);
    h_add(mx2, one);
    for (unsigned i = 0; i < d; ++i) {
        unsigned cnt = 0;
        for (unsigned j = 0; j < nl; ++j)
            if (i >= j && i - j < nr) ++cnt;
        std::array<uint64_t, 3> v = {0, 0, 0};
        for (unsigned k = 0; k < cnt; ++k) h_add(v.data(), mx2);
        muled.push_back(v);
    }
    unsigned cur = 0, n = 0;
    while (cur < muled.size()) {
        if (n >= CIRC_MAXF) return PZ_ERR_UNSUPPORTED;
        const unsigned bits = h_bits(muled[cur].data());
        unsigned chunks = (bits + W - 1) / W;
        if (chunks == 0) chunks = 1;
        if (chunks > CIRC_MAXJ) return PZ_ERR_UNSUPPORTED;
        inc[n++] = (unsigned char)(chunks - 1);
        uint64_t val[3] = {muled[cur][0], muled[cur][1], muled[cur][2]};
        for (unsigned i = 0; i < chunks; ++i) {
            // piece = val mod 2^W ; val >>= W
            uint64_t piece[3] = {val[0], val[1], val[2]};
            if (W < 64) { piece[0] &= (1ull << W) - 1; piece[1] = 0; piece[2] = 0; }
            else if (W == 64) { piece[1] = 0; piece[2] = 0; }
            else { piece[1] &= (1ull << (W - 64)) - 1; piece[2] = 0; }
            unsigned sft = W;
            while (sft >= 64) { val[0] = val[1]; val[1] = val[2]; val[2] = 0; sft -= 64; }
            if (sft) { val[0] = (val[0] >> sft) | (val[1] << (64 - sft)); val[1] = (val[1] >> sft) | (val[2] << (64 - sft)); val[2] >>= sft; }
            if (cur + i < muled.size()) {
                if (i == 0) muled[cur] = {piece[0], piece[1], piece[2]};
                else h_add(muled[cur + i].data(), piece);
            } else muled.push_back({piece[0], piece[1], piece[2]});
        }
        ++cur;
    }
    *n_out = n;
    return PZ_OK;
}

// ---- the parts every kind's parameter builder is made of
// what all kinds start from: the mul_mod shape at 2 Ln limbs, n's word count, the range check of a limb, refresh's limb counts
static int circ_base(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, unsigned kind, CircP& C) {
    if (limbs_n < 1 || 2 * limbs_n > CIRC_MAXF || 2 * limbs_n > EXP_MAXL) return PZ_ERR_UNSUPPORTED;
    memset(&C, 0, sizeof C);
    PZCHK(make_params(2 * limbs_n, limb_bits, lb, C.e));
    C.Ln = limbs_n;
    C.kind = kind;
    C.words_n = (limbs_n * limb_bits + 63) / 64;
    C.rc_adv = C.e.rc64_adv;
    C.rc_lk = C.e.rc64_lk;
    PZCHK(refresh_aux_host(limb_bits, limbs_n, limbs_n, C.inc, &C.nf));
    if (C.nf != 2 * limbs_n) return PZ_ERR_UNSUPPORTED;   // the chip's mul_mod needs n^2 at the operands' limb count
    return PZ_OK;
}
// cells of assign_integer(Ln limbs); a full-width integer (2 Ln limbs) takes twice as many
static size_t asg_adv(const CircP& C) { return (size_t)C.Ln * (1 + C.rc_adv); }
static size_t asg_lk(const CircP& C) { return (size_t)C.Ln * C.rc_lk; }
// assert_equal_fresh of two integers of nf limbs
static size_t equal_cells(size_t nf) { return 2 + 16 * nf; }
// a result block: assign_integer(2 Ln limbs) + assert_equal_fresh
static size_t res_cells(const CircP& C) { return 2 * asg_adv(C) + equal_cells(C.nf); }
// the n_in Ln-limb inputs that head every stream
static void assign_inputs(CircP& C, unsigned n_in, size_t& a, size_t& l) {
    C.n_in = n_in;
    for (unsigned k = 0; k < n_in; ++k) { C.a_assign[k] = a; C.l_assign[k] = l; a += asg_adv(C); l += asg_lk(C); }
}
static size_t square_cells(uint32_t limbs) {
    size_t a = 1;
    for (unsigned i = 0; i + 1 < 2 * limbs; ++i) a += 1 + 3 * ((size_t)i + 1);
    return a;
}
static void refresh_cells(const unsigned char* inc, unsigned nf, unsigned rc_adv, unsigned rc_lk, size_t& a, size_t& l) {
    a += 1;
    for (unsigned i = 0; i < nf; ++i) a += ((size_t)inc[i] + 1) * 22 + (size_t)inc[i] * 4;
    a += (size_t)nf * rc_adv;
    l += (size_t)nf * rc_lk;
}
// square(n) and refresh at the running offsets (a, l), which move past them
static void square_refresh_cells(CircP& C, size_t& a, size_t& l) {
    C.a_square = a;
    a += square_cells(C.Ln);
    C.a_refresh = a; C.l_refresh = l;
    refresh_cells(C.inc, C.nf, C.rc_adv, C.rc_lk, a, l);
}
// load_zero at the running offset
static void load_zero_cell(CircP& C, size_t& a) {
    C.has_zero = true;
    C.a_zero = a;
    a += 1;
}
// an exponent bit of a chain: mul_mod, select (8 cells per limb), square_mod
static size_t bit_stride(const CircP& C) { return 2 * C.e.cells + 8 * (size_t)C.e.L; }
// `count` result blocks at the running offsets, their res_i side by side from word in_res of `inputs`; the misc kernel writes none
static void result_blocks(CircP& C, ResP& R, size_t count, size_t in_res, size_t& a, size_t& l) {
    C.no_res = true;
    R.in_res = in_res; R.in_stride = C.e.L64;
    R.a_res = a; R.l_res = l; R.res_stride = res_cells(C);
    a += count * R.res_stride; l += count * 2 * asg_lk(C);
}

static int make_circuit_params(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t ng, size_t nr, CircP& C,
                               size_t* adv_total, size_t* lk_total, size_t step_off[3]) {
    if (kind < 0 || kind > 5) return PZ_ERR_INVALID;
    if (kind == 5) kind = 2;   // "decrypt": kind 2's cells exactly (its statement alone differs: pz_circuit_public_cells)
    if (kind == 3 && (ng < 1 || ng > PZ_TALLY_MAX - 1 || nr)) return PZ_ERR_INVALID;   // the tally of ng + 1 ciphertexts: ng mul_mod blocks
    // the weighted tally of B = nr + 1 ciphertexts: nr tree blocks, ng = 2 B W chain records
    if (kind == 4 && (nr > PZ_TALLY_MAX - 1 || ng == 0 || ng % (2 * (nr + 1)) || ng / (2 * (nr + 1)) > PZ_WORD_BITS_MAX)) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, (unsigned)kind, C));
    size_t a = 0, l = 0;
    const size_t asg_a = asg_adv(C), asg_l = asg_lk(C);
    assign_inputs(C, kind >= 3 ? 1 : 4, a, l);
    C.res_off = 4 * (size_t)C.words_n;
    if (kind >= 3) {   // n | c_1 .. c_B | res: the ciphertexts are full-width integers (2 Ln limbs)
        C.n_cts = kind == 3 ? ng + 1 : nr + 1;
        C.a_cts = a; C.l_cts = l;
        a += C.n_cts * 2 * asg_a; l += C.n_cts * 2 * asg_l;
        C.res_off = C.words_n + C.n_cts * (size_t)C.e.L64;
        if (kind == 4) {   // ... | w_1 .. w_B | res: one 64-bit word and one load_witness cell per weight
            C.w_bits = (unsigned)(ng / (2 * C.n_cts));
            C.a_wts = a;
            a += C.n_cts;
            C.res_off += C.n_cts;
        }
    }
    square_refresh_cells(C, a, l);
    size_t lstep[3] = {0, 0, 0};
    if (kind < 3) load_zero_cell(C, a);   // (the tallies extend nothing: no load_zero, no pow_mod_fixed_exp constants)
    if (kind == 0) {
        C.a_pow[0] = a; a += 2; step_off[0] = a; lstep[0] = l; a += ng * C.e.cells; l += ng * C.e.lookups;
        C.a_pow[1] = a; a += 2; step_off[1] = a; lstep[1] = l; a += nr * C.e.cells; l += nr * C.e.lookups;
    } else if (kind == 2) {
        // uniform shape: per limb of m [num_to_bits | per bit: mul_mod, select (8 cells per limb), square_mod]
        const size_t m_bits = (size_t)limbs_n * limb_bits;
        if (ng != 2 * m_bits) return PZ_ERR_INVALID;
        C.a_pow[0] = a; a += 2; step_off[0] = a; lstep[0] = l;
        a += (size_t)limbs_n * nbits_cells(limb_bits) + m_bits * bit_stride(C);
        l += ng * C.e.lookups;
        C.a_pow[1] = a; a += 2; step_off[1] = a; lstep[1] = l; a += nr * C.e.cells; l += nr * C.e.lookups;
    } else if (kind == 3) {   // the product tree's ng blocks, in record order; no further step
        step_off[0] = a; lstep[0] = l; a += ng * C.e.cells; l += ng * C.e.lookups;
    } else if (kind == 4) {
        // per chain [1, 0 | num_to_bits | per bit: mul_mod, select (8 cells per limb), square_mod]; step_off[0] is the FIRST CHAIN'S
        // HEAD (its [1, 0]); then the tree's nr blocks in record order
        const size_t W = C.w_bits;
        step_off[0] = a; lstep[0] = l;
        a += C.n_cts * (2 + nbits_cells(W) + W * bit_stride(C));
        l += ng * C.e.lookups;
        step_off[1] = a; lstep[1] = l; a += nr * C.e.cells; l += nr * C.e.lookups;
    } else if (ng || nr) return PZ_ERR_INVALID;
    step_off[2] = a; lstep[2] = l;
    if (kind < 3) { a += C.e.cells; l += C.e.lookups; }
    C.a_res = a; C.l_res = l;
    a += res_cells(C); l += 2 * asg_l;
    *adv_total = a;
    *lk_total = l;
    // step_off[0..2]: advice offsets of the three runs of mul_mod steps (g^m, r^n, final); [3..5]: their lookup offsets
    memcpy(step_off + 3, lstep, sizeof lstep);
    return PZ_OK;
}

// RefreshAux::new(limb_bits, l, r).increased_limbs_vec for the host mirror (paillier.rs:40-44)
extern "C" int pz_refresh_aux(uint32_t limb_bits, uint32_t num_limbs_l, uint32_t num_limbs_r, uint8_t* increased_limbs,
                              uint32_t capacity, uint32_t* n_out) {
    if (!increased_limbs || !n_out || limb_bits < 16 || limb_bits > 90 || !num_limbs_l || !num_limbs_r) return PZ_ERR_INVALID;
    unsigned char inc[CIRC_MAXF];
    unsigned n = 0;
    PZCHK(refresh_aux_host(limb_bits, num_limbs_l, num_limbs_r, inc, &n));
    if (n > capacity) return PZ_ERR_CAPACITY;
    memcpy(increased_limbs, inc, n);
    *n_out = n;
    return PZ_OK;
}

// cells one chip operation pushes (the terms pz_circuit_cells sums): op 0 assign_integer(limbs), 1 square(limbs),
// 2 refresh of a limbs x limbs product, 3 load_zero / load_constant (one cell), 4 mul_mod(limbs), 5 assert_equal_fresh(limbs)
extern "C" int pz_op_cells(int op, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits, size_t* advice_cells,
                           size_t* lookup_cells) {
    size_t a = 0, l = 0;
    unsigned k, rem, rc_a, rc_l;
    if (limb_bits < 16 || limb_bits > 90 || lookup_bits < 4 || lookup_bits > 32) return PZ_ERR_INVALID;
    rc_counts(limb_bits, lookup_bits, k, rem, rc_a, rc_l);
    switch (op) {
        case 0: a = (size_t)limbs * (1 + rc_a); l = (size_t)limbs * rc_l; break;
        case 1: a = square_cells(limbs); break;
        case 2: {
            unsigned char inc[CIRC_MAXF];
            unsigned n = 0;
            PZCHK(refresh_aux_host(limb_bits, limbs, limbs, inc, &n));
            refresh_cells(inc, n, rc_a, rc_l, a, l);
            break;
        }
        case 3: a = 1; break;
        case 4: {
            ExpP P;
            PZCHK(make_params(limbs, limb_bits, lookup_bits, P));
            a = P.cells;
            l = P.lookups;
            break;
        }
        case 5: a = equal_cells(limbs); break;
        default: return PZ_ERR_INVALID;
    }
    return put_cells(PZ_OK, a, l, advice_cells, lookup_cells);
}

extern "C" int pz_circuit_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g,
                                size_t n_steps_r, size_t* advice_cells, size_t* lookup_cells) {
    CircP C;
    size_t a, l, so[6];
    const int rc = make_circuit_params(kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r, C, &a, &l, so);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

// halo2-lib's column break rule (assign_with_constraints of the dependency [D]), from the selector mask of the advice stream: walking
// the stream with row_offset r inside the current column, cell i is placed at (column, r); then, if (q[i] && r + 4 > max_rows) ||
// r >= max_rows - 1, the column ends with this cell, the next column starts with a COPY of it at row 0 (tied by an equality
// constraint) and -- if q[i] -- its gate is enabled there, not in the column it left.  starts[j] = the stream index of column j's row 0.
extern "C" int pz_circuit_break_points(const uint8_t* gate_mask, size_t n_cells, size_t max_rows, uint64_t* starts_out, size_t capacity,
                                       size_t* n_cols) {
    if (!gate_mask || !n_cols || max_rows < 8) return PZ_ERR_INVALID;
    size_t cols = 0, s = 0;
    for (;;) {
        if (starts_out) {
            if (cols >= capacity) return PZ_ERR_CAPACITY;
            starts_out[cols] = s;
        }
        ++cols;
        // the column ends at the first i with (q[i] && i - s + 4 > max_rows) || i - s >= max_rows - 1
        size_t end = s + max_rows - 1;
        for (size_t i = s + max_rows - 3; i < s + max_rows - 1 && i < n_cells; ++i)
            if (gate_mask[i]) {
                // the dependency asserts that no gate started one or two cells earlier (overlaps are by exactly three cells)
                if ((i >= 1 && gate_mask[i - 1] && i - 1 > s) || (i >= 2 && gate_mask[i - 2] && i - 2 > s)) return PZ_ERR_UNSUPPORTED;
                end = i;
                break;
            }
        if (end >= n_cells) break;     // the stream ends inside this column
        s = end;
    }
    if (starts_out) {
        if (cols >= capacity) return PZ_ERR_CAPACITY;
        starts_out[cols] = n_cells;
    }
    *n_cols = cols;
    return PZ_OK;
}

// ---- what every expansion entry point takes besides its kind's own counts, and the steps all of them open with
struct ExpandArgs {
    pz_ctx* ctx;
    const uint64_t *inputs, *d_steps, *d_modulus;
    uint64_t *d_advice, *d_lookup;
    bool cols;                      // the break-point column form: d_col_starts is required and `rows` are the lookup columns' rows
    size_t rows, col_stride;
    const uint64_t* d_col_starts;
    size_t n_adv_cols, max_rows;
};
// the refusals in front of the kind's parameter builder
static int expand_check(const ExpandArgs& A) {
    if (A.cols && (!A.d_col_starts || A.rows == 0 || A.rows > A.col_stride)) return PZ_ERR_INVALID;
    if (!A.ctx || !A.inputs || !A.d_steps || !A.d_modulus || !A.d_advice) return PZ_ERR_INVALID;
    if ((A.rows == 0) != (A.col_stride == 0) || A.col_stride < A.rows) return PZ_ERR_INVALID;
    return PZ_OK;
}
// behind it: the column cut and the break points of the streams
static int expand_layout(const ExpandArgs& A, CircP& C) {
    C.e.rows = A.rows;
    C.e.pad = A.col_stride - A.rows;
    if (A.d_col_starts) {
        if (A.n_adv_cols == 0 || A.n_adv_cols > 0xffffffffu || A.max_rows < 8 || A.max_rows > A.col_stride) return PZ_ERR_INVALID;
        C.e.bp_starts = (const u64*)A.d_col_starts;
        C.e.bp_ncols = (unsigned)A.n_adv_cols;
        C.e.bp_div = A.max_rows - 1;
        C.e.bp_stride = A.col_stride;
    }
    return PZ_OK;
}
// `inputs` (in_words words) and then `tail` (tail_bytes bytes; the mix's switch bits) to the device, behind the kind's own checks of
// them.  `inputs` is the caller's (pageable) memory and may go away when the entry point returns: it goes through a pinned staging
// block of the context, so the copy is truly asynchronous and reads nothing of the caller's afterwards.  Kinds 0 to 2: a few hundred
// bytes.  Kind 3 carries the B ciphertexts (525 KB at B = 1024, 33 MB at B = 65536 for a 2048-bit key): one host memcpy of that size
// per call, and the staging block grows to it once (grow-only, so a second tally of the size allocates nothing)
static int expand_stage(const ExpandArgs& A, size_t in_words, const void* tail, size_t tail_bytes, const u64** d_in) {
    void* d;
    PZCHK(pz_ws_get(A.ctx, WS_MISC, in_words * 8 + tail_bytes + 64, &d));
    PZCHK(pz_upload_small_async(A.ctx, d, A.inputs, in_words * 8));
    if (tail_bytes) PZCHK(pz_upload_small_async(A.ctx, (char*)d + in_words * 8, tail, tail_bytes));
    *d_in = (const u64*)d;
    return PZ_OK;
}
// `chains` runs of n whole mul_mod blocks: run i starts at advice cell cell0 + i * chain_stride and expands the records
// rec0 + i * rec_stride .. of `recs`; a block's lookups are numbered by its record, from lk0
static void launch_runs(const ExpandArgs& A, const CircP& C, size_t cell0, size_t lk0, const u64* recs, size_t n, size_t chains = 1,
                        size_t chain_stride = 0, size_t rec_stride = 0, size_t rec0 = 0) {
    ExpP Q = C.e;
    Q.cell0 = cell0;
    Q.lk0 = lk0;
    if (rec_stride) { Q.chain_steps = n; Q.chain_stride = chain_stride; Q.chain_recs = rec_stride; Q.rec0 = rec0; }   // (else: one dense run)
    hipLaunchKernelGGL(k_witness_expand, dim3((unsigned)(chains * n)), dim3(EXP_THREADS), 0, A.ctx->stream, Q, recs, (const u64*)A.d_modulus,
                       (Fr*)A.d_advice, (Fr*)A.d_lookup);
}
// the (mul_mod, square_mod) record pairs of `chains` exponent chains of nbits bits: chain i's num_to_bits block stands at advice cell
// a_bits + i * chain_stride, its 2 nbits records from record i * rec_stride of `recs` on
static void launch_chains(const ExpandArgs& A, const CircP& C, size_t a_bits, size_t lk0, const u64* recs, size_t nbits, size_t chains,
                          size_t chain_stride, size_t rec_stride) {
    ExpP Q = C.e;
    Q.cell0 = a_bits + nbits_cells(nbits);
    Q.lk0 = lk0;
    Q.pair_stride = bit_stride(C);
    Q.odd_off = C.e.cells + 8 * (size_t)C.e.L;   // the square_mod of a pair: behind the mul_mod and the select
    Q.chain_steps = 2 * nbits;
    Q.chain_stride = chain_stride;
    Q.chain_recs = rec_stride;
    hipLaunchKernelGGL(k_witness_expand, dim3((unsigned)(chains * 2 * nbits)), dim3(EXP_THREADS), 0, A.ctx->stream, Q, recs,
                       (const u64*)A.d_modulus, (Fr*)A.d_advice, (Fr*)A.d_lookup);
}
// the hs-chains of `count` entries (pow_mod(hs, s_i) limb by limb of s_i: kinds 9, 10 and 11): per entry s_i's num_to_bits and the
// selects; then limb by limb the record pairs of ALL entries in one launch.  s_i: s_words words from word in_ss + i s_words of the staged
// inputs; entry i's first num_to_bits block stands at advice cell bits0 + i cell_stride, its chain's records run from record
// rec0 + i rec_stride -- limb li's start 2 li W further, and so do their lookups behind lk0
static void launch_hs_chains(const ExpandArgs& A, const CircP& C, const u64* in, size_t in_ss, size_t s_limbs, size_t s_words, size_t count,
                             size_t bits0, size_t cell_stride, size_t lk0, const u64* recs, size_t rec0, size_t rec_stride) {
    const size_t W = C.e.W, rec = 4 * (size_t)C.e.L64, limb_stride = nbits_cells(W) + W * bit_stride(C);
    for (size_t i = 0; i < count; ++i) {
        const u64 *d_s = in + in_ss + i * s_words, *d_chain = recs + (i * rec_stride + rec0) * rec;
        hipLaunchKernelGGL(k_circuit_bits, dim3((unsigned)s_limbs), dim3(256), 0, A.ctx->stream, C.e, (unsigned)s_limbs, (unsigned)s_words, d_s,
                           bits0 + i * cell_stride, limb_stride, (Fr*)A.d_advice);
        hipLaunchKernelGGL(k_circuit_select, dim3((unsigned)(s_limbs * W)), dim3(256), 0, A.ctx->stream, C.e, (unsigned)s_limbs, (unsigned)s_words,
                           d_s, d_chain, bits0 + i * cell_stride, limb_stride, bit_stride(C), nbits_cells(W), (Fr*)A.d_advice);
    }
    for (size_t li = 0; li < s_limbs; ++li) {
        const size_t r0 = rec0 + li * 2 * W;
        launch_chains(A, C, bits0 + li * limb_stride, lk0 + r0 * C.e.lookups, recs + r0 * rec, W, count, cell_stride, rec_stride);
    }
}
// num_to_bits of a short exponent's top limb cannot hold a bit at or above s_bits: s_i is the s_words words from word in_ss + i s_words
static int short_exp_check(const uint64_t* inputs, size_t in_ss, size_t s_words, size_t s_bits, size_t count) {
    if (s_bits & 63)
        for (size_t i = 0; i < count; ++i)
            if (inputs[in_ss + (i + 1) * s_words - 1] >> (s_bits & 63)) return PZ_ERR_MESSAGE_RANGE;
    return PZ_OK;
}
// a run of `count` assign_integer blocks of nl limbs each, the integers `words` words apart from word in_off of the staged inputs
static void launch_assign(const ExpandArgs& A, const CircP& C, const u64* in, size_t in_off, unsigned nl, unsigned words, size_t count, size_t a0,
                          size_t l0) {
    hipLaunchKernelGGL(k_circuit_assign_many, dim3((unsigned)count), dim3(256), 0, A.ctx->stream, C, nl, words, in + in_off, a0, l0, (Fr*)A.d_advice,
                       (Fr*)A.d_lookup);
}
// `count` result blocks with their heads (ResP); the ballot's sum takes 16 bytes of shared memory per message
static void launch_results(const ExpandArgs& A, const CircP& C, const ResP& R, size_t count, const u64* in, const u64* recs) {
    hipLaunchKernelGGL(k_circuit_results, dim3((unsigned)count), dim3(256), R.sum_n >= 2 ? R.sum_n * 16 : 0, A.ctx->stream, C, R, in, recs,
                       (Fr*)A.d_advice, (Fr*)A.d_lookup);
}

// ---- the by-kind circuits (kinds 0 .. 5): one result, written by k_circuit_misc.  Kind 2 (and 5): g^m as an exponent chain per limb of m;
// kind 3: B full-width ciphertexts and the product tree's blocks; kind 4: a one-word weight and a chain per ciphertext, then the tree
static int circuit_expand_impl(const ExpandArgs& A, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g,
                               size_t n_steps_r) {
    PZCHK(expand_check(A));
    if (kind == 5) kind = 2;   // the same cells from the same records (make_circuit_params)
    CircP C;
    size_t a, l, so[6];
    PZCHK(make_circuit_params(kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r, C, &a, &l, so));
    PZCHK(expand_layout(A, C));
    const u64* wts = kind == 4 ? A.inputs + C.res_off - C.n_cts : nullptr;   // the weights, one word each, in front of res
    if (kind == 4 && C.w_bits < 64)
        for (size_t i = 0; i < C.n_cts; ++i)
            if (wts[i] >> C.w_bits) return PZ_ERR_MESSAGE_RANGE;   // num_to_bits of such a weight cannot hold
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const u64* in;
    PZCHK(expand_stage(A, C.res_off + C.e.L64, nullptr, 0, &in));
    pz_timer tm(ctx, PZ_T_EXPAND);
    const u64* d_steps = A.d_steps;
    Fr* adv = (Fr*)A.d_advice;
    const size_t rec = 4 * (size_t)C.e.L64;   // words per step record
    const size_t runs[3] = {kind != 1 ? n_steps_g : 0, kind != 1 ? n_steps_r : 0, kind < 3 ? (size_t)1 : 0};
    size_t first = 0;
    for (int k = 0; k < 3; first += runs[k], ++k) {
        if (!runs[k]) continue;
        if (kind == 2 && k == 0) {
            // a num_to_bits block in front of every limb's W bits: the pairs are launched limb by limb
            const size_t W = limb_bits, limb_stride = nbits_cells(W) + W * bit_stride(C);
            const u64* d_m = in + 2 * (size_t)C.words_n;
            hipLaunchKernelGGL(k_circuit_bits, dim3(limbs_n), dim3(256), 0, ctx->stream, C.e, limbs_n, C.words_n, d_m, so[0], limb_stride, adv);
            hipLaunchKernelGGL(k_circuit_select, dim3((unsigned)(limbs_n * W)), dim3(256), 0, ctx->stream, C.e, limbs_n, C.words_n, d_m, d_steps, so[0],
                               limb_stride, bit_stride(C), nbits_cells(W), adv);
            for (unsigned li = 0; li < limbs_n; ++li)
                launch_chains(A, C, so[0] + li * limb_stride, so[3] + (size_t)li * 2 * W * C.e.lookups, d_steps + (size_t)li * 2 * W * rec, W, 1, 0,
                              2 * W);
        } else if (kind == 4 && k == 0) {
            // step_off[0] is the first chain's [1, 0]; one launch each for the heads, the selects and the 2 B W records, whatever B is
            const size_t W = C.w_bits, head = 2 + nbits_cells(W), chain_stride = head + W * bit_stride(C);
            const u64* d_w = in + C.res_off - C.n_cts;
            hipLaunchKernelGGL(k_circuit_bits_many, dim3((unsigned)C.n_cts), dim3(256), 0, ctx->stream, C.e, (unsigned)W, d_w, C.a_wts, so[0],
                               chain_stride, adv);
            hipLaunchKernelGGL(k_circuit_select_many, dim3((unsigned)(C.n_cts * W)), dim3(256), 0, ctx->stream, C.e, (unsigned)W, d_w, d_steps,
                               2 * W, so[0], chain_stride, bit_stride(C), head, adv);
            launch_chains(A, C, so[0] + 2, so[3], d_steps, W, C.n_cts, chain_stride, 2 * W);
        } else
            launch_runs(A, C, so[k], so[3 + k], d_steps + first * rec, runs[k]);
    }
    if (kind >= 3) launch_assign(A, C, in, C.words_n, C.nf, C.e.L64, C.n_cts, C.a_cts, C.l_cts);
    // the circuit's result c = remainder of the last step (the final mul_mod; the tally's root)
    const u64* d_c = d_steps + (first - 1) * rec + 3 * (size_t)C.e.L64;
    if (kind == 4 && C.n_cts == 1) {
        // one ciphertext has no tree: the result is the chain's last select output -- the product of the last (acc, sq) step where the
        // weight's top bit is set, its acc otherwise
        const bool top = (wts[0] >> (C.w_bits - 1)) & 1;
        d_c = d_steps + (n_steps_g - 2) * rec + (top ? 3 : 0) * (size_t)C.e.L64;
    }
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, d_c, adv, (Fr*)A.d_lookup);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_circuit_expand_dev(pz_ctx* ctx, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits,
                                     const uint64_t* inputs, const uint64_t* d_steps, size_t n_steps_g, size_t n_steps_r,
                                     const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows,
                                     size_t col_stride) {
    return circuit_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, kind, limbs_n,
                               limb_bits, lookup_bits, n_steps_g, n_steps_r);
}
extern "C" int pz_circuit_expand_cols_dev(pz_ctx* ctx, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits,
                                          const uint64_t* inputs, const uint64_t* d_steps, size_t n_steps_g, size_t n_steps_r,
                                          const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup,
                                          const uint64_t* d_col_starts, size_t n_adv_cols, size_t max_rows, size_t lookup_rows,
                                          size_t col_stride) {
    return circuit_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                               kind, limbs_n, limb_bits, lookup_bits, n_steps_g, n_steps_r);
}

// ---- the ballot (circuit kind 6): K ciphertexts under one key.  Stream: assign n, g; load_witness(m_1 .. m_K);
// K >= 2: FlexGate::sum (1 + 3 (K - 1) cells); assign r_1 .. r_K; square + refresh, load_zero; per entry [the chain of m_i, b bits |
// 1, 0 | nr x mul_mod | mul_mod]; per entry a result block (res_i against the remainder of the entry's last record).
// inputs: n | g | m_1 .. m_K (one word each) | r_1 .. r_K | res_1 .. res_K.  Records: entry-major, 2 b + nr + 1 each.
struct BallotP {
    size_t K, per, a_msgs, a_rs, l_rs, a_ent, l_ent, ent_stride, head;
    size_t in_ms, in_rs;   // word offsets inside `inputs`
    ResP res;              // with the sum: block 0 of k_circuit_results writes it
};
static int make_ballot_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, uint32_t m_bits, size_t n_steps_r, CircP& C,
                              BallotP& B, size_t* adv_total, size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX) || !pz_word_bits_ok(m_bits) || n_steps_r < 1 || n_steps_r > 0x7fffffffu) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 6, C));
    memset(&B, 0, sizeof B);
    B.K = count;
    B.per = 2 * (size_t)m_bits + n_steps_r + 1;
    B.in_ms = 2 * (size_t)C.words_n;
    B.in_rs = B.in_ms + count;
    size_t a = 0, l = 0;
    assign_inputs(C, 2, a, l);
    B.a_msgs = a; a += count;
    B.res.sum_n = count; B.res.in_ms = B.in_ms;
    B.res.a_sum = a; a += count >= 2 ? 1 + 3 * (count - 1) : 0;
    B.a_rs = a; B.l_rs = l; a += count * asg_adv(C); l += count * asg_lk(C);
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.head = 2 + nbits_cells(m_bits);
    B.ent_stride = B.head + m_bits * bit_stride(C) + 2 + (n_steps_r + 1) * C.e.cells;
    B.a_ent = a; B.l_ent = l;
    a += count * B.ent_stride; l += count * B.per * C.e.lookups;
    // the [1, 0] of r_i^n stands behind the g-chain
    B.res.a_head = B.a_ent + B.head + m_bits * bit_stride(C); B.res.head_stride = B.ent_stride;
    B.res.rec0 = B.per - 1; B.res.rec_stride = B.per; B.res.field = 3;
    result_blocks(C, B.res, count, B.in_rs + count * C.words_n, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}

extern "C" int pz_ballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_r,
                               size_t* advice_cells, size_t* lookup_cells) {
    CircP C;
    BallotP B;
    size_t a, l;
    const int rc = make_ballot_params(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int ballot_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                              size_t n_steps_r) {
    PZCHK(expand_check(A));
    CircP C;
    BallotP B;
    size_t a, l;
    PZCHK(make_ballot_params(limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r, C, B, &a, &l));
    PZCHK(expand_layout(A, C));
    if (m_bits < 64)
        for (size_t i = 0; i < count; ++i)
            if (A.inputs[B.in_ms + i] >> m_bits) return PZ_ERR_MESSAGE_RANGE;   // num_to_bits of such a message cannot hold
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const u64* in;
    PZCHK(expand_stage(A, B.res.in_res + count * C.e.L64, nullptr, 0, &in));
    pz_timer tm(ctx, PZ_T_EXPAND);
    const u64* d_steps = A.d_steps;
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    // n, g, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer(r_i): Ln limbs from words_n words each
    launch_assign(A, C, in, B.in_rs, C.Ln, C.words_n, count, B.a_rs, B.l_rs);
    // per entry: the load_witness cell and the chain's head; the selects; the g-chain's record pairs; the r-chain's and the final record
    hipLaunchKernelGGL(k_circuit_bits_many, dim3((unsigned)count), dim3(256), 0, ctx->stream, C.e, m_bits, in + B.in_ms, B.a_msgs, B.a_ent,
                       B.ent_stride, adv);
    hipLaunchKernelGGL(k_circuit_select_many, dim3((unsigned)(count * m_bits)), dim3(256), 0, ctx->stream, C.e, m_bits, in + B.in_ms, d_steps,
                       B.per, B.a_ent, B.ent_stride, bit_stride(C), B.head, adv);
    launch_chains(A, C, B.a_ent + 2, B.l_ent, d_steps, m_bits, count, B.ent_stride, B.per);
    launch_runs(A, C, B.res.a_head + 2, B.l_ent, d_steps, n_steps_r + 1, count, B.ent_stride, B.per, 2 * (size_t)m_bits);
    launch_results(A, C, B.res, count, in, d_steps);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_ballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                                    size_t n_steps_r, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                                    uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return ballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                              lookup_bits, count, m_bits, n_steps_r);
}
extern "C" int pz_ballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                                         size_t n_steps_r, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                                         uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts, size_t n_adv_cols,
                                         size_t max_rows, size_t lookup_rows, size_t col_stride) {
    return ballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                              limbs_n, limb_bits, lookup_bits, count, m_bits, n_steps_r);
}

// ---- a trustee's partial decryptions (circuit kind 7): K ciphertexts opened under ONE share theta.  Stream:
// assign n; assign v, theta, c_1 .. c_K at full width; square + refresh, load_zero; chain 0 = pow_mod(v, theta) as kind 2 emits it
// ([1, 0], then per limb of theta a chain of W bits) over ALL 2 Ln limbs; per ciphertext the block mul_mod(c_j, c_j) and chain j =
// pow_mod(s_j, theta); then K + 1 result blocks: h, u_1 .. u_K against the chains' results, each taken from its chain's last
// (acc, sq) record -- the product where theta's top bit is set, the accumulator otherwise.
// inputs: n | v | theta | c_1 .. c_K | h | u_1 .. u_K.  Records (pz_paillier_partial_dev): the K squarings, then chain i at K + i 2 E,
// E = 2 Ln W bits.  Lookups follow the STREAM: chain 0's, then per ciphertext its squaring's and its chain's.
struct PartialP {
    size_t K, E, a_wide, l_wide, a_ch, l_ch, limb_stride, chain_cells;
    size_t in_v, in_theta;   // word offsets inside `inputs`
    ResP res;
};
static int make_partial_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, CircP& C, PartialP& B, size_t* adv_total,
                               size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX)) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 7, C));
    memset(&B, 0, sizeof B);
    const size_t W = limb_bits, L = C.e.L;
    B.K = count;
    B.E = L * W;
    B.in_v = C.words_n;
    B.in_theta = B.in_v + C.e.L64;
    size_t a = 0, l = 0;
    assign_inputs(C, 1, a, l);
    B.a_wide = a; B.l_wide = l;
    a += (count + 2) * 2 * asg_adv(C); l += (count + 2) * 2 * asg_lk(C);
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.limb_stride = nbits_cells(W) + W * bit_stride(C);
    B.chain_cells = 2 + L * B.limb_stride;
    B.a_ch = a; B.l_ch = l;
    a += (count + 1) * B.chain_cells + count * C.e.cells;
    l += (count + (count + 1) * 2 * B.E) * C.e.lookups;
    B.res.a_head = B.a_ch; B.res.head_stride = B.chain_cells + C.e.cells;
    B.res.rec0 = count + 2 * B.E - 2; B.res.rec_stride = 2 * B.E;   // (the field depends on theta: partial_expand_impl)
    result_blocks(C, B.res, count + 1, B.in_theta + (1 + count) * C.e.L64, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}

extern "C" int pz_partial_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t* advice_cells,
                                size_t* lookup_cells) {
    CircP C;
    PartialP B;
    size_t a, l;
    const int rc = make_partial_params(limbs_n, limb_bits, lookup_bits, count, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int partial_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count) {
    PZCHK(expand_check(A));
    CircP C;
    PartialP B;
    size_t a, l;
    PZCHK(make_partial_params(limbs_n, limb_bits, lookup_bits, count, C, B, &a, &l));
    PZCHK(expand_layout(A, C));
    const size_t E = B.E, L64 = C.e.L64;
    const u64* theta = A.inputs + B.in_theta;
    for (size_t k = E / 64; k < L64; ++k)   // theta >= 2^E: num_to_bits of its limbs cannot hold
        if (k == E / 64 ? theta[k] >> (E & 63) : theta[k]) return PZ_ERR_MESSAGE_RANGE;
    B.res.field = (theta[(E - 1) / 64] >> ((E - 1) & 63)) & 1 ? 3 : 0;
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const u64* in;
    PZCHK(expand_stage(A, B.res.in_res + (count + 1) * L64, nullptr, 0, &in));
    pz_timer tm(ctx, PZ_T_EXPAND);
    const u64* d_steps = A.d_steps;
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    const size_t rec = 4 * L64;   // words per step record
    const unsigned W = limb_bits, Lf = C.e.L;
    // n, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer of v, theta and the c_j: 2 Ln limbs from L64 words each
    launch_assign(A, C, in, B.in_v, C.nf, (unsigned)L64, count + 2, B.a_wide, B.l_wide);
    // chain by chain (kind 2's walk, limb by limb inside one launch): the squaring block in front of it, theta's num_to_bits per limb, the
    // selects, the chain's 2 E records in (mul_mod, square_mod) pairs
    for (size_t i = 0; i <= count; ++i) {
        const size_t head = B.a_ch + i * (B.chain_cells + C.e.cells), lk_chain = B.l_ch + i * (2 * E + 1) * C.e.lookups;
        const u64* d_chain = d_steps + (count + i * 2 * E) * rec;
        if (i) launch_runs(A, C, head - C.e.cells, lk_chain - C.e.lookups, d_steps + (i - 1) * rec, 1);
        hipLaunchKernelGGL(k_circuit_bits, dim3(Lf), dim3(256), 0, ctx->stream, C.e, Lf, (unsigned)L64, in + B.in_theta, head + 2, B.limb_stride,
                           adv);
        hipLaunchKernelGGL(k_circuit_select, dim3((unsigned)E), dim3(256), 0, ctx->stream, C.e, Lf, (unsigned)L64, in + B.in_theta, d_chain,
                           head + 2, B.limb_stride, bit_stride(C), nbits_cells(W), adv);
        launch_chains(A, C, head + 2, lk_chain, d_chain, W, Lf, B.limb_stride, 2 * (size_t)W);
    }
    launch_results(A, C, B.res, count + 1, in, d_steps);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_partial_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count,
                                     const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice,
                                     uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return partial_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                               lookup_bits, count);
}
extern "C" int pz_partial_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count,
                                          const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice,
                                          uint64_t* d_lookup, const uint64_t* d_col_starts, size_t n_adv_cols, size_t max_rows,
                                          size_t lookup_rows, size_t col_stride) {
    return partial_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                               limbs_n, limb_bits, lookup_bits, count);
}

// ---- the mix (circuit kind 8): K = 2^d ciphertexts through the Benes network, then c'_i = d_i r_i^n mod n^2.
// Stream: assign n; assign c_1 .. c_K at full width; assign r_1 .. r_K; square + refresh, load_zero; per layer and switch [0, b, b, b]
// and per limb select(in[j'], in[j], b), select(in[j], in[j'], b); per output [1, 0 | nr x mul_mod | mul_mod]; per output a result
// block (res_i against the remainder of the output's last record).  inputs: n | c_1 .. c_K | r_1 .. r_K | res_1 .. res_K.  Routes,
// bits and records are pz_paillier_mix_dev's, as it leaves them: fields of 2 ceil(Ln W / 64) words.
struct MixP {
    size_t K, half, layers, per, a_cts, l_cts, a_rs, l_rs, a_net, sw_cells, a_out, l_out, out_stride;
    size_t in_cts, in_rs;           // word offsets inside `inputs`
    unsigned d, rw;                 // log2 K; words per field of a route or record as K3 writes them
    ResP res;
};
static int make_mix_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, size_t n_steps_r, CircP& C, MixP& B,
                           size_t* adv_total, size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX) || (count & (count - 1)) != 0 || n_steps_r < 1 || n_steps_r > 0x7fffffffu) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 8, C));
    memset(&B, 0, sizeof B);
    B.K = count; B.half = count / 2; B.per = n_steps_r + 1; B.rw = 2 * C.words_n;
    while (((size_t)1 << B.d) < count) ++B.d;
    B.layers = count > 1 ? 2 * (size_t)B.d - 1 : 0;
    B.in_cts = C.words_n;
    B.in_rs = B.in_cts + count * C.e.L64;
    size_t a = 0, l = 0;
    assign_inputs(C, 1, a, l);
    B.a_cts = a; B.l_cts = l; a += count * 2 * asg_adv(C); l += count * 2 * asg_lk(C);
    B.a_rs = a; B.l_rs = l; a += count * asg_adv(C); l += count * asg_lk(C);
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.sw_cells = 4 + 16 * (size_t)C.e.L;
    B.a_net = a; a += B.layers * B.half * B.sw_cells;
    B.out_stride = 2 + B.per * C.e.cells;
    B.a_out = a; B.l_out = l;
    a += count * B.out_stride; l += count * B.per * C.e.lookups;
    B.res.a_head = B.a_out; B.res.head_stride = B.out_stride;
    B.res.rec0 = B.per - 1; B.res.rec_stride = B.per; B.res.field = 3;
    result_blocks(C, B.res, count, B.in_rs + count * C.words_n, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}
// one thread per (switch, limb): the limb's two selects -- [d | 1 | y | x | y | b | d | out] for (x, y) = (in[j'], in[j]) and then for
// (in[j], in[j']) -- and, from the thread of limb 0, the switch's [0, b, b, b].  in: the layer below (layer 0: the ciphertexts inside
// `inputs`, fields of in_words words), out: this layer of the routes; bits: this layer's.
__global__ __launch_bounds__(256) void k_mix_switch(ExpP P, unsigned beta, unsigned half, const u64* __restrict__ in, unsigned in_words,
                                                    const u64* __restrict__ out, unsigned out_words, const unsigned char* __restrict__ bits,
                                                    size_t cell_base, size_t sw_cells, Fr* __restrict__ advice) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned L = P.L, W = P.W;
    if (g >= (size_t)half * L) return;
    const unsigned s = (unsigned)(g / L), t = (unsigned)(g % L);
    const size_t j = ((size_t)(s >> beta) << (beta + 1)) | (s & ((1u << beta) - 1u)), jp = j | ((size_t)1 << beta);
    const unsigned b = bits[s];
    const Fr fb = fr_from_u(u_make(b));
    const CellPtr a = adv_ptr(P, advice, cell_base + (size_t)s * sw_cells);
    if (t == 0) {
        fp_store(a, fp_zero<FrTag>());
        fp_store(a + 1, fb);
        fp_store(a + 2, fb);
        fp_store(a + 3, fb);
    }
    u64 w[4][2];
    limb_extract(in + j * in_words, in_words, t, W, w[0]);
    limb_extract(in + jp * in_words, in_words, t, W, w[1]);
    limb_extract(out + j * out_words, out_words, t, W, w[2]);
    limb_extract(out + jp * out_words, out_words, t, W, w[3]);
    const U192 vj = u_make(w[0][0], w[0][1]), vjp = u_make(w[1][0], w[1][1]);
    const Fr fj = fr_from_u(vj), fjp = fr_from_u(vjp), d = fr_from_s(s_sub(vjp, vj)), nd = fr_from_s(s_sub(vj, vjp)), one = fp_one<FrTag>();
    const CellPtr c = a + 4 + 16 * (size_t)t;
    fp_store(c, d);      fp_store(c + 1, one); fp_store(c + 2, fj);   fp_store(c + 3, fjp);
    fp_store(c + 4, fj); fp_store(c + 5, fb);  fp_store(c + 6, d);    fp_store(c + 7, fr_from_u(u_make(w[2][0], w[2][1])));
    fp_store(c + 8, nd);   fp_store(c + 9, one); fp_store(c + 10, fjp); fp_store(c + 11, fj);
    fp_store(c + 12, fjp); fp_store(c + 13, fb); fp_store(c + 14, nd);  fp_store(c + 15, fr_from_u(u_make(w[3][0], w[3][1])));
}
// the records' fields from rw words (as K3 writes them) to L64 (as k_witness_expand reads them), where the two differ
__global__ __launch_bounds__(256) void k_mix_repack(const u64* __restrict__ src, unsigned rw, u64* __restrict__ dst, unsigned L64, size_t fields) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= fields * L64) return;
    const size_t f = g / L64;
    const unsigned k = (unsigned)(g % L64);
    dst[g] = k < rw ? src[f * rw + k] : 0;
}
// *recs (`fields` fields of rw words, as K3 leaves them) as k_witness_expand reads them: K3's fields are whole words of n twice over,
// K4's are the words 2 Ln limbs take; where the two differ the records are repacked into the workspace first
static int repack_records(pz_ctx* ctx, const CircP& C, unsigned rw, size_t fields, const u64** recs) {
    if (rw == C.e.L64) return PZ_OK;
    void* t;
    PZCHK(pz_ws_get(ctx, WS_BIG_C, fields * C.e.L64 * 8, &t));
    hipLaunchKernelGGL(k_mix_repack, dim3((unsigned)((fields * C.e.L64 + 255) / 256)), dim3(256), 0, ctx->stream, *recs, rw, (u64*)t, C.e.L64, fields);
    *recs = (const u64*)t;
    return PZ_OK;
}
// the network of kinds 8 and 10 over K = 2^d positions, layer by layer: a layer reads the one below (layer 0: the ciphertexts inside
// the staged inputs, fields of L64 words) and its own, both of the routes at rw words a field; its switches' cells start at a_net
static void launch_network(const ExpandArgs& A, const CircP& C, const u64* in_cts, const uint64_t* d_routes, const unsigned char* d_bits, size_t K,
                           unsigned d, size_t layers, unsigned rw, size_t a_net, size_t sw_cells) {
    const size_t half = K / 2, layer_words = K * rw;
    for (size_t ly = 0; ly < layers; ++ly) {
        const unsigned beta = (unsigned)(ly < d ? ly : layers - 1 - ly);
        const u64* below = ly ? (const u64*)d_routes + (ly - 1) * layer_words : in_cts;
        hipLaunchKernelGGL(k_mix_switch, dim3((unsigned)((half * C.e.L + 255) / 256)), dim3(256), 0, A.ctx->stream, C.e, beta, (unsigned)half, below,
                           ly ? rw : C.e.L64, (const u64*)d_routes + ly * layer_words, rw, d_bits + ly * half, a_net + ly * half * sw_cells, sw_cells,
                           (Fr*)A.d_advice);
    }
}
extern "C" int pz_mix_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r, size_t* advice_cells,
                            size_t* lookup_cells) {
    CircP C;
    MixP B;
    size_t a, l;
    const int rc = make_mix_params(limbs_n, limb_bits, lookup_bits, count, n_steps_r, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int mix_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                           const uint8_t* bits, const uint64_t* d_routes) {
    PZCHK(expand_check(A));
    CircP C;
    MixP B;
    size_t a, l;
    PZCHK(make_mix_params(limbs_n, limb_bits, lookup_bits, count, n_steps_r, C, B, &a, &l));
    if (B.layers && (!bits || !d_routes)) return PZ_ERR_INVALID;
    PZCHK(expand_layout(A, C));
    const size_t n_switch = B.layers * B.half;
    for (size_t i = 0; i < n_switch; ++i)
        if (bits[i] > 1) return PZ_ERR_MESSAGE_RANGE;   // assert_bit of such a byte cannot hold
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const size_t in_words = B.res.in_res + count * C.e.L64;
    const u64* in;
    PZCHK(expand_stage(A, in_words, bits, n_switch, &in));   // the switch bits behind the inputs
    const unsigned char* d_bits = (const unsigned char*)(in + in_words);
    const u64* recs = A.d_steps;
    PZCHK(repack_records(ctx, C, B.rw, count * B.per * 4, &recs));
    pz_timer tm(ctx, PZ_T_EXPAND);
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    // n, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer(c_j): 2 Ln limbs from L64 words each; assign_integer(r_i): Ln limbs from words_n words each
    launch_assign(A, C, in, B.in_cts, C.nf, C.e.L64, count, B.a_cts, B.l_cts);
    launch_assign(A, C, in, B.in_rs, C.Ln, C.words_n, count, B.a_rs, B.l_rs);
    launch_network(A, C, in + B.in_cts, d_routes, d_bits, count, B.d, B.layers, B.rw, B.a_net, B.sw_cells);
    // per output: the r-chain's records and the final one
    launch_runs(A, C, B.a_out + 2, B.l_out, recs, B.per, count, B.out_stride, B.per);
    launch_results(A, C, B.res, count, in, recs);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_mix_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                                 const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                                 const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return mix_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                           lookup_bits, count, n_steps_r, bits, d_routes);
}
extern "C" int pz_mix_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                                      const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                                      const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                                      size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride) {
    return mix_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                           limbs_n, limb_bits, lookup_bits, count, n_steps_r, bits, d_routes);
}

// ---- the short-randomness ballot (circuit kind 9): K ciphertexts c_i = g^m_i hs^s_i mod n^2 under one key.
// Stream: assign n, g; assign hs at full width; load_witness(m_1 .. m_K); K >= 2: FlexGate::sum; assign s_1 .. s_K (s_limbs limbs
// each); square + refresh, load_zero; per entry [the chain of m_i, b bits, as kind 6 | pow_mod(hs, s_i) as kind 7 emits a chain: 1, 0,
// then per limb of s_i num_to_bits and W bit blocks | mul_mod(gm_i, hss_i)]; per entry a result block (res_i against the remainder of
// the entry's last record).  inputs: n | g | hs (L64 words) | m_1 .. m_K (one word each) | s_1 .. s_K (ceil(s_limbs W / 64) words
// each) | res_1 .. res_K.  Records are pz_paillier_sballot_dev's, as it leaves them: entry-major, 2 b + 2 s_limbs W + 1 each, fields
// of 2 ceil(Ln W / 64) words.  No arithmetic of its own: the bits, select, expand, assign and result kernels above.
struct SballotP {
    size_t K, per, s_limbs, s_words, a_hs, l_hs, a_msgs, a_ss, l_ss, a_ent, l_ent, ent_stride, head, g_cells, limb_stride;
    size_t in_hs, in_ms, in_ss;   // word offsets inside `inputs`
    unsigned rw;                  // words per field of a record as K3 writes them
    ResP res;                     // with the sum: block 0 of k_circuit_results writes it
};
static int make_sballot_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, uint32_t m_bits, uint32_t s_limbs, CircP& C,
                               SballotP& B, size_t* adv_total, size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX) || !pz_word_bits_ok(m_bits) || !pz_short_exp_ok(s_limbs, limbs_n)) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 9, C));
    memset(&B, 0, sizeof B);
    const size_t W = limb_bits, s_bits = (size_t)s_limbs * W;
    B.K = count;
    B.s_limbs = s_limbs;
    B.s_words = (s_bits + 63) / 64;
    B.per = 2 * (size_t)m_bits + 2 * s_bits + 1;
    B.rw = 2 * C.words_n;
    B.in_hs = 2 * (size_t)C.words_n;
    B.in_ms = B.in_hs + C.e.L64;
    B.in_ss = B.in_ms + count;
    size_t a = 0, l = 0;
    assign_inputs(C, 2, a, l);
    B.a_hs = a; B.l_hs = l; a += 2 * asg_adv(C); l += 2 * asg_lk(C);
    B.a_msgs = a; a += count;
    B.res.sum_n = count; B.res.in_ms = B.in_ms;
    B.res.a_sum = a; a += count >= 2 ? 1 + 3 * (count - 1) : 0;
    B.a_ss = a; B.l_ss = l;
    a += count * s_limbs * (1 + (size_t)C.rc_adv); l += count * s_limbs * (size_t)C.rc_lk;
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.head = 2 + nbits_cells(m_bits);
    B.g_cells = B.head + m_bits * bit_stride(C);
    B.limb_stride = nbits_cells(W) + W * bit_stride(C);
    B.ent_stride = B.g_cells + 2 + s_limbs * B.limb_stride + C.e.cells;
    B.a_ent = a; B.l_ent = l;
    a += count * B.ent_stride; l += count * B.per * C.e.lookups;
    // the [1, 0] of pow_mod(hs, s_i) stands behind the g-chain
    B.res.a_head = B.a_ent + B.g_cells; B.res.head_stride = B.ent_stride;
    B.res.rec0 = B.per - 1; B.res.rec_stride = B.per; B.res.field = 3;
    result_blocks(C, B.res, count, B.in_ss + count * B.s_words, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}

extern "C" int pz_sballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, uint32_t s_limbs,
                                size_t* advice_cells, size_t* lookup_cells) {
    CircP C;
    SballotP B;
    size_t a, l;
    const int rc = make_sballot_params(limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int sballot_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                               uint32_t s_limbs) {
    PZCHK(expand_check(A));
    CircP C;
    SballotP B;
    size_t a, l;
    PZCHK(make_sballot_params(limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs, C, B, &a, &l));
    PZCHK(expand_layout(A, C));
    for (size_t i = 0; i < count; ++i)   // num_to_bits of such a message cannot hold
        if (m_bits < 64 && A.inputs[B.in_ms + i] >> m_bits) return PZ_ERR_MESSAGE_RANGE;
    PZCHK(short_exp_check(A.inputs, B.in_ss, B.s_words, (size_t)s_limbs * limb_bits, count));
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const u64* in;
    PZCHK(expand_stage(A, B.res.in_res + count * C.e.L64, nullptr, 0, &in));
    const u64* recs = A.d_steps;
    PZCHK(repack_records(ctx, C, B.rw, count * B.per * 4, &recs));
    pz_timer tm(ctx, PZ_T_EXPAND);
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    // n, g, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer(hs): 2 Ln limbs from L64 words; assign_integer(s_i): s_limbs limbs from s_words words each
    launch_assign(A, C, in, B.in_hs, C.nf, C.e.L64, 1, B.a_hs, B.l_hs);
    launch_assign(A, C, in, B.in_ss, (unsigned)s_limbs, (unsigned)B.s_words, count, B.a_ss, B.l_ss);
    // the g-chains, as the ballot's: the load_witness cell and the chain's head; the selects; the record pairs
    hipLaunchKernelGGL(k_circuit_bits_many, dim3((unsigned)count), dim3(256), 0, ctx->stream, C.e, m_bits, in + B.in_ms, B.a_msgs, B.a_ent,
                       B.ent_stride, adv);
    hipLaunchKernelGGL(k_circuit_select_many, dim3((unsigned)(count * m_bits)), dim3(256), 0, ctx->stream, C.e, m_bits, in + B.in_ms, recs, B.per,
                       B.a_ent, B.ent_stride, bit_stride(C), B.head, adv);
    launch_chains(A, C, B.a_ent + 2, B.l_ent, recs, m_bits, count, B.ent_stride, B.per);
    // the hs-chains behind the g-chains: their records start 2 b into an entry's
    launch_hs_chains(A, C, in, B.in_ss, s_limbs, B.s_words, count, B.a_ent + B.g_cells + 2, B.ent_stride, B.l_ent, recs, 2 * (size_t)m_bits, B.per);
    // the final block of every entry, and the result blocks with the [1, 0] of the hs-chains
    launch_runs(A, C, B.a_ent + B.ent_stride - C.e.cells, B.l_ent, recs, 1, count, B.ent_stride, B.per, B.per - 1);
    launch_results(A, C, B.res, count, in, recs);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_sballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                                     uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                                     uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return sballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                               lookup_bits, count, m_bits, s_limbs);
}
extern "C" int pz_sballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                                          uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                                          uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts, size_t n_adv_cols,
                                          size_t max_rows, size_t lookup_rows, size_t col_stride) {
    return sballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                               limbs_n, limb_bits, lookup_bits, count, m_bits, s_limbs);
}

// ---- the packed ballot (circuit kind 11): R ciphertexts of K slots each, c_i = (prod_j G_j^v_ij) hs^s_i mod
// n^2 under one key and the public slot bases G_j.  Stream: assign n; assign hs, G_0 .. G_{K-1} at full width; load_witness of the R K
// values, ciphertext-major; K >= 2: one FlexGate::sum per ciphertext; assign s_1 .. s_R (s_limbs limbs each); square + refresh,
// load_zero; per ciphertext [per slot: 1, 0, num_to_bits(v_ij, b), b bit blocks as kind 6's g-chain | pow_mod(hs, s_i) as kind 9 |
// the K fold blocks]; per ciphertext a result block (res_i against the remainder of the entry's last record).  inputs: n | hs | G_0 ..
// G_{K-1} (L64 words each) | v_11 .. v_RK (one word each) | s_1 .. s_R (ceil(s_limbs W / 64) words each) | res_1 .. res_R.  Records are
// pz_paillier_pballot_dev's, as it leaves them: entry-major, 2 b K + 2 s_limbs W + K each.  One kernel of its own, the R sums; the
// rest are the bits, select, expand, assign and result kernels above.
struct PballotP {
    size_t R, K, per, s_limbs, s_words, a_hs, l_hs, a_vals, a_sum, sum_cells, a_ss, l_ss, a_ent, l_ent, ent_stride, head, g_cells, limb_stride;
    size_t in_hs, in_vs, in_ss;   // word offsets inside `inputs`
    unsigned rw;                  // words per field of a record as K3 writes them
    ResP res;                     // (no sum: k_pballot_sums writes the R of them)
};
// grid.x = ciphertext: FlexGate::sum over its K one-word values.  Dynamic shared memory: 16 bytes per value.
__global__ __launch_bounds__(256) void k_pballot_sums(ExpP P, const u64* __restrict__ vals, size_t K, size_t a_sum, size_t sum_cells,
                                                      Fr* __restrict__ advice) {
    extern __shared__ u64 s_pre[][2];
    const size_t i = blockIdx.x;
    flex_sum_cells(vals + i * K, K, s_pre, adv_ptr(P, advice, a_sum + i * sum_cells));
}
static int make_pballot_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, uint32_t slots, uint32_t m_bits,
                               uint32_t s_limbs, CircP& C, PballotP& B, size_t* adv_total, size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX) || !pz_slots_ok(count, slots)) return PZ_ERR_INVALID;
    if (!pz_word_bits_ok(m_bits) || !pz_short_exp_ok(s_limbs, limbs_n)) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 11, C));
    memset(&B, 0, sizeof B);
    const size_t W = limb_bits, s_bits = (size_t)s_limbs * W, K = slots;
    B.R = count;
    B.K = K;
    B.s_limbs = s_limbs;
    B.s_words = (s_bits + 63) / 64;
    B.per = 2 * (size_t)m_bits * K + 2 * s_bits + K;
    B.rw = 2 * C.words_n;
    B.in_hs = C.words_n;
    B.in_vs = B.in_hs + (1 + K) * C.e.L64;
    B.in_ss = B.in_vs + count * K;
    size_t a = 0, l = 0;
    assign_inputs(C, 1, a, l);
    B.a_hs = a; B.l_hs = l; a += (1 + K) * 2 * asg_adv(C); l += (1 + K) * 2 * asg_lk(C);
    B.a_vals = a; a += count * K;
    B.sum_cells = K >= 2 ? 1 + 3 * (K - 1) : 0;
    B.a_sum = a; a += count * B.sum_cells;
    B.a_ss = a; B.l_ss = l;
    a += count * s_limbs * (1 + (size_t)C.rc_adv); l += count * s_limbs * (size_t)C.rc_lk;
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.head = 2 + nbits_cells(m_bits);
    B.g_cells = B.head + m_bits * bit_stride(C);
    B.limb_stride = nbits_cells(W) + W * bit_stride(C);
    B.ent_stride = K * B.g_cells + 2 + s_limbs * B.limb_stride + K * C.e.cells;
    B.a_ent = a; B.l_ent = l;
    a += count * B.ent_stride; l += count * B.per * C.e.lookups;
    // the [1, 0] of pow_mod(hs, s_i) stands behind the K slot chains
    B.res.a_head = B.a_ent + K * B.g_cells; B.res.head_stride = B.ent_stride;
    B.res.rec0 = B.per - 1; B.res.rec_stride = B.per; B.res.field = 3;
    result_blocks(C, B.res, count, B.in_ss + count * B.s_words, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}

extern "C" int pz_pballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots, uint32_t m_bits,
                                uint32_t s_limbs, size_t* advice_cells, size_t* lookup_cells) {
    CircP C;
    PballotP B;
    size_t a, l;
    const int rc = make_pballot_params(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int pballot_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots,
                               uint32_t m_bits, uint32_t s_limbs) {
    PZCHK(expand_check(A));
    CircP C;
    PballotP B;
    size_t a, l;
    PZCHK(make_pballot_params(limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs, C, B, &a, &l));
    PZCHK(expand_layout(A, C));
    const size_t K = slots;
    for (size_t i = 0; i < count * K; ++i)   // num_to_bits of such a value cannot hold
        if (m_bits < 64 && A.inputs[B.in_vs + i] >> m_bits) return PZ_ERR_MESSAGE_RANGE;
    PZCHK(short_exp_check(A.inputs, B.in_ss, B.s_words, (size_t)s_limbs * limb_bits, count));
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const u64* in;
    PZCHK(expand_stage(A, B.res.in_res + count * C.e.L64, nullptr, 0, &in));
    const u64* recs = A.d_steps;
    PZCHK(repack_records(ctx, C, B.rw, count * B.per * 4, &recs));
    pz_timer tm(ctx, PZ_T_EXPAND);
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    const size_t rec = 4 * (size_t)C.e.L64;   // words per step record
    // n, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer(hs), assign_integer(G_j): 1 + K integers of 2 Ln limbs from L64 words each; assign_integer(s_i): s_limbs limbs
    launch_assign(A, C, in, B.in_hs, C.nf, C.e.L64, 1 + K, B.a_hs, B.l_hs);
    launch_assign(A, C, in, B.in_ss, (unsigned)s_limbs, (unsigned)B.s_words, count, B.a_ss, B.l_ss);
    if (K >= 2)
        hipLaunchKernelGGL(k_pballot_sums, dim3((unsigned)count), dim3(256), K * 16, ctx->stream, C.e, in + B.in_vs, K, B.a_sum, B.sum_cells, adv);
    // the slot chains of a ciphertext stand g_cells apart and their records 2 b apart: per ciphertext the K load_witness cells, heads
    // and num_to_bits, and the selects; then slot by slot the record pairs of ALL ciphertexts in one launch
    for (size_t i = 0; i < count; ++i) {
        const u64* d_v = in + B.in_vs + i * K;
        const size_t ent = B.a_ent + i * B.ent_stride;
        hipLaunchKernelGGL(k_circuit_bits_many, dim3((unsigned)K), dim3(256), 0, ctx->stream, C.e, m_bits, d_v, B.a_vals + i * K, ent, B.g_cells, adv);
        hipLaunchKernelGGL(k_circuit_select_many, dim3((unsigned)(K * m_bits)), dim3(256), 0, ctx->stream, C.e, m_bits, d_v, recs + i * B.per * rec,
                           2 * (size_t)m_bits, ent, B.g_cells, bit_stride(C), B.head, adv);
    }
    for (size_t j = 0; j < K; ++j) {
        const size_t r0 = 2 * (size_t)m_bits * j;
        launch_chains(A, C, B.a_ent + j * B.g_cells + 2, B.l_ent + r0 * C.e.lookups, recs + r0 * rec, m_bits, count, B.ent_stride, B.per);
    }
    // the hs-chains as kind 9's, behind the slot chains: their records start 2 b K into a ciphertext's
    launch_hs_chains(A, C, in, B.in_ss, s_limbs, B.s_words, count, B.a_ent + K * B.g_cells + 2, B.ent_stride, B.l_ent, recs,
                     2 * (size_t)m_bits * K, B.per);
    // the K fold blocks of every ciphertext, and the result blocks with the [1, 0] of the hs-chains
    launch_runs(A, C, B.a_ent + B.ent_stride - K * C.e.cells, B.l_ent, recs, K, count, B.ent_stride, B.per, B.per - K);
    launch_results(A, C, B.res, count, in, recs);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_pballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots,
                                     uint32_t m_bits, uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps,
                                     const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return pballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                               lookup_bits, count, slots, m_bits, s_limbs);
}
extern "C" int pz_pballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots,
                                          uint32_t m_bits, uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps,
                                          const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                                          size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride) {
    return pballot_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                               limbs_n, limb_bits, lookup_bits, count, slots, m_bits, s_limbs);
}

// ---- the short-randomness mix (circuit kind 10): K = 2^d ciphertexts through the Benes network, then c'_i =
// d_i hs^s_i mod n^2.  Stream: assign n; assign hs, c_1 .. c_K at full width; assign s_1 .. s_K (s_limbs limbs each); square + refresh,
// load_zero; the network as kind 8; per output [1, 0 | pow_mod(hs, s_i) as kind 9 emits its hs-chain: per limb of s_i num_to_bits and W
// bit blocks | mul_mod(d_i, hss_i)]; per output a result block (res_i against the remainder of the output's last record).  inputs: n |
// hs | c_1 .. c_K | s_1 .. s_K (ceil(s_limbs W / 64) words each) | res_1 .. res_K.  Routes, bits and records are
// pz_paillier_smix_dev's, as it leaves them: fields of 2 ceil(Ln W / 64) words.  No arithmetic of its own: kind 8's switch kernel and
// the bits, select, expand, assign and result kernels above.
struct SmixP {
    size_t K, half, layers, per, s_limbs, s_words, a_hs, l_hs, a_cts, l_cts, a_ss, l_ss, a_net, sw_cells, a_out, l_out, out_stride, limb_stride;
    size_t in_hs, in_cts, in_ss;    // word offsets inside `inputs`
    unsigned d, rw;                 // log2 K; words per field of a route or record as K3 writes them
    ResP res;
};
static int make_smix_params(uint32_t limbs_n, uint32_t limb_bits, uint32_t lb, size_t count, uint32_t s_limbs, CircP& C, SmixP& B,
                            size_t* adv_total, size_t* lk_total) {
    if (!pz_count_ok(count, 1, PZ_ENTRIES_MAX) || (count & (count - 1)) != 0 || !pz_short_exp_ok(s_limbs, limbs_n)) return PZ_ERR_INVALID;
    PZCHK(circ_base(limbs_n, limb_bits, lb, 10, C));
    memset(&B, 0, sizeof B);
    const size_t W = limb_bits, s_bits = (size_t)s_limbs * W;
    B.K = count; B.half = count / 2; B.per = 2 * s_bits + 1; B.rw = 2 * C.words_n;
    B.s_limbs = s_limbs;
    B.s_words = (s_bits + 63) / 64;
    while (((size_t)1 << B.d) < count) ++B.d;
    B.layers = count > 1 ? 2 * (size_t)B.d - 1 : 0;
    B.in_hs = C.words_n;
    B.in_cts = B.in_hs + C.e.L64;
    B.in_ss = B.in_cts + count * C.e.L64;
    size_t a = 0, l = 0;
    assign_inputs(C, 1, a, l);
    B.a_hs = a; B.l_hs = l; a += 2 * asg_adv(C); l += 2 * asg_lk(C);
    B.a_cts = a; B.l_cts = l; a += count * 2 * asg_adv(C); l += count * 2 * asg_lk(C);
    B.a_ss = a; B.l_ss = l;
    a += count * s_limbs * (1 + (size_t)C.rc_adv); l += count * s_limbs * (size_t)C.rc_lk;
    square_refresh_cells(C, a, l);
    load_zero_cell(C, a);
    B.sw_cells = 4 + 16 * (size_t)C.e.L;
    B.a_net = a; a += B.layers * B.half * B.sw_cells;
    B.limb_stride = nbits_cells(W) + W * bit_stride(C);
    B.out_stride = 2 + s_limbs * B.limb_stride + C.e.cells;
    B.a_out = a; B.l_out = l;
    a += count * B.out_stride; l += count * B.per * C.e.lookups;
    B.res.a_head = B.a_out; B.res.head_stride = B.out_stride;
    B.res.rec0 = B.per - 1; B.res.rec_stride = B.per; B.res.field = 3;
    result_blocks(C, B.res, count, B.in_ss + count * B.s_words, a, l);
    *adv_total = a;
    *lk_total = l;
    return PZ_OK;
}
extern "C" int pz_smix_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs, size_t* advice_cells,
                             size_t* lookup_cells) {
    CircP C;
    SmixP B;
    size_t a, l;
    const int rc = make_smix_params(limbs_n, limb_bits, lookup_bits, count, s_limbs, C, B, &a, &l);
    return put_cells(rc, a, l, advice_cells, lookup_cells);
}

static int smix_expand_impl(const ExpandArgs& A, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                            const uint8_t* bits, const uint64_t* d_routes) {
    PZCHK(expand_check(A));
    CircP C;
    SmixP B;
    size_t a, l;
    PZCHK(make_smix_params(limbs_n, limb_bits, lookup_bits, count, s_limbs, C, B, &a, &l));
    if (B.layers && (!bits || !d_routes)) return PZ_ERR_INVALID;
    PZCHK(expand_layout(A, C));
    const size_t n_switch = B.layers * B.half;
    for (size_t i = 0; i < n_switch; ++i)
        if (bits[i] > 1) return PZ_ERR_MESSAGE_RANGE;   // assert_bit of such a byte cannot hold
    PZCHK(short_exp_check(A.inputs, B.in_ss, B.s_words, (size_t)s_limbs * limb_bits, count));
    pz_ctx* ctx = A.ctx;
    PZ_ENTER(ctx);
    const size_t in_words = B.res.in_res + count * C.e.L64;
    const u64* in;
    PZCHK(expand_stage(A, in_words, bits, n_switch, &in));   // the switch bits behind the inputs
    const unsigned char* d_bits = (const unsigned char*)(in + in_words);
    const u64* recs = A.d_steps;
    PZCHK(repack_records(ctx, C, B.rw, count * B.per * 4, &recs));
    pz_timer tm(ctx, PZ_T_EXPAND);
    Fr *adv = (Fr*)A.d_advice, *lk = (Fr*)A.d_lookup;
    // n, square, refresh, load_zero
    hipLaunchKernelGGL(k_circuit_misc, dim3(1), dim3(256), 0, ctx->stream, C, in, (const u64*)nullptr, adv, lk);
    // assign_integer(hs), assign_integer(c_j): 2 Ln limbs from L64 words each; assign_integer(s_i): s_limbs limbs from s_words words each
    launch_assign(A, C, in, B.in_hs, C.nf, C.e.L64, 1 + count, B.a_hs, B.l_hs);
    launch_assign(A, C, in, B.in_ss, (unsigned)s_limbs, (unsigned)B.s_words, count, B.a_ss, B.l_ss);
    launch_network(A, C, in + B.in_cts, d_routes, d_bits, count, B.d, B.layers, B.rw, B.a_net, B.sw_cells);
    // the hs-chains as kind 9's: an output's records start with them
    launch_hs_chains(A, C, in, B.in_ss, s_limbs, B.s_words, count, B.a_out + 2, B.out_stride, B.l_out, recs, 0, B.per);
    // the final block of every output, and the result blocks with the [1, 0] of the chains
    launch_runs(A, C, B.a_out + B.out_stride - C.e.cells, B.l_out, recs, 1, count, B.out_stride, B.per, B.per - 1);
    launch_results(A, C, B.res, count, in, recs);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
extern "C" int pz_smix_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                                  const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                                  const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride) {
    return smix_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, false, rows, col_stride, nullptr, 0, 0}, limbs_n, limb_bits,
                            lookup_bits, count, s_limbs, bits, d_routes);
}
extern "C" int pz_smix_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                                       const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                                       const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                                       size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride) {
    return smix_expand_impl({ctx, inputs, d_steps, d_modulus, d_advice, d_lookup, true, lookup_rows, col_stride, d_col_starts, n_adv_cols, max_rows},
                            limbs_n, limb_bits, lookup_bits, count, s_limbs, bits, d_routes);
}
#undef LIMB

// host-pointer form (SURVEY.md section 8b `pz_witness_expand`): stages the trace up, expands on the device in groups
// of steps and copies the cell streams back; the prover pipeline keeps everything resident and uses the _dev form.
extern "C" int pz_witness_expand(pz_ctx* ctx, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits, const uint64_t* steps,
                                 size_t n_steps, const uint64_t* modulus, uint64_t* advice_out, uint64_t* lookup_out) {
    if (!ctx || (n_steps && (!steps || !modulus))) return PZ_ERR_INVALID;
    ExpP P;
    PZCHK(make_params(limbs, limb_bits, lookup_bits, P));
    if (!n_steps || (!advice_out && !lookup_out)) return PZ_OK;
    PZ_ENTER(ctx);
    const size_t rec = 4 * (size_t)P.L64 * 8;  // bytes per step record
    // groups of steps bounded to ~512 MiB of cells
    size_t group = ((size_t)512 << 20) / (P.cells * 32 + 1);
    if (group == 0) group = 1;
    if (group > n_steps) group = n_steps;
    void *d_steps, *d_mod, *d_adv = nullptr, *d_lk = nullptr;
    PZCHK(pz_ws_get(ctx, WS_IO_A, group * rec + 64, &d_steps));
    PZCHK(pz_ws_get(ctx, WS_MISC, (size_t)P.L64 * 8, &d_mod));
    if (advice_out) PZCHK(pz_ws_get(ctx, WS_IO_B, group * P.cells * 32, &d_adv));
    if (lookup_out) PZCHK(pz_ws_get(ctx, WS_IO_C, group * P.lookups * 32 + 32, &d_lk));
    HIPCHK(ctx, hipMemcpyAsync(d_mod, modulus, (size_t)P.L64 * 8, hipMemcpyHostToDevice, ctx->stream));
    for (size_t s0 = 0; s0 < n_steps; s0 += group) {
        const size_t ns = n_steps - s0 < group ? n_steps - s0 : group;
        HIPCHK(ctx, hipMemcpyAsync(d_steps, (const char*)steps + s0 * rec, ns * rec, hipMemcpyHostToDevice, ctx->stream));
        PZCHK(pz_witness_expand_dev(ctx, limbs, limb_bits, lookup_bits, (const uint64_t*)d_steps, ns, (const uint64_t*)d_mod,
                                    (uint64_t*)d_adv, (uint64_t*)d_lk));
        if (advice_out)
            HIPCHK(ctx, hipMemcpyAsync((char*)advice_out + s0 * P.cells * 32, d_adv, ns * P.cells * 32, hipMemcpyDeviceToHost,
                                       ctx->stream));
        if (lookup_out)
            HIPCHK(ctx, hipMemcpyAsync((char*)lookup_out + s0 * P.lookups * 32, d_lk, ns * P.lookups * 32, hipMemcpyDeviceToHost,
                                       ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PZ_OK;
}
