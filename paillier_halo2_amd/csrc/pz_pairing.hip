// pz_pairing.hip -- the BN254 optimal-ate pairing on gfx950: G2 scalar multiplication, e(P, Q) and batched pairing-product
// checks (the verifier's final step, halo2's `multi_miller_loop(..).final_exponentiation() == 1`).
//
// One lane per check (or per pairing / per G2 multiplication): the state of a Miller loop is one Fq12 (96 VGPRs) plus the
// running point and a line, far too much to split across lanes profitably, and checks are independent.  A wave covers 64
// of them; no lane waits on another.
//
// Miller loop over the binary digits of 6x + 2 (x = 0x44E992B44A6909F1), homogeneous projective T on the twist, lines
// evaluated at P in the sparse form l0 + l1 w + l3 w^3, then the two closing lines through pi(Q) and -pi^2(Q).  The lines
// are the affine ones scaled by Fq2 factors, which the final exponentiation removes.  A check's m pairs share the
// squarings of f (multi-Miller loop); each pair's T lives in a global workspace between the digits, its P and Q are read
// from global memory at each digit.  Final exponentiation to exactly (p^12 - 1)/r: f^((p^6 - 1)(p^2 + 1)) by conjugation,
// one inversion and one Frobenius, then plain square-and-multiply by (p^4 - p^2 + 1)/r (761 bits).
#include "fp12.cuh"
#include "pz_internal.h"

namespace {

struct G2Proj {
    Fq2 x, y, z;   // (X / Z, Y / Z)
};

__device__ __forceinline__ Fq2 f2_half(const Fq2& a) { return f2_mul_fq(a, fq_const(PZ_TWO_INV)); }

// T <- 2T, returns the tangent line at P (xp, yp): l0 = -2YZ yp, l1 = 3X^2 xp, l3 = 3b'Z^2 - Y^2
__device__ __forceinline__ void dbl_step(G2Proj& t, const G1Pt& p, Fq2& l0, Fq2& l1, Fq2& l3) {
    const Fq2 a = f2_half(f2_mul(t.x, t.y));
    const Fq2 b = f2_sqr(t.y), c = f2_sqr(t.z);
    const Fq2 e = f2_mul(f2_add(f2_dbl(c), c), f2_const(PZ_TWIST_B));
    const Fq2 f = f2_add(f2_dbl(e), e);
    const Fq2 g = f2_half(f2_add(b, f));
    const Fq2 h = f2_sub(f2_sqr(f2_add(t.y, t.z)), f2_add(b, c));
    const Fq2 j = f2_sqr(t.x);
    const Fq2 e2 = f2_sqr(e);
    l0 = f2_mul_fq(f2_neg(h), p.y);
    l1 = f2_mul_fq(f2_add(f2_dbl(j), j), p.x);
    l3 = f2_sub(e, b);
    t.x = f2_mul(a, f2_sub(b, f));
    t.y = f2_sub(f2_sqr(g), f2_add(f2_dbl(e2), e2));
    t.z = f2_mul(b, h);
}

// T <- T + Q (Q affine), returns the line through T and Q at P: l0 = lambda yp, l1 = -theta xp, l3 = theta xq - lambda yq
__device__ __forceinline__ void add_step(G2Proj& t, const G2Aff& q, const G1Pt& p, Fq2& l0, Fq2& l1, Fq2& l3) {
    const Fq2 theta = f2_sub(t.y, f2_mul(q.y, t.z));
    const Fq2 lambda = f2_sub(t.x, f2_mul(q.x, t.z));
    const Fq2 c = f2_sqr(theta), d = f2_sqr(lambda);
    const Fq2 e = f2_mul(lambda, d), f = f2_mul(t.z, c), g = f2_mul(t.x, d);
    const Fq2 h = f2_sub(f2_add(e, f), f2_dbl(g));
    l0 = f2_mul_fq(lambda, p.y);
    l1 = f2_mul_fq(f2_neg(theta), p.x);
    l3 = f2_sub(f2_mul(theta, q.x), f2_mul(lambda, q.y));
    t.x = f2_mul(lambda, h);
    t.y = f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, t.y));
    t.z = f2_mul(t.z, e);
}

__device__ __forceinline__ G2Proj proj_load(const G2Proj* p) { return *p; }
__device__ __forceinline__ void proj_store(G2Proj* p, const G2Proj& t) { *p = t; }

// pi(Q) = (conj(x) FROB_1_2, conj(y) FROB_1_3);  -pi^2(Q) = (x FROB_2_2, -y FROB_2_3)
__device__ __forceinline__ G2Aff twist_frob1(const G2Aff& q) {
    return G2Aff{f2_mul(f2_conj(q.x), frob_const(1, 2)), f2_mul(f2_conj(q.y), frob_const(1, 3))};
}
__device__ __forceinline__ G2Aff twist_neg_frob2(const G2Aff& q) {
    return G2Aff{f2_mul(q.x, frob_const(2, 2)), f2_neg(f2_mul(q.y, frob_const(2, 3)))};
}

// prod_j f_{6x+2,Q_j}(P_j) * closing lines, over the m pairs of one check: g1 + 8 j, g2 + 16 j; ts[j * stride] holds T_j.
// *bad is set if a point is off its curve (or not canonical); pairs with an identity contribute 1.
__device__ Fq12 multi_miller(const uint64_t* g1, const uint64_t* g2, uint32_t m, G2Proj* ts, size_t stride, bool* bad) {
    bool any_bad = false;
    for (uint32_t j = 0; j < m; ++j) {
        const G1Pt p = g1_load(g1 + 8 * (size_t)j);
        const G2Aff q = g2_load(g2 + 16 * (size_t)j);
        any_bad |= !g1_on_curve(p) || !g2_on_curve(q);
        proj_store(ts + j * stride, G2Proj{q.x, q.y, f2_one()});
    }
    *bad = any_bad;
    Fq12 f = f12_one();
    if (any_bad) return f;
    for (int i = PZ_ATE_BITS - 2; i >= 0; --i) {
        if (i != PZ_ATE_BITS - 2) f = f12_sqr(f);
        const bool bit = (PZ_ATE[i >> 5] >> (i & 31)) & 1;
        for (uint32_t j = 0; j < m; ++j) {
            const G1Pt p = g1_load(g1 + 8 * (size_t)j);
            const G2Aff q = g2_load(g2 + 16 * (size_t)j);
            if (g1_is_inf(p) || g2_is_inf(q)) continue;
            G2Proj t = proj_load(ts + j * stride);
            Fq2 l0, l1, l3;
            dbl_step(t, p, l0, l1, l3);
            f = f12_mul_line(f, l0, l1, l3);
            if (bit) {
                add_step(t, q, p, l0, l1, l3);
                f = f12_mul_line(f, l0, l1, l3);
            }
            proj_store(ts + j * stride, t);
        }
    }
    for (uint32_t j = 0; j < m; ++j) {
        const G1Pt p = g1_load(g1 + 8 * (size_t)j);
        const G2Aff q = g2_load(g2 + 16 * (size_t)j);
        if (g1_is_inf(p) || g2_is_inf(q)) continue;
        G2Proj t = proj_load(ts + j * stride);
        Fq2 l0, l1, l3;
        add_step(t, twist_frob1(q), p, l0, l1, l3);
        f = f12_mul_line(f, l0, l1, l3);
        add_step(t, twist_neg_frob2(q), p, l0, l1, l3);
        f = f12_mul_line(f, l0, l1, l3);
    }
    return f;
}

// f^((p^12 - 1)/r)
__device__ Fq12 final_exp(const Fq12& f) {
    Fq12 a = f12_mul(f12_conj(f), f12_inv(f));   // ^(p^6 - 1)
    a = f12_mul(f12_frob<2>(a), a);              // ^(p^2 + 1)
    Fq12 r = a;
    for (int i = PZ_HARD_BITS - 2; i >= 0; --i) {
        r = f12_sqr(r);
        if ((PZ_HARD[i >> 5] >> (i & 31)) & 1) r = f12_mul(r, a);
    }
    return r;
}

__device__ __forceinline__ void f2_store(uint64_t* p, const Fq2& a) {
    fp_store(p, a.c0);
    fp_store(p + 4, a.c1);
}
__device__ __forceinline__ void f12_store(uint64_t* p, const Fq12& a) {
    f2_store(p, a.c0.c0);
    f2_store(p + 8, a.c0.c1);
    f2_store(p + 16, a.c0.c2);
    f2_store(p + 24, a.c1.c0);
    f2_store(p + 32, a.c1.c1);
    f2_store(p + 40, a.c1.c2);
}

__global__ __launch_bounds__(64) void k_pairing_check(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2, size_t n_checks,
                                                       uint32_t m, G2Proj* __restrict__ ts, int32_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_checks) return;
    bool bad;
    const Fq12 f = multi_miller(g1 + i * m * 8, g2 + i * m * 16, m, ts + i, n_checks, &bad);
    if (bad) {
        ok[i] = -1;
        return;
    }
    ok[i] = f12_is_one(final_exp(f)) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_pairing(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2, size_t n,
                                                G2Proj* __restrict__ ts, uint64_t* __restrict__ gt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool bad;
    const Fq12 f = multi_miller(g1 + i * 8, g2 + i * 16, 1, ts + i, n, &bad);
    if (bad) {   // not a GT element: all zero
        for (int k = 0; k < 48; ++k) gt[i * 48 + k] = 0;
        return;
    }
    f12_store(gt + i * 48, final_exp(f));
}

// out[i] = [s_i] Q_i: MSB-first double-and-add in Jacobian coordinates over the canonical scalar
__global__ __launch_bounds__(64) void k_g2_mul(const uint64_t* __restrict__ g2, const uint64_t* __restrict__ scalars, size_t n,
                                               uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G2Aff q = g2_load(g2 + i * 16);
    const Fr s = fp_canon(fp_from_mont(fp_load<FrTag>(scalars + i * 4)));
    G2Jac acc{f2_one(), f2_one(), f2_zero()};
    if (!g2_is_inf(q)) {
        for (int b = 253; b >= 0; --b) {
            acc = g2_dbl(acc);
            if ((s.v[b >> 5] >> (b & 31)) & 1) acc = g2_add_mixed(acc, q);
        }
    }
    g2_store(out + i * 16, g2_to_affine(acc));
}

}  // namespace

extern "C" int pz_g2_generator(uint64_t out[16]) {
    if (!out) return PZ_ERR_INVALID;
    memcpy(out, PZ_G2_GEN, sizeof PZ_G2_GEN);
    return PZ_OK;
}

extern "C" int pz_g2_mul_dev(pz_ctx* ctx, const uint64_t* d_g2, const uint64_t* d_scalars, size_t n, uint64_t* d_out) {
    if (!ctx || (n && (!d_g2 || !d_scalars || !d_out))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_g2_mul, dim3(pz_div_up(n, 64)), dim3(64), 0, ctx->stream, d_g2, d_scalars, n, d_out);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_pairing_dev(pz_ctx* ctx, const uint64_t* d_g1, const uint64_t* d_g2, size_t n, uint64_t* d_gt) {
    if (!ctx || (n && (!d_g1 || !d_g2 || !d_gt))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void* ts;
    PZCHK(pz_ws_get(ctx, WS_PAIR, n * sizeof(G2Proj), &ts));
    hipLaunchKernelGGL(k_pairing, dim3(pz_div_up(n, 64)), dim3(64), 0, ctx->stream, d_g1, d_g2, n, (G2Proj*)ts, d_gt);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_pairing_check_dev(pz_ctx* ctx, const uint64_t* d_g1, const uint64_t* d_g2, size_t n_checks, uint32_t pairs_per_check,
                                    int32_t* d_ok) {
    if (!ctx || (n_checks && (!d_g1 || !d_g2 || !d_ok || !pairs_per_check))) return PZ_ERR_INVALID;
    if (!n_checks) return PZ_OK;
    PZ_ENTER(ctx);
    void* ts;
    PZCHK(pz_ws_get(ctx, WS_PAIR, n_checks * pairs_per_check * sizeof(G2Proj), &ts));
    hipLaunchKernelGGL(k_pairing_check, dim3(pz_div_up(n_checks, 64)), dim3(64), 0, ctx->stream, d_g1, d_g2, n_checks, pairs_per_check,
                       (G2Proj*)ts, d_ok);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
