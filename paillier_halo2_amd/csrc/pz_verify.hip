// pz_verify.hip -- the Fr side of the device batch verifier (pz_verify_batch, csrc/pz_verify.cpp): per proof the constraint
// expression at x, SHPLONK's scalars for every base of the final MSM, and the fold of a batch into K1's two scalar columns.
// paillier_halo2_amd/verifier.py (`constraint_expression`, `_terms`, `_fold_and_check`) is the Python statement of the same values.
//
// A proof on the device: its evaluations (pz_proof_evaluate's array, vshape offsets below) and a block of host-derived scalars
// (VP_* in pz_internal.h: the replayed challenges, the Lagrange values at x, the SHPLONK vanishing values and interpolation bases at u).
// Own bases of proof p are its commitments in the order of the proof, so a scalar slot is the index of a commitment.
//   own[p][0][i]  A-side scalar of commitment i,  own[p][1][i]  B-side (only W2's is not zero)
//   vksc[p][j]    A-side scalar of vk base j (fixed | sigma | g0); gpart[p][s] = set s's share of the g0 scalar
// Workgroups of 256 lanes.  The field is exact, so neither the lane count nor the tree shape changes a result.
#include "fp.cuh"
#include "pz_internal.h"

namespace {

constexpr unsigned VT = 256;

__device__ __forceinline__ Fr ld(const uint64_t* p) { return fp_load<FrTag>(p); }
__device__ __forceinline__ Fr pow_u32(Fr b, unsigned e) {
    Fr acc = fp_one<FrTag>();
    while (e) {
        if (e & 1) acc = fp_mul(acc, b);
        b = fp_sqr(b);
        e >>= 1;
    }
    return acc;
}

// line L of the constraint expression (verifier.constraint_expression's order): gates | l0 (1 - z_0) | l_last line | S - 1 chunk links |
// S chunked permutation lines | 5 per lookup
__device__ Fr expr_line(const pz_vshape& s, unsigned L, const uint64_t* ev, const uint64_t* pp, const uint64_t* delta) {
    const unsigned A = s.A, Lk = s.Lk, S = s.S, m = s.m;
    auto e = [&](unsigned el) { return ld(ev + 4ull * el); };
    const Fr one = fp_one<FrTag>();
    if (L < A) {   // q (a0 + a1 a2 - a3)
        const unsigned o = s.e_adv + 4 * L;
        return fp_mul(e(s.e_fix + L), fp_sub(fp_add(e(o), fp_mul(e(o + 1), e(o + 2))), e(o + 3)));
    }
    L -= A;
    const Fr l0 = ld(pp + 4 * VP_L0), llast = ld(pp + 4 * VP_LLAST), lact = ld(pp + 4 * VP_LACT);
    if (L == 0) return fp_mul(l0, fp_sub(one, e(s.e_pz)));
    if (L == 1) {
        const Fr z = e(s.e_pz + 3 * (S - 1));
        return fp_mul(llast, fp_sub(fp_sqr(z), z));
    }
    L -= 2;
    if (L < S - 1) return fp_mul(l0, fp_sub(e(s.e_pz + 3 * (L + 1)), e(s.e_pz + 3 * L + 2)));
    L -= S - 1;
    if (L < S) {   // chunk L: columns 2L, 2L + 1 (< m); column c's identity term beta x delta^c
        const Fr beta = ld(pp + 4 * VP_BETA), gamma = ld(pp + 4 * VP_GAMMA), bx = ld(pp + 4 * VP_BX);
        Fr left = e(s.e_pz + 3 * L + 1), right = e(s.e_pz + 3 * L);
        for (unsigned c = 2 * L; c < 2 * L + 2 && c < m; ++c) {
            // (the instance column, last when the key has one, is not opened: its value at x comes from pz_public.hip's k_instance_eval)
            const Fr v = c < A ? e(s.e_adv + 4 * c) : c < A + Lk ? e(s.e_lka + (c - A)) : c == A + Lk ? e(s.e_fix + A) : ld(pp + 4 * VP_INST);
            const Fr vg = fp_add(v, gamma);
            left = fp_mul(left, fp_add(vg, fp_mul(beta, e(s.e_sig + c))));
            right = fp_mul(right, fp_add(vg, fp_mul(bx, ld(delta + 4ull * c))));
        }
        return fp_mul(lact, fp_sub(left, right));
    }
    L -= S;
    const unsigned j = L / 5, t = L % 5;
    const Fr zx = e(s.e_lz + 2 * j), ap = e(s.e_ap + 2 * j), sp = e(s.e_sp + j);
    switch (t) {
    case 0: return fp_mul(l0, fp_sub(one, zx));
    case 1: return fp_mul(llast, fp_sub(fp_sqr(zx), zx));
    case 2: {
        const Fr beta = ld(pp + 4 * VP_BETA), gamma = ld(pp + 4 * VP_GAMMA);
        const Fr lhs = fp_mul(fp_mul(e(s.e_lz + 2 * j + 1), fp_add(ap, beta)), fp_add(sp, gamma));
        const Fr rhs = fp_mul(fp_mul(zx, fp_add(e(s.e_lka + j), beta)), fp_add(e(s.e_fix + A + 1), gamma));
        return fp_mul(lact, fp_sub(lhs, rhs));
    }
    case 3: return fp_mul(l0, fp_sub(ap, sp));
    default: return fp_mul(fp_mul(lact, fp_sub(ap, sp)), fp_sub(ap, e(s.e_ap + 2 * j + 1)));
    }
}

// one workgroup per proof: acc = acc y + line over all lines.  Lane t folds lines [t NL / 256, (t + 1) NL / 256) into (h_t, y^len_t);
// the tree combines neighbours as h_l y^len_r + h_r.  -> h(x) = acc / (x^n - 1) and whether the proof states that value.
__global__ __launch_bounds__(256) void k_verify_expression(pz_vshape s, const uint64_t* __restrict__ evals, const uint64_t* __restrict__ pps,
                                                           const uint64_t* __restrict__ delta, uint64_t* __restrict__ h_out,
                                                           int32_t* __restrict__ ident) {
    __shared__ Fr s_h[VT], s_p[VT];
    const unsigned p = blockIdx.x, t = threadIdx.x;
    const uint64_t* ev = evals + (size_t)p * 4 * s.n_ev;
    const uint64_t* pp = pps + (size_t)p * 4 * VP_COUNT;
    const unsigned NL = s.A + 2 + (s.S - 1) + s.S + 5 * s.Lk;
    const unsigned lo = (unsigned)((uint64_t)NL * t / VT), hi = (unsigned)((uint64_t)NL * (t + 1) / VT);
    const Fr y = ld(pp + 4 * VP_Y);
    Fr h = fp_zero<FrTag>(), pw = fp_one<FrTag>();
    for (unsigned L = lo; L < hi; ++L) {
        h = fp_add(fp_mul(h, y), expr_line(s, L, ev, pp, delta));
        pw = fp_mul(pw, y);
    }
    s_h[t] = h;
    s_p[t] = pw;
    __syncthreads();
    for (unsigned w = 1; w < VT; w <<= 1) {
        if ((t & (2 * w - 1)) == 0) {
            s_h[t] = fp_add(fp_mul(s_h[t], s_p[t + w]), s_h[t + w]);
            s_p[t] = fp_mul(s_p[t], s_p[t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const Fr hx = fp_mul(s_h[0], ld(pp + 4 * VP_INV));
        fp_store(h_out + 4 * p, hx);
        ident[p] = fp_eq(hx, ld(ev + 4ull * s.e_h)) ? 1 : 0;
    }
}

// one workgroup per (query set, proof).  Member j of the set gets c_j = v^k Z_k(u) sy^j (VP_COEF + k), written to its base's slot; the
// evaluations fold to f_q = sum_j sy^j e_j(point q); the set's g0 share is -v^k Z_k(u) sum_q f_q L_q(u).  Lane t takes members
// [t M / 256, (t + 1) M / 256): one pow for its first sy^j, then products forward.
__global__ __launch_bounds__(256) void k_verify_shplonk(pz_vshape s, const uint32_t* __restrict__ members, const uint64_t* __restrict__ evals,
                                                        const uint64_t* __restrict__ pps, const uint64_t* __restrict__ h_in,
                                                        uint64_t* __restrict__ own, uint64_t* __restrict__ vksc, uint64_t* __restrict__ gpart) {
    __shared__ Fr s_acc[VT];
    const unsigned k = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const uint64_t* ev = evals + (size_t)p * 4 * s.n_ev;
    const uint64_t* pp = pps + (size_t)p * 4 * VP_COUNT;
    uint64_t* ownA = own + (size_t)p * 8 * s.n_own;
    uint64_t* vk = vksc + (size_t)p * 4 * s.n_vkb;
    const unsigned M = s.set_count[k], npt = s.set_npts[k];
    const uint32_t* mem = members + 2 * s.set_start[k];
    const unsigned lo = (unsigned)((uint64_t)M * t / VT), hi = (unsigned)((uint64_t)M * (t + 1) / VT);
    const Fr sy = ld(pp + 4 * VP_SY), coef = ld(pp + 4 * (VP_COEF + k)), xn = ld(pp + 4 * VP_XN);
    Fr f[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) f[q] = fp_zero<FrTag>();
    Fr syj = pow_u32(sy, lo);
    for (unsigned j = lo; j < hi; ++j) {
        const uint32_t eoff = mem[2 * j], dest = mem[2 * j + 1];
        const uint32_t kind = dest >> 30, slot = dest & 0x3fffffffu;
        const Fr c = fp_mul(coef, syj);
        if (kind == PZ_VM_OWN) {
            fp_store(ownA + 4ull * slot, c);
        } else if (kind == PZ_VM_VK) {
            fp_store(vk + 4ull * slot, c);
        } else {   // h: [h] = sum_i x^(n i) [h_i], its value the h(x) the expression implies
            fp_store(ownA + 4ull * slot, c);
            const Fr c1 = fp_mul(c, xn);
            fp_store(ownA + 4ull * (slot + 1), c1);
            fp_store(ownA + 4ull * (slot + 2), fp_mul(c1, xn));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < (int)npt) {
                const Fr e = kind == PZ_VM_H ? ld(h_in + 4 * p) : ld(ev + 4ull * (eoff + q));
                f[q] = fp_add(f[q], fp_mul(syj, e));
            }
        syj = fp_mul(syj, sy);
    }
    Fr interp = fp_zero<FrTag>();
    for (unsigned q = 0; q < npt; ++q) {
        Fr v = fp_zero<FrTag>();
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) v = qq == (int)q ? f[qq] : v;
        s_acc[t] = v;
        __syncthreads();
        for (unsigned off = VT / 2; off > 0; off >>= 1) {
            if (t < off) s_acc[t] = fp_add(s_acc[t], s_acc[t + off]);
            __syncthreads();
        }
        if (t == 0) interp = fp_add(interp, fp_mul(s_acc[0], ld(pp + 4 * (VP_LAG + 4 * k + q))));
        __syncthreads();
    }
    if (t == 0) {
        fp_store(gpart + 4 * ((size_t)p * PZ_VSETS_MAX + k), fp_neg(fp_mul(coef, interp)));
        if (k == 0) {   // W1: -Z_T(u); W2: z_0 u on A, -z_0 on B
            const unsigned w1 = s.n_own - 2, w2 = s.n_own - 1;
            fp_store(ownA + 4ull * w1, ld(pp + 4 * VP_W1A));
            fp_store(ownA + 4ull * w2, ld(pp + 4 * VP_W2A));
            fp_store(ownA + 4ull * (s.n_own + w2), ld(pp + 4 * VP_W2B));
        }
    }
}

// mode 0: K1's two columns over [fixed | sigma | g0 | own bases of proof 0, 1, ...] folded with the weights r_p: a vk base (and g0)
// sums r_p times its scalar over the proofs, an own base is r_p times its proof's scalar.  mode 1 (per-proof checks): the g0 slot of
// every proof's vk column, sum of its sets' shares.
__global__ __launch_bounds__(256) void k_verify_fold(pz_vshape s, unsigned B, int mode, const uint64_t* __restrict__ r,
                                                     uint64_t* __restrict__ vksc, const uint64_t* __restrict__ gpart,
                                                     const uint64_t* __restrict__ own, uint64_t* __restrict__ cols) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned gslot = s.n_vkb - 1;
    if (mode == 1) {
        if (i >= B) return;
        Fr g = fp_zero<FrTag>();
        for (unsigned k = 0; k < s.n_sets; ++k) g = fp_add(g, ld(gpart + 4 * (i * PZ_VSETS_MAX + k)));
        fp_store(vksc + 4 * (i * s.n_vkb + gslot), g);
        return;
    }
    const size_t nb = s.n_vkb + (size_t)B * s.n_own;
    if (i >= nb) return;
    Fr a = fp_zero<FrTag>(), b = fp_zero<FrTag>();
    if (i < gslot) {
        for (unsigned p = 0; p < B; ++p) a = fp_add(a, fp_mul(ld(r + 4 * p), ld(vksc + 4 * ((size_t)p * s.n_vkb + i))));
    } else if (i == gslot) {
        for (unsigned p = 0; p < B; ++p) {
            Fr g = fp_zero<FrTag>();
            for (unsigned k = 0; k < s.n_sets; ++k) g = fp_add(g, ld(gpart + 4 * ((size_t)p * PZ_VSETS_MAX + k)));
            a = fp_add(a, fp_mul(ld(r + 4 * p), g));
        }
    } else {
        const size_t o = i - s.n_vkb;
        const size_t p = o / s.n_own, j = o % s.n_own;
        const Fr rp = ld(r + 4 * p);
        const uint64_t* op = own + p * 8 * s.n_own;
        a = fp_mul(rp, ld(op + 4 * j));
        b = fp_mul(rp, ld(op + 4 * (s.n_own + j)));
    }
    fp_store(cols + 4 * i, a);
    fp_store(cols + 4 * (nb + i), b);
}

}  // namespace

int pz_verify_terms_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, const uint32_t* d_members, const uint64_t* d_evals,
                           const uint64_t* d_pp, const uint64_t* d_delta, uint64_t* d_h, int32_t* d_ident, uint64_t* d_own,
                           uint64_t* d_vksc, uint64_t* d_gpart) {
    if (!B) return PZ_OK;
    hipLaunchKernelGGL(k_verify_expression, dim3((unsigned)B), dim3(VT), 0, ctx->stream, s, d_evals, d_pp, d_delta, d_h, d_ident);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_verify_shplonk, dim3(s.n_sets, (unsigned)B), dim3(VT), 0, ctx->stream, s, d_members, d_evals, d_pp,
                       (const uint64_t*)d_h, d_own, d_vksc, d_gpart);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

int pz_verify_fold_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, int mode, const uint64_t* d_r, uint64_t* d_vksc,
                          const uint64_t* d_gpart, const uint64_t* d_own, uint64_t* d_cols) {
    if (!B) return PZ_OK;
    const size_t n = mode == 1 ? B : s.n_vkb + B * s.n_own;
    hipLaunchKernelGGL(k_verify_fold, dim3(pz_div_up(n, VT)), dim3(VT), 0, ctx->stream, s, (unsigned)B, mode, d_r, d_vksc, d_gpart, d_own,
                       d_cols);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
