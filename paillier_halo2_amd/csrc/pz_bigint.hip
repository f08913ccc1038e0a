// pz_bigint.hip -- K3: big-integer witness generation for c = g^m * r^n mod n^2.
// Replaces the num-bigint arithmetic inside biguint-halo2's BigUintChip::{mul_mod,
// pow_mod_fixed_exp} (call sites /root/reference/src/paillier.rs:51,55,57,81) and
// paillier_enc_native / paillier_add_native (paillier.rs:87-97): every step yields the exact
// quotient and remainder (q, r) of a*b by the modulus, because the circuit assigns both.
//
// Mapping to CDNA4: one 64-lane wavefront owns one big integer, lane j holds limbs [j*E, j*E+E)
// (E = 1: up to 64 x 64-bit limbs = 4096 bits, the 2048-bit-n case; E = 2: up to 128 limbs, the
// 3072-bit-n case).  A product is a lane-systolic schoolbook: per outer limb A_i (broadcast with
// v_readlane) every lane multiplies its limbs (v_mad_u64_u32), adds into its column sums and the
// column array shifts one lane down; carries are kept as per-column counters and resolved once
// per product with a ballot-based carry look-ahead (64-bit scalar add of generate/propagate
// masks).  Reduction is Barrett with a normalised modulus, so the exact quotient falls out; the
// reciprocal is computed on the device once per modulus by restoring division.
// The modexp chain (k_pow_mod_chain) is latency-bound by construction -- every step depends on the one before -- and one
// wavefront is ISSUE-bound inside a product (one VALU instruction per ~4.5 cycles: 64 outer limbs x ~22 instructions), so a
// product is worked by a TEAM of four wavefronts, one per SIMD of the CU: wave w takes the outer limbs [16w, 16w + 16) of a
// against all of b, the four partial products meet in LDS (one workgroup barrier per product, double-buffered) and every wave of
// the team sums them, so all four hold the full result and the O(n) parts of a step (shifts, additions, comparisons) simply run
// redundantly.  A chain is TWO workgroups (two CUs: with both on one CU their waves halve each other's issue slots): the SQUARER
// runs sq <- sq^2 for every exponent bit, never waits, and publishes every square through global memory (a release counter); the
// MULTIPLIER consumes the squares of the set bits (acc <- acc * sq_i) as they appear.  Squarers have the lower workgroup ids, so
// they are resident before any multiplier starts to wait.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pz_internal.h"

typedef uint32_t u32;
typedef uint64_t u64;

template <int E> struct LD {
    u64 v[E];
};

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ u64 bcast64(u64 x, unsigned src) {
    u32 lo = __builtin_amdgcn_readlane((u32)x, src);
    u32 hi = __builtin_amdgcn_readlane((u32)(x >> 32), src);
    return ((u64)hi << 32) | lo;
}
// one-lane shifts of the whole wave as DPP moves (wave_shl:1 / wave_shr:1, bound_ctrl: the lane without a
// source reads 0): a VALU op of a few cycles.  __shfl_down/__shfl_up compile to ds_bpermute_b32, whose LDS-crossbar
// latency (~100 cycles) sat on the critical path of every iteration of the systolic product.
__device__ __forceinline__ u32 dpp_down1(u32 x) { return __builtin_amdgcn_update_dpp(0u, x, 0x130, 0xf, 0xf, true); }
__device__ __forceinline__ u32 dpp_up1(u32 x) { return __builtin_amdgcn_update_dpp(0u, x, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ u64 shfl_down1(u64 x) {  // lane j <- lane j+1, lane 63 <- 0
    return ((u64)dpp_down1((u32)(x >> 32)) << 32) | dpp_down1((u32)x);
}
__device__ __forceinline__ u64 shfl_up1(u64 x) {  // lane j <- lane j-1, lane 0 <- 0
    return ((u64)dpp_up1((u32)(x >> 32)) << 32) | dpp_up1((u32)x);
}

template <int E> __device__ __forceinline__ LD<E> ld_zero() {
    LD<E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) r.v[e] = 0;
    return r;
}
template <int E> __device__ __forceinline__ LD<E> ld_small(u64 x) {  // the integer x
    LD<E> r = ld_zero<E>();
    if (lane_id() == 0) r.v[0] = x;
    return r;
}
template <int E> __device__ __forceinline__ bool ld_is_zero(const LD<E>& a) {
    u64 o = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) o |= a.v[e];
    return __ballot(o != 0) == 0;
}
// load `limbs` u64 limbs from memory (zero extended to the 64*E capacity)
template <int E> __device__ __forceinline__ LD<E> ld_load(const u64* p, unsigned limbs) {
    LD<E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        unsigned idx = lane_id() * E + e;
        r.v[e] = idx < limbs ? p[idx] : 0;
    }
    return r;
}
template <int E> __device__ __forceinline__ void ld_store(u64* p, const LD<E>& a, unsigned limbs) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        unsigned idx = lane_id() * E + e;
        if (idx < limbs) p[idx] = a.v[e];
    }
}
// true if any limb with index >= limbs is non-zero
template <int E> __device__ __forceinline__ bool ld_exceeds(const LD<E>& a, unsigned limbs) {
    bool bad = false;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        unsigned idx = lane_id() * E + e;
        bad |= (idx >= limbs) && (a.v[e] != 0);
    }
    return __ballot(bad) != 0;
}

// s = a + b + cin ; returns carry out.  Local ripple, then a wave-wide carry look-ahead: with
// per-lane generate g and (exclusive) propagate p, the carries of the 64-"bit" addition
// (G|P) + G + cin are exactly the inter-lane carries.
template <int E> __device__ __forceinline__ bool ld_add(LD<E>& s, const LD<E>& a, const LD<E>& b, bool cin) {
    u64 c = 0;
    bool allones = true;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        u64 t = a.v[e] + b.v[e];
        u64 c1 = t < a.v[e];
        u64 t2 = t + c;
        u64 c2 = t2 < t;
        s.v[e] = t2;
        c = c1 | c2;
        allones = allones && (t2 == ~0ull);
    }
    const bool g = c != 0;
    const bool p = allones && !g;
    const u64 G = __ballot(g), P = __ballot(p);
    const u64 X = G | P, Y = G;
    const u64 t = X + Y;
    const u64 o1 = t < X;
    const u64 t2 = t + (cin ? 1ull : 0ull);
    const u64 o2 = t2 < t;
    const u64 cmask = t2 ^ P;  // bit j = carry into lane j
    u64 ci = (cmask >> lane_id()) & 1ull;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        u64 t3 = s.v[e] + ci;
        ci = t3 < s.v[e];
        s.v[e] = t3;
    }
    return (o1 | o2) != 0;
}
// d = a - b ; returns borrow out (true if a < b)
template <int E> __device__ __forceinline__ bool ld_sub(LD<E>& d, const LD<E>& a, const LD<E>& b) {
    LD<E> nb;
#pragma unroll
    for (int e = 0; e < E; ++e) nb.v[e] = ~b.v[e];
    return !ld_add(d, a, nb, true);
}

__device__ __forceinline__ void mul64(u64 a, u64 b, u64& hi, u64& lo) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p00 = (u64)a0 * b0;
    const u64 t = (u64)a0 * b1 + (p00 >> 32);
    const u64 u = (u64)a1 * b0 + (u32)t;
    lo = (u << 32) | (u32)p00;
    hi = (u64)a1 * b1 + (t >> 32) + (u >> 32);
}

// full product of two capacity-sized integers: lo = low 64*E limbs, hi = high 64*E limbs
#ifndef PZ_K3_UNROLL
#define PZ_K3_UNROLL 64  // full unroll: lane indices become immediates and the next round's broadcasts + products overlap the carry chain (52 -> 34 ms per 2048-bit encrypt)
#endif
template <int E> __device__ __noinline__ void ld_mul(LD<E>& lo, LD<E>& hi, const LD<E> a, const LD<E> b) {
    u64 col[E];
    u32 cc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        col[e] = 0;
        cc[e] = 0;
        lo.v[e] = 0;
    }
    const unsigned lane = lane_id();
#pragma unroll PZ_K3_UNROLL
    for (unsigned jj = 0; jj < 64; ++jj) {
#pragma unroll
        for (int ee = 0; ee < E; ++ee) {
            const u64 A = bcast64(a.v[ee], jj);
            u64 pend = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                u64 ph, pl;
                mul64(A, b.v[e], ph, pl);
                u64 t = col[e] + pl;
                cc[e] += t < pl;
                col[e] = t;
                if (e + 1 < E) {
                    u64 t2 = col[e + 1] + ph;
                    cc[e + 1] += t2 < ph;
                    col[e + 1] = t2;
                } else {
                    pend = ph;
                }
            }
            const u64 emit = bcast64(col[0], 0);
            if (lane == jj) lo.v[ee] = emit;
            // shift the column array one limb down
            // (a column's overflow count is consumed here, by the lane that holds it, into the next
            // column arriving in the same slot; it does not travel with the column)
            const u64 n0 = shfl_down1(col[0]);
            u64 ncol[E];
            u32 ncc[E];
#pragma unroll
            for (int e = 0; e + 1 < E; ++e) {
                u64 t = col[e + 1] + cc[e];
                ncc[e] = (t < col[e + 1]);
                ncol[e] = t;
            }
            {
                u64 t = n0 + pend;
                u32 k = (t < pend);
                u64 t2 = t + cc[E - 1];
                k += t2 < t;
                ncol[E - 1] = t2;
                ncc[E - 1] = k;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                col[e] = ncol[e];
                cc[e] = ncc[e];
            }
        }
    }
    // resolve: hi = col + (cc shifted up by one limb)
    LD<E> cv, sh;
#pragma unroll
    for (int e = 0; e < E; ++e) cv.v[e] = col[e];
    sh.v[0] = shfl_up1((u64)cc[E - 1]);
#pragma unroll
    for (int e = 1; e < E; ++e) sh.v[e] = cc[e - 1];
    (void)ld_add(hi, cv, sh, false);
}

// ---- the same product by a team of TEAM wavefronts (k_pow_mod_chain).  P_w = sum_{i in slice w} a_i * b * 2^(64 (i - i0_w)), i0_w =
// w * C / TEAM: C / TEAM low limbs (emitted one per outer iteration) + C high limbs (the column array once its deferred carries are
// resolved) -- exactly ld_mul's loop over a quarter of the outer limbs.  X = sum_w 2^(64 i0_w) P_w: the low limbs are disjoint
// (limb m belongs to slice m / (C / TEAM)); high limb t of P_w has weight i0_w + C / TEAM + t.
#define K3_TEAM 4
template <int E> struct TeamBuf {         // one buffer of a team's exchange area (two per team: double-buffered)
    u64 lo[64 * E];                       // emitted low limbs, by absolute limb index
    u64 sink[64 + 64 / K3_TEAM];          // where lanes 1..63 drop their copy of the per-iteration store (no exec-mask juggling)
    u64 row[K3_TEAM][2 * 64 * E];         // wave w's resolved high limbs AT THEIR WEIGHT: [(w + 1) C / TEAM, ... + C); the rest of a row
                                          // is zero from the kernel's start and never written, so the sum below reads unconditionally
};
template <int E> struct TeamCtx {
    TeamBuf<E>* buf;    // this team's two buffers
    unsigned w;         // this wave's index in the team
    unsigned parity;    // which buffer the next product uses (advanced by every call, identically in all waves of the team)
#ifdef PZ_K3_PROF
    unsigned long long t_loop = 0, t_res = 0, t_bar = 0, t_comb = 0, n_mul = 0;
#endif
};
#ifdef PZ_K3_PROF
#define K3_T0() const unsigned long long t0_ = clock64()
#define K3_T(acc, prev) const unsigned long long acc##_now = clock64(); T.acc += acc##_now - prev
#else
#define K3_T0()
#define K3_T(acc, prev)
#endif
// (forceinline, like mul_mod below: a TeamCtx / BarrettCtx whose address reaches a real call lives in scratch memory, and every
// T.parity / B.mu access of the callee becomes a private-memory round trip -- ~2000 clock units per product were exactly that)
// Wait states inside the hand-written multi-instruction asm blocks.  gfx940 / gfx950 require two wait states between a VALU
// instruction that writes an SGPR or VCC (v_readlane, v_add_co / v_addc_co carry-out) and a VALU instruction that reads it (LLVM's
// GCNHazardRecognizer: VALUWriteSGPRVALURead, the `s_nop 1` hipcc pads its own carry chains with on this target).  The recogniser
// does not look inside asm strings, so the blocks carry the `s_nop 1` themselves.  Measured round 4: identical traces without them on
// every box (the carry looked interlocked) and 12 % less time per step -- an empirical observation for a lone wave per SIMD, not an
// ISA guarantee, and in the pipelined prover K3 shares its CUs with K1 / K2 waves.  -DPZ_K3_NO_WAITSTATES builds the nop-free chain
// for measurement only.
#ifdef PZ_K3_NO_WAITSTATES
#define K3_WS ""
#else
#define K3_WS "s_nop 1\n\t"
#endif
template <int E> __device__ __forceinline__ void ld_mul_team(TeamCtx<E>& T, LD<E>& lo, LD<E>& hi, const LD<E> a, const LD<E> b) {
    constexpr unsigned C = 64 * E, SL = 64 / K3_TEAM;   // SL outer lanes (SL * E limbs) per wave
    u64 col[E];
    u32 cc[E];
    LD<E> plo;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        col[e] = 0;
        cc[e] = 0;
        plo.v[e] = 0;
    }
    const unsigned lane = lane_id();
    const unsigned j0 = T.w * SL;
    K3_T0();
    TeamBuf<E>& B = T.buf[T.parity & 1u];
    T.parity ^= 1u;
    if constexpr (E == 1) {
        // The same systolic step on 32-bit words with explicit carries: hipcc's code for the u64 version below is ~38 VALU instructions
        // per outer limb (64-bit additions as v_lshl_add_u64 at ~9.5 cycles, carries by 64-bit compares); this one is 5 mads + 2 DPP
        // moves + 2 readlanes + 6 carry instructions.  Column of this lane: (c1:c0) + c2 * 2^64; the finished low limb of every
        // iteration is lane 0's column, stored straight into the team's exchange area.
        const u32 b0 = (u32)b.v[0], b1 = (u32)(b.v[0] >> 32);
        const u32 a_lo = (u32)a.v[0], a_hi = (u32)(a.v[0] >> 32);
        // (1) the SL products A_jj * b of this wave's outer limbs: four mads each, independent of the column chain and of each other,
        // so they issue back to back (a mad's result is ~20 cycles away: chained through the column they made the loop latency-bound)
        u32 p0[SL], p1[SL], p2[SL], p3[SL];
        const u32 one = 1u;
#pragma unroll
        for (unsigned jl = 0; jl < SL; ++jl) {
            const unsigned jj = j0 + jl;
            const u32 A0 = __builtin_amdgcn_readlane(a_lo, jj), A1 = __builtin_amdgcn_readlane(a_hi, jj);
            u64 xx = 0;
            asm(K3_WS "v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(xx) : "s"(A0), "v"(b0) : "vcc");   // A0 / A1 come from v_readlane
            u64 y = xx >> 32;
            asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(y) : "s"(A0), "v"(b1) : "vcc");
            u64 z = (u32)y;
            asm(K3_WS "v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(z) : "s"(A1), "v"(b0) : "vcc");
            u64 w = y >> 32;
            asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w) : "s"(A1), "v"(b1) : "vcc");
            const u32 zh = (u32)(z >> 32);
            asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w) : "v"(zh), "v"(one) : "vcc");   // A * b < 2^128: no carry out
            p0[jl] = (u32)xx;
            p1[jl] = (u32)z;
            p2[jl] = (u32)w;
            p3[jl] = (u32)(w >> 32);
        }
        // (2) the column chain: additions only, every carry consumer behind its two wait states (K3_WS above)
        u32 c0 = 0, c1 = 0, c2 = 0;
        volatile u64* lo_dst = lane == 0 ? &B.lo[j0] : &B.sink[lane];   // one ds_write_b64 with an immediate offset per iteration
#pragma unroll
        for (unsigned jl = 0; jl < SL; ++jl) {
            asm("v_add_co_u32 %0, vcc, %0, %3\n\t" K3_WS "v_addc_co_u32 %1, vcc, %1, %4, vcc\n\t" K3_WS "v_addc_co_u32 %2, vcc, 0, %2, vcc"
                : "+v"(c0), "+v"(c1), "+v"(c2) : "v"(p0[jl]), "v"(p1[jl]) : "vcc");
            lo_dst[jl] = ((u64)c1 << 32) | c0;     // lane 0: the finished low limb of this outer limb; other lanes: into the sink
            // shift one limb down: new column = column of lane + 1 (without its overflow count) + high half of the product + this
            // lane's overflow count
            u32 t0 = dpp_down1(c0), t1 = dpp_down1(c1), k = 0;
            asm("v_add_co_u32 %0, vcc, %0, %3\n\t" K3_WS "v_addc_co_u32 %1, vcc, %1, %4, vcc\n\t" K3_WS "v_addc_co_u32 %2, vcc, 0, %2, vcc"
                : "+v"(t0), "+v"(t1), "+v"(k) : "v"(p2[jl]), "v"(p3[jl]) : "vcc");
            asm("v_add_co_u32 %0, vcc, %0, %3\n\t" K3_WS "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t" K3_WS "v_addc_co_u32 %2, vcc, 0, %2, vcc"
                : "+v"(t0), "+v"(t1), "+v"(k) : "v"(c2) : "vcc");
            c0 = t0;
            c1 = t1;
            c2 = k;
        }
        const u64 x = ((u64)c1 << 32) | c0;
        col[0] = x;
        cc[0] = c2;
    } else {
#ifndef PZ_K3_TEAM_UNROLL
#define PZ_K3_TEAM_UNROLL 16
#endif
#pragma unroll PZ_K3_TEAM_UNROLL
    for (unsigned jl = 0; jl < SL; ++jl) {
        const unsigned jj = j0 + jl;    // wave-uniform: v_readlane takes it from an SGPR
#pragma unroll
        for (int ee = 0; ee < E; ++ee) {
            const u64 A = bcast64(a.v[ee], jj);
            u64 pend = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                u64 ph, pl;
                mul64(A, b.v[e], ph, pl);
                u64 t = col[e] + pl;
                cc[e] += t < pl;
                col[e] = t;
                if (e + 1 < E) {
                    u64 t2 = col[e + 1] + ph;
                    cc[e + 1] += t2 < ph;
                    col[e + 1] = t2;
                } else {
                    pend = ph;
                }
            }
            const u64 emit = bcast64(col[0], 0);
            if (lane == jj) plo.v[ee] = emit;
            const u64 n0 = shfl_down1(col[0]);
            u64 ncol[E];
            u32 ncc[E];
#pragma unroll
            for (int e = 0; e + 1 < E; ++e) {
                u64 t = col[e + 1] + cc[e];
                ncc[e] = (t < col[e + 1]);
                ncol[e] = t;
            }
            {
                u64 t = n0 + pend;
                u32 k = (t < pend);
                u64 t2 = t + cc[E - 1];
                k += t2 < t;
                ncol[E - 1] = t2;
                ncc[E - 1] = k;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                col[e] = ncol[e];
                cc[e] = ncc[e];
            }
        }
    }
    }
    K3_T(t_loop, t0_);
    // this wave's high limbs: col + (cc shifted up by one limb); cannot carry out (P_w < 2^(64 (C + SL E)))
    LD<E> cv, sh, ph_;
#pragma unroll
    for (int e = 0; e < E; ++e) cv.v[e] = col[e];
    sh.v[0] = shfl_up1((u64)cc[E - 1]);
#pragma unroll
    for (int e = 1; e < E; ++e) sh.v[e] = cc[e - 1];
    (void)ld_add(ph_, cv, sh, false);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (E > 1 && lane >= j0 && lane < j0 + SL) B.lo[lane * E + e] = plo.v[e];   // (E == 1: stored inside the loop)
        B.row[T.w][(T.w + 1) * SL * E + lane * E + e] = ph_.v[e];
    }
    K3_T(t_res, t_loop_now);
    __syncthreads();   // the team is the workgroup
    K3_T(t_bar, t_res_now);
    // every wave sums the partials: limb m = lane * E + e of the low half, m + C of the high half.  The 64-bit terms are added as two
    // 32-bit digits into 64-bit accumulators (a mad by one: no carry out to catch, one issue slot per digit), then the digits are
    // put back together: limb + an overflow count below 2^3, resolved by two look-ahead additions
    LD<E> s_lo, s_hi, c_lo, c_hi;
    const u32 one_ = 1u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned m = lane * E + e;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u64 d0 = 0, d1 = 0;
            if (half == 0) {
                const u64 v = B.lo[m];
                d0 = (u32)v;
                d1 = v >> 32;
            }
#pragma unroll
            for (unsigned w = 0; w < K3_TEAM; ++w) {
                const u64 v = B.row[w][half * C + m];
                const u32 v0 = (u32)v, v1 = (u32)(v >> 32);
                asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(d0) : "v"(v0), "v"(one_) : "vcc");
                asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(d1) : "v"(v1), "v"(one_) : "vcc");
            }
            const u64 mid = (d0 >> 32) + (u32)d1;
            const u64 limb = (u64)(u32)d0 | (mid << 32), cnt = (mid >> 32) + (d1 >> 32);
            if (half == 0) { s_lo.v[e] = limb; c_lo.v[e] = cnt; }
            else { s_hi.v[e] = limb; c_hi.v[e] = cnt; }
        }
    }
    // X = S + (carry counts shifted up one limb): low half, then the high half with the low half's carry out
    LD<E> k_lo, k_hi;
    const u64 top_cnt = bcast64(c_lo.v[E - 1], 63);    // count of the low half's top limb moves into the high half's limb 0
    k_lo.v[0] = shfl_up1(c_lo.v[E - 1]);
    k_hi.v[0] = shfl_up1(c_hi.v[E - 1]);
    if (lane == 0) k_hi.v[0] = top_cnt;
#pragma unroll
    for (int e = 1; e < E; ++e) {
        k_lo.v[e] = c_lo.v[e - 1];
        k_hi.v[e] = c_hi.v[e - 1];
    }
    const bool co = ld_add(lo, s_lo, k_lo, false);
    (void)ld_add(hi, s_hi, k_hi, co);
    K3_T(t_comb, t_bar_now);
#ifdef PZ_K3_PROF
    T.n_mul++;
#endif
}

// per-wave LDS scratch: 4*64*E u64 (a 2C-limb value twice)
template <int E> struct BarrettCtx {
    LD<E> M;      // modulus << s (top bit of the capacity set)
    LD<E> mu;     // floor(2^(2N)/M') - 2^N, N = 64*64*E
    unsigned s;   // normalisation shift in bits
    unsigned limbs;  // real limb count L of operands / results
    volatile u64* sm;  // this wave's LDS scratch, 2*64*E limbs
};

// y = (x_hi:x_lo) << s, as two halves; returns true if non-zero bits were shifted out
template <int E>
__device__ __forceinline__ bool shl_2c(const BarrettCtx<E>& B, LD<E>& ylo, LD<E>& yhi, const LD<E>& xlo, const LD<E>& xhi) {
    constexpr unsigned C = 64 * E;
    const unsigned ls = B.s >> 6, bs = B.s & 63;
    const unsigned lane = lane_id();
    if (E == 1 && ls == 0) {
        // a shift below one limb (a modulus that nearly fills the capacity: n^2 of a full-size key): neighbours by DPP, no LDS round trip
        if (bs == 0) {
            ylo = xlo;
            yhi = xhi;
            return false;
        }
        const u64 pl = shfl_up1(xlo.v[0]);
        u64 ph = shfl_up1(xhi.v[0]);
        const u64 top_lo = bcast64(xlo.v[0], 63), top_hi = bcast64(xhi.v[0], 63);
        if (lane == 0) ph = top_lo;
        ylo.v[0] = (xlo.v[0] << bs) | (pl >> (64 - bs));
        yhi.v[0] = (xhi.v[0] << bs) | (ph >> (64 - bs));
        return (top_hi >> (64 - bs)) != 0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        B.sm[lane * E + e] = xlo.v[e];
        B.sm[C + lane * E + e] = xhi.v[e];
    }
    __builtin_amdgcn_wave_barrier();
    bool lost = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned t = h * C + lane * E + e;
            u64 cur = t >= ls ? B.sm[t - ls] : 0;
            u64 prv = t >= ls + 1 ? B.sm[t - ls - 1] : 0;
            u64 v = bs ? (cur << bs) | (prv >> (64 - bs)) : cur;
            if (h == 0) ylo.v[e] = v; else yhi.v[e] = v;
            // source limb t is shifted (partly) out if t + ls >= 2C, or its top bs bits if t + ls == 2C-1
            const u64 src = B.sm[t];
            if (t + ls >= 2 * C) lost |= src != 0;
            else if (t + ls == 2 * C - 1 && bs) lost |= (src >> (64 - bs)) != 0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    return __ballot(lost) != 0;
}
// y = x >> s (single capacity-sized value)
template <int E> __device__ __forceinline__ LD<E> shr_c(const BarrettCtx<E>& B, const LD<E>& x) {
    constexpr unsigned C = 64 * E;
    const unsigned ls = B.s >> 6, bs = B.s & 63;
    const unsigned lane = lane_id();
    if (E == 1 && ls == 0) {   // see shl_2c
        if (bs == 0) return x;
        LD<E> y;
        y.v[0] = (x.v[0] >> bs) | (shfl_down1(x.v[0]) << (64 - bs));
        return y;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) B.sm[lane * E + e] = x.v[e];
    __builtin_amdgcn_wave_barrier();
    LD<E> y;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned t = lane * E + e;
        u64 cur = t + ls < C ? B.sm[t + ls] : 0;
        u64 nxt = t + ls + 1 < C ? B.sm[t + ls + 1] : 0;
        y.v[e] = bs ? (cur >> bs) | (nxt << (64 - bs)) : cur;
    }
    __builtin_amdgcn_wave_barrier();
    return y;
}
// y = x << s within the capacity (bits shifted out are dropped; used for the modulus only)
template <int E> __device__ __forceinline__ LD<E> shl_c(const BarrettCtx<E>& B, const LD<E>& x) {
    const unsigned ls = B.s >> 6, bs = B.s & 63;
    const unsigned lane = lane_id();
#pragma unroll
    for (int e = 0; e < E; ++e) B.sm[lane * E + e] = x.v[e];
    __builtin_amdgcn_wave_barrier();
    LD<E> y;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned t = lane * E + e;
        u64 cur = t >= ls ? B.sm[t - ls] : 0;
        u64 prv = t >= ls + 1 ? B.sm[t - ls - 1] : 0;
        y.v[e] = bs ? (cur << bs) | (prv >> (64 - bs)) : cur;
    }
    __builtin_amdgcn_wave_barrier();
    return y;
}

// bit length of a capacity-sized integer (0 for zero)
template <int E> __device__ __forceinline__ unsigned ld_bitlen(const LD<E>& a) {
    unsigned best = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (a.v[e]) best = (lane_id() * E + e) * 64 + (64 - __clzll(a.v[e]));
    }
    // max over lanes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    return best;
}

// Barrett constants for modulus m (must be non-zero): returns false if m == 0
template <int E> __device__ __forceinline__ bool barrett_setup(BarrettCtx<E>& B, const LD<E> m) {   // (inlined: B stays in registers)
    constexpr unsigned N = 64 * 64 * E;
    const unsigned bl = ld_bitlen(m);
    if (bl == 0) return false;
    B.s = N - bl;
    B.M = shl_c(B, m);
    // R0 = 2^N - M' ; mu' = floor(2^N * R0 / M') by N steps of restoring division
    LD<E> R, zero = ld_zero<E>();
    (void)ld_sub(R, zero, B.M);  // wraps to 2^N - M'
    LD<E> mu = ld_zero<E>();
    LD<E> d;
    if (!ld_sub(d, R, B.M)) {
        // R0 >= M' only when M' == 2^(N-1): reciprocal would be 2^N, clamp to 2^N - 1
#pragma unroll
        for (int e = 0; e < E; ++e) mu.v[e] = ~0ull;
        B.mu = mu;
        return true;
    }
    for (unsigned i = 0; i < N; ++i) {
        // R <<= 1 (top bit out in `top`)
        u64 carry_in = shfl_up1(R.v[E - 1] >> 63);
        const bool top = (bcast64(R.v[E - 1], 63) >> 63) != 0;
#pragma unroll
        for (int e = E - 1; e >= 1; --e) R.v[e] = (R.v[e] << 1) | (R.v[e - 1] >> 63);
        R.v[0] = (R.v[0] << 1) | carry_in;
        const bool borrow = ld_sub(d, R, B.M);
        const bool bit = top || !borrow;
        if (bit) R = d;
        // mu = (mu << 1) | bit
        u64 mc = shfl_up1(mu.v[E - 1] >> 63);
#pragma unroll
        for (int e = E - 1; e >= 1; --e) mu.v[e] = (mu.v[e] << 1) | (mu.v[e - 1] >> 63);
        mu.v[0] = (mu.v[0] << 1) | mc;
        if (bit && lane_id() == 0) mu.v[0] |= 1ull;
    }
    B.mu = mu;
    return true;
}

enum { ST_OK = 0, ST_RANGE = 1, ST_ZERO_MOD = 2, ST_INTERNAL = 4, ST_TIMEOUT = 8 };

// the product routine of a mul_mod: one wave on its own (k_mul_mod) or a team of waves (k_pow_mod_chain)
template <int E> struct SoloMul {
    __device__ __forceinline__ void operator()(LD<E>& lo, LD<E>& hi, const LD<E>& a, const LD<E>& b) { ld_mul(lo, hi, a, b); }
};
template <int E> struct TeamMul {
    TeamCtx<E>* T;
    __device__ __forceinline__ void operator()(LD<E>& lo, LD<E>& hi, const LD<E>& a, const LD<E>& b) { ld_mul_team(*T, lo, hi, a, b); }
};
#ifdef PZ_K3_PROF
__device__ unsigned long long g_k3_phase[16];
#define K3_STAMP(i)                                                             \
    do {                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                      \
        const unsigned long long now_ = clock64();                              \
        __builtin_amdgcn_sched_barrier(0);                                      \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_k3_phase[i] += now_ - last_; \
        last_ = now_;                                                           \
    } while (0)
#define K3_STAMP0() unsigned long long last_ = clock64()
#else
#define K3_STAMP(i)
#define K3_STAMP0()
#endif
// (q, r) = divmod(a*b, modulus).  Returns status bits.
template <int E, class Mul>
__device__ __forceinline__ unsigned mul_mod(const BarrettCtx<E>& B, LD<E>& q, LD<E>& r, const LD<E> a, const LD<E> b, Mul ld_mul) {
    unsigned st = ST_OK;
    K3_STAMP0();
    LD<E> xlo, xhi;
    ld_mul(xlo, xhi, a, b);
    K3_STAMP(0);
    LD<E> ylo, yhi;
    if (shl_2c(B, ylo, yhi, xlo, xhi)) st |= ST_RANGE;  // quotient cannot fit the capacity
    K3_STAMP(1);
    // qhat = yhi + hi(yhi * mu)
    LD<E> plo, phi;
    ld_mul(plo, phi, yhi, B.mu);
    K3_STAMP(2);
    LD<E> qh;
    if (ld_add(qh, yhi, phi, false)) st |= ST_RANGE;
    K3_STAMP(3);
    // r' = y - qhat*M'  (low capacity limbs + one limb above)
    LD<E> zlo, zhi;
    ld_mul(zlo, zhi, qh, B.M);
    K3_STAMP(4);
    LD<E> rr;
    const bool b0 = ld_sub(rr, ylo, zlo);
    K3_STAMP(5);
    u64 top = bcast64(yhi.v[0], 0) - bcast64(zhi.v[0], 0) - (b0 ? 1ull : 0ull);
    for (int it = 0; it < 8; ++it) {
        LD<E> d;
        const bool borrow = ld_sub(d, rr, B.M);
        if (top == 0 && borrow) break;  // 0 <= r' < M'
        if (it == 7) { st |= ST_INTERNAL; break; }
        rr = d;
        top -= borrow ? 1ull : 0ull;
        LD<E> z = ld_zero<E>();
        if (ld_add(qh, qh, z, true)) st |= ST_RANGE;
    }
    K3_STAMP(6);
    r = shr_c(B, rr);
    q = qh;
    if (ld_exceeds(q, B.limbs)) st |= ST_RANGE;
    K3_STAMP(7);
    return st;
}

// ------------------------------------------------------------------------------------------------
// what the kernels share.  Every helper is forceinline and takes its contexts by reference (see ld_mul_team: a TeamCtx / BarrettCtx
// whose address reaches a real call lives in scratch memory).
// ------------------------------------------------------------------------------------------------
// The Barrett block of a modulus, written once by k_tally_setup and read by every team: M' | mu | modulus (C words each) | shift | ok.
__host__ __device__ constexpr size_t mod_block_words(unsigned C) { return (size_t)3 * C + 2; }
template <int E, class W> __device__ __forceinline__ W* block_mu(W* blk) { return blk + 64 * E; }
template <int E, class W> __device__ __forceinline__ W* block_modulus(W* blk) { return blk + 2 * 64 * E; }
template <int E, class W> __device__ __forceinline__ W* block_shift(W* blk) { return blk + mod_block_words(64 * E) - 2; }
template <int E, class W> __device__ __forceinline__ W* block_ok(W* blk) { return blk + mod_block_words(64 * E) - 1; }   // 0: a zero modulus

// this wave's place in its team (the workgroup); the exchange rows are zero outside the ranges the products write (TeamBuf::row)
template <int E> __device__ __forceinline__ void team_init(TeamCtx<E>& T, TeamBuf<E> (&buf)[2]) {
    T.buf = buf;
    T.w = threadIdx.x >> 6;
    T.parity = 0;
    u64* z = (u64*)buf;
    for (unsigned t = threadIdx.x; t < sizeof(buf) / 8; t += blockDim.x) z[t] = 0;
    __syncthreads();
}
// the constants of a block's modulus for operands of `limbs` limbs; scratch: this wave's 2 * 64 * E words of LDS
template <int E> __device__ __forceinline__ void barrett_from_block(BarrettCtx<E>& B, const u64* blk, unsigned limbs, volatile u64* scratch) {
    B.sm = scratch;
    B.limbs = limbs;
    B.s = (unsigned)*block_shift<E>(blk);
    B.M = ld_load<E>(blk, 64 * E);
    B.mu = ld_load<E>(block_mu<E>(blk), 64 * E);
}
// one step's record: a | b | q | r, L limbs each
template <int E> __device__ __forceinline__ void rec_store(u64* o, const LD<E>& a, const LD<E>& b, const LD<E>& q, const LD<E>& r, unsigned L) {
    ld_store(o, a, L);
    ld_store(o + L, b, L);
    ld_store(o + 2 * L, q, L);
    ld_store(o + 3 * L, r, L);
}
// acc = bit ? r : acc under a lane-wise mask over both candidates: a SECRET bit never becomes a branch or an address
template <int E> __device__ __forceinline__ void ld_select(LD<E>& acc, const LD<E>& r, u64 bit) {
    u64 keep = 0ull - (bit & 1);
    asm volatile("" : "+v"(keep));   // a per-lane value from here on: nothing below can become a branch
#pragma unroll
    for (int e = 0; e < E; ++e) acc.v[e] = (r.v[e] & keep) | (acc.v[e] & ~keep);
}
// BigUintChip::pow_mod's uniform schedule over exactly `bits` bits of exp, LSB first: (acc, sq) then (sq, sq) for EVERY bit, acc takes
// the product only where the bit is set (ld_select: the exponent may be secret; bit t is read from word t / 64, an address that follows
// the loop counter alone).  acc *= sq^exp, sq leaves as the trailing square.  rec (may be null: the values only): two records per bit.
// Returns status bits.
template <int E>
__device__ __forceinline__ unsigned pow_mod_uniform(const BarrettCtx<E>& B, TeamCtx<E>& T, LD<E>& acc, LD<E>& sq, const u64* exp, unsigned bits,
                                                    u64* rec) {
    const size_t L = B.limbs;
    unsigned st = ST_OK;
    for (unsigned t = 0; t < bits; ++t) {
        LD<E> q, r;
        st |= mul_mod(B, q, r, acc, sq, TeamMul<E>{&T});
        if (rec) rec_store(rec, acc, sq, q, r, B.limbs);
        ld_select(acc, r, exp[t >> 6] >> (t & 63));
        st |= mul_mod(B, q, r, sq, sq, TeamMul<E>{&T});
        if (rec) {
            rec_store(rec + 4 * L, sq, sq, q, r, B.limbs);
            rec += 8 * L;
        }
        sq = r;
    }
    return st;
}
// decryption's last step on U = c^lambda (or the partials' product) mod n^2, by n's Barrett context at this capacity: U mod n must be 1,
// m = floor(U / n) * mu mod n (zero where it is not).  Returns whether U mod n != 1.
template <int E>
__device__ __forceinline__ bool lfn_tail(const BarrettCtx<E>& N, TeamCtx<E>& T, LD<E>& m, const LD<E>& U, const u64* mu, unsigned Ln, unsigned& st) {
    const LD<E> one = ld_small<E>(1);
    LD<E> x, rem, q;
    st |= mul_mod(N, x, rem, U, one, TeamMul<E>{&T});
    bool ne = false;
#pragma unroll
    for (int e = 0; e < E; ++e) ne |= rem.v[e] != one.v[e];
    const bool bad = __ballot(ne) != 0;
    st |= mul_mod(N, q, m, x, ld_load<E>(mu, Ln), TeamMul<E>{&T});
    if (bad) m = ld_zero<E>();
    return bad;
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct ChainDesc {
    const u64* modulus;  // limbs_mod limbs; if square_modulus: n (limbs_mod = Ln) and the modulus is n*n
    const u64* base;     // limbs_base limbs
    const u64* exp;      // exp_limbs limbs
    u64* steps;          // optional trace output (a|b|q|r per step, L limbs each)
    u64* result;         // L limbs
    u32* n_steps;        // optional
    u32* status;         // status bits (atomicOr)
    u32 limbs_mod, limbs_base, exp_limbs;
    u32 L;               // operand/result limb count (limbs of the modulus n^2)
    u32 square_modulus;
    u32 steps_cap;
    u32 uniform_bits;    // != 0: pow_mod with the exponent's bits IN the circuit: exactly this many
                         // bits, per bit the step (acc, sq) then the step (sq, sq); acc takes the product only if the bit is set
    u64* sq_buf;         // hand-off from the squarer to the multiplier: square i at sq_buf + i * L (max exponent bits x L limbs)
    u32* ready;          // number of squares published so far (zeroed by the host before the launch)
    u32 spin_limit;      // polls a multiplier wave makes for one square before it gives up (ST_TIMEOUT); K3_SPIN_LIMIT unless a test lowers it
    u32 test_no_publish; // test hook (PZ_K3_TEST_NO_PUBLISH): the squarer never advances `ready`, so the bounded wait is exercised
};
#define K3_SPIN_LIMIT (1u << 27)   // x >= 100 ns per poll: tens of seconds, far beyond any chain

template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_pow_mod_chain(const ChainDesc* __restrict__ descs, unsigned n_chains,
                                                                                    u32* __restrict__ ticket) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];   // per-wave shift scratch
    __shared__ TeamBuf<E> s_team[2];            // [parity]
    __shared__ unsigned s_role, s_dead_step;
    // Roles by ARRIVAL, not by workgroup id: the first n workgroups that start running are the squarers of chains 0..n-1, the next n the
    // multipliers.  A multiplier only ever waits for the squarer of its chain, whose ticket is lower, i.e. which has already started
    // (and a squarer waits for nobody), so forward progress needs nothing from the dispatcher but that a workgroup which has started
    // keeps running -- no assumption on the order in which workgroup ids are dispatched, or on how many are resident.
    if (threadIdx.x == 0) {
        s_role = atomicAdd(ticket, 1u);
        s_dead_step = 0;
    }
    __syncthreads();
    const unsigned role = s_role;
    const bool squarer = role < n_chains;
    const ChainDesc D = descs[squarer ? role : role - n_chains];
#ifdef PZ_K3_PROF
    const unsigned long long k_t0 = clock64();
#endif
    const unsigned wave = threadIdx.x >> 6;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    const bool writer = wave == 0;   // the four waves of the team hold the same values: one of them writes
    BarrettCtx<E> B;
    B.sm = s_scratch[wave];
    B.limbs = D.L;
    B.s = 0;
    unsigned st = ST_OK;
    LD<E> m = ld_load<E>(D.modulus, D.limbs_mod);
    if (D.square_modulus) {
        LD<E> lo, hi;
        tmul(lo, hi, m, m);
        m = lo;
    }
    const bool mod_ok = barrett_setup(B, m);
    if (!mod_ok) st |= ST_ZERO_MOD;
    // exponent bit length (uniform)
    unsigned nbits = 0;
    for (int i = (int)D.exp_limbs - 1; i >= 0; --i) {
        u64 w = D.exp[i];
        if (w) {
            nbits = (unsigned)i * 64 + (64 - __clzll(w));
            break;
        }
    }
    LD<E> sq = ld_load<E>(D.base, D.limbs_base);
    LD<E> acc = ld_small<E>(1);
    unsigned step_idx = 0;  // index of this bit's first step
    const bool uni = D.uniform_bits != 0;
    if (uni) nbits = D.uniform_bits;
    if (mod_ok) {
        for (unsigned i = 0; i < nbits; ++i) {
            const bool bit = (i >> 6) < D.exp_limbs && ((D.exp[i >> 6] >> (i & 63)) & 1);
            // reference schedule (pow_mod_fixed_exp): squaring step, then the multiply step on set bits;
            // uniform schedule (pow_mod): multiply step for EVERY bit, then the squaring step
            const unsigned sq_slot = uni ? step_idx + 1 : step_idx, mul_slot = uni ? step_idx : step_idx + 1;
            if (squarer) {
                // publish sq_i: the limbs leave as agent-scope stores BEFORE the step, the counter follows AFTER it with RELEASE
                // semantics at agent scope (the multiplier reads it and then fences with ACQUIRE: a textbook release / acquire pair, no
                // reliance on how gfx950 orders relaxed accesses).  Measured (profiles/r05_k3_ab_waitstates_release.txt): the release
                // costs 0.1 us of a 8.9-us step -- by the time the step's products are done the limb stores have long been
                // acknowledged, so its write-back / wait finds nothing in flight.  (-DPZ_K3_RELAXED_PUBLISH: round 4's relaxed store
                // behind s_waitcnt vmcnt(0), for measurement.)
                if (writer) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const unsigned idx = lane_id() * E + e;
                        if (idx < D.L) __hip_atomic_store(D.sq_buf + (size_t)i * D.L + idx, sq.v[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                LD<E> q, r;
                st |= mul_mod(B, q, r, sq, sq, tmul);
                if (writer && !D.test_no_publish) {
#ifndef PZ_K3_RELAXED_PUBLISH
                    // every lane of the writer wave stored limbs: all of them wait for their own stores, lane 0 then releases the counter
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane_id() == 0) __hip_atomic_store(D.ready, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane_id() == 0) __hip_atomic_store(D.ready, i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
                }
                if (writer && D.steps && sq_slot < D.steps_cap) rec_store(D.steps + (size_t)sq_slot * 4 * D.L, sq, sq, q, r, D.L);
                sq = r;
            } else if (bit || uni) {
                // wait for square i (every wave polls for itself: no workgroup barrier on this path); the squarer never waits for
                // anyone and was dispatched first, so the wait is bounded by its progress
                // (bounded: ~2^27 polls of >= 100 ns are tens of seconds, far beyond any chain -- a wave must have an exit it reaches
                // whatever happens to the other workgroup; the step then runs on stale limbs and the status says so)
                for (unsigned spins = 0; __hip_atomic_load(D.ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= i; ++spins) {
                    if (spins > D.spin_limit) {
                        st |= ST_TIMEOUT;
                        s_dead_step = i + 1;   // every wave of the team gives up at the END of this step (see below): same value from all
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                // acquire at agent scope: orders the limb loads below after the counter's (the compiler and the hardware both), and
                // invalidates what this CU may hold of the hand-off lines
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                LD<E> cur;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const unsigned idx = lane_id() * E + e;
                    cur.v[e] = idx < D.L ? __hip_atomic_load(D.sq_buf + (size_t)i * D.L + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                }
                LD<E> q, r;
                st |= mul_mod(B, q, r, acc, cur, tmul);
                if (writer && D.steps && mul_slot < D.steps_cap) rec_store(D.steps + (size_t)mul_slot * 4 * D.L, acc, cur, q, r, D.L);
                if (bit) acc = r;   // select(bit, muled, acc)
                // a wave whose wait ran out has said so BEFORE this step's product barriers; every wave reads the flag after them,
                // so the whole team leaves at the same step (a wave leaving alone would hang the others at the next barrier)
                const unsigned dead = *(volatile unsigned*)&s_dead_step;
                if (dead != 0 && dead <= i + 1) {
                    st |= ST_TIMEOUT;
                    break;
                }
            }
            step_idx += (bit || uni) ? 2 : 1;
        }
    }
    if (D.steps && step_idx > D.steps_cap && !(st & ST_TIMEOUT)) st |= ST_INTERNAL;
    if (!squarer && writer && !(st & ST_TIMEOUT)) {   // after a timeout neither the result nor the step count is written
        ld_store(D.result, acc, D.L);
        if (D.n_steps && lane_id() == 0) *D.n_steps = step_idx;
    }
    if (st && lane_id() == 0) atomicOr(D.status, st);
#ifdef PZ_K3_PROF
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        printf("K3 phases (cycles per step, squarer wg 0): mul1 %llu shl %llu mul2 %llu add %llu mul3 %llu sub %llu fixup %llu shr %llu | whole kernel %llu per bit\n",
               g_k3_phase[0] / nbits, g_k3_phase[1] / nbits, g_k3_phase[2] / nbits, g_k3_phase[3] / nbits, g_k3_phase[4] / nbits, g_k3_phase[5] / nbits,
               g_k3_phase[6] / nbits, g_k3_phase[7] / nbits, (unsigned long long)(clock64() - k_t0) / nbits);
        for (int i = 0; i < 16; ++i) g_k3_phase[i] = 0;
    }
    if (lane_id() == 0 && wave == 0 && (blockIdx.x == 0 || blockIdx.x == n_chains))
        printf("K3 prof wg %u: products %llu; cycles per product: loop %llu, resolve+lds %llu, barrier %llu, combine %llu; total cycles %llu\n", blockIdx.x,
               T.n_mul, T.t_loop / T.n_mul, T.t_res / T.n_mul, T.t_bar / T.n_mul, T.t_comb / T.n_mul, (unsigned long long)(clock64() - k_t0));
#endif
}

struct MulDesc {
    const u64 *a, *b, *modulus;
    u64 *q, *r;
    u64* step;  // optional a|b|q|r record
    u32* status;
    u32 limbs_a, limbs_b, limbs_mod, L, square_modulus;
};

template <int E> __global__ __launch_bounds__(64) void k_mul_mod(const MulDesc* __restrict__ descs) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[2 * C];
    const MulDesc D = descs[blockIdx.x];
    BarrettCtx<E> B;
    B.sm = s_scratch;
    B.limbs = D.L;
    B.s = 0;
    unsigned st = ST_OK;
    LD<E> m = ld_load<E>(D.modulus, D.limbs_mod);
    if (D.square_modulus) {
        LD<E> lo, hi;
        ld_mul(lo, hi, m, m);
        m = lo;
    }
    if (!barrett_setup(B, m)) {
        if (lane_id() == 0) atomicOr(D.status, (u32)ST_ZERO_MOD);
        return;
    }
    LD<E> a = ld_load<E>(D.a, D.limbs_a), b = ld_load<E>(D.b, D.limbs_b);
    LD<E> q, r;
    st |= mul_mod(B, q, r, a, b, SoloMul<E>());
    if (D.q) ld_store(D.q, q, D.L);
    if (D.r) ld_store(D.r, r, D.L);
    if (D.step) rec_store(D.step, a, b, q, r, D.L);
    if (st && lane_id() == 0) atomicOr(D.status, st);
}

// ---- the product tree of a tally (pz_paillier_tally): prod c_i mod n^2 as ceil(log2 B) levels of independent mul_mods.  One launch
// per level, ordered by the stream alone -- no workgroup waits for another.  One team per product (the last levels are a handful of
// products: latency-bound, like a chain step).  A workgroup finds its operands from its index: element e of the level's list is
// `elems + e * stride` for e < n_regular (level 0: the ciphertext array; above: the remainders of the records one level down) and
// `tail` for the odd element carried up without a product; it writes its own record in place.  The Barrett constants of n^2 are
// computed once (k_tally_setup: the reciprocal is 64 * 64 * E steps of restoring division) and read by every workgroup:
// mod = M' | mu | n^2 (C words each) | shift | ok.  (square = 0: the same block for n itself -- the decryption's second modulus.)
template <int E> __global__ __launch_bounds__(64) void k_tally_setup(const u64* __restrict__ n, unsigned Ln, unsigned square,
                                                                      u64* __restrict__ mod, u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[2 * C];
    BarrettCtx<E> B;
    B.sm = s_scratch;
    B.limbs = square ? 2 * Ln : Ln;
    B.s = 0;
    LD<E> m = ld_load<E>(n, Ln), lo = m, hi;
    if (square) ld_mul(lo, hi, m, m);
    const bool ok = barrett_setup(B, lo);
    if (ok) {
        ld_store(mod, B.M, C);
        ld_store(block_mu<E>(mod), B.mu, C);
        ld_store(block_modulus<E>(mod), lo, C);
    }
    if (lane_id() == 0) {
        *block_shift<E>(mod) = ok ? B.s : 0;
        *block_ok<E>(mod) = ok ? 1 : 0;
        if (!ok) atomicOr(status, (u32)ST_ZERO_MOD);
    }
}
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_tally_level(const u64* __restrict__ mod, const u64* __restrict__ elems,
                                                                                  size_t stride, unsigned n_regular, const u64* __restrict__ tail,
                                                                                  u64* __restrict__ recs, unsigned L, u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup of every level)
    const unsigned wave = threadIdx.x >> 6;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const LD<E> n2 = ld_load<E>(block_modulus<E>(mod), C);
    const size_t ia = 2 * (size_t)blockIdx.x, ib = ia + 1;       // (only b can be the carried element: it is the list's last)
    const LD<E> a = ld_load<E>(elems + ia * stride, L);
    const LD<E> b = ld_load<E>(ib < n_regular ? elems + ib * stride : tail, L);
    unsigned st = ST_OK;
    LD<E> d;
    if (!ld_sub(d, a, n2) || !ld_sub(d, b, n2)) st |= ST_RANGE;   // an operand >= n^2: the circuit's r < n^2 check of whatever made it fails
    LD<E> q, r;
    st |= mul_mod(B, q, r, a, b, tmul);
    if (wave == 0) rec_store(recs + (size_t)blockIdx.x * 4 * L, a, b, q, r, L);   // the four waves of the team hold the same values: one of them writes
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- the chains of a weighted tally (pz_paillier_wtally): power_i = c_i^w_i mod n^2 by BigUintChip::pow_mod's uniform schedule over
// exactly w_bits bits, LSB first: (acc, sq) then (sq, sq) for EVERY bit, acc takes the product only where the bit is set.  One team
// per chain runs both steps of every bit itself: no ticket, no hand-off, no workgroup waits on another (k_pow_mod_chain's two
// workgroups per chain buy latency when chains are few; here they are many and short).  The Barrett constants come from
// k_tally_setup, computed once for all chains.  recs (may be null: the value only): chain i, bit j at records 2 (i w_bits + j) and
// the next; powers: L limbs per chain, the level-0 list of the product tree.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_wtally_pow(const u64* __restrict__ mod, const u64* __restrict__ cts,
                                                                                 const u64* __restrict__ weights, unsigned w_bits,
                                                                                 u64* __restrict__ recs, u64* __restrict__ powers, unsigned L,
                                                                                 u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    const unsigned wave = threadIdx.x >> 6;
    TeamCtx<E> T;
    team_init(T, s_team);
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t chain = blockIdx.x;
    LD<E> sq = ld_load<E>(cts + chain * L, L);
    LD<E> acc = ld_small<E>(1);
    unsigned st = ST_OK;
    {
        LD<E> d;
        if (!ld_sub(d, sq, ld_load<E>(block_modulus<E>(mod), C))) st |= ST_RANGE;   // a ciphertext >= n^2
    }
    const bool writer = wave == 0 && recs != nullptr;   // the four waves of the team hold the same values: one of them writes
    st |= pow_mod_uniform(B, T, acc, sq, weights + chain, w_bits, writer ? recs + chain * w_bits * 8 * (size_t)L : nullptr);
    if (wave == 0) ld_store(powers + chain * L, acc, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- the entries of a ballot (pz_paillier_ballot): c_i = g^m_i r_i^n mod n^2 for K messages under ONE key.  One team per ciphertext
// runs the entry's whole schedule itself -- g^m_i by BigUintChip::pow_mod over exactly m_bits bits (pow_mod_uniform), r_i^n by
// pow_mod_fixed_exp over n's bits, LSB first (the square of EVERY bit, then the product where the bit is set), and the final product --
// so K entries are one launch with no ticket, no spin, no hand-off.  The Barrett constants come from k_tally_setup, once for all.
// m_i and r_i are SECRET: the message's bit reaches the accumulator as a lane-wise mask over both candidates (k_dec_pow's read of its
// table), never as a branch or an address; n's bits are public and steer the second loop.  (What a mul_mod does with its VALUES is
// K3's as everywhere: the Barrett correction's trip count follows the operands.)
// recs (may be null: the values only): entry i at records i * per .. + per, per = 2 m_bits + nr + 1: the g-chain's, the r-chain's, the
// final one.  per is the host's count of the same bits the loop reads; a disagreement is ST_INTERNAL, never a write past the entry.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_ballot_enc(const u64* __restrict__ mod, const u64* __restrict__ n,
                                                                                 const u64* __restrict__ g, const u64* __restrict__ ms,
                                                                                 const u64* __restrict__ rs, unsigned m_bits, unsigned n_bits,
                                                                                 unsigned per, u64* __restrict__ recs, u64* __restrict__ c_out,
                                                                                 unsigned Ln, u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    const unsigned wave = threadIdx.x >> 6, L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t entry = blockIdx.x;
    // the four waves of the team hold the same values: one of them writes.  (A per below the g-chain's own count is the disagreement
    // the last lines flag: no record is written then.)
    const bool writer = wave == 0 && recs != nullptr && 2 * m_bits <= per;
    u64* const base = writer ? recs + entry * per * 4 * (size_t)L : nullptr;
    unsigned idx = 0, st = ST_OK;
    auto step = [&](LD<E>& r, const LD<E>& a, const LD<E>& b) {   // one recorded mul_mod
        LD<E> q;
        st |= mul_mod(B, q, r, a, b, tmul);
        if (writer && idx < per) rec_store(base + (size_t)idx * 4 * L, a, b, q, r, L);
        ++idx;
    };
    LD<E> gm = ld_small<E>(1);
    {
        LD<E> sq = ld_load<E>(g, Ln);
        st |= pow_mod_uniform(B, T, gm, sq, ms + entry, m_bits, base);
        idx = 2 * m_bits;
    }
    LD<E> rn = ld_small<E>(1);
    {
        LD<E> sq = ld_load<E>(rs + entry * Ln, Ln);
        for (unsigned i = 0; i < n_bits; ++i) {
            const LD<E> cur = sq;
            step(sq, cur, cur);
            if ((n[i >> 6] >> (i & 63)) & 1) {   // (n is the public key)
                LD<E> r;
                step(r, rn, cur);
                rn = r;
            }
        }
    }
    LD<E> c;
    step(c, gm, rn);
    if (idx != per) st |= ST_INTERNAL;
    if (wave == 0) ld_store(c_out + entry * L, c, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- the entries of a short-randomness ballot (pz_paillier_sballot): c_i = g^m_i hs^s_i mod n^2 for K messages under
// ONE key whose hs = h^n mod n^2 is public.  k_ballot_enc with its r^n chain replaced by k_partial_pow's: one team per ciphertext runs
// g^m_i over exactly m_bits bits, then hs^s_i over exactly s_bits bits (pow_mod_uniform both: (acc, sq) then (sq, sq) for EVERY bit,
// the trailing square kept), then the final product -- K entries in one launch, no team waits on another.  The Barrett constants come
// from k_tally_setup, once for all.  m_i and s_i are SECRET: bit t of s_i is read from word t / 64 of the entry's s_words words, an
// address that follows the loop counter alone, and both reach their accumulator as a lane-wise mask over both candidates (ld_select),
// never as a branch or an address.  Every trip count is a launch argument.  (What a mul_mod does with its VALUES is K3's as everywhere:
// the Barrett correction's trip count follows the operands.)  An hs >= n^2 (public) is ST_RANGE.
// recs (may be null: the values only): entry i at records i * per .. + per, per = 2 m_bits + 2 s_bits + 1: the g-chain's, the hs-chain's,
// then (gm_i, hss_i, q, c_i).  per is held against the loops' own counts before any store; a disagreement is ST_INTERNAL, never a write
// past the entry.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_sballot_enc(const u64* __restrict__ mod, const u64* __restrict__ g,
                                                                                  const u64* __restrict__ hs, const u64* __restrict__ ms,
                                                                                  const u64* __restrict__ ss, unsigned m_bits, unsigned s_bits,
                                                                                  unsigned s_words, unsigned per, unsigned count,
                                                                                  u64* __restrict__ recs, u64* __restrict__ c_out, unsigned Ln,
                                                                                  u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    if (blockIdx.x >= count) return;
    const unsigned wave = threadIdx.x >> 6, L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t entry = blockIdx.x;
    unsigned st = ST_OK;
    const unsigned chains = 2 * m_bits + 2 * s_bits;   // the records of both chains; the final product is record `chains`
    if (chains + 1 != per) st |= ST_INTERNAL;
    // the four waves of the team hold the same values: one of them writes, and only where every record index of the entry is below per
    const bool writer = wave == 0 && recs != nullptr && chains + 1 == per;
    u64* const base = writer ? recs + entry * per * 4 * (size_t)L : nullptr;
    const LD<E> hs0 = ld_load<E>(hs, L);
    {
        LD<E> d;
        if (!ld_sub(d, hs0, ld_load<E>(block_modulus<E>(mod), C))) {   // hs >= n^2 (public, the same for every team): nothing is written
            if (lane_id() == 0) atomicOr(status, st | ST_RANGE);
            return;
        }
    }
    LD<E> gm = ld_small<E>(1);
    {
        LD<E> sq = ld_load<E>(g, Ln);
        st |= pow_mod_uniform(B, T, gm, sq, ms + entry, m_bits, base);
    }
    LD<E> hss = ld_small<E>(1);
    {
        LD<E> sq = hs0;
        st |= pow_mod_uniform(B, T, hss, sq, ss + entry * s_words, s_bits, writer ? base + (size_t)2 * m_bits * 4 * L : nullptr);
    }
    LD<E> q, c;
    st |= mul_mod(B, q, c, gm, hss, TeamMul<E>{&T});
    if (writer) rec_store(base + (size_t)chains * 4 * L, gm, hss, q, c, L);
    if (wave == 0) ld_store(c_out + entry * L, c, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- the entries of a packed ballot (pz_paillier_pballot): c_i = (prod_j G_j^v_ij) hs^s_i mod n^2 for R ciphertexts
// of K slots each under ONE key, G_j = g^(2^(j w)) mod n^2 public.  k_sballot_enc with K slot chains in place of its one g-chain: one
// team per ciphertext runs, per slot j, acc = 1, sq = G_j over exactly m_bits bits of v_ij (pow_mod_uniform), folding the slot's power
// into ONE running product as soon as the chain ends, then hs^s_i over exactly s_bits bits, then the last fold with hss -- R entries in
// one launch, no team waits on another.  The Barrett constants come from k_tally_setup, once for all.  The v_ij (one word each, at
// entry * slots + j: the loop counter alone) and s_i are SECRET: both reach their accumulator as a lane-wise mask over both candidates
// (ld_select), never as a branch or an address, and every trip count is a launch argument.  (What a mul_mod does with its VALUES is
// K3's as everywhere.)  An hs or a G_j >= n^2 (public, the same for every team) is ST_RANGE and nothing is written.
// recs (may be null: the values only): entry i at records i * per .. + per, per = 2 m_bits slots + 2 s_bits + slots: slot j's chain at
// 2 m_bits j, the hs-chain at 2 m_bits slots, then the folds (P_0, P_1), (t_1, P_2), .., (t_{K-1}, hss) whose last remainder is c_i.
// per is held against the loops' own counts before any store; a disagreement is ST_INTERNAL, never a write past the entry.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_pballot_enc(const u64* __restrict__ mod, const u64* __restrict__ hs,
                                                                                  const u64* __restrict__ gs, const u64* __restrict__ vs,
                                                                                  const u64* __restrict__ ss, unsigned slots, unsigned m_bits,
                                                                                  unsigned s_bits, unsigned s_words, unsigned per,
                                                                                  unsigned count, u64* __restrict__ recs,
                                                                                  u64* __restrict__ c_out, unsigned Ln,
                                                                                  u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    if (blockIdx.x >= count) return;
    const unsigned wave = threadIdx.x >> 6, L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t entry = blockIdx.x;
    unsigned st = ST_OK;
    const unsigned slot_recs = 2 * m_bits * slots, chains = slot_recs + 2 * s_bits;   // the folds are records chains .. chains + slots - 1
    if (chains + slots != per) st |= ST_INTERNAL;
    // the four waves of the team hold the same values: one of them writes, and only where every record index of the entry is below per
    const bool writer = wave == 0 && recs != nullptr && chains + slots == per;
    const size_t rec = 4 * (size_t)L;
    u64* const base = writer ? recs + entry * per * rec : nullptr;
    const LD<E> hs0 = ld_load<E>(hs, L);
    {
        // hs or a G_j >= n^2 (public, the same for every team): nothing is written
        const LD<E> M = ld_load<E>(block_modulus<E>(mod), C);
        LD<E> d;
        bool bad = !ld_sub(d, hs0, M);
        for (unsigned j = 0; j < slots; ++j) bad |= !ld_sub(d, ld_load<E>(gs + (size_t)j * L, L), M);
        if (bad) {
            if (lane_id() == 0) atomicOr(status, st | ST_RANGE);
            return;
        }
    }
    LD<E> run = ld_small<E>(1);
    for (unsigned j = 0; j < slots; ++j) {
        LD<E> p = ld_small<E>(1), sq = ld_load<E>(gs + (size_t)j * L, L);
        st |= pow_mod_uniform(B, T, p, sq, vs + entry * slots + j, m_bits, writer ? base + (size_t)2 * m_bits * j * rec : nullptr);
        if (j == 0) {
            run = p;
        } else {
            LD<E> q, r;
            st |= mul_mod(B, q, r, run, p, TeamMul<E>{&T});
            if (writer) rec_store(base + (size_t)(chains + j - 1) * rec, run, p, q, r, L);
            run = r;
        }
    }
    LD<E> hss = ld_small<E>(1);
    {
        LD<E> sq = hs0;
        st |= pow_mod_uniform(B, T, hss, sq, ss + entry * s_words, s_bits, writer ? base + (size_t)slot_recs * rec : nullptr);
    }
    LD<E> q, c;
    st |= mul_mod(B, q, c, run, hss, TeamMul<E>{&T});
    if (writer) rec_store(base + (size_t)(chains + slots - 1) * rec, run, hss, q, c, L);
    if (wave == 0) ld_store(c_out + entry * L, c, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- a mixer's shuffle (pz_paillier_mix): one layer of the Benes network over `count` integers of L limbs that stay
// in place.  One launch per layer, ordered by the stream alone; one wave per switch.  Switch s of a layer on bit beta is the s-th
// position j with that bit clear, its partner j | 2^beta: both follow from s and beta.  The switch's bit is SECRET (the bits are the
// permutation): the wave reads BOTH inputs and writes BOTH outputs, each output chosen limb-wise under ld_select's mask -- no address and
// no branch depends on the bit, whose own address is the switch's index.  in / out: count x L words; a layer never runs in place.
template <int E> __global__ __launch_bounds__(64) void k_mix_route(const u64* __restrict__ in, u64* __restrict__ out,
                                                                    const uint8_t* __restrict__ layer_bits, unsigned beta, unsigned half,
                                                                    unsigned L) {
    const unsigned s = blockIdx.x;
    if (s >= half) return;
    const unsigned low = s & ((1u << beta) - 1u);
    const size_t j = ((size_t)(s >> beta) << (beta + 1)) | low, jp = j | ((size_t)1 << beta);
    const LD<E> a = ld_load<E>(in + j * L, L), b = ld_load<E>(in + jp * L, L);
    const u64 bit = layer_bits[s];
    LD<E> lo = a, hi = b;
    ld_select(lo, b, bit);
    ld_select(hi, a, bit);
    ld_store(out + j * L, lo, L);
    ld_store(out + jp * L, hi, L);
}

// ---- a mixer's re-randomisation (pz_paillier_mix): c'_i = d_i r_i^n mod n^2, d_i the network's output at position i.  k_ballot_enc
// without its g-chain: one team per output runs r_i^n by pow_mod_fixed_exp over n's PUBLIC bits (the square of every bit, then the
// product where the bit is set) and the product with d_i, all `count` outputs in one launch, no team waits on another.  r_i and d_i are
// SECRET (d_i's position in the input list is the permutation); d_i's address follows the team's index alone.  The Barrett constants
// come from k_tally_setup, once.  A d_i >= n^2 (an input >= n^2: every input reaches one output) is ST_RANGE.
// recs (may be null: the values only): output i at records i * per .. + per, per = nr + 1: the chain's, then (d_i, rn_i, q, c'_i).  The
// record index is held against per before every store; a disagreement is ST_INTERNAL, never a write past the output's own records.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_mix_rerand(const u64* __restrict__ mod, const u64* __restrict__ n,
                                                                                 const u64* __restrict__ routed, const u64* __restrict__ rs,
                                                                                 unsigned n_bits, unsigned per, unsigned count,
                                                                                 u64* __restrict__ recs, u64* __restrict__ c_out, unsigned Ln,
                                                                                 u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    if (blockIdx.x >= count) return;
    const unsigned wave = threadIdx.x >> 6, L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t entry = blockIdx.x;
    const bool writer = wave == 0 && recs != nullptr;   // the four waves of the team hold the same values: one of them writes
    u64* const base = writer ? recs + entry * per * 4 * (size_t)L : nullptr;
    unsigned idx = 0, st = ST_OK;
    auto step = [&](LD<E>& r, const LD<E>& a, const LD<E>& b) {   // one recorded mul_mod
        LD<E> q;
        st |= mul_mod(B, q, r, a, b, tmul);
        if (writer && idx < per) rec_store(base + (size_t)idx * 4 * L, a, b, q, r, L);
        ++idx;
    };
    const LD<E> d = ld_load<E>(routed + entry * L, L);
    {
        LD<E> t;
        if (!ld_sub(t, d, ld_load<E>(block_modulus<E>(mod), C))) st |= ST_RANGE;   // an input >= n^2
    }
    LD<E> rn = ld_small<E>(1);
    {
        LD<E> sq = ld_load<E>(rs + entry * Ln, Ln);
        for (unsigned i = 0; i < n_bits; ++i) {
            const LD<E> cur = sq;
            step(sq, cur, cur);
            if ((n[i >> 6] >> (i & 63)) & 1) {   // (n is the public key)
                LD<E> r;
                step(r, rn, cur);
                rn = r;
            }
        }
    }
    LD<E> c;
    step(c, d, rn);
    if (idx != per) st |= ST_INTERNAL;
    if (wave == 0) ld_store(c_out + entry * L, c, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- a mixer's re-randomisation with short randomness (pz_paillier_smix): c'_i = d_i hs^s_i mod n^2, d_i the network's
// output at position i, hs = h^n mod n^2 the key's public element.  k_sballot_enc without its g-chain, or k_mix_rerand with a
// secret-exponent chain: one team per output runs hs^s_i over exactly s_bits bits (pow_mod_uniform: (acc, sq) then (sq, sq) for EVERY
// bit, the trailing square kept) and the product with d_i, all `count` outputs in one launch, no team waits on another.  The Barrett
// constants come from k_tally_setup, once.  s_i and d_i are SECRET (d_i's position in the input list is the permutation): bit t of s_i
// is read from word t / 64 of the entry's s_words words, an address that follows the loop counter alone, and reaches the accumulator as
// a lane-wise mask over both candidates (ld_select); d_i's address follows the team's index alone.  Every trip count is a launch
// argument.  (What a mul_mod does with its VALUES is K3's as everywhere: the Barrett correction's trip count follows the operands.)
// An hs >= n^2 (public, the same for every team) is ST_RANGE and nothing is written; a d_i >= n^2 (an input >= n^2: every input
// reaches one output) is ST_RANGE.
// recs (may be null: the values only): output i at records i * per .. + per, per = 2 s_bits + 1: the chain's, then (d_i, hss_i, q,
// c'_i).  per is held against the loop's own count before any store; a disagreement is ST_INTERNAL, never a write past the output's
// own records.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_smix_rerand(const u64* __restrict__ mod, const u64* __restrict__ hs,
                                                                                  const u64* __restrict__ routed, const u64* __restrict__ ss,
                                                                                  unsigned s_bits, unsigned s_words, unsigned per, unsigned count,
                                                                                  u64* __restrict__ recs, u64* __restrict__ c_out, unsigned Ln,
                                                                                  u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    if (blockIdx.x >= count) return;
    const unsigned wave = threadIdx.x >> 6, L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t entry = blockIdx.x;
    unsigned st = ST_OK;
    const unsigned chain = 2 * s_bits;   // the chain's records; the final product is record `chain`
    if (chain + 1 != per) st |= ST_INTERNAL;
    // the four waves of the team hold the same values: one of them writes, and only where every record index of the output is below per
    const bool writer = wave == 0 && recs != nullptr && chain + 1 == per;
    u64* const base = writer ? recs + entry * per * 4 * (size_t)L : nullptr;
    const LD<E> n2 = ld_load<E>(block_modulus<E>(mod), C);
    LD<E> sq = ld_load<E>(hs, L);
    {
        LD<E> t;
        if (!ld_sub(t, sq, n2)) {   // hs >= n^2 (public, the same for every team): nothing is written
            if (lane_id() == 0) atomicOr(status, st | ST_RANGE);
            return;
        }
    }
    const LD<E> d = ld_load<E>(routed + entry * L, L);
    {
        LD<E> t;
        if (!ld_sub(t, d, n2)) st |= ST_RANGE;   // an input >= n^2
    }
    LD<E> hss = ld_small<E>(1);
    st |= pow_mod_uniform(B, T, hss, sq, ss + entry * s_words, s_bits, base);
    LD<E> q, c;
    st |= mul_mod(B, q, c, d, hss, TeamMul<E>{&T});
    if (writer) rec_store(base + (size_t)chain * 4 * L, d, hss, q, c, L);
    if (wave == 0) ld_store(c_out + entry * L, c, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- a trustee's partial decryptions (pz_paillier_partial): h = v^theta and u_j = (c_j^2)^theta mod n^2 for K ciphertexts under ONE
// secret share theta of e_bits bits.  K + 1 teams in one launch: team 0 runs pow_mod(v, theta), team j >= 1 first squares c_j itself
// (record j - 1) and then runs pow_mod(s_j, theta) -- pow_mod_uniform: (acc, sq) then (sq, sq) for EVERY bit, the trailing square
// kept -- so no team waits for another: no ticket, no spin, no hand-off.  The Barrett constants come from k_tally_setup, once for all.
// theta is SECRET and e_bits long (many words): bit t is read from word t / 64, an address that follows the loop counter alone, and
// reaches the accumulator as a lane-wise mask over both candidates (pow_mod_uniform's ld_select), never as a branch.  Every trip count is a
// launch argument.  (What a mul_mod does with its VALUES is K3's as everywhere: the Barrett correction's trip count follows the operands.)
// recs (may be null: the values only): the K squaring records, then chain i (0 .. K), bit t at records K + 2 (i e_bits + t) and the next.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_partial_pow(const u64* __restrict__ mod, const u64* __restrict__ v,
                                                                                  const u64* __restrict__ cts, const u64* __restrict__ theta,
                                                                                  unsigned e_bits, unsigned count, u64* __restrict__ recs,
                                                                                  u64* __restrict__ h_out, u64* __restrict__ u_out, unsigned L,
                                                                                  u32* __restrict__ status) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod) == 0) return;   // zero modulus (the same word for every workgroup)
    const unsigned wave = threadIdx.x >> 6;
    TeamCtx<E> T;
    team_init(T, s_team);
    BarrettCtx<E> B;
    barrett_from_block(B, mod, L, s_scratch[wave]);
    const size_t chain = blockIdx.x;   // 0: the key's base v; j >= 1: ciphertext j - 1
    if (chain > count) return;
    const bool writer = wave == 0 && recs != nullptr;   // the four waves of the team hold the same values: one of them writes
    unsigned st = ST_OK;
    LD<E> sq = ld_load<E>(chain == 0 ? v : cts + (chain - 1) * L, L);
    {
        LD<E> d;
        if (!ld_sub(d, sq, ld_load<E>(block_modulus<E>(mod), C))) st |= ST_RANGE;   // v or a ciphertext >= n^2 (both public)
    }
    if (chain != 0) {   // s_j = c_j^2: the chain's base
        LD<E> q, r;
        st |= mul_mod(B, q, r, sq, sq, TeamMul<E>{&T});
        if (writer) rec_store(recs + (chain - 1) * 4 * (size_t)L, sq, sq, q, r, L);
        sq = r;
    }
    LD<E> acc = ld_small<E>(1);
    st |= pow_mod_uniform(B, T, acc, sq, theta, e_bits, writer ? recs + ((size_t)count + chain * 2 * (size_t)e_bits) * 4 * L : nullptr);
    if (wave == 0) ld_store(chain == 0 ? h_out : u_out + (chain - 1) * L, acc, L);
    if (st && lane_id() == 0) atomicOr(status, st);
}

// ---- the combiner of a threshold decryption (pz_paillier_combine): per ciphertext U = prod_i u_i mod n^2 over the T trustees' partials
// (T - 1 products, one team per ciphertext, one launch), then decryption's last step on U: U mod n must be 1, m = floor(U / n) mu2 mod n
// (lfn_tail, shared with k_dec_pow's DEC_LFN, by n's Barrett block at this capacity).  Nothing here is secret: the partials are
// published with their proofs.  partials trustee-major: trustee i, ciphertext j at (i count + j) L.  flags: bit 0 U mod n != 1 (m = 0),
// bit 1 a partial >= n^2 (m = 0, no product is formed), bit 2 an internal check failed.
enum { CMB_F_NOT_ONE = 1, CMB_F_RANGE = 2, CMB_F_INTERNAL = 4 };
// whether all `members` partials of ciphertext j are below n^2 (public).  Where one is not: m_j = 0 and CMB_F_RANGE, and the caller
// returns -- the four waves hold the same values, so the team leaves together
template <int E>
__device__ __forceinline__ bool partials_in_range(const LD<E>& n2, const u64* partials, unsigned members, unsigned count, size_t j, unsigned Ln,
                                                  u64* m_out, uint8_t* flags) {
    bool over = false;
    for (unsigned i = 0; i < members; ++i) {
        LD<E> d;
        over |= !ld_sub(d, ld_load<E>(partials + ((size_t)i * count + j) * 2 * Ln, 2 * Ln), n2);
    }
    if (over && threadIdx.x < 64) {
        ld_store(m_out + j * Ln, ld_zero<E>(), Ln);
        if (lane_id() == 0) flags[j] = CMB_F_RANGE;
    }
    return !over;
}
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_partial_combine(const u64* __restrict__ mod2, const u64* __restrict__ modn,
                                                                                      const u64* __restrict__ partials, unsigned count,
                                                                                      unsigned trustees, const u64* __restrict__ mu2,
                                                                                      u64* __restrict__ m_out, uint8_t* __restrict__ flags,
                                                                                      unsigned Ln) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod2) == 0 || *block_ok<E>(modn) == 0) return;   // zero modulus (refused on the host: no launch reaches here with one)
    const unsigned wave = threadIdx.x >> 6, lane = lane_id(), L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    const size_t j = blockIdx.x;
    if (j >= count) return;
    if (!partials_in_range(ld_load<E>(block_modulus<E>(mod2), C), partials, trustees, count, j, Ln, m_out, flags)) return;
    BarrettCtx<E> B;
    barrett_from_block(B, mod2, L, s_scratch[wave]);
    unsigned st = ST_OK;
    LD<E> U = ld_load<E>(partials + j * L, L);
    for (unsigned i = 1; i < trustees; ++i) {
        LD<E> q, r;
        st |= mul_mod(B, q, r, U, ld_load<E>(partials + ((size_t)i * count + j) * L, L), TeamMul<E>{&T});
        U = r;
    }
    BarrettCtx<E> N;
    barrett_from_block(N, modn, L, s_scratch[wave]);
    LD<E> m;
    const bool bad = lfn_tail(N, T, m, U, mu2, Ln, st);
    if (wave == 0) {
        ld_store(m_out + j * Ln, m, Ln);
        if (lane == 0) flags[j] = (uint8_t)((bad ? CMB_F_NOT_ONE : 0) | (st ? CMB_F_INTERNAL : 0));
    }
}

// ---- the modular inverse (pz_bigint_mod_inverse, and the t-of-T combiner's one inverse).  One wavefront owns one value:
// there is no product in it, so no team, no LDS and no barrier.  A right-shift binary extended Euclid over (u, v, x1, x2) with
// x1 x = u and x2 x = v (mod m), v odd throughout (m is odd).  One step: u = 0 ends it (gcd = v, the inverse is x2 where v = 1); an even u
// is halved with x1; otherwise the smaller of u and v goes to v, u takes the (even) difference, x1 the difference of the coefficients
// mod m, and both are halved at once.  Every step takes at least one bit off bitlen(u) + bitlen(v) <= 2 bitlen(m), so 2 bitlen(m) + 4
// steps always suffice for x < m and an odd m; the bound is the caller's (a launch argument, derived from the modulus length alone), and
// a wave that exhausts it (an even m can) leaves with INV_ITER: no loop here is unbounded on any input.  Every branch is wave-uniform:
// parity is lane 0's low bit, comparisons are ld_sub's borrow, zero tests are ballots.  Nothing here is secret: the trip count and the
// branches follow the operands, which are public values (a modulus n and what published partials combine to).
//
// a >> 1 with carry_in as the new top bit of the capacity.  (x + m) / 2 needs it: at limbs = 64 E the sum does not fit the capacity and
// ld_add's carry-out IS bit 64 * 64 E of it.
template <int E> __device__ __forceinline__ LD<E> ld_shr1(const LD<E>& a, bool carry_in) {
    u64 nxt = shfl_down1(a.v[0]);   // the next lane's first limb; lane 63 reads 0
    if (lane_id() == 63) nxt = carry_in ? 1ull : 0ull;
    LD<E> y;
#pragma unroll
    for (int e = 0; e < E; ++e) y.v[e] = (a.v[e] >> 1) | ((e + 1 < E ? a.v[e + 1] : nxt) << 63);
    return y;
}
template <int E> __device__ __forceinline__ bool ld_odd(const LD<E>& a) { return (__builtin_amdgcn_readfirstlane((u32)a.v[0]) & 1u) != 0; }
// x / 2 mod m for x < m, m odd
template <int E> __device__ __forceinline__ LD<E> ld_half_mod(const LD<E>& x, const LD<E>& m) {
    if (!ld_odd(x)) return ld_shr1(x, false);
    LD<E> s;
    const bool c = ld_add(s, x, m, false);
    return ld_shr1(s, c);
}
enum { INV_OK = 0, INV_NOT_UNIT = 1, INV_ITER = 4 };
// inv = x^-1 mod m for x < m; returns INV_OK, INV_NOT_UNIT (gcd(x, m) != 1, x = 0 included: inv = 0) or INV_ITER (max_iters ran out: inv = 0)
template <int E> __device__ __forceinline__ unsigned ld_inv_mod(LD<E>& inv, const LD<E>& x, const LD<E>& m, unsigned max_iters) {
    const LD<E> one = ld_small<E>(1);
    LD<E> u = x, v = m, x1 = one, x2 = ld_zero<E>();
    inv = ld_zero<E>();
    for (unsigned it = 0; it < max_iters; ++it) {
        if (ld_is_zero(u)) {
            bool ne = false;
#pragma unroll
            for (int e = 0; e < E; ++e) ne |= v.v[e] != one.v[e];
            if (__ballot(ne) != 0) return INV_NOT_UNIT;
            inv = x2;
            return INV_OK;
        }
        if (ld_odd(u)) {
            LD<E> d;
            if (ld_sub(d, u, v)) {   // u < v: they change places
                (void)ld_sub(d, v, u);
                v = u;
                const LD<E> t = x1;
                x1 = x2;
                x2 = t;
            }
            u = d;
            if (ld_sub(d, x1, x2)) (void)ld_add(d, d, m, false);   // x1 - x2 + 2^capacity + m: the carry-out is that 2^capacity
            x1 = d;
        }
        u = ld_shr1(u, false);
        x1 = ld_half_mod(x1, m);
    }
    return INV_ITER;
}

// xs, inv_out: count x limbs words; flags: bit 0 not a unit, bit 1 x >= mod, bit 2 the iteration bound ran out (output zero in each case).
// Four independent waves per workgroup, one value each; nothing is shared between them.
#define K3_INV_WAVES 4
template <int E> __global__ __launch_bounds__(64 * K3_INV_WAVES) void k_mod_inverse(const u64* __restrict__ mod, const u64* __restrict__ xs,
                                                                                     u64* __restrict__ inv_out, uint8_t* __restrict__ flags,
                                                                                     unsigned limbs, unsigned count, unsigned max_iters) {
    const size_t j = (size_t)blockIdx.x * K3_INV_WAVES + (threadIdx.x >> 6);
    if (j >= count) return;
    const LD<E> m = ld_load<E>(mod, limbs), x = ld_load<E>(xs + j * limbs, limbs);
    LD<E> inv = ld_zero<E>(), d;
    unsigned f = 2;   // x >= mod
    if (ld_sub(d, x, m)) f = ld_inv_mod(inv, x, m, max_iters);
    ld_store(inv_out + j * limbs, inv, limbs);
    if (lane_id() == 0) flags[j] = (uint8_t)f;
}

// ---- the t-of-T combiner (pz_paillier_combine_t): per ciphertext A = prod_{neg_i = 0} u_i^e_i and B = prod_{neg_i = 1}
// u_i^e_i mod n^2 over the members' partials and the magnitudes e_i = |mu_i| of their Lagrange exponents, each as ONE interleaved
// (Straus) left-to-right chain -- per bit one squaring of the accumulator, then one product per member of that sign whose bit is set --
// then the tail: A = B mod n must hold (honest partials give A = B (1 + x n)), x = ((A - B mod n^2) / n) (B mod n)^-1 mod n, m = x mu2
// mod n.  One team per ciphertext, A then B, one launch; no workgroup waits on another.  The exponents, the signs and max_bits are
// public and the same for every wave of every team, so branching on them is allowed and the four waves of a team execute the same
// sequence of mul_mods (the team product has a workgroup barrier); the inverse runs redundantly in the four waves on the same values,
// so they leave it together too.  An accumulator that is still 1 takes its first factor by assignment and is not squared: with every
// exponent 1 and no negative sign this is k_partial_combine's product, bit for bit.
// partials member-major: member i, ciphertext j at (i count + j) L.  flags: bits 0 .. 2 as k_partial_combine, bit 3 B mod n is no unit.
enum { CMB_F_NOT_UNIT = 8 };
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_combine_t(const u64* __restrict__ mod2, const u64* __restrict__ modn,
                                                                                const u64* __restrict__ partials, unsigned count,
                                                                                unsigned members, const u64* __restrict__ exps,
                                                                                unsigned exp_words, const uint8_t* __restrict__ neg,
                                                                                unsigned max_bits, unsigned inv_iters,
                                                                                const u64* __restrict__ mu2, u64* __restrict__ m_out,
                                                                                uint8_t* __restrict__ flags, unsigned Ln) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    if (*block_ok<E>(mod2) == 0 || *block_ok<E>(modn) == 0) return;   // zero modulus (refused on the host: no launch reaches here with one)
    const unsigned wave = threadIdx.x >> 6, lane = lane_id(), L = 2 * Ln;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    const size_t j = blockIdx.x;
    if (j >= count) return;
    const LD<E> n2 = ld_load<E>(block_modulus<E>(mod2), C);
    if (!partials_in_range(n2, partials, members, count, j, Ln, m_out, flags)) return;
    BarrettCtx<E> B;
    barrett_from_block(B, mod2, L, s_scratch[wave]);
    unsigned st = ST_OK;
    LD<E> A = ld_zero<E>(), Bv = A;
    for (unsigned sign = 0; sign < 2; ++sign) {
        LD<E> acc = ld_small<E>(1);
        bool started = false;
        for (unsigned bit = max_bits; bit-- > 0;) {
            LD<E> q, r;
            if (started) {
                st |= mul_mod(B, q, r, acc, acc, tmul);
                acc = r;
            }
            for (unsigned i = 0; i < members; ++i) {
                const u32 take = (neg[i] == sign) & (u32)((exps[(size_t)i * exp_words + (bit >> 6)] >> (bit & 63)) & 1);
                if (!__builtin_amdgcn_readfirstlane(take)) continue;   // the same word for every lane of every wave: a scalar branch
                const LD<E> u = ld_load<E>(partials + ((size_t)i * count + j) * L, L);
                if (started) {
                    st |= mul_mod(B, q, r, acc, u, tmul);
                    acc = r;
                } else {
                    acc = u;
                    started = true;
                }
            }
        }
        if (sign == 0) A = acc; else Bv = acc;
    }
    // the tail: A = B mod n must hold; x = ((A - B mod n^2) / n) (B mod n)^-1 mod n; plaintext = x mu2 mod n
    BarrettCtx<E> N;
    barrett_from_block(N, modn, L, s_scratch[wave]);
    const LD<E> one = ld_small<E>(1);
    LD<E> q, ra, rb, D, x, rem, inv, t, m;
    st |= mul_mod(N, q, ra, A, one, tmul);
    st |= mul_mod(N, q, rb, Bv, one, tmul);
    bool ne = false;
#pragma unroll
    for (int e = 0; e < E; ++e) ne |= ra.v[e] != rb.v[e];
    const bool bad = __ballot(ne) != 0;
    if (ld_sub(D, A, Bv)) (void)ld_add(D, D, n2, false);   // A - B + 2^capacity + n^2: the carry-out is that 2^capacity
    st |= mul_mod(N, x, rem, D, one, tmul);   // an exact division where A = B mod n
    const unsigned fi = ld_inv_mod(inv, rb, ld_load<E>(block_modulus<E>(modn), C), inv_iters);
    st |= mul_mod(N, q, t, x, inv, tmul);
    st |= mul_mod(N, q, m, t, ld_load<E>(mu2, Ln), tmul);
    if (bad || fi != INV_OK) m = ld_zero<E>();
    if (wave == 0) {
        ld_store(m_out + j * Ln, m, Ln);
        if (lane == 0)
            flags[j] = (uint8_t)((bad ? CMB_F_NOT_ONE : 0) | ((st || (fi & INV_ITER)) ? CMB_F_INTERNAL : 0) | ((fi & INV_NOT_UNIT) ? CMB_F_NOT_UNIT : 0));
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int status_to_rc(pz_ctx* ctx, u32 st) {
    if (st & ST_TIMEOUT) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: a multiplier workgroup's bounded wait for its squarer ran out (status %u)", st);
        return PZ_ERR_INTERNAL;
    }
    if (st & ST_ZERO_MOD) return PZ_ERR_ZERO_MODULUS;
    if (st & ST_RANGE) return PZ_ERR_RANGE;
    if (st & ST_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (status %u)", st);
        return PZ_ERR_HIP;
    }
    return PZ_OK;
}

// The hand-off area of a launch: per chain `bits` squares of L limbs; then ONE block of counters for the whole call, cleared by a single
// memset in stream order -- per launch a role ticket, per chain the number of squares published (a 64-byte line each: a counter is polled
// by the four waves of one multiplier while its squarer writes it; neighbours in one line would share that traffic).
// The squares of a batch are bounded: at most K3_HANDOFF_CAP bytes of them exist at a time, larger batches run as several launches
// one after the other on the stream (the multiplier consumes squares strictly in order, but a ring with a consumer counter would make
// the squarer wait for a workgroup that may not have started: that is the one dependency the role tickets exclude).
#define K3_HANDOFF_CAP ((size_t)1 << 30)
static size_t chain_squares_bytes(unsigned bits, unsigned L) { return (size_t)bits * L * 8; }
static unsigned env_u32(const char* name, unsigned dflt) {
    const char* v = getenv(name);
    return v && *v ? (unsigned)strtoul(v, nullptr, 0) : dflt;
}
// Test hooks (tests/test_gpu_kernels.py::test_k3_bounded_wait_reports_internal, test_encrypt_batch_beyond_residency): honoured only
// when PZ_K3_TEST_HOOKS=1 is set as well, and read ONCE PER CALL (chain_handoff_alloc), never inside the per-chain loop -- a stray
// PZ_K3_* variable in a deployment changes nothing, and the production path makes one getenv per entry point.
struct K3Hooks {
    unsigned spin_limit = K3_SPIN_LIMIT, test_no_publish = 0;
    size_t cap_kib = 0;
};
static K3Hooks k3_hooks() {
    K3Hooks h;
    const char* on = getenv("PZ_K3_TEST_HOOKS");
    if (!(on && on[0] == '1')) return h;
    h.spin_limit = env_u32("PZ_K3_SPIN_LIMIT", K3_SPIN_LIMIT);
    h.test_no_publish = env_u32("PZ_K3_TEST_NO_PUBLISH", 0);
    h.cap_kib = env_u32("PZ_K3_HANDOFF_CAP_KIB", 0);   // a small cap splits a small batch into several launches
    return h;
}
static size_t chains_per_launch(unsigned bits, unsigned L, size_t n_chains, size_t cap_kib) {
    size_t per = (cap_kib ? cap_kib << 10 : K3_HANDOFF_CAP) / chain_squares_bytes(bits, L);
    per = per < 2 ? 2 : per & ~(size_t)1;   // the two chains of an instance stay in one launch
    return per < n_chains ? per : n_chains;
}
struct ChainHandoff {
    char* squares;     // chains_per_launch x chain_squares_bytes, reused by every launch of the call
    char* counters;    // n_launches tickets, then n_chains ready counters, 64 bytes apart
    size_t per_launch, n_launches;
    K3Hooks hooks;
};
static int chain_handoff_alloc(pz_ctx* ctx, size_t n_chains, unsigned bits, unsigned L, ChainHandoff* h) {
    h->hooks = k3_hooks();
    h->per_launch = chains_per_launch(bits, L, n_chains, h->hooks.cap_kib);
    h->n_launches = (n_chains + h->per_launch - 1) / h->per_launch;
    const size_t sq = h->per_launch * chain_squares_bytes(bits, L), cnt = (h->n_launches + n_chains) * 64;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_K3, sq + cnt + 256, &d));
    h->squares = (char*)d;
    h->counters = (char*)d + ((sq + 255) & ~(size_t)255);
    HIPCHK(ctx, hipMemsetAsync(h->counters, 0, cnt, ctx->stream));
    return PZ_OK;
}
static void chain_handoff_set(ChainDesc& d, const ChainHandoff& h, size_t i, unsigned bits, unsigned L) {
    d.sq_buf = (u64*)(h.squares + (i % h.per_launch) * chain_squares_bytes(bits, L));
    d.ready = (u32*)(h.counters + (h.n_launches + i) * 64);
    d.spin_limit = h.hooks.spin_limit;
    d.test_no_publish = h.hooks.test_no_publish;
}
// the capacity (limbs) of the instantiation that serves operands of L limbs: E = 1 up to 64, E = 2 above
static unsigned capacity(unsigned L) { return L <= 64 ? 64 : 128; }
// one launch on the context's stream of kernel<E> at capacity C = 64 E, checked; `lds`: dynamic LDS bytes
#define K3_LAUNCH(ctx, kernel, C, grid, block, lds, ...)                                                 \
    do {                                                                                                 \
        if ((C) == 64) hipLaunchKernelGGL(kernel<1>, grid, block, lds, (ctx)->stream, __VA_ARGS__);      \
        else hipLaunchKernelGGL(kernel<2>, grid, block, lds, (ctx)->stream, __VA_ARGS__);                \
        HIPCHK(ctx, hipGetLastError());                                                                  \
    } while (0)
// the Barrett block (mod_block_words(C) words at d_block) of n (Ln limbs), or of n^2 where square != 0
static int launch_barrett_setup(pz_ctx* ctx, unsigned C, const u64* d_n, unsigned Ln, unsigned square, u64* d_block, u32* d_status) {
    K3_LAUNCH(ctx, k_tally_setup, C, dim3(1), dim3(64), 0, d_n, Ln, square, d_block, d_status);
    return PZ_OK;
}
static int launch_chains(pz_ctx* ctx, const ChainDesc* d_descs, size_t n, unsigned L, const ChainHandoff& h) {
    // per launch: 2 m workgroups for m chains; who squares and who multiplies is decided by arrival (k_pow_mod_chain)
    for (size_t l = 0, off = 0; off < n; ++l, off += h.per_launch) {
        const size_t m = n - off < h.per_launch ? n - off : h.per_launch;
        u32* ticket = (u32*)(h.counters + l * 64);
        K3_LAUNCH(ctx, k_pow_mod_chain, capacity(L), dim3((unsigned)(2 * m)), dim3(64 * K3_TEAM), 0, d_descs + off, (unsigned)m, ticket);
    }
    return PZ_OK;
}
static int launch_muls(pz_ctx* ctx, const MulDesc* d_descs, size_t n, unsigned L) {
    K3_LAUNCH(ctx, k_mul_mod, capacity(L), dim3((unsigned)n), dim3(64), 0, d_descs);
    return PZ_OK;
}
static unsigned bitlen_limbs(const uint64_t* a, uint32_t n) {
    for (uint32_t i = n; i-- > 0;)
        if (a[i]) return 64 * i + (64 - (unsigned)__builtin_clzll(a[i]));
    return 0;
}
// records of pow_mod_fixed_exp over the exponent e: a square per bit and a product per set bit
static size_t fixed_exp_steps(const uint64_t* e, uint32_t limbs) {
    size_t need = bitlen_limbs(e, limbs);
    for (uint32_t i = 0; i < limbs; ++i) need += (size_t)__builtin_popcountll(e[i]);
    return need;
}
// the epilogue of a traced call: the result, the status word and -- for a host trace (steps_out non-null) -- the records come back,
// the stream is drained once and the status mapped
static int fetch_and_status(pz_ctx* ctx, void* result, const void* d_result, size_t result_bytes, const u32* d_status, void* steps_out,
                            const void* d_steps, size_t steps_bytes) {
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(result, d_result, result_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (steps_out) HIPCHK(ctx, hipMemcpyAsync(steps_out, d_steps, steps_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return status_to_rc(ctx, st);
}
// the epilogue of a call that staged SECRETS (d_secret; in the host form d_recs too, whose records repeat them): both are overwritten
// and the stream drained on every path past the staging, whatever the run returned; the run's error wins over the wipe's
static int wipe_secrets_and_sync(pz_ctx* ctx, int rc, void* d_secret, size_t secret_bytes, void* d_recs, size_t rec_bytes) {
    hipError_t e = hipMemsetAsync(d_secret, 0, secret_bytes, ctx->stream);
    if (e == hipSuccess && rec_bytes) e = hipMemsetAsync(d_recs, 0, rec_bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (rc != PZ_OK) return rc;
    HIPCHK(ctx, e);
    return PZ_OK;
}

extern "C" int pz_mul_mod(pz_ctx* ctx, uint32_t limbs, const uint64_t* a, const uint64_t* b, const uint64_t* modulus,
                          uint64_t* q, uint64_t* r) {
    if (!ctx || !a || !b || !modulus || !q || !r || limbs == 0) return PZ_ERR_INVALID;
    if (limbs > 128) return PZ_ERR_UNSUPPORTED;
    PZ_ENTER(ctx);
    const size_t lb = (size_t)limbs * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, 5 * lb + 256, &d));
    char* base = (char*)d;
    u32* d_status = (u32*)(base + 5 * lb);
    MulDesc* d_desc = (MulDesc*)(base + 5 * lb + 64);
    HIPCHK(ctx, hipMemcpyAsync(base, a, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(base + lb, b, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(base + 2 * lb, modulus, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 4, ctx->stream));
    MulDesc h{};
    h.a = (const u64*)base;
    h.b = (const u64*)(base + lb);
    h.modulus = (const u64*)(base + 2 * lb);
    h.q = (u64*)(base + 3 * lb);
    h.r = (u64*)(base + 4 * lb);
    h.step = nullptr;
    h.status = d_status;
    h.limbs_a = h.limbs_b = h.limbs_mod = h.L = limbs;
    h.square_modulus = 0;
    HIPCHK(ctx, hipMemcpyAsync(d_desc, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(launch_muls(ctx, d_desc, 1, limbs));
    HIPCHK(ctx, hipMemcpyAsync(q, base + 3 * lb, lb, hipMemcpyDeviceToHost, ctx->stream));
    return fetch_and_status(ctx, r, base + 4 * lb, lb, d_status, nullptr, nullptr, 0);
}

extern "C" int pz_paillier_trace(pz_ctx* ctx, uint32_t limbs_n2, const uint64_t* n2, const uint64_t* base,
                                 const uint64_t* exp, uint32_t exp_limbs, uint64_t* steps_out, size_t* n_steps,
                                 uint64_t* result) {
    if (!ctx || !n2 || !base || !exp || !result || limbs_n2 == 0 || exp_limbs == 0) return PZ_ERR_INVALID;
    if (steps_out && !n_steps) return PZ_ERR_INVALID;
    if (limbs_n2 > 128) return PZ_ERR_UNSUPPORTED;
    PZ_ENTER(ctx);
    const unsigned L = limbs_n2;
    const size_t lb = (size_t)L * 8, eb = (size_t)exp_limbs * 8;
    const size_t need = fixed_exp_steps(exp, exp_limbs);
    const size_t cap = steps_out ? *n_steps : 0;
    if (steps_out && cap < need) return PZ_ERR_CAPACITY;
    void *d_in, *d_steps = nullptr;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, 3 * lb + eb + 512, &d_in));
    if (steps_out && need) PZCHK(pz_ws_get(ctx, WS_BIG_B, need * 4 * lb, &d_steps));
    char* p = (char*)d_in;
    HIPCHK(ctx, hipMemcpyAsync(p, n2, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(p + lb, base, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(p + 2 * lb, exp, eb, hipMemcpyHostToDevice, ctx->stream));
    u32* d_status = (u32*)(p + 3 * lb + eb);
    u32* d_nsteps = d_status + 1;
    ChainDesc* d_desc = (ChainDesc*)(p + 3 * lb + eb + 64);
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 8, ctx->stream));
    ChainDesc h{};
    h.modulus = (const u64*)p;
    h.base = (const u64*)(p + lb);
    h.exp = (const u64*)(p + 2 * lb);
    h.steps = (u64*)d_steps;
    h.result = (u64*)(p + 2 * lb + eb);
    h.n_steps = d_nsteps;
    h.status = d_status;
    h.limbs_mod = L;
    h.limbs_base = L;
    h.exp_limbs = exp_limbs;
    h.L = L;
    h.square_modulus = 0;
    h.steps_cap = (u32)need;
    ChainHandoff hb;
    PZCHK(chain_handoff_alloc(ctx, 1, 64 * exp_limbs, L, &hb));
    chain_handoff_set(h, hb, 0, 64 * exp_limbs, L);
    HIPCHK(ctx, hipMemcpyAsync(d_desc, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_chains(ctx, d_desc, 1, L, hb));
    }
    u32 st[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(result, p + 2 * lb + eb, lb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(st, d_status, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (steps_out && need)
        HIPCHK(ctx, hipMemcpyAsync(steps_out, d_steps, need * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_steps) *n_steps = st[1];
    return status_to_rc(ctx, st[0]);
}

static int encrypt_impl(pz_ctx* ctx, uint32_t Ln, size_t batch, const uint64_t* n, const uint64_t* g,
                        const uint64_t* m, const uint64_t* r, uint64_t* steps_out, int steps_on_device,
                        size_t steps_cap, uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out, uint32_t uniform_m_bits = 0) {
    if (!ctx || !n || !g || !m || !r || !c_out || Ln == 0 || batch == 0) return PZ_ERR_INVALID;
    if (uniform_m_bits > 64 * Ln) return PZ_ERR_INVALID;
    const unsigned L = 2 * Ln;
    if (L > 128) return PZ_ERR_UNSUPPORTED;
    if (steps_cap > 0x7fffffffu) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // exact per-instance step counts from the exponents (host side: they are public structure of the
    // circuit, paillier.rs:50,54)
    std::vector<uint32_t> ng(batch), nr(batch);
    for (size_t i = 0; i < batch; ++i) {
        ng[i] = uniform_m_bits ? 2 * uniform_m_bits : (uint32_t)fixed_exp_steps(m + i * Ln, Ln);
        nr[i] = (uint32_t)fixed_exp_steps(n + i * Ln, Ln);
        if (uniform_m_bits) {   // the message must fit the bits the circuit decomposes
            for (uint32_t b = uniform_m_bits; b < 64 * Ln; ++b)
                if ((m[i * Ln + (b >> 6)] >> (b & 63)) & 1) return PZ_ERR_MESSAGE_RANGE;
        }
        if (steps_out && (size_t)ng[i] + nr[i] + 1 > steps_cap) return PZ_ERR_CAPACITY;
    }
    // device staging: inputs n,g,m,r (batch x Ln each), results gm, rn, c (batch x L), status, descs
    const size_t in_bytes = 4 * batch * nb;
    const size_t res_bytes = 3 * batch * lb;
    const size_t desc_bytes = batch * (2 * sizeof(ChainDesc) + sizeof(MulDesc));
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, in_bytes + res_bytes + desc_bytes + 1024, &d));
    char* p = (char*)d;
    u64* d_n = (u64*)p;
    u64* d_g = (u64*)(p + batch * nb);
    u64* d_m = (u64*)(p + 2 * batch * nb);
    u64* d_r = (u64*)(p + 3 * batch * nb);
    u64* d_gm = (u64*)(p + in_bytes);
    u64* d_rn = (u64*)(p + in_bytes + batch * lb);
    u64* d_c = (u64*)(p + in_bytes + 2 * batch * lb);
    u32* d_status = (u32*)(p + in_bytes + res_bytes);
    char* d_descs = p + in_bytes + res_bytes + 256;
    u64* d_steps = nullptr;
    if (steps_out) {
        if (steps_on_device) d_steps = steps_out;
        else {
            void* t;
            PZCHK(pz_ws_get(ctx, WS_BIG_B, batch * steps_cap * 4 * lb, &t));
            d_steps = (u64*)t;
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(d_n, n, batch * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_g, g, batch * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_m, m, batch * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_r, r, batch * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 4, ctx->stream));
    std::vector<ChainDesc> ch(2 * batch);
    std::vector<MulDesc> mu(batch);
    ChainHandoff hb;
    PZCHK(chain_handoff_alloc(ctx, 2 * batch, 64 * Ln, L, &hb));
    for (size_t i = 0; i < batch; ++i) {
        u64* st_i = d_steps ? d_steps + i * steps_cap * 4 * L : nullptr;
        ChainDesc& a = ch[2 * i];
        a = ChainDesc{};
        a.modulus = d_n + i * Ln;
        a.base = d_g + i * Ln;
        a.exp = d_m + i * Ln;
        a.steps = st_i;
        a.result = d_gm + i * L;
        a.n_steps = nullptr;
        a.status = d_status;
        a.limbs_mod = Ln;
        a.limbs_base = Ln;
        a.exp_limbs = Ln;
        a.L = L;
        a.square_modulus = 1;
        a.steps_cap = ng[i];
        a.uniform_bits = uniform_m_bits;
        ChainDesc& b = ch[2 * i + 1];
        b = a;
        b.uniform_bits = 0;   // n is the public key: its bits stay circuit structure (pow_mod_fixed_exp)
        b.base = d_r + i * Ln;
        b.exp = d_n + i * Ln;
        b.steps = st_i ? st_i + (size_t)ng[i] * 4 * L : nullptr;
        b.result = d_rn + i * L;
        b.steps_cap = nr[i];
        chain_handoff_set(a, hb, 2 * i, 64 * Ln, L);
        chain_handoff_set(b, hb, 2 * i + 1, 64 * Ln, L);
        MulDesc& f = mu[i];
        f = MulDesc{};
        f.a = d_gm + i * L;
        f.b = d_rn + i * L;
        f.modulus = d_n + i * Ln;
        f.q = nullptr;
        f.r = d_c + i * L;
        f.step = st_i ? st_i + (size_t)(ng[i] + nr[i]) * 4 * L : nullptr;
        f.status = d_status;
        f.limbs_a = f.limbs_b = L;
        f.limbs_mod = Ln;
        f.L = L;
        f.square_modulus = 1;
    }
    ChainDesc* d_ch = (ChainDesc*)d_descs;
    MulDesc* d_mu = (MulDesc*)(d_descs + 2 * batch * sizeof(ChainDesc));
    HIPCHK(ctx, hipMemcpyAsync(d_ch, ch.data(), ch.size() * sizeof(ChainDesc), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_mu, mu.data(), mu.size() * sizeof(MulDesc), hipMemcpyHostToDevice, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_chains(ctx, d_ch, 2 * batch, L, hb));
        PZCHK(launch_muls(ctx, d_mu, batch, L));
    }
    if (steps_out && !steps_on_device)   // every instance's own count of records, not the whole capacity
        for (size_t i = 0; i < batch; ++i) {
            size_t cnt = (size_t)ng[i] + nr[i] + 1;
            HIPCHK(ctx, hipMemcpyAsync(steps_out + i * steps_cap * 4 * L, d_steps + i * steps_cap * 4 * L,
                                       cnt * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
        }
    for (size_t i = 0; i < batch; ++i) {
        if (n_steps_g) n_steps_g[i] = ng[i];
        if (n_steps_r) n_steps_r[i] = nr[i];
    }
    return fetch_and_status(ctx, c_out, d_c, batch * lb, d_status, nullptr, nullptr, 0);
}

extern "C" int pz_paillier_encrypt(pz_ctx* ctx, uint32_t limbs_n, size_t batch, const uint64_t* n, const uint64_t* g,
                                   const uint64_t* m, const uint64_t* r, uint64_t* steps_out, size_t steps_cap,
                                   uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out) {
    return encrypt_impl(ctx, limbs_n, batch, n, g, m, r, steps_out, 0, steps_cap, n_steps_g, n_steps_r, c_out);
}
extern "C" int pz_paillier_encrypt_dev(pz_ctx* ctx, uint32_t limbs_n, size_t batch, const uint64_t* n,
                                       const uint64_t* g, const uint64_t* m, const uint64_t* r, uint64_t* d_steps_out,
                                       size_t steps_cap, uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out) {
    return encrypt_impl(ctx, limbs_n, batch, n, g, m, r, d_steps_out, 1, steps_cap, n_steps_g, n_steps_r, c_out);
}

// the UNIFORM-SHAPE encrypt circuit's witness.  The reference pulls the exponent m out of the
// witness (paillier.rs:50: pow_mod_fixed_exp), so its circuit -- hence vk / pk -- is shaped by the secret message; here
// g^m runs as BigUintChip::pow_mod over exactly `m_bits` in-circuit bits (per bit: mul_mod(acc, sq), select, square_mod),
// so every message of a key shares one circuit shape: 2 * m_bits steps for g^m, then the r^n chain (n is public: fixed
// exponent as in the reference) and the final mul_mod.  `batch` independent messages per call.  Not bit-compatible with
// the reference's circuit by construction (a different constraint system proving the same statement).
extern "C" int pz_paillier_encrypt_uniform(pz_ctx* ctx, uint32_t limbs_n, size_t batch, uint32_t m_bits, const uint64_t* n,
                                           const uint64_t* g, const uint64_t* m, const uint64_t* r, uint64_t* steps_out,
                                           size_t steps_cap, uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out) {
    if (m_bits == 0) return PZ_ERR_INVALID;
    return encrypt_impl(ctx, limbs_n, batch, n, g, m, r, steps_out, 0, steps_cap, n_steps_g, n_steps_r, c_out, m_bits);
}
extern "C" int pz_paillier_encrypt_uniform_dev(pz_ctx* ctx, uint32_t limbs_n, size_t batch, uint32_t m_bits, const uint64_t* n,
                                               const uint64_t* g, const uint64_t* m, const uint64_t* r, uint64_t* d_steps_out,
                                               size_t steps_cap, uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out) {
    if (m_bits == 0) return PZ_ERR_INVALID;
    return encrypt_impl(ctx, limbs_n, batch, n, g, m, r, d_steps_out, 1, steps_cap, n_steps_g, n_steps_r, c_out, m_bits);
}

// PaillierChip::add folded over `count` ciphertexts (paillier.rs:62-85, one mul_mod each) as a product tree: level 0 multiplies
// (c_1, c_2), (c_3, c_4), ...; an odd last element is carried up without a product; records are numbered level-major.
#define K3_TALLY_MAX 65536
// the product tree over `count` elements of L limbs at `elems` (stride L): one k_tally_level launch per level on the context's stream,
// the count - 1 records written to d_steps in level-major order.  *root = the last level's remainder (count = 1: the element itself).
static int tally_levels(pz_ctx* ctx, unsigned C, const u64* d_mod, const u64* elems, size_t count, unsigned L, u64* d_steps, u32* d_status,
                        const u64** root) {
    const size_t rec = 4 * (size_t)L;
    // the level's list: n_regular strided elements, then (len > n_regular) the carried one
    const u64* tail = nullptr;
    size_t len = count, stride = L, n_regular = count, rec_off = 0;
    while (len > 1) {
        const size_t blocks = len / 2;
        u64* out = d_steps + rec_off * rec;
        K3_LAUNCH(ctx, k_tally_level, C, dim3((unsigned)blocks), dim3(64 * K3_TEAM), 0, d_mod, elems, stride, (unsigned)n_regular, tail, out, L,
                  d_status);
        const u64* last = n_regular == len ? elems + (len - 1) * stride : tail;
        tail = (len & 1) ? last : nullptr;
        elems = out + 3 * (size_t)L;
        stride = rec;
        n_regular = blocks;
        len = blocks + (len & 1);
        rec_off += blocks;
    }
    *root = elems;   // the last level is one product of two elements: its remainder
    return PZ_OK;
}
static int tally_impl(pz_ctx* ctx, uint32_t Ln, size_t count, const uint64_t* n, const uint64_t* cts, uint64_t* steps_out,
                      int steps_on_device, size_t steps_cap, uint64_t* c_out) {
    if (!ctx || !n || !cts || !c_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 2 || count > K3_TALLY_MAX) return PZ_ERR_INVALID;
    const unsigned L = 2 * Ln;
    if (L > 128) return PZ_ERR_UNSUPPORTED;
    if (steps_out && steps_cap < count - 1) return PZ_ERR_CAPACITY;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, rec = 4 * (size_t)L;
    const unsigned C = capacity(L);
    const size_t in_bytes = (nb + count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(C) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, in_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    u64* d_n = (u64*)p;
    u64* d_cts = (u64*)(p + nb);
    u64* d_mod = (u64*)(p + in_bytes);
    u32* d_status = (u32*)(p + in_bytes + mod_bytes + 64);
    u64* d_steps = steps_on_device ? steps_out : nullptr;
    if (!d_steps) {   // value only, or a host trace: the records live in a workspace (the levels read each other's remainders there)
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, (count - 1) * rec * 8, &t));
        d_steps = (u64*)t;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_n, n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_cts, cts, count * lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 4, ctx->stream));
    const u64* root = nullptr;
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, d_n, Ln, 1, d_mod, d_status));
        PZCHK(tally_levels(ctx, C, d_mod, d_cts, count, L, d_steps, d_status, &root));
    }
    return fetch_and_status(ctx, c_out, root, lb, d_status, steps_on_device ? nullptr : steps_out, d_steps, (count - 1) * rec * 8);
}
extern "C" int pz_paillier_tally(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts,
                                 uint64_t* steps_out, size_t steps_cap, uint64_t* c_out) {
    return tally_impl(ctx, limbs_n, count, n, cts, steps_out, 0, steps_cap, c_out);
}
extern "C" int pz_paillier_tally_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts,
                                     uint64_t* d_steps_out, size_t steps_cap, uint64_t* c_out) {
    return tally_impl(ctx, limbs_n, count, n, cts, d_steps_out, 1, steps_cap, c_out);
}

// The weighted tally: C = prod c_i^w_i mod n^2 -- per ciphertext BigUintChip::pow_mod over w_bits in-circuit bits (k_wtally_pow, one
// team per chain), then the tally's product tree over the powers.  Records: the chains' 2 * count * w_bits chain-major, then the tree's
// count - 1.  Every launch goes on the context's stream; the host synchronises once, at the end.
static int wtally_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t w_bits, const uint64_t* n, const uint64_t* cts,
                       const uint64_t* weights, uint64_t* steps_out, int steps_on_device, size_t steps_cap, uint64_t* c_out) {
    if (!ctx || !n || !cts || !weights || !c_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_TALLY_MAX || w_bits < 1 || w_bits > 64) return PZ_ERR_INVALID;
    const unsigned L = 2 * Ln;
    if (L > 128) return PZ_ERR_UNSUPPORTED;
    const size_t n_chain = 2 * count * w_bits, n_tree = count - 1;
    if (steps_out && steps_cap < n_chain + n_tree) return PZ_ERR_CAPACITY;
    if (w_bits < 64)   // before any launch: the circuit's num_to_bits of such a weight cannot hold
        for (size_t i = 0; i < count; ++i)
            if (weights[i] >> w_bits) return PZ_ERR_MESSAGE_RANGE;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, rec = 4 * (size_t)L;
    const unsigned C = capacity(L);
    // n | c_1 .. c_count | w_1 .. w_count | the powers | Barrett constants | status
    const size_t in_bytes = (nb + count * lb + count * 8 + 255) & ~(size_t)255, pow_bytes = (count * lb + 255) & ~(size_t)255;
    const size_t mod_bytes = mod_block_words(C) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, in_bytes + pow_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    u64* d_n = (u64*)p;
    u64* d_cts = (u64*)(p + nb);
    u64* d_w = (u64*)(p + nb + count * lb);
    u64* d_pow = (u64*)(p + in_bytes);
    u64* d_mod = (u64*)(p + in_bytes + pow_bytes);
    u32* d_status = (u32*)(p + in_bytes + pow_bytes + mod_bytes + 64);
    u64* d_steps = steps_on_device ? steps_out : nullptr;
    u64* d_tree = d_steps ? d_steps + n_chain * rec : nullptr;
    if (!d_steps && (steps_out || n_tree)) {
        // a host trace: all records live in a workspace; the value only: the tree's alone (its levels read each other's remainders
        // there) -- the chains then write no records at all
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, ((steps_out ? n_chain : 0) + n_tree) * rec * 8 + 8, &t));
        if (steps_out) {
            d_steps = (u64*)t;
            d_tree = d_steps + n_chain * rec;
        } else d_tree = (u64*)t;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_n, n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_cts, cts, count * lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_w, weights, count * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 4, ctx->stream));
    const u64* root = nullptr;
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, d_n, Ln, 1, d_mod, d_status));
        K3_LAUNCH(ctx, k_wtally_pow, C, dim3((unsigned)count), dim3(64 * K3_TEAM), 0, d_mod, d_cts, d_w, w_bits, d_steps, d_pow, L, d_status);
        PZCHK(tally_levels(ctx, C, d_mod, d_pow, count, L, d_tree, d_status, &root));
    }
    return fetch_and_status(ctx, c_out, root, lb, d_status, steps_on_device ? nullptr : steps_out, d_steps, (n_chain + n_tree) * rec * 8);
}
extern "C" int pz_paillier_wtally(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t w_bits, const uint64_t* n, const uint64_t* cts,
                                  const uint64_t* weights, uint64_t* steps_out, size_t steps_cap, uint64_t* c_out) {
    return wtally_impl(ctx, limbs_n, count, w_bits, n, cts, weights, steps_out, 0, steps_cap, c_out);
}
extern "C" int pz_paillier_wtally_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t w_bits, const uint64_t* n, const uint64_t* cts,
                                      const uint64_t* weights, uint64_t* d_steps_out, size_t steps_cap, uint64_t* c_out) {
    return wtally_impl(ctx, limbs_n, count, w_bits, n, cts, weights, d_steps_out, 1, steps_cap, c_out);
}

// The ballot: c_i = g^m_i r_i^n mod n^2 for `count` messages of m_bits bits under one key (k_ballot_enc, one team per ciphertext, one
// launch).  Records ciphertext-major, 2 m_bits + nr + 1 per entry.  The messages and the r_i are secrets: their staged copies (and, in
// the host form, the staged records, which repeat them) are overwritten before the call returns, on every path past the staging.
#define K3_BALLOT_MAX 1024
struct BallotArgs {
    uint32_t Ln, m_bits, n_bits, per;
    size_t count;
    const uint64_t *n, *g, *ms, *rs;
    uint64_t *steps_out, *c_out;
    int steps_on_device;
    u64 *d_n, *d_g, *d_ms, *d_rs, *d_c, *d_mod, *d_steps;
    u32* d_status;
};
static int ballot_run(pz_ctx* ctx, const BallotArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_g, a.g, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_ms, a.ms, a.count * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_rs, a.rs, a.count * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        K3_LAUNCH(ctx, k_ballot_enc, C, dim3((unsigned)a.count), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_n, a.d_g, a.d_ms, a.d_rs, a.m_bits, a.n_bits,
                  a.per, a.d_steps, a.d_c, a.Ln, a.d_status);
    }
    return fetch_and_status(ctx, a.c_out, a.d_c, a.count * lb, a.d_status, a.steps_on_device ? nullptr : a.steps_out, a.d_steps,
                            a.count * a.per * 4 * lb);
}
static int ballot_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t m_bits, const uint64_t* n, const uint64_t* g, const uint64_t* ms,
                       const uint64_t* rs, uint64_t* steps_out, int steps_on_device, size_t steps_cap, uint32_t* n_steps_r, uint64_t* c_out) {
    if (!ctx || !n || !g || !ms || !rs || !c_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_BALLOT_MAX || m_bits < 1 || m_bits > 64) return PZ_ERR_INVALID;
    const unsigned L = 2 * Ln;
    if (L > 128) return PZ_ERR_UNSUPPORTED;
    // n's bits are public structure of the circuit (pow_mod_fixed_exp): the records of one r^n chain are counted here
    const uint32_t n_bits = bitlen_limbs(n, Ln), nr = (uint32_t)fixed_exp_steps(n, Ln);
    const uint32_t per = 2 * m_bits + nr + 1;
    if (steps_out && steps_cap < count * per) return PZ_ERR_CAPACITY;
    if (m_bits < 64)   // before any launch: the circuit's num_to_bits of such a message cannot hold
        for (size_t i = 0; i < count; ++i)
            if (ms[i] >> m_bits) return PZ_ERR_MESSAGE_RANGE;
    if (n_bits == 0) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // n | g | m_1 .. m_count | r_1 .. r_count | c_1 .. c_count | Barrett constants | status
    const size_t pub_bytes = (2 * nb + 255) & ~(size_t)255, sec_bytes = (count * 8 + count * nb + 255) & ~(size_t)255;
    const size_t c_bytes = (count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + c_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    BallotArgs a{};
    a.Ln = Ln; a.m_bits = m_bits; a.n_bits = n_bits; a.per = per; a.count = count;
    a.n = n; a.g = g; a.ms = ms; a.rs = rs; a.steps_out = steps_out; a.c_out = c_out; a.steps_on_device = steps_on_device;
    a.d_n = (u64*)p;
    a.d_g = (u64*)(p + nb);
    a.d_ms = (u64*)(p + pub_bytes);
    a.d_rs = a.d_ms + count;
    a.d_c = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + c_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + c_bytes + mod_bytes + 64);
    a.d_steps = steps_on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !steps_on_device ? count * per * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    PZCHK(wipe_secrets_and_sync(ctx, ballot_run(ctx, a), a.d_ms, sec_bytes, a.d_steps, rec_bytes));
    if (n_steps_r) *n_steps_r = nr;
    return PZ_OK;
}
extern "C" int pz_paillier_ballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, const uint64_t* n, const uint64_t* g,
                                  const uint64_t* ms, const uint64_t* rs, uint64_t* steps_out, size_t steps_cap, uint32_t* n_steps_r,
                                  uint64_t* c_out) {
    return ballot_impl(ctx, limbs_n, count, m_bits, n, g, ms, rs, steps_out, 0, steps_cap, n_steps_r, c_out);
}
extern "C" int pz_paillier_ballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, const uint64_t* n, const uint64_t* g,
                                      const uint64_t* ms, const uint64_t* rs, uint64_t* d_steps_out, size_t steps_cap, uint32_t* n_steps_r,
                                      uint64_t* c_out) {
    return ballot_impl(ctx, limbs_n, count, m_bits, n, g, ms, rs, d_steps_out, 1, steps_cap, n_steps_r, c_out);
}

// The short-randomness ballot: c_i = g^m_i hs^s_i mod n^2 for `count` messages of m_bits bits and exponents of s_bits
// bits under one key (k_sballot_enc, one team per ciphertext, one launch).  Records ciphertext-major, 2 m_bits + 2 s_bits + 1 per
// entry.  The messages and the s_i are secrets: their staged copies (and, in the host form, the staged records, which repeat them) are
// overwritten before the call returns, on every path past the staging.  The status is read before anything is copied out: a refused
// call (an hs >= n^2) writes nothing.
struct SballotArgs {
    uint32_t Ln, m_bits, s_bits, s_words, per;
    size_t count;
    const uint64_t *n, *g, *hs, *ms, *ss;
    uint64_t *steps_out, *c_out;
    int steps_on_device;
    u64 *d_n, *d_g, *d_hs, *d_ms, *d_ss, *d_c, *d_mod, *d_steps;
    u32* d_status;
};
static int sballot_run(pz_ctx* ctx, const SballotArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_g, a.g, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_hs, a.hs, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_ms, a.ms, a.count * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_ss, a.ss, a.count * a.s_words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        K3_LAUNCH(ctx, k_sballot_enc, C, dim3((unsigned)a.count), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_g, a.d_hs, a.d_ms, a.d_ss, a.m_bits,
                  a.s_bits, a.s_words, a.per, (unsigned)a.count, a.d_steps, a.d_c, a.Ln, a.d_status);
    }
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(&st, a.d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    PZCHK(status_to_rc(ctx, st));
    HIPCHK(ctx, hipMemcpyAsync(a.c_out, a.d_c, a.count * lb, hipMemcpyDeviceToHost, ctx->stream));
    if (a.steps_out && !a.steps_on_device)
        HIPCHK(ctx, hipMemcpyAsync(a.steps_out, a.d_steps, a.count * a.per * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
static int sballot_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t m_bits, uint32_t s_bits, const uint64_t* n, const uint64_t* g,
                        const uint64_t* hs, const uint64_t* ms, const uint64_t* ss, uint64_t* steps_out, int steps_on_device,
                        size_t steps_cap, uint64_t* c_out) {
    if (!ctx || !n || !g || !hs || !ms || !ss || !c_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_BALLOT_MAX || m_bits < 1 || m_bits > 64 || s_bits < 1 || s_bits > 128 * (uint64_t)Ln) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    const unsigned L = 2 * Ln;
    const uint32_t per = 2 * m_bits + 2 * s_bits + 1, s_words = (s_bits + 63) / 64;
    if (steps_out && steps_cap < count * per) return PZ_ERR_CAPACITY;
    // before any launch: the circuit's num_to_bits of such a message or exponent cannot hold, and the chain reads s_bits bits and no more
    for (size_t i = 0; i < count; ++i) {
        if (m_bits < 64 && ms[i] >> m_bits) return PZ_ERR_MESSAGE_RANGE;
        if ((s_bits & 63) && ss[i * s_words + s_words - 1] >> (s_bits & 63)) return PZ_ERR_MESSAGE_RANGE;
    }
    if (bitlen_limbs(n, Ln) == 0) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // n | g | hs | m_1 .. m_count | s_1 .. s_count | c_1 .. c_count | Barrett constants | status
    const size_t pub_bytes = (2 * nb + lb + 255) & ~(size_t)255, sec_bytes = (count * 8 + count * s_words * 8 + 255) & ~(size_t)255;
    const size_t c_bytes = (count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + c_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    SballotArgs a{};
    a.Ln = Ln; a.m_bits = m_bits; a.s_bits = s_bits; a.s_words = s_words; a.per = per; a.count = count;
    a.n = n; a.g = g; a.hs = hs; a.ms = ms; a.ss = ss; a.steps_out = steps_out; a.c_out = c_out; a.steps_on_device = steps_on_device;
    a.d_n = (u64*)p;
    a.d_g = (u64*)(p + nb);
    a.d_hs = (u64*)(p + 2 * nb);
    a.d_ms = (u64*)(p + pub_bytes);
    a.d_ss = a.d_ms + count;
    a.d_c = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + c_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + c_bytes + mod_bytes + 64);
    a.d_steps = steps_on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !steps_on_device ? count * per * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    return wipe_secrets_and_sync(ctx, sballot_run(ctx, a), a.d_ms, sec_bytes, a.d_steps, rec_bytes);
}
extern "C" int pz_paillier_sballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                                   const uint64_t* g, const uint64_t* hs, const uint64_t* ms, const uint64_t* ss, uint64_t* steps_out,
                                   size_t steps_cap, uint64_t* c_out) {
    return sballot_impl(ctx, limbs_n, count, m_bits, s_bits, n, g, hs, ms, ss, steps_out, 0, steps_cap, c_out);
}
extern "C" int pz_paillier_sballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                                       const uint64_t* g, const uint64_t* hs, const uint64_t* ms, const uint64_t* ss, uint64_t* d_steps_out,
                                       size_t steps_cap, uint64_t* c_out) {
    return sballot_impl(ctx, limbs_n, count, m_bits, s_bits, n, g, hs, ms, ss, d_steps_out, 1, steps_cap, c_out);
}

// The packed ballot: c_i = (prod_j G_j^v_ij) hs^s_i mod n^2 for `count` ciphertexts of `slots` values of m_bits bits
// and exponents of s_bits bits under one key (k_pballot_enc, one team per ciphertext, one launch).  Records ciphertext-major,
// 2 m_bits slots + 2 s_bits + slots per entry.  The values and the s_i are secrets: their staged copies (and, in the host form, the
// staged records, which repeat them) are overwritten before the call returns, on every path past the staging.  The status is read
// before anything is copied out: a refused call (an hs or a G_j >= n^2) writes nothing.
#define K3_PBALLOT_SLOTS_MAX 64
struct PballotArgs {
    uint32_t Ln, slots, m_bits, s_bits, s_words, per;
    size_t count;
    const uint64_t *n, *hs, *gs, *vs, *ss;
    uint64_t *steps_out, *c_out;
    int steps_on_device;
    u64 *d_n, *d_hs, *d_gs, *d_vs, *d_ss, *d_c, *d_mod, *d_steps;
    u32* d_status;
};
static int pballot_run(pz_ctx* ctx, const PballotArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_hs, a.hs, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_gs, a.gs, a.slots * lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_vs, a.vs, a.count * a.slots * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_ss, a.ss, a.count * a.s_words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        K3_LAUNCH(ctx, k_pballot_enc, C, dim3((unsigned)a.count), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_hs, a.d_gs, a.d_vs, a.d_ss, a.slots,
                  a.m_bits, a.s_bits, a.s_words, a.per, (unsigned)a.count, a.d_steps, a.d_c, a.Ln, a.d_status);
    }
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(&st, a.d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    PZCHK(status_to_rc(ctx, st));
    HIPCHK(ctx, hipMemcpyAsync(a.c_out, a.d_c, a.count * lb, hipMemcpyDeviceToHost, ctx->stream));
    if (a.steps_out && !a.steps_on_device)
        HIPCHK(ctx, hipMemcpyAsync(a.steps_out, a.d_steps, a.count * a.per * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
static int pballot_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t slots, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                        const uint64_t* hs, const uint64_t* gs, const uint64_t* vs, const uint64_t* ss, uint64_t* steps_out,
                        int steps_on_device, size_t steps_cap, uint64_t* c_out) {
    if (!ctx || !n || !hs || !gs || !vs || !ss || !c_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_BALLOT_MAX || slots < 1 || slots > K3_PBALLOT_SLOTS_MAX || count * slots > K3_BALLOT_MAX) return PZ_ERR_INVALID;
    if (m_bits < 1 || m_bits > 64 || s_bits < 1 || s_bits > 128 * (uint64_t)Ln) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    const unsigned L = 2 * Ln;
    const uint32_t per = 2 * m_bits * slots + 2 * s_bits + slots, s_words = (s_bits + 63) / 64;
    if (steps_out && steps_cap < count * per) return PZ_ERR_CAPACITY;
    // before any launch: the circuit's num_to_bits of such a value or exponent cannot hold, and a chain reads its bits and no more
    for (size_t i = 0; i < count; ++i) {
        for (uint32_t j = 0; j < slots; ++j)
            if (m_bits < 64 && vs[i * slots + j] >> m_bits) return PZ_ERR_MESSAGE_RANGE;
        if ((s_bits & 63) && ss[i * s_words + s_words - 1] >> (s_bits & 63)) return PZ_ERR_MESSAGE_RANGE;
    }
    if (bitlen_limbs(n, Ln) == 0) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // n | hs | G_0 .. G_{slots-1} | v_11 .. v_{count,slots} | s_1 .. s_count | c_1 .. c_count | Barrett constants | status
    const size_t pub_bytes = (nb + lb + slots * lb + 255) & ~(size_t)255;
    const size_t sec_bytes = (count * slots * 8 + count * s_words * 8 + 255) & ~(size_t)255;
    const size_t c_bytes = (count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + c_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    PballotArgs a{};
    a.Ln = Ln; a.slots = slots; a.m_bits = m_bits; a.s_bits = s_bits; a.s_words = s_words; a.per = per; a.count = count;
    a.n = n; a.hs = hs; a.gs = gs; a.vs = vs; a.ss = ss; a.steps_out = steps_out; a.c_out = c_out; a.steps_on_device = steps_on_device;
    a.d_n = (u64*)p;
    a.d_hs = (u64*)(p + nb);
    a.d_gs = (u64*)(p + nb + lb);
    a.d_vs = (u64*)(p + pub_bytes);
    a.d_ss = a.d_vs + count * slots;
    a.d_c = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + c_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + c_bytes + mod_bytes + 64);
    a.d_steps = steps_on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !steps_on_device ? count * per * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    return wipe_secrets_and_sync(ctx, pballot_run(ctx, a), a.d_vs, sec_bytes, a.d_steps, rec_bytes);
}
extern "C" int pz_paillier_pballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t slots, uint32_t m_bits, uint32_t s_bits,
                                   const uint64_t* n, const uint64_t* hs, const uint64_t* gs, const uint64_t* vs, const uint64_t* ss,
                                   uint64_t* steps_out, size_t steps_cap, uint64_t* c_out) {
    return pballot_impl(ctx, limbs_n, count, slots, m_bits, s_bits, n, hs, gs, vs, ss, steps_out, 0, steps_cap, c_out);
}
extern "C" int pz_paillier_pballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t slots, uint32_t m_bits, uint32_t s_bits,
                                       const uint64_t* n, const uint64_t* hs, const uint64_t* gs, const uint64_t* vs, const uint64_t* ss,
                                       uint64_t* d_steps_out, size_t steps_cap, uint64_t* c_out) {
    return pballot_impl(ctx, limbs_n, count, slots, m_bits, s_bits, n, hs, gs, vs, ss, d_steps_out, 1, steps_cap, c_out);
}

// The mix: c'_i = c_perm(i) r_i^n mod n^2 for `count` = 2^d ciphertexts under one key.  The 2d - 1 layers of the
// Benes network (k_mix_route, one launch each, layer l on bit l for l < d and 2d - 2 - l above) move the inputs to their outputs, then
// k_mix_rerand runs the `count` r^n chains and final products in one launch.  routes: every layer's outputs, (2d - 1) x count x L words;
// records output-major, nr + 1 per output.  The switch bits, the r_i and the route layers (which show the permutation) are secrets:
// the staged bits and r_i, and in the host form the staged routes and records, are overwritten before the call returns, on every path
// past the staging.
#define K3_MIX_MAX 1024
struct MixArgs {
    uint32_t Ln, n_bits, per, layers;
    size_t count;
    const uint64_t *n, *cts, *rs;
    const uint8_t* bits;
    uint64_t *routes_out, *steps_out, *mixed_out;
    int on_device;
    u64 *d_n, *d_cts, *d_rs, *d_routes, *d_c, *d_mod, *d_steps;
    uint8_t* d_bits;
    u32* d_status;
};
// the network's layers over d_cts (count x L words), layer l's outputs at d_routes + l * count * L; *routed: the last layer, or d_cts
// itself where count = 1 has no switch
static int mix_route_layers(pz_ctx* ctx, unsigned C, const u64* d_cts, u64* d_routes, const uint8_t* d_bits, unsigned layers, size_t count,
                            unsigned L, const u64** routed) {
    const unsigned half = (unsigned)(count / 2), d = (layers + 1) / 2;
    *routed = d_cts;
    for (unsigned l = 0; l < layers; ++l) {
        const unsigned beta = l < d ? l : layers - 1 - l;
        u64* out = d_routes + l * count * L;
        K3_LAUNCH(ctx, k_mix_route, C, dim3(half), dim3(64), 0, *routed, out, d_bits + (size_t)l * half, beta, half, L);
        *routed = out;
    }
    return PZ_OK;
}
static int mix_run(pz_ctx* ctx, const MixArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L), half = (unsigned)(a.count / 2);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8, layer_words = a.count * L;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_cts, a.cts, a.count * lb, hipMemcpyHostToDevice, ctx->stream));
    if (a.layers) HIPCHK(ctx, hipMemcpyAsync(a.d_bits, a.bits, (size_t)a.layers * half, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_rs, a.rs, a.count * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    const u64* routed;
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        PZCHK(mix_route_layers(ctx, C, a.d_cts, a.d_routes, a.d_bits, a.layers, a.count, L, &routed));
        K3_LAUNCH(ctx, k_mix_rerand, C, dim3((unsigned)a.count), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_n, routed, a.d_rs, a.n_bits, a.per,
                  (unsigned)a.count, a.d_steps, a.d_c, a.Ln, a.d_status);
    }
    // the status first: nothing reaches the caller's buffers from a refused call
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(&st, a.d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    PZCHK(status_to_rc(ctx, st));
    HIPCHK(ctx, hipMemcpyAsync(a.mixed_out, a.d_c, a.count * lb, hipMemcpyDeviceToHost, ctx->stream));
    if (!a.on_device) {
        if (a.routes_out && a.layers)
            HIPCHK(ctx, hipMemcpyAsync(a.routes_out, a.d_routes, a.layers * layer_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (a.steps_out) HIPCHK(ctx, hipMemcpyAsync(a.steps_out, a.d_steps, a.count * a.per * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
static int mix_impl(pz_ctx* ctx, uint32_t Ln, size_t count, const uint64_t* n, const uint64_t* cts, const uint8_t* bits, const uint64_t* rs,
                    uint64_t* routes_out, uint64_t* steps_out, int on_device, size_t steps_cap, uint64_t* mixed_out) {
    if (!ctx || !n || !cts || !rs || !mixed_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_MIX_MAX || (count & (count - 1)) != 0 || (!bits && count > 1)) return PZ_ERR_INVALID;
    const unsigned L = 2 * Ln;
    if (L > 128) return PZ_ERR_UNSUPPORTED;
    // n's bits are public structure of the circuit (pow_mod_fixed_exp): the records of one r^n chain are counted here
    const uint32_t n_bits = bitlen_limbs(n, Ln), nr = (uint32_t)fixed_exp_steps(n, Ln), per = nr + 1;
    if (steps_out && steps_cap < count * per) return PZ_ERR_CAPACITY;
    uint32_t layers = 0;
    for (size_t c = count; c > 1; c >>= 1) layers += 2;
    if (layers) --layers;
    const size_t n_switch = (size_t)layers * (count / 2);
    {   // before any launch: a switch bit is 0 or 1 (every byte is looked at, whatever the others hold)
        unsigned any = 0;
        for (size_t i = 0; i < n_switch; ++i) any |= bits[i];
        if (any > 1) return PZ_ERR_MESSAGE_RANGE;
    }
    if (n_bits == 0) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, route_bytes = (size_t)layers * count * lb;
    const bool ws_routes = layers && !(on_device && routes_out);
    // n | c_1 .. c_count | bits | r_1 .. r_count | the route layers (unless the caller's device buffer takes them) | c'_1 .. c'_count |
    // Barrett constants | status
    const size_t pub_bytes = (nb + count * lb + 255) & ~(size_t)255, bit_bytes = (n_switch + 255) & ~(size_t)255;
    const size_t sec_bytes = bit_bytes + ((count * nb + (ws_routes ? route_bytes : 0) + 255) & ~(size_t)255);
    const size_t c_bytes = (count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + c_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    MixArgs a{};
    a.Ln = Ln; a.n_bits = n_bits; a.per = per; a.layers = layers; a.count = count;
    a.n = n; a.cts = cts; a.rs = rs; a.bits = bits; a.routes_out = routes_out; a.steps_out = steps_out; a.mixed_out = mixed_out;
    a.on_device = on_device;
    a.d_n = (u64*)p;
    a.d_cts = (u64*)(p + nb);
    a.d_bits = (uint8_t*)(p + pub_bytes);
    a.d_rs = (u64*)(p + pub_bytes + bit_bytes);
    a.d_routes = ws_routes ? a.d_rs + count * Ln : routes_out;
    a.d_c = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + c_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + c_bytes + mod_bytes + 64);
    a.d_steps = on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !on_device ? count * per * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    return wipe_secrets_and_sync(ctx, mix_run(ctx, a), a.d_bits, sec_bytes, a.d_steps, rec_bytes);
}
extern "C" int pz_paillier_mix(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, const uint8_t* bits,
                               const uint64_t* rs, uint64_t* routes_out, uint64_t* steps_out, size_t steps_cap, uint64_t* mixed_out) {
    return mix_impl(ctx, limbs_n, count, n, cts, bits, rs, routes_out, steps_out, 0, steps_cap, mixed_out);
}
extern "C" int pz_paillier_mix_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, const uint8_t* bits,
                                   const uint64_t* rs, uint64_t* d_routes_out, uint64_t* d_steps_out, size_t steps_cap, uint64_t* mixed_out) {
    return mix_impl(ctx, limbs_n, count, n, cts, bits, rs, d_routes_out, d_steps_out, 1, steps_cap, mixed_out);
}

// The short-randomness mix: c'_i = c_perm(i) hs^s_i mod n^2 for `count` = 2^d ciphertexts under one key (n, hs).  The
// network is the mix's (mix_route_layers: the same launches, the same route words); k_smix_rerand then runs the `count` hs-chains over
// exactly s_bits bits and the final products in one launch.  Records output-major, 2 s_bits + 1 per output.  The switch bits, the s_i
// and the route layers are secrets: the staged bits and s_i, and in the host form the staged routes and records, are overwritten
// before the call returns, on every path past the staging.  The status is read before anything is copied out.
struct SmixArgs {
    uint32_t Ln, s_bits, s_words, per, layers;
    size_t count;
    const uint64_t *n, *hs, *cts, *ss;
    const uint8_t* bits;
    uint64_t *routes_out, *steps_out, *mixed_out;
    int on_device;
    u64 *d_n, *d_hs, *d_cts, *d_ss, *d_routes, *d_c, *d_mod, *d_steps;
    uint8_t* d_bits;
    u32* d_status;
};
static int smix_run(pz_ctx* ctx, const SmixArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L), half = (unsigned)(a.count / 2);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8, layer_words = a.count * L;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_hs, a.hs, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_cts, a.cts, a.count * lb, hipMemcpyHostToDevice, ctx->stream));
    if (a.layers) HIPCHK(ctx, hipMemcpyAsync(a.d_bits, a.bits, (size_t)a.layers * half, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_ss, a.ss, a.count * a.s_words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    const u64* routed;
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        PZCHK(mix_route_layers(ctx, C, a.d_cts, a.d_routes, a.d_bits, a.layers, a.count, L, &routed));
        K3_LAUNCH(ctx, k_smix_rerand, C, dim3((unsigned)a.count), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_hs, routed, a.d_ss, a.s_bits, a.s_words,
                  a.per, (unsigned)a.count, a.d_steps, a.d_c, a.Ln, a.d_status);
    }
    // the status first: nothing reaches the caller's buffers from a refused call
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(&st, a.d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    PZCHK(status_to_rc(ctx, st));
    HIPCHK(ctx, hipMemcpyAsync(a.mixed_out, a.d_c, a.count * lb, hipMemcpyDeviceToHost, ctx->stream));
    if (!a.on_device) {
        if (a.routes_out && a.layers)
            HIPCHK(ctx, hipMemcpyAsync(a.routes_out, a.d_routes, a.layers * layer_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (a.steps_out) HIPCHK(ctx, hipMemcpyAsync(a.steps_out, a.d_steps, a.count * a.per * 4 * lb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
static int smix_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t s_bits, const uint64_t* n, const uint64_t* hs, const uint64_t* cts,
                     const uint8_t* bits, const uint64_t* ss, uint64_t* routes_out, uint64_t* steps_out, int on_device, size_t steps_cap,
                     uint64_t* mixed_out) {
    if (!ctx || !n || !hs || !cts || !ss || !mixed_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_MIX_MAX || (count & (count - 1)) != 0 || (!bits && count > 1)) return PZ_ERR_INVALID;
    if (s_bits < 1 || s_bits > 128 * (uint64_t)Ln) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    const unsigned L = 2 * Ln;
    const uint32_t per = 2 * s_bits + 1, s_words = (s_bits + 63) / 64;
    if (steps_out && steps_cap < count * per) return PZ_ERR_CAPACITY;
    uint32_t layers = 0;
    for (size_t c = count; c > 1; c >>= 1) layers += 2;
    if (layers) --layers;
    const size_t n_switch = (size_t)layers * (count / 2);
    {   // before any launch: a switch bit is 0 or 1 (every byte is looked at, whatever the others hold), and the chain reads s_bits bits
        unsigned any = 0;
        for (size_t i = 0; i < n_switch; ++i) any |= bits[i];
        if (any > 1) return PZ_ERR_MESSAGE_RANGE;
        uint64_t over = 0;
        if (s_bits & 63)
            for (size_t i = 0; i < count; ++i) over |= ss[i * s_words + s_words - 1] >> (s_bits & 63);
        if (over) return PZ_ERR_MESSAGE_RANGE;
    }
    if (bitlen_limbs(n, Ln) == 0) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, route_bytes = (size_t)layers * count * lb, ss_bytes = count * s_words * 8;
    const bool ws_routes = layers && !(on_device && routes_out);
    // n | hs | c_1 .. c_count | bits | s_1 .. s_count | the route layers (unless the caller's device buffer takes them) | c'_1 ..
    // c'_count | Barrett constants | status
    const size_t pub_bytes = (nb + lb + count * lb + 255) & ~(size_t)255, bit_bytes = (n_switch + 255) & ~(size_t)255;
    const size_t sec_bytes = bit_bytes + ((ss_bytes + (ws_routes ? route_bytes : 0) + 255) & ~(size_t)255);
    const size_t c_bytes = (count * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + c_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    SmixArgs a{};
    a.Ln = Ln; a.s_bits = s_bits; a.s_words = s_words; a.per = per; a.layers = layers; a.count = count;
    a.n = n; a.hs = hs; a.cts = cts; a.ss = ss; a.bits = bits; a.routes_out = routes_out; a.steps_out = steps_out; a.mixed_out = mixed_out;
    a.on_device = on_device;
    a.d_n = (u64*)p;
    a.d_hs = (u64*)(p + nb);
    a.d_cts = (u64*)(p + nb + lb);
    a.d_bits = (uint8_t*)(p + pub_bytes);
    a.d_ss = (u64*)(p + pub_bytes + bit_bytes);
    a.d_routes = ws_routes ? a.d_ss + count * s_words : routes_out;
    a.d_c = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + c_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + c_bytes + mod_bytes + 64);
    a.d_steps = on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !on_device ? count * per * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    return wipe_secrets_and_sync(ctx, smix_run(ctx, a), a.d_bits, sec_bytes, a.d_steps, rec_bytes);
}
extern "C" int pz_paillier_smix(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t s_bits, const uint64_t* n, const uint64_t* hs,
                                const uint64_t* cts, const uint8_t* bits, const uint64_t* ss, uint64_t* routes_out, uint64_t* steps_out,
                                size_t steps_cap, uint64_t* mixed_out) {
    return smix_impl(ctx, limbs_n, count, s_bits, n, hs, cts, bits, ss, routes_out, steps_out, 0, steps_cap, mixed_out);
}
extern "C" int pz_paillier_smix_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t s_bits, const uint64_t* n, const uint64_t* hs,
                                    const uint64_t* cts, const uint8_t* bits, const uint64_t* ss, uint64_t* d_routes_out,
                                    uint64_t* d_steps_out, size_t steps_cap, uint64_t* mixed_out) {
    return smix_impl(ctx, limbs_n, count, s_bits, n, hs, cts, bits, ss, d_routes_out, d_steps_out, 1, steps_cap, mixed_out);
}

// A trustee's partial decryptions: h = v^theta, u_j = (c_j^2)^theta mod n^2 for `count` ciphertexts under one share
// (k_partial_pow, count + 1 teams, one launch).  Records: the count squarings, then chain i at count + i 2 e_bits.  theta is the
// trustee's secret: its staged copy (and, in the host form, the staged records, whose quotients and accumulators follow its bits) are
// overwritten before the call returns, on every path past the staging.
#define K3_PARTIAL_MAX 1024
static bool is_zero_limbs(const uint64_t* a, uint32_t n) {
    uint64_t any = 0;
    for (uint32_t i = 0; i < n; ++i) any |= a[i];
    return any == 0;
}
struct PartialArgs {
    uint32_t Ln, e_bits;
    size_t count, n_rec;
    const uint64_t *n, *v, *theta, *cts;
    uint64_t *steps_out, *h_out, *u_out;
    int steps_on_device;
    u64 *d_n, *d_v, *d_cts, *d_theta, *d_out, *d_mod, *d_steps;
    u32* d_status;
};
static int partial_run(pz_ctx* ctx, const PartialArgs& a) {
    const unsigned L = 2 * a.Ln, C = capacity(L);
    const size_t nb = (size_t)a.Ln * 8, lb = (size_t)L * 8;
    HIPCHK(ctx, hipMemcpyAsync(a.d_n, a.n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_v, a.v, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_cts, a.cts, a.count * lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(a.d_theta, a.theta, lb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(a.d_status, 0, 4, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        PZCHK(launch_barrett_setup(ctx, C, a.d_n, a.Ln, 1, a.d_mod, a.d_status));
        K3_LAUNCH(ctx, k_partial_pow, C, dim3((unsigned)a.count + 1), dim3(64 * K3_TEAM), 0, a.d_mod, a.d_v, a.d_cts, a.d_theta, a.e_bits,
                  (unsigned)a.count, a.d_steps, a.d_out, a.d_out + L, L, a.d_status);
    }
    HIPCHK(ctx, hipMemcpyAsync(a.h_out, a.d_out, lb, hipMemcpyDeviceToHost, ctx->stream));
    return fetch_and_status(ctx, a.u_out, a.d_out + L, a.count * lb, a.d_status, a.steps_on_device ? nullptr : a.steps_out, a.d_steps,
                            a.n_rec * 4 * lb);
}
static int partial_impl(pz_ctx* ctx, uint32_t Ln, size_t count, uint32_t e_bits, const uint64_t* n, const uint64_t* v, const uint64_t* theta,
                        const uint64_t* cts, uint64_t* steps_out, int steps_on_device, size_t steps_cap, uint64_t* h_out, uint64_t* u_out) {
    if (!ctx || !n || !v || !theta || !cts || !h_out || !u_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_PARTIAL_MAX || e_bits < 1 || e_bits > 128 * (uint64_t)Ln) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    const unsigned L = 2 * Ln;
    const size_t n_rec = count + (count + 1) * 2 * (size_t)e_bits;
    if (steps_out && steps_cap < n_rec) return PZ_ERR_CAPACITY;
    for (uint32_t k = e_bits / 64; k < L; ++k)   // before any launch: the chain reads e_bits bits and the circuit's decomposition no more
        if (k == e_bits / 64 ? theta[k] >> (e_bits & 63) : theta[k]) return PZ_ERR_MESSAGE_RANGE;
    if (is_zero_limbs(n, Ln)) return PZ_ERR_ZERO_MODULUS;
    PZ_ENTER(ctx);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // n | v | c_1 .. c_count | theta | h | u_1 .. u_count | Barrett constants | status
    const size_t pub_bytes = (nb + lb + count * lb + 255) & ~(size_t)255, sec_bytes = (lb + 255) & ~(size_t)255;
    const size_t out_bytes = ((count + 1) * lb + 255) & ~(size_t)255, mod_bytes = mod_block_words(capacity(L)) * 8;
    void* d;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, pub_bytes + sec_bytes + out_bytes + mod_bytes + 256, &d));
    char* p = (char*)d;
    PartialArgs a{};
    a.Ln = Ln; a.e_bits = e_bits; a.count = count; a.n_rec = n_rec;
    a.n = n; a.v = v; a.theta = theta; a.cts = cts; a.steps_out = steps_out; a.h_out = h_out; a.u_out = u_out;
    a.steps_on_device = steps_on_device;
    a.d_n = (u64*)p;
    a.d_v = (u64*)(p + nb);
    a.d_cts = (u64*)(p + nb + lb);
    a.d_theta = (u64*)(p + pub_bytes);
    a.d_out = (u64*)(p + pub_bytes + sec_bytes);
    a.d_mod = (u64*)(p + pub_bytes + sec_bytes + out_bytes);
    a.d_status = (u32*)(p + pub_bytes + sec_bytes + out_bytes + mod_bytes + 64);
    a.d_steps = steps_on_device ? steps_out : nullptr;
    const size_t rec_bytes = steps_out && !steps_on_device ? n_rec * 4 * lb : 0;
    if (rec_bytes) {
        void* t;
        PZCHK(pz_ws_get(ctx, WS_BIG_B, rec_bytes, &t));
        a.d_steps = (u64*)t;
    }
    return wipe_secrets_and_sync(ctx, partial_run(ctx, a), a.d_theta, sec_bytes, a.d_steps, rec_bytes);
}
extern "C" int pz_paillier_partial(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t e_bits, const uint64_t* n, const uint64_t* v,
                                   const uint64_t* theta, const uint64_t* cts, uint64_t* steps_out, size_t steps_cap, uint64_t* h_out,
                                   uint64_t* u_out) {
    return partial_impl(ctx, limbs_n, count, e_bits, n, v, theta, cts, steps_out, 0, steps_cap, h_out, u_out);
}
extern "C" int pz_paillier_partial_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t e_bits, const uint64_t* n, const uint64_t* v,
                                       const uint64_t* theta, const uint64_t* cts, uint64_t* d_steps_out, size_t steps_cap, uint64_t* h_out,
                                       uint64_t* u_out) {
    return partial_impl(ctx, limbs_n, count, e_bits, n, v, theta, cts, d_steps_out, 1, steps_cap, h_out, u_out);
}

// The combiner: m_j = L(prod_i u_ij mod n^2) mu2 mod n (k_partial_combine, one team per ciphertext, one launch).  n and mu2 are the
// public threshold key's (HOST words in both forms); the host form stages the partials and fetches m and the flags, the device form
// queues everything on the context's stream and returns.
// The t-of-T combiner shares all of it (combine_run) and adds its public exponents and signs (CombineExps; null: k_partial_combine).
struct CombineExps {
    const uint64_t* exps;   // members x exp_words HOST words
    uint32_t exp_words;
    const uint8_t* neg;     // members HOST bytes
    unsigned max_bits;      // the longest exponent: the chain length
};
static int combine_run(pz_ctx* ctx, uint32_t Ln, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2, const CombineExps* x,
                       const uint64_t* partials, uint64_t* m_out, uint8_t* flags_out, int on_device) {
    PZ_ENTER(ctx);
    const unsigned L = 2 * Ln, C = capacity(L);
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, mod_words = mod_block_words(C);
    // n | mu2 | t-of-T: exponents | signs | Barrett constants of n^2 and of n | status | host form: the partials, m, the flags
    const size_t exp_bytes = x ? members * x->exp_words * 8 : 0, neg_bytes = x ? (members + 7) & ~(size_t)7 : 0;
    const size_t key_bytes = (2 * nb + exp_bytes + neg_bytes + 255) & ~(size_t)255, mod_bytes = 2 * mod_words * 8 + 64;
    const size_t io_bytes = on_device ? 0 : members * count * lb + count * nb + ((count + 7) & ~(size_t)7);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, key_bytes + mod_bytes + io_bytes + 64, &ws));
    char* p = (char*)ws;
    u64 *d_n = (u64*)p, *d_mu2 = d_n + Ln, *d_exps = d_mu2 + Ln;
    uint8_t* d_neg = (uint8_t*)d_exps + exp_bytes;
    u64 *d_mod2 = (u64*)(p + key_bytes), *d_modn = d_mod2 + mod_words;
    u32* d_status = (u32*)(d_modn + mod_words);
    const u64* d_parts = partials;
    u64* d_m = m_out;
    uint8_t* d_flags = flags_out;
    if (!on_device) {
        u64* q = (u64*)(p + key_bytes + mod_bytes);
        d_parts = q;
        d_m = q + members * count * L;
        d_flags = (uint8_t*)(d_m + count * Ln);
        HIPCHK(ctx, hipMemcpyAsync(q, partials, members * count * lb, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(d_n, n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_mu2, mu2, nb, hipMemcpyHostToDevice, ctx->stream));
    if (x) {
        HIPCHK(ctx, hipMemcpyAsync(d_exps, x->exps, exp_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_neg, x->neg, members, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, 4, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        const dim3 grid((unsigned)count), block(64 * K3_TEAM);
        PZCHK(launch_barrett_setup(ctx, C, d_n, Ln, 1, d_mod2, d_status));
        PZCHK(launch_barrett_setup(ctx, C, d_n, Ln, 0, d_modn, d_status));
        if (x)
            K3_LAUNCH(ctx, k_combine_t, C, grid, block, 0, d_mod2, d_modn, d_parts, (unsigned)count, (unsigned)members, d_exps, x->exp_words, d_neg,
                      x->max_bits, 2 * bitlen_limbs(n, Ln) + 4, d_mu2, d_m, d_flags, Ln);
        else
            K3_LAUNCH(ctx, k_partial_combine, C, grid, block, 0, d_mod2, d_modn, d_parts, (unsigned)count, (unsigned)members, d_mu2, d_m, d_flags, Ln);
    }
    if (on_device) return PZ_OK;
    HIPCHK(ctx, hipMemcpyAsync(m_out, d_m, count * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags_out, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned any = 0;
    for (size_t i = 0; i < count; ++i) any |= flags_out[i];
    if (any & CMB_F_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (%scombination)", x ? "t-of-T " : "");
        return PZ_ERR_HIP;
    }
    return (any & CMB_F_RANGE) ? PZ_ERR_RANGE : PZ_OK;
}
static int combine_impl(pz_ctx* ctx, uint32_t Ln, size_t count, size_t trustees, const uint64_t* n, const uint64_t* mu2,
                        const uint64_t* partials, uint64_t* m_out, uint8_t* flags_out, int on_device) {
    if (!ctx || !n || !mu2 || !partials || !m_out || !flags_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_PARTIAL_MAX || trustees < 1 || trustees > 256) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    if (is_zero_limbs(n, Ln)) return PZ_ERR_ZERO_MODULUS;
    return combine_run(ctx, Ln, count, trustees, n, mu2, nullptr, partials, m_out, flags_out, on_device);
}
extern "C" int pz_paillier_combine(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t trustees, const uint64_t* n, const uint64_t* mu2,
                                   const uint64_t* partials, uint64_t* m_out, uint8_t* flags_out) {
    return combine_impl(ctx, limbs_n, count, trustees, n, mu2, partials, m_out, flags_out, 0);
}
extern "C" int pz_paillier_combine_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t trustees, const uint64_t* n, const uint64_t* mu2,
                                       const uint64_t* d_partials, uint64_t* d_m_out, uint8_t* d_flags_out) {
    return combine_impl(ctx, limbs_n, count, trustees, n, mu2, d_partials, d_m_out, d_flags_out, 1);
}

// Batch modular inverse under ONE odd modulus: k_mod_inverse, one wave per value.  The modulus is HOST words in both
// forms; the iteration bound of every wave is 2 bitlen(mod) + 4, from the modulus alone.
#define K3_INV_MAX 65536
static int mod_inverse_impl(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* mod, const uint64_t* xs, uint64_t* inv_out,
                            uint8_t* flags_out, int on_device) {
    if (!ctx || !mod || !xs || !inv_out || !flags_out || limbs == 0 || count < 1 || count > K3_INV_MAX) return PZ_ERR_INVALID;
    if (limbs > 128) return PZ_ERR_UNSUPPORTED;
    if (is_zero_limbs(mod, limbs)) return PZ_ERR_ZERO_MODULUS;
    if (!(mod[0] & 1) || (mod[0] == 1 && is_zero_limbs(mod + 1, limbs - 1))) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    const size_t vb = (size_t)limbs * 8, mod_bytes = (vb + 255) & ~(size_t)255;
    const size_t io_bytes = on_device ? 0 : 2 * count * vb + ((count + 7) & ~(size_t)7);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, mod_bytes + io_bytes, &ws));
    u64* d_mod = (u64*)ws;
    const u64* d_xs = xs;
    u64* d_inv = inv_out;
    uint8_t* d_flags = flags_out;
    if (!on_device) {
        u64* q = (u64*)((char*)ws + mod_bytes);
        d_xs = q;
        d_inv = q + count * limbs;
        d_flags = (uint8_t*)(d_inv + count * limbs);
        HIPCHK(ctx, hipMemcpyAsync(q, xs, count * vb, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(d_mod, mod, vb, hipMemcpyHostToDevice, ctx->stream));
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        const dim3 grid((unsigned)((count + K3_INV_WAVES - 1) / K3_INV_WAVES)), block(64 * K3_INV_WAVES);
        const unsigned iters = 2 * bitlen_limbs(mod, limbs) + 4;
        K3_LAUNCH(ctx, k_mod_inverse, capacity(limbs), grid, block, 0, d_mod, d_xs, d_inv, d_flags, limbs, (unsigned)count, iters);
    }
    if (on_device) return PZ_OK;
    HIPCHK(ctx, hipMemcpyAsync(inv_out, d_inv, count * vb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags_out, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned any = 0;
    for (size_t i = 0; i < count; ++i) any |= flags_out[i];
    if (any & 4) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: the modular inverse's iteration bound ran out");
        return PZ_ERR_HIP;
    }
    return (any & 2) ? PZ_ERR_RANGE : PZ_OK;
}
extern "C" int pz_bigint_mod_inverse(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* mod, const uint64_t* xs, uint64_t* inv_out,
                                     uint8_t* flags_out) {
    return mod_inverse_impl(ctx, limbs, count, mod, xs, inv_out, flags_out, 0);
}
extern "C" int pz_bigint_mod_inverse_dev(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* mod, const uint64_t* d_xs,
                                         uint64_t* d_inv_out, uint8_t* d_flags_out) {
    return mod_inverse_impl(ctx, limbs, count, mod, d_xs, d_inv_out, d_flags_out, 1);
}

// The t-of-T combiner: k_combine_t, one team per ciphertext, one launch.  n, mu2, the exponents and the signs are
// public HOST values in both forms; the chain length (the longest exponent) is found here and passed to the launch.
static int combine_t_impl(pz_ctx* ctx, uint32_t Ln, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2,
                          const uint64_t* exps, uint32_t exp_words, const uint8_t* neg, const uint64_t* partials, uint64_t* m_out,
                          uint8_t* flags_out, int on_device) {
    if (!ctx || !n || !mu2 || !exps || !neg || !partials || !m_out || !flags_out || Ln == 0) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_PARTIAL_MAX || members < 1 || members > 256 || exp_words < 1 || exp_words > 64) return PZ_ERR_INVALID;
    if (2 * (uint64_t)Ln > 128) return PZ_ERR_UNSUPPORTED;
    if (is_zero_limbs(n, Ln)) return PZ_ERR_ZERO_MODULUS;
    unsigned max_bits = 0;
    for (size_t i = 0; i < members; ++i) {
        const unsigned b = bitlen_limbs(exps + i * exp_words, exp_words);
        if (b == 0) return PZ_ERR_INVALID;
        max_bits = b > max_bits ? b : max_bits;
    }
    for (size_t i = 0; i < members; ++i)
        if (neg[i] > 1) return PZ_ERR_INVALID;
    const CombineExps x{exps, exp_words, neg, max_bits};
    return combine_run(ctx, Ln, count, members, n, mu2, &x, partials, m_out, flags_out, on_device);
}
extern "C" int pz_paillier_combine_t(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2,
                                     const uint64_t* exps, uint32_t exp_words, const uint8_t* neg, const uint64_t* partials,
                                     uint64_t* m_out, uint8_t* flags_out) {
    return combine_t_impl(ctx, limbs_n, count, members, n, mu2, exps, exp_words, neg, partials, m_out, flags_out, 0);
}
extern "C" int pz_paillier_combine_t_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2,
                                         const uint64_t* exps, uint32_t exp_words, const uint8_t* neg, const uint64_t* d_partials,
                                         uint64_t* d_m_out, uint8_t* d_flags_out) {
    return combine_t_impl(ctx, limbs_n, count, members, n, mu2, exps, exp_words, neg, d_partials, d_m_out, d_flags_out, 1);
}

// ------------------------------------------------------------------------------------------------
// decryption (pz_paillier_sk_*, pz_paillier_decrypt[_dev])
// ------------------------------------------------------------------------------------------------
// The powers of a decryption carry SECRET exponents (lambda, d, the plaintext), and nothing of them is proved, so no records are written
// and the schedule is a fixed-window one: the exponent is cut into ceil(nbits / w) windows of w bits, most significant first, nbits the
// bit length of n (public); every window below the top one does w squarings and ONE product by a table entry (the table's 1 for a zero
// window).  The table base^0 .. base^(2^w - 1) lives in the team's LDS; an entry is chosen by reading ALL 2^w entries and keeping one
// lane-wise under a mask, so neither the instruction stream nor an address depends on the exponent.  (What a mul_mod does with its
// VALUES is K3's as everywhere: the Barrett correction's trip count follows the operands.)  One team per chain, one launch per power
// over all chains, no ticket, no spin, no hand-off: k_wtally_pow's shape.
// Entry flags: bit 0 the ciphertext is no unit (c^lambda mod n != 1), bit 1 it is >= n^2, bit 2 an internal check failed.
#define K3_DEC_WINDOW 5   // 64 decryptions with r at 2048 bits: 59.0 ms against 60.5 (w = 4) and 95.7 (w = 1), profiles/decrypt_probe.jsonl
enum { DEC_POW = 0, DEC_LFN = 1 };
enum { DEC_F_NOT_UNIT = 1, DEC_F_RANGE = 2, DEC_F_INTERNAL = 4 };
struct DecPow {
    const u64* modP;     // Barrett block (k_tally_setup's layout at THIS instantiation's capacity) of the power's modulus
    const u64* modN;     // DEC_LFN: the same for n
    const u64* base;     // chain i: base + i * base_stride, base_limbs limbs, below the modulus
    const u64* exp;      // chain i: exp + i * exp_stride, exp_limbs limbs, below 2^nbits
    const u64* aux;      // DEC_POW, may be null: the power is multiplied by aux + i * Lp (mod the modulus)
    const u64* mu;       // DEC_LFN: Ln limbs
    u64 *out0, *out1;    // DEC_POW: out0 + i * Lp the power (zero where flags[i] != 0).  DEC_LFN: out0 + i * Ln the plaintext
                         // floor(u / n) * mu mod n (zero where flagged), out1 + i * Ln the base mod n
    uint8_t* flags;      // DEC_POW: read (may be null); DEC_LFN: written
    size_t base_stride, exp_stride;
    u32 base_limbs, exp_limbs, nbits, w, mode, Lp, Ln;
};
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_dec_pow(const DecPow A) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    extern __shared__ u64 s_table[];   // 2^w entries of Lp limbs
    if (*block_ok<E>(A.modP) == 0) return;   // zero modulus (pz_paillier_sk_create refuses it: no handle reaches here with one)
    const unsigned wave = threadIdx.x >> 6, lane = lane_id();
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    BarrettCtx<E> B;
    barrett_from_block(B, A.modP, A.Lp, s_scratch[wave]);
    const size_t chain = blockIdx.x;
    const unsigned Lp = A.Lp, Ln = A.Ln, nent = 1u << A.w;
    const LD<E> base = ld_load<E>(A.base + chain * A.base_stride, A.base_limbs);
    {   // a base >= the modulus (a ciphertext >= n^2: public).  The four waves hold the same values: the team leaves together
        LD<E> d;
        if (!ld_sub(d, base, ld_load<E>(block_modulus<E>(A.modP), C))) {
            if (wave == 0) {
                const unsigned Lo = A.mode == DEC_LFN ? Ln : Lp;
                ld_store(A.out0 + chain * Lo, ld_zero<E>(), Lo);
                if (A.mode == DEC_LFN) {
                    ld_store(A.out1 + chain * Lo, ld_zero<E>(), Lo);
                    if (lane == 0) A.flags[chain] = DEC_F_RANGE;
                }
            }
            return;
        }
    }
    unsigned st = ST_OK;
    const LD<E> one = ld_small<E>(1);
    {   // the table: entry k = base^k
        LD<E> cur = one;
        for (unsigned k = 0; k < nent; ++k) {
            if (wave == 0) ld_store(s_table + (size_t)k * Lp, cur, Lp);
            if (k + 1 < nent) {
                LD<E> q, r;
                st |= mul_mod(B, q, r, cur, base, tmul);
                cur = r;
            }
        }
        __syncthreads();
    }
    const u64* ex = A.exp + chain * A.exp_stride;
    // window at bit p (a position: public), and the entry it names, read under a mask from all of them
    auto pick = [&](unsigned p) {
        const unsigned wi = p >> 6, sh = p & 63;
        const u64 lo = wi < A.exp_limbs ? ex[wi] : 0, hi = wi + 1 < A.exp_limbs ? ex[wi + 1] : 0;
        u64 v = lo >> sh;
        if (sh) v |= hi << (64 - sh);
        u32 idx = (u32)v & (nent - 1);
        asm volatile("" : "+v"(idx));   // a per-lane value from here on: nothing below can become a branch or an address
        LD<E> r = ld_zero<E>();
        for (unsigned k = 0; k < nent; ++k) {
            const u64 keep = 0ull - (u64)(idx == k);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const unsigned t = lane * E + e;
                const u64 v2 = t < Lp ? s_table[(size_t)k * Lp + t] : 0;
                r.v[e] |= v2 & keep;
            }
        }
        return r;
    };
    const unsigned nwin = (A.nbits + A.w - 1) / A.w;
    LD<E> acc = pick((nwin - 1) * A.w);
    for (unsigned i = nwin - 1; i-- > 0;) {
        LD<E> q, r;
        for (unsigned s = 0; s < A.w; ++s) {
            st |= mul_mod(B, q, r, acc, acc, tmul);
            acc = r;
        }
        st |= mul_mod(B, q, r, acc, pick(i * A.w), tmul);
        acc = r;
    }
    if (A.mode == DEC_POW) {
        if (A.aux) {
            LD<E> q, r;
            st |= mul_mod(B, q, r, acc, ld_load<E>(A.aux + chain * Lp, Lp), tmul);
            acc = r;
        }
        if (A.flags && A.flags[chain]) acc = ld_zero<E>();
        if (wave == 0) ld_store(A.out0 + chain * Lp, acc, Lp);
        if (st && A.flags && wave == 0 && lane == 0) A.flags[chain] |= DEC_F_INTERNAL;   // (the key derivation passes none: its checks catch a wrong mu)
        return;
    }
    // u = acc = c^lambda mod n^2: the plaintext, and the base mod n
    BarrettCtx<E> N;
    barrett_from_block(N, A.modN, Lp, s_scratch[wave]);
    LD<E> m, q, cn;
    const bool bad = lfn_tail(N, T, m, acc, A.mu, Ln, st);
    st |= mul_mod(N, q, cn, base, one, tmul);
    if (wave == 0) {
        ld_store(A.out0 + chain * Ln, m, Ln);
        ld_store(A.out1 + chain * Ln, cn, Ln);
        if (lane == 0) A.flags[chain] = (uint8_t)((bad ? DEC_F_NOT_UNIT : 0) | (st ? DEC_F_INTERNAL : 0));
    }
}

// The key handle.  One device block: Barrett constants of n^2 (at the capacity C of 2 * limbs_n limbs), of n at C and of n at 64
// limbs (the powers mod n always fit one limb per lane: limbs_n <= 64), then n | lambda | d | mu | ginv.  mu and ginv are kept on the
// host as well (pz_paillier_sk_params has no context to fetch them with).
struct pz_paillier_sk {
    uint32_t Ln = 0, nbits = 0;
    unsigned C = 64;
    u64* d_block = nullptr;
    size_t block_bytes = 0;
    u64 *d_mod2 = nullptr, *d_modn_c = nullptr, *d_modn = nullptr, *d_n = nullptr, *d_lam = nullptr, *d_d = nullptr, *d_mu = nullptr, *d_ginv = nullptr;
    std::vector<u64> h_mu, h_ginv;
    bool ginv_one = false;
    // the CRT part (pz_paillier_sk_create_crt), behind ginv in the same block: side p | side q (crt_side_words each) |
    // qinv | where n^2 leaves the 64-limb instantiation, the Barrett blocks of p^2 and q^2 at its capacity (k_crt_split)
    size_t crt_words = 0;
    bool crt = false;
    u64 *d_side[2] = {nullptr, nullptr}, *d_qinv = nullptr, *d_p2c[2] = {nullptr, nullptr};
    uint32_t pbits[2] = {0, 0};
};
static unsigned dec_window() {   // PZ_K3_DEC_WINDOW (1 .. 5) is a measurement hook, honoured only with PZ_K3_TEST_HOOKS=1 like the others
    const char* on = getenv("PZ_K3_TEST_HOOKS");
    if (!(on && on[0] == '1')) return K3_DEC_WINDOW;
    const unsigned w = env_u32("PZ_K3_DEC_WINDOW", K3_DEC_WINDOW);
    return w >= 1 && w <= 5 ? w : K3_DEC_WINDOW;
}
static int launch_dec_pow(pz_ctx* ctx, unsigned C, size_t chains, const DecPow& a) {
    const size_t table = ((size_t)8 << a.w) * a.Lp;
    K3_LAUNCH(ctx, k_dec_pow, C, dim3((unsigned)chains), dim3(64 * K3_TEAM), table, a);
    return PZ_OK;
}
static int cmp_limbs(const uint64_t* a, const uint64_t* b, uint32_t n) {
    for (uint32_t i = n; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
static bool is_small(const uint64_t* a, uint32_t n, uint64_t v) {
    for (uint32_t i = 1; i < n; ++i)
        if (a[i]) return false;
    return a[0] == v;
}
// overwrite in stream order, then release (pz_dev_free waits for the queued work)
static int sk_release(pz_ctx* ctx, pz_paillier_sk* sk) {
    int rc = PZ_OK;
    if (sk->d_block) {
        if (hipMemsetAsync(sk->d_block, 0, sk->block_bytes, ctx->stream) != hipSuccess) rc = PZ_ERR_HIP;
        const int rf = pz_dev_free(ctx, sk->d_block);
        if (rc == PZ_OK) rc = rf;
    }
    std::fill(sk->h_mu.begin(), sk->h_mu.end(), 0);
    std::fill(sk->h_ginv.begin(), sk->h_ginv.end(), 0);
    delete sk;
    return rc;
}
static int sk_create_impl(pz_ctx* ctx, pz_paillier_sk* sk, const uint64_t* n, const uint64_t* g, const uint64_t* lambda, const uint64_t* d) {
    const uint32_t Ln = sk->Ln;
    const unsigned L = 2 * Ln, C = sk->C;
    const size_t nb = (size_t)Ln * 8, blk = mod_block_words(C), blk1 = mod_block_words(64);
    sk->block_bytes = (2 * blk + blk1 + 5 * (size_t)Ln + sk->crt_words) * 8;   // (crt_words: 0 unless pz_paillier_sk_create_crt made the handle)
    void* dv;
    PZCHK(pz_dev_alloc(ctx, sk->block_bytes, &dv));
    sk->d_block = (u64*)dv;
    sk->d_mod2 = sk->d_block;
    sk->d_modn_c = sk->d_mod2 + blk;
    sk->d_modn = C == 64 ? sk->d_modn_c : sk->d_modn_c + blk;
    sk->d_n = sk->d_modn_c + blk + blk1;
    sk->d_lam = sk->d_n + Ln;
    sk->d_d = sk->d_lam + Ln;
    sk->d_mu = sk->d_d + Ln;
    sk->d_ginv = sk->d_mu + Ln;
    // staging (shared workspace, overwritten below): g | lambda - 1 | 1 | x | g mod n | x mu mod n | n d mod lambda | flag | status | descs
    std::vector<u64> lam1(lambda, lambda + Ln), one(Ln, 0);
    for (uint32_t i = 0; i < Ln && lam1[i]-- == 0; ++i) {}
    one[0] = 1;
    const size_t stage_bytes = 7 * nb + 128 + 2 * sizeof(MulDesc);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, stage_bytes, &ws));
    char* p = (char*)ws;
    u64 *s_g = (u64*)p, *s_lam1 = s_g + Ln, *s_one = s_lam1 + Ln, *s_x = s_one + Ln, *s_gn = s_x + Ln, *s_c1 = s_gn + Ln, *s_c2 = s_c1 + Ln;
    uint8_t* s_flag = (uint8_t*)(p + 7 * nb);
    u32* s_status = (u32*)(p + 7 * nb + 64);
    MulDesc* s_desc = (MulDesc*)(p + 7 * nb + 128);
    struct Wipe {   // on every path out: the staging copies are overwritten and the queue drained (lam1 goes through pageable memory)
        pz_ctx* c; void* p; size_t n; std::vector<u64>& h;
        ~Wipe() {
            (void)hipMemsetAsync(p, 0, n, c->stream);
            (void)hipStreamSynchronize(c->stream);
            std::fill(h.begin(), h.end(), 0);
        }
    } wipe{ctx, ws, stage_bytes, lam1};
    HIPCHK(ctx, hipMemsetAsync(p + 7 * nb, 0, 128, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sk->d_n, n, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sk->d_lam, lambda, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sk->d_d, d, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s_g, g, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s_lam1, lam1.data(), nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s_one, one.data(), nb, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(launch_barrett_setup(ctx, C, sk->d_n, Ln, 1, sk->d_mod2, s_status));
    PZCHK(launch_barrett_setup(ctx, C, sk->d_n, Ln, 0, sk->d_modn_c, s_status));
    if (C != 64) PZCHK(launch_barrett_setup(ctx, 64, sk->d_n, Ln, 0, sk->d_modn, s_status));   // (C = 64: d_modn is d_modn_c)
    const unsigned w = dec_window();
    DecPow a{};
    // x = L(g^lambda mod n^2) (the plaintext of g under mu = 1), g mod n, and the flag g^lambda mod n != 1
    a.modP = sk->d_mod2; a.modN = sk->d_modn_c; a.base = s_g; a.base_limbs = Ln; a.exp = sk->d_lam; a.exp_limbs = Ln; a.mu = s_one;
    a.out0 = s_x; a.out1 = s_gn; a.flags = s_flag; a.nbits = sk->nbits; a.w = w; a.mode = DEC_LFN; a.Lp = L; a.Ln = Ln;
    PZCHK(launch_dec_pow(ctx, C, 1, a));
    // mu = x^(lambda - 1), ginv = (g mod n)^(lambda - 1) mod n: both orders divide lambda
    DecPow b{};
    b.modP = sk->d_modn; b.base = s_x; b.base_stride = Ln; b.base_limbs = Ln; b.exp = s_lam1; b.exp_limbs = Ln; b.out0 = sk->d_mu;
    b.nbits = sk->nbits; b.w = w; b.mode = DEC_POW; b.Lp = Ln; b.Ln = Ln;
    PZCHK(launch_dec_pow(ctx, 64, 2, b));
    // x mu mod n and n d mod lambda, both to be 1
    MulDesc md[2] = {};
    md[0].a = s_x; md[0].b = sk->d_mu; md[0].modulus = sk->d_n; md[0].r = s_c1;
    md[1].a = sk->d_n; md[1].b = sk->d_d; md[1].modulus = sk->d_lam; md[1].r = s_c2;
    for (auto& m : md) {
        m.status = s_status;
        m.limbs_a = m.limbs_b = m.limbs_mod = m.L = Ln;
    }
    HIPCHK(ctx, hipMemcpyAsync(s_desc, md, sizeof md, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(launch_muls(ctx, s_desc, 2, Ln));
    std::vector<u64> c1(Ln), c2(Ln);
    sk->h_mu.assign(Ln, 0);
    sk->h_ginv.assign(Ln, 0);
    uint8_t flag = 0;
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(c1.data(), s_c1, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(c2.data(), s_c2, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sk->h_mu.data(), sk->d_mu, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sk->h_ginv.data(), sk->d_ginv, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&flag, s_flag, 1, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&st, s_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    PZCHK(status_to_rc(ctx, st));
    if (flag & DEC_F_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (key derivation)");
        return PZ_ERR_HIP;
    }
    if (flag || !is_small(c1.data(), Ln, 1) || !is_small(c2.data(), Ln, 1)) return PZ_ERR_INVALID;
    sk->ginv_one = is_small(sk->h_ginv.data(), Ln, 1);
    return PZ_OK;
}
static size_t sk_crt_words(uint32_t Ln, unsigned C);
static int sk_crt_precheck(uint32_t Ln, const uint64_t* p, const uint64_t* q);
static int sk_create_crt_impl(pz_ctx* ctx, pz_paillier_sk* sk, const uint64_t* g, const uint64_t* p, const uint64_t* q);
// both creators: p and q null is pz_paillier_sk_create; else the CRT part follows the lambda path's handle, which is made by the same code
static int sk_create_common(pz_ctx* ctx, uint32_t limbs_n, const uint64_t* n, const uint64_t* g, const uint64_t* lambda, const uint64_t* d,
                            const uint64_t* p, const uint64_t* q, pz_paillier_sk** out) {
    if (2 * (uint64_t)limbs_n > 128) return PZ_ERR_UNSUPPORTED;
    if (is_small(n, limbs_n, 0)) return PZ_ERR_ZERO_MODULUS;
    // 0 < d < lambda < n: what fixes the powers' schedule at the bit length of n
    if (is_small(lambda, limbs_n, 0) || cmp_limbs(lambda, n, limbs_n) >= 0 || cmp_limbs(d, lambda, limbs_n) >= 0) return PZ_ERR_INVALID;
    if (p) PZCHK(sk_crt_precheck(limbs_n, p, q));
    PZ_ENTER(ctx);
    pz_paillier_sk* sk = new pz_paillier_sk;
    sk->Ln = limbs_n;
    sk->C = capacity(2 * limbs_n);
    sk->nbits = bitlen_limbs(n, limbs_n);
    if (p) sk->crt_words = sk_crt_words(limbs_n, sk->C);
    int rc = sk_create_impl(ctx, sk, n, g, lambda, d);
    if (rc == PZ_OK && p) rc = sk_create_crt_impl(ctx, sk, g, p, q);
    if (rc != PZ_OK) {
        (void)sk_release(ctx, sk);
        return rc;
    }
    *out = sk;
    return PZ_OK;
}
extern "C" int pz_paillier_sk_create(pz_ctx* ctx, uint32_t limbs_n, const uint64_t* n, const uint64_t* g, const uint64_t* lambda,
                                     const uint64_t* d, pz_paillier_sk** out) {
    if (out) *out = nullptr;
    if (!ctx || !n || !g || !lambda || !d || !out || limbs_n == 0) return PZ_ERR_INVALID;
    return sk_create_common(ctx, limbs_n, n, g, lambda, d, nullptr, nullptr, out);
}
extern "C" int pz_paillier_sk_params(const pz_paillier_sk* sk, uint64_t* mu_out, uint64_t* ginv_out) {
    if (!sk || !mu_out || !ginv_out) return PZ_ERR_INVALID;
    memcpy(mu_out, sk->h_mu.data(), (size_t)sk->Ln * 8);
    memcpy(ginv_out, sk->h_ginv.data(), (size_t)sk->Ln * 8);
    return PZ_OK;
}
extern "C" int pz_paillier_sk_free(pz_ctx* ctx, pz_paillier_sk* sk) {
    if (!ctx) return PZ_ERR_INVALID;
    if (!sk) return PZ_OK;
    PZ_ENTER(ctx);
    return sk_release(ctx, sk);
}

// m_i = L(c_i^lambda mod n^2) mu mod n and, if asked for, the randomness r_i = ((c_i mod n) ginv^m_i)^d mod n: one launch per power
// over all ciphertexts (c^lambda; ginv^m unless ginv = 1 -- g is public; the d-th power), all on the context's stream.
static int decrypt_impl(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out, uint64_t* r_out,
                        uint8_t* flags_out, int on_device) {
    if (!ctx || !sk || !cts || !m_out || !flags_out) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_TALLY_MAX) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    const uint32_t Ln = sk->Ln;
    const unsigned L = 2 * Ln;
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8;
    // c mod n | (c mod n) ginv^m | host form: the ciphertexts, m, r, the flags
    const size_t io_bytes = on_device ? 0 : count * (lb + 2 * nb) + ((count + 7) & ~(size_t)7);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, 2 * count * nb + io_bytes + 64, &ws));
    u64 *d_cn = (u64*)ws, *d_v = d_cn + count * Ln;
    const u64* d_cts = cts;
    u64 *d_m = m_out, *d_r = r_out;
    uint8_t* d_flags = flags_out;
    if (!on_device) {
        u64* q = d_v + count * Ln;
        d_cts = q;
        d_m = q + count * L;
        d_r = d_m + count * Ln;
        d_flags = (uint8_t*)(d_r + count * Ln);
        HIPCHK(ctx, hipMemcpyAsync(q, cts, count * lb, hipMemcpyHostToDevice, ctx->stream));
    }
    const unsigned w = dec_window();
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        DecPow a{};
        a.modP = sk->d_mod2; a.modN = sk->d_modn_c; a.base = d_cts; a.base_stride = L; a.base_limbs = L; a.exp = sk->d_lam; a.exp_limbs = Ln;
        a.mu = sk->d_mu; a.out0 = d_m; a.out1 = d_cn; a.flags = d_flags; a.nbits = sk->nbits; a.w = w; a.mode = DEC_LFN; a.Lp = L; a.Ln = Ln;
        PZCHK(launch_dec_pow(ctx, sk->C, count, a));
        if (r_out) {
            DecPow b{};
            b.modP = sk->d_modn; b.base_limbs = Ln; b.exp_limbs = Ln; b.nbits = sk->nbits; b.w = w; b.mode = DEC_POW; b.Lp = Ln; b.Ln = Ln;
            if (!sk->ginv_one) {
                b.base = sk->d_ginv; b.exp = d_m; b.exp_stride = Ln; b.aux = d_cn; b.out0 = d_v; b.flags = d_flags;
                PZCHK(launch_dec_pow(ctx, 64, count, b));
            }
            b.base = sk->ginv_one ? d_cn : d_v; b.base_stride = Ln; b.exp = sk->d_d; b.exp_stride = 0; b.aux = nullptr; b.out0 = d_r; b.flags = d_flags;
            PZCHK(launch_dec_pow(ctx, 64, count, b));
        }
    }
    if (on_device) return PZ_OK;
    HIPCHK(ctx, hipMemcpyAsync(m_out, d_m, count * nb, hipMemcpyDeviceToHost, ctx->stream));
    if (r_out) HIPCHK(ctx, hipMemcpyAsync(r_out, d_r, count * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags_out, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned any = 0;
    for (size_t i = 0; i < count; ++i) any |= flags_out[i];
    if (any & DEC_F_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (decryption)");
        return PZ_ERR_HIP;
    }
    return (any & DEC_F_RANGE) ? PZ_ERR_RANGE : PZ_OK;
}
extern "C" int pz_paillier_decrypt(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out,
                                   uint64_t* r_out, uint8_t* flags_out) {
    return decrypt_impl(ctx, sk, count, cts, m_out, r_out, flags_out, 0);
}
extern "C" int pz_paillier_decrypt_dev(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* d_cts, uint64_t* d_m_out,
                                       uint64_t* d_r_out, uint8_t* d_flags_out) {
    return decrypt_impl(ctx, sk, count, d_cts, d_m_out, d_r_out, d_flags_out, 1);
}

// ------------------------------------------------------------------------------------------------
// CRT decryption (pz_paillier_sk_create_crt, pz_paillier_sk_has_crt, pz_paillier_decrypt_crt[_dev])
// ------------------------------------------------------------------------------------------------
// The same plaintext and randomness from the two primes: per side P in {p, q} the half-length power u_P = (c mod P^2)^(P-1) mod P^2,
// m_P = ((u_P - 1) / P) h_P mod P, then Garner; for r the powers (ginv mod P)^(m mod (P-1)) and the d mod (P-1)-th one, mod P.  Unit
// u = 2 i + side is ciphertext i on side `side` (0: p, 1: q): the two sides of every ciphertext are teams of ONE launch and never wait
// on each other.  p^2 and q^2 fit limbs_n words (the handle's acceptance rule), so the powers run at 64 limbs whatever the key size;
// only the split of c (2 limbs_n words) runs at the capacity of n^2.
// SECRET here: p, q, P - 1, h_P, qinv, d_P, the residues c mod P^2 (c - (c mod p^2) is a multiple of p^2: one of them factors n), m_P,
// e_P, y_P, r_P.  None of them becomes a branch or an address: exponent windows are read at addresses that follow the loop counter and
// choose their table entry under a lane mask (k_dec_pow's schedule), Garner's borrow acts through ld_select.  (What a mul_mod does with
// its VALUES is K3's as everywhere -- the Barrett correction's trip count follows the operands, here under secret moduli too.)  The
// bit lengths of p and q are the key's public shape, as n's is.  Side flags: k_dec_pow's bits, one byte per unit.
// A side's part of the handle's block: Barrett blocks (64 limbs) of P^2 | P | P - 1, then P | P - 1 | h_P | d_P | ginv mod P.
enum { CRT_V_P = 0, CRT_V_PM1 = 1, CRT_V_H = 2, CRT_V_D = 3, CRT_V_GINV = 4, CRT_V_COUNT = 5 };
__host__ __device__ constexpr size_t crt_side_words(unsigned Ln) { return 3 * mod_block_words(64) + (size_t)CRT_V_COUNT * Ln; }
template <class W> __host__ __device__ __forceinline__ W* crt_blk_p2(W* side) { return side; }
template <class W> __host__ __device__ __forceinline__ W* crt_blk_p(W* side) { return side + mod_block_words(64); }
template <class W> __host__ __device__ __forceinline__ W* crt_blk_pm1(W* side) { return side + 2 * mod_block_words(64); }
template <class W> __host__ __device__ __forceinline__ W* crt_vec(W* side, unsigned which, unsigned Ln) {
    return side + 3 * mod_block_words(64) + (size_t)which * Ln;
}

// c mod P^2 for unit u, at the capacity of n^2 (above 2048 bits that is the 128-limb instantiation; the powers stay at 64).  One team
// per unit, k_tally_level's shape (the team product is inlined: no call, no stack).  c >= n^2 is public: the range flag goes to the
// unit's own byte and the residue is zero.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_crt_split(const u64* __restrict__ mod2, const u64* __restrict__ p2_p,
                                                                               const u64* __restrict__ p2_q, const u64* __restrict__ cts,
                                                                               u64* __restrict__ res, uint8_t* __restrict__ sflags, unsigned Ln) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    const unsigned wave = threadIdx.x >> 6;
    const size_t u = blockIdx.x, i = u >> 1;
    const u64* blk = (u & 1) ? p2_q : p2_p;
    if (*block_ok<E>(blk) == 0) return;   // (no handle reaches here with a zero modulus)
    TeamCtx<E> T;
    team_init(T, s_team);
    const LD<E> c = ld_load<E>(cts + i * 2 * Ln, 2 * Ln);
    LD<E> d;
    if (!ld_sub(d, c, ld_load<E>(block_modulus<E>(mod2), C))) {   // the four waves hold the same values: the team leaves together
        if (wave == 0) {
            ld_store(res + u * Ln, ld_zero<E>(), Ln);
            if (lane_id() == 0) sflags[u] = DEC_F_RANGE;
        }
        return;
    }
    BarrettCtx<E> B;
    barrett_from_block(B, blk, 2 * Ln, s_scratch[wave]);
    LD<E> q, r;
    const unsigned st = mul_mod(B, q, r, c, ld_small<E>(1), TeamMul<E>{&T});
    if (wave == 0) {
        ld_store(res + u * Ln, r, Ln);
        if (lane_id() == 0) sflags[u] = st ? DEC_F_INTERNAL : 0;
    }
}

enum { CRT_M = 0, CRT_R = 1 };
struct CrtPow {
    const u64 *side0, *side1;   // the sides' parts of the handle's block
    const u64* in;              // unit u: in + u * Ln.  CRT_M: c mod P^2; CRT_R: c mod P
    const u64* e;               // CRT_R: e_P = m mod (P - 1) per unit; null: ginv = 1 (g is public), the first power is skipped
    u64 *out0, *out1;           // CRT_M: m_P and c mod P; CRT_R: r_P (out1 unused)
    uint8_t* sflags;            // one byte per unit: two teams never write one byte
    u32 bits0, bits1;           // bit lengths of p and q
    u32 mode, w, Ln;
};
// One team per unit.  CRT_M: u_P = in^(P-1) mod P^2 by k_dec_pow's fixed-window schedule (ceil(bitlen(P) / w) windows, the table in
// LDS, every entry read and one kept under a lane mask), then lfn_tail by P's block and h_P, and c mod P.  CRT_R: two powers mod P back
// to back, y_P = in ginvP^e_P (skipped where ginv = 1) and r_P = y_P^d_P.  The powers are ONE loop body run once or twice.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_dec_crt_pow(const CrtPow A) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    extern __shared__ u64 s_table[];   // 2^w entries of Ln limbs
    const unsigned wave = threadIdx.x >> 6, lane = lane_id();
    const size_t u = blockIdx.x;
    const u64* side = (u & 1) ? A.side1 : A.side0;
    const unsigned nbits = (u & 1) ? A.bits1 : A.bits0;
    const unsigned Ln = A.Ln, nent = 1u << A.w;
    if (*block_ok<E>(crt_blk_p2(side)) == 0 || *block_ok<E>(crt_blk_p(side)) == 0) return;   // (no handle reaches here with a zero modulus)
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    const LD<E> in = ld_load<E>(A.in + u * Ln, Ln);
    if (A.mode == CRT_M && A.sflags[u]) {   // c >= n^2 (k_crt_split: public).  The four waves read the same byte: the team leaves together
        if (wave == 0) {
            ld_store(A.out0 + u * Ln, ld_zero<E>(), Ln);
            ld_store(A.out1 + u * Ln, ld_zero<E>(), Ln);
        }
        return;
    }
    unsigned st = ST_OK;
    const LD<E> one = ld_small<E>(1);
    BarrettCtx<E> B;
    barrett_from_block(B, A.mode == CRT_M ? crt_blk_p2(side) : crt_blk_p(side), Ln, s_scratch[wave]);
    LD<E> base = in, acc = in;
    const u64* ex = crt_vec(side, A.mode == CRT_M ? CRT_V_PM1 : CRT_V_D, Ln);
    for (unsigned ph = (A.mode == CRT_R && A.e) ? 0 : 1; ph < 2; ++ph) {
        if (ph == 0) {   // (ginv mod P)^e_P, then times c mod P
            base = ld_load<E>(crt_vec(side, CRT_V_GINV, Ln), Ln);
            ex = A.e + u * Ln;
        }
        __syncthreads();   // (a second power: every wave is done with the first one's table)
        {   // the table: entry k = base^k
            LD<E> cur = one;
            for (unsigned k = 0; k < nent; ++k) {
                if (wave == 0) ld_store(s_table + (size_t)k * Ln, cur, Ln);
                if (k + 1 < nent) {
                    LD<E> q, r;
                    st |= mul_mod(B, q, r, cur, base, tmul);
                    cur = r;
                }
            }
            __syncthreads();
        }
        // window at bit p (a position: public), and the entry it names, read under a mask from all of them
        auto pick = [&](unsigned p) {
            const unsigned wi = p >> 6, sh = p & 63;
            const u64 lo = wi < Ln ? ex[wi] : 0, hi = wi + 1 < Ln ? ex[wi + 1] : 0;
            u64 v = lo >> sh;
            if (sh) v |= hi << (64 - sh);
            u32 idx = (u32)v & (nent - 1);
            asm volatile("" : "+v"(idx));   // a per-lane value from here on: nothing below can become a branch or an address
            LD<E> r = ld_zero<E>();
            for (unsigned k = 0; k < nent; ++k) {
                const u64 keep = 0ull - (u64)(idx == k);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const unsigned t = lane * E + e;
                    const u64 v2 = t < Ln ? s_table[(size_t)k * Ln + t] : 0;
                    r.v[e] |= v2 & keep;
                }
            }
            return r;
        };
        const unsigned nwin = (nbits + A.w - 1) / A.w;
        acc = pick((nwin - 1) * A.w);
        for (unsigned i = nwin - 1; i-- > 0;) {
            LD<E> q, r;
            for (unsigned s = 0; s < A.w; ++s) {
                st |= mul_mod(B, q, r, acc, acc, tmul);
                acc = r;
            }
            st |= mul_mod(B, q, r, acc, pick(i * A.w), tmul);
            acc = r;
        }
        if (ph == 0) {
            LD<E> q, r;
            st |= mul_mod(B, q, r, acc, in, tmul);
            ex = crt_vec(side, CRT_V_D, Ln);
            base = acc = r;   // y_P: it lives in registers only
        }
    }
    if (A.mode == CRT_R) {
        if (wave == 0) {
            ld_store(A.out0 + u * Ln, acc, Ln);
            if (st && lane == 0) A.sflags[u] |= DEC_F_INTERNAL;
        }
        return;
    }
    BarrettCtx<E> N;
    barrett_from_block(N, crt_blk_p(side), Ln, s_scratch[wave]);
    LD<E> m, q, cP;
    const bool bad = lfn_tail(N, T, m, acc, crt_vec(side, CRT_V_H, Ln), Ln, st);
    st |= mul_mod(N, q, cP, in, one, tmul);
    if (wave == 0) {
        ld_store(A.out0 + u * Ln, m, Ln);
        ld_store(A.out1 + u * Ln, cP, Ln);
        if (lane == 0) A.sflags[u] = (uint8_t)((bad ? DEC_F_NOT_UNIT : 0) | (st ? DEC_F_INTERNAL : 0));
    }
}

struct CrtGarner {
    const u64 *side0, *side1, *qinv;
    const u64* a;             // unit u: a + u * Ln, the side results (a_p below p, a_q below q)
    u64* out;                 // ciphertext i: out + i * Ln = a_q + q (((a_p - a_q) mod p) qinv mod p), below n without a reduction
    u64* e;                   // may be null; else unit u: e + u * Ln = out mod (P - 1), the first exponent of the r pass
    const uint8_t* sflags;    // the two side bytes of ciphertext i are merged into flags[i]; a flagged entry's outputs are zero
    uint8_t* flags;
    u32 Ln;
};
// One team per ciphertext.  a_p - (a_q mod p) takes p back or 0 under ld_select's lane mask: its borrow is never a branch.
template <int E> __global__ __launch_bounds__(64 * K3_TEAM) void k_crt_garner(const CrtGarner A) {
    constexpr unsigned C = 64 * E;
    __shared__ u64 s_scratch[K3_TEAM][2 * C];
    __shared__ TeamBuf<E> s_team[2];
    const unsigned wave = threadIdx.x >> 6, lane = lane_id();
    const size_t i = blockIdx.x;
    const unsigned Ln = A.Ln;
    if (*block_ok<E>(crt_blk_p(A.side0)) == 0) return;
    TeamCtx<E> T;
    team_init(T, s_team);
    TeamMul<E> tmul{&T};
    BarrettCtx<E> B;
    barrett_from_block(B, crt_blk_p(A.side0), Ln, s_scratch[wave]);
    const LD<E> one = ld_small<E>(1);
    const LD<E> ap = ld_load<E>(A.a + (2 * i) * Ln, Ln), aq = ld_load<E>(A.a + (2 * i + 1) * Ln, Ln);
    unsigned st = ST_OK;
    LD<E> qq, aqp, d, d2, t, lo, hi, res;
    st |= mul_mod(B, qq, aqp, aq, one, tmul);
    const bool borrow = ld_sub(d, ap, aqp);
    (void)ld_add(d2, d, ld_load<E>(crt_vec(A.side0, CRT_V_P, Ln), Ln), false);   // (d wrapped: the carry-out is that 2^capacity)
    ld_select(d, d2, (u64)borrow);
    st |= mul_mod(B, qq, t, d, ld_load<E>(A.qinv, Ln), tmul);
    tmul(lo, hi, ld_load<E>(crt_vec(A.side1, CRT_V_P, Ln), Ln), t);
    (void)ld_add(res, lo, aq, false);
    const unsigned fs = A.sflags[2 * i] | A.sflags[2 * i + 1];
    if (fs) res = ld_zero<E>();
    if (A.e) {
        LD<E> ep, eq;
        barrett_from_block(B, crt_blk_pm1(A.side0), Ln, s_scratch[wave]);
        st |= mul_mod(B, qq, ep, res, one, tmul);
        barrett_from_block(B, crt_blk_pm1(A.side1), Ln, s_scratch[wave]);
        st |= mul_mod(B, qq, eq, res, one, tmul);
        if (wave == 0) {
            ld_store(A.e + (2 * i) * Ln, ep, Ln);
            ld_store(A.e + (2 * i + 1) * Ln, eq, Ln);
        }
    }
    if (st) res = ld_zero<E>();
    if (wave == 0) {
        ld_store(A.out + i * Ln, res, Ln);
        if (lane == 0) A.flags[i] = (uint8_t)(fs | (st ? DEC_F_INTERNAL : 0));
    }
}

static size_t sk_crt_words(uint32_t Ln, unsigned C) { return 2 * crt_side_words(Ln) + Ln + (C != 64 ? 2 * mod_block_words(C) : 0); }
// p and q odd and at least 3 (else PZ_ERR_INVALID), p^2 and q^2 within Ln words (else PZ_ERR_UNSUPPORTED): P^2 has 2 bitlen(P) or one
// bit fewer, and 64 Ln is even, so the rule is 2 bitlen(P) <= 64 Ln exactly.  It makes every quotient of the reductions fit and asks
// nothing about the primes being of equal length.
static int sk_crt_precheck(uint32_t Ln, const uint64_t* p, const uint64_t* q) {
    for (const uint64_t* v : {p, q})
        if (!(v[0] & 1) || is_small(v, Ln, 1)) return PZ_ERR_INVALID;
    for (const uint64_t* v : {p, q})
        if (2 * (uint64_t)bitlen_limbs(v, Ln) > 64 * (uint64_t)Ln) return PZ_ERR_UNSUPPORTED;
    return PZ_OK;
}
static int launch_crt_pow(pz_ctx* ctx, size_t units, const CrtPow& a) {
    hipLaunchKernelGGL(k_dec_crt_pow<1>, dim3((unsigned)units), dim3(64 * K3_TEAM), ((size_t)8 << a.w) * a.Ln, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
static int launch_crt_garner(pz_ctx* ctx, size_t count, const CrtGarner& a) {
    hipLaunchKernelGGL(k_crt_garner<1>, dim3((unsigned)count), dim3(64 * K3_TEAM), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
// on every path out: a device region that held secrets is overwritten in stream order; `drain` waits for it (host forms: the staged
// host copies behind `h` go through pageable memory and are overwritten once the queue is empty)
struct CrtWipe {
    pz_ctx* c; void* p; size_t n; bool drain; std::vector<u64>* h;
    ~CrtWipe() {
        (void)hipMemsetAsync(p, 0, n, c->stream);
        if (drain) (void)hipStreamSynchronize(c->stream);
        if (h) std::fill(h->begin(), h->end(), 0);
    }
};
// The CRT part of a handle whose lambda path stands (sk_create_impl): everything is derived on the device -- the Barrett blocks by
// k_tally_setup; d_P, ginv mod P, q mod p, g mod P^2 and the check p q = n by k_mul_mod; x_P = L_P(g^(P-1) mod P^2) by k_dec_crt_pow
// with 1 in h_P's place; h_P = x_P^(P-2) mod P and qinv = (q mod p)^(p-2) mod p by k_dec_pow (no inversion routine); and the checks
// x_P h_P = 1 (mod P), q qinv = 1 (mod p), which a composite "prime" fails.  Primality itself is not tested (pz_bigint_is_prime).
static int sk_create_crt_impl(pz_ctx* ctx, pz_paillier_sk* sk, const uint64_t* g, const uint64_t* p, const uint64_t* q) {
    const uint32_t Ln = sk->Ln;
    const unsigned C = sk->C;
    const size_t nb = (size_t)Ln * 8;
    u64* part = sk->d_ginv + Ln;
    sk->d_side[0] = part;
    sk->d_side[1] = part + crt_side_words(Ln);
    sk->d_qinv = part + 2 * crt_side_words(Ln);
    for (int s = 0; s < 2; ++s) sk->d_p2c[s] = C != 64 ? sk->d_qinv + Ln + s * mod_block_words(C) : crt_blk_p2(sk->d_side[s]);
    // host staging: per side P | P - 1 | P - 2, then 1
    std::vector<u64> hs(7 * (size_t)Ln, 0);
    for (int s = 0; s < 2; ++s) {
        const uint64_t* v = s ? q : p;
        sk->pbits[s] = bitlen_limbs(v, Ln);
        for (int k = 0; k < 3; ++k) {
            u64* o = hs.data() + (3 * s + k) * (size_t)Ln;
            memcpy(o, v, nb);
            for (int j = 0; j < k; ++j)
                for (uint32_t i = 0; i < Ln && o[i]-- == 0; ++i) {}
        }
    }
    hs[6 * (size_t)Ln] = 1;
    // device staging (shared workspace, overwritten on every path out):
    // 1 | p - 2 | q - 2 | g | g mod P^2 (2) | x_P (2) | g mod P (2) | q mod p | checks (5) | side flags | status | descs
    enum { S_ONE = 0, S_PM2 = 1, S_G = 3, S_GP2 = 4, S_X = 6, S_GP = 8, S_QMP = 10, S_CHK = 11, S_WORDS = 16 };
    const size_t stage_bytes = S_WORDS * nb + 128 + 11 * sizeof(MulDesc);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, stage_bytes, &ws));
    CrtWipe wipe{ctx, ws, stage_bytes, true, &hs};
    u64* sw = (u64*)ws;
    auto S = [&](int k) { return sw + (size_t)k * Ln; };
    uint8_t* s_flag = (uint8_t*)ws + S_WORDS * nb;
    u32* s_status = (u32*)((char*)ws + S_WORDS * nb + 64);
    MulDesc* s_desc = (MulDesc*)((char*)ws + S_WORDS * nb + 128);
    HIPCHK(ctx, hipMemsetAsync((char*)ws + S_WORDS * nb, 0, 128, ctx->stream));
    const u64* h_one = hs.data() + 6 * (size_t)Ln;
    HIPCHK(ctx, hipMemcpyAsync(S(S_ONE), h_one, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(S(S_G), g, nb, hipMemcpyHostToDevice, ctx->stream));
    for (int s = 0; s < 2; ++s) {
        const u64* hv = hs.data() + 3 * s * (size_t)Ln;
        u64* side = sk->d_side[s];
        HIPCHK(ctx, hipMemcpyAsync(crt_vec(side, CRT_V_P, Ln), hv, nb, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(crt_vec(side, CRT_V_PM1, Ln), hv + Ln, nb, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(S(S_PM2 + s), hv + 2 * (size_t)Ln, nb, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(crt_vec(side, CRT_V_H, Ln), h_one, nb, hipMemcpyHostToDevice, ctx->stream));   // (x_P is L_P under h = 1)
        PZCHK(launch_barrett_setup(ctx, 64, crt_vec(side, CRT_V_P, Ln), Ln, 1, crt_blk_p2(side), s_status));
        PZCHK(launch_barrett_setup(ctx, 64, crt_vec(side, CRT_V_P, Ln), Ln, 0, crt_blk_p(side), s_status));
        PZCHK(launch_barrett_setup(ctx, 64, crt_vec(side, CRT_V_PM1, Ln), Ln, 0, crt_blk_pm1(side), s_status));
        if (C != 64) PZCHK(launch_barrett_setup(ctx, C, crt_vec(side, CRT_V_P, Ln), Ln, 1, sk->d_p2c[s], s_status));
    }
    MulDesc md[11] = {};
    for (int s = 0; s < 2; ++s) {
        u64* side = sk->d_side[s];
        md[s].a = sk->d_d; md[s].b = S(S_ONE); md[s].modulus = crt_vec(side, CRT_V_PM1, Ln); md[s].r = crt_vec(side, CRT_V_D, Ln);
        md[2 + s].a = sk->d_ginv; md[2 + s].b = S(S_ONE); md[2 + s].modulus = crt_vec(side, CRT_V_P, Ln); md[2 + s].r = crt_vec(side, CRT_V_GINV, Ln);
        md[4 + s].a = S(S_G); md[4 + s].b = S(S_ONE); md[4 + s].modulus = crt_vec(side, CRT_V_P, Ln); md[4 + s].square_modulus = 1; md[4 + s].r = S(S_GP2 + s);
        md[8 + s].a = S(S_X + s); md[8 + s].b = crt_vec(side, CRT_V_H, Ln); md[8 + s].modulus = crt_vec(side, CRT_V_P, Ln); md[8 + s].r = S(S_CHK + 2 + s);
    }
    md[6].a = crt_vec(sk->d_side[1], CRT_V_P, Ln); md[6].b = S(S_ONE); md[6].modulus = crt_vec(sk->d_side[0], CRT_V_P, Ln); md[6].r = S(S_QMP);
    md[7].a = crt_vec(sk->d_side[0], CRT_V_P, Ln); md[7].b = crt_vec(sk->d_side[1], CRT_V_P, Ln); md[7].modulus = sk->d_n;
    md[7].q = S(S_CHK); md[7].r = S(S_CHK + 1);
    md[10].a = S(S_QMP); md[10].b = sk->d_qinv; md[10].modulus = crt_vec(sk->d_side[0], CRT_V_P, Ln); md[10].r = S(S_CHK + 4);
    for (auto& m : md) {
        m.status = s_status;
        m.limbs_a = m.limbs_b = m.limbs_mod = m.L = Ln;
    }
    HIPCHK(ctx, hipMemcpyAsync(s_desc, md, sizeof md, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(launch_muls(ctx, s_desc, 8, Ln));
    const unsigned w = dec_window();
    CrtPow a{};
    a.side0 = sk->d_side[0]; a.side1 = sk->d_side[1]; a.in = S(S_GP2); a.out0 = S(S_X); a.out1 = S(S_GP); a.sflags = s_flag;
    a.bits0 = sk->pbits[0]; a.bits1 = sk->pbits[1]; a.mode = CRT_M; a.w = w; a.Ln = Ln;
    PZCHK(launch_crt_pow(ctx, 2, a));
    for (int k = 0; k < 3; ++k) {   // h_p, h_q, qinv
        const int s = k == 1;
        DecPow b{};
        b.modP = crt_blk_p(sk->d_side[s]); b.base = k < 2 ? S(S_X + s) : S(S_QMP); b.base_limbs = Ln; b.exp = S(S_PM2 + s); b.exp_limbs = Ln;
        b.out0 = k < 2 ? crt_vec(sk->d_side[s], CRT_V_H, Ln) : sk->d_qinv; b.nbits = sk->pbits[s]; b.w = w; b.mode = DEC_POW; b.Lp = Ln; b.Ln = Ln;
        PZCHK(launch_dec_pow(ctx, 64, 1, b));
    }
    PZCHK(launch_muls(ctx, s_desc + 8, 3, Ln));
    std::vector<u64> chk(5 * (size_t)Ln);
    uint8_t flag[2] = {0, 0};
    u32 st = 0;
    HIPCHK(ctx, hipMemcpyAsync(chk.data(), S(S_CHK), 5 * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flag, s_flag, 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&st, s_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    auto C_ = [&](int k) { return chk.data() + (size_t)k * Ln; };
    if (!is_small(C_(0), Ln, 1) || !is_small(C_(1), Ln, 0)) return PZ_ERR_INVALID;   // p q != n (what follows ran on a wrong modulus: its status says nothing)
    PZCHK(status_to_rc(ctx, st));
    if ((flag[0] | flag[1]) & DEC_F_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (CRT key derivation)");
        return PZ_ERR_HIP;
    }
    if (flag[0] || flag[1] || !is_small(C_(2), Ln, 1) || !is_small(C_(3), Ln, 1) || !is_small(C_(4), Ln, 1)) return PZ_ERR_INVALID;
    sk->crt = true;
    return PZ_OK;
}
extern "C" int pz_paillier_sk_create_crt(pz_ctx* ctx, uint32_t limbs_n, const uint64_t* n, const uint64_t* g, const uint64_t* lambda,
                                         const uint64_t* d, const uint64_t* p, const uint64_t* q, pz_paillier_sk** out) {
    if (out) *out = nullptr;
    if (!ctx || !n || !g || !lambda || !d || !p || !q || !out || limbs_n == 0) return PZ_ERR_INVALID;
    return sk_create_common(ctx, limbs_n, n, g, lambda, d, p, q, out);
}
extern "C" int pz_paillier_sk_has_crt(const pz_paillier_sk* sk) { return sk && sk->crt ? 1 : 0; }

// split, power, Garner for m; power, Garner more for r.  The workspace holds the residues c mod P^2, the side results, c mod P and
// e_P (2 count x limbs_n words each) and the side flags: all of it is overwritten behind the last kernel -- before the host form
// returns, on every path; in stream order for the device form.
static int decrypt_crt_impl(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out, uint64_t* r_out,
                            uint8_t* flags_out, int on_device) {
    if (!ctx || !sk || !cts || !m_out || !flags_out) return PZ_ERR_INVALID;
    if (!sk->crt) return PZ_ERR_INVALID;
    if (count < 1 || count > K3_TALLY_MAX) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    const uint32_t Ln = sk->Ln;
    const unsigned L = 2 * Ln;
    const size_t nb = (size_t)Ln * 8, lb = (size_t)L * 8, units = 2 * count;
    const size_t secret_bytes = 4 * units * nb + ((units + 7) & ~(size_t)7);
    const size_t io_bytes = on_device ? 0 : count * (lb + 2 * nb) + ((count + 7) & ~(size_t)7);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_BIG_A, secret_bytes + io_bytes + 64, &ws));
    CrtWipe wipe{ctx, ws, secret_bytes + io_bytes, !on_device, nullptr};
    u64 *d_res = (u64*)ws, *d_a = d_res + units * Ln, *d_cp = d_a + units * Ln, *d_e = d_cp + units * Ln;
    uint8_t* d_sf = (uint8_t*)(d_e + units * Ln);
    const u64* d_cts = cts;
    u64 *d_m = m_out, *d_r = r_out;
    uint8_t* d_flags = flags_out;
    if (!on_device) {
        u64* q = (u64*)((char*)ws + secret_bytes);
        d_cts = q;
        d_m = q + count * L;
        d_r = d_m + count * Ln;
        d_flags = (uint8_t*)(d_r + count * Ln);
        HIPCHK(ctx, hipMemcpyAsync(q, cts, count * lb, hipMemcpyHostToDevice, ctx->stream));
    }
    const unsigned w = dec_window();
    {
        pz_timer tm(ctx, PZ_T_TRACE);
        K3_LAUNCH(ctx, k_crt_split, sk->C, dim3((unsigned)units), dim3(64 * K3_TEAM), 0, sk->d_mod2, sk->d_p2c[0], sk->d_p2c[1], d_cts, d_res, d_sf, Ln);
        const bool want_e = r_out && !sk->ginv_one;
        CrtPow a{};
        a.side0 = sk->d_side[0]; a.side1 = sk->d_side[1]; a.in = d_res; a.out0 = d_a; a.out1 = d_cp; a.sflags = d_sf;
        a.bits0 = sk->pbits[0]; a.bits1 = sk->pbits[1]; a.mode = CRT_M; a.w = w; a.Ln = Ln;
        PZCHK(launch_crt_pow(ctx, units, a));
        CrtGarner gm{};
        gm.side0 = sk->d_side[0]; gm.side1 = sk->d_side[1]; gm.qinv = sk->d_qinv; gm.a = d_a; gm.out = d_m; gm.e = want_e ? d_e : nullptr;
        gm.sflags = d_sf; gm.flags = d_flags; gm.Ln = Ln;
        PZCHK(launch_crt_garner(ctx, count, gm));
        if (r_out) {
            a.in = d_cp; a.e = want_e ? d_e : nullptr; a.out0 = d_a; a.out1 = nullptr; a.mode = CRT_R;
            PZCHK(launch_crt_pow(ctx, units, a));
            gm.out = d_r; gm.e = nullptr;
            PZCHK(launch_crt_garner(ctx, count, gm));
        }
    }
    if (on_device) return PZ_OK;
    HIPCHK(ctx, hipMemcpyAsync(m_out, d_m, count * nb, hipMemcpyDeviceToHost, ctx->stream));
    if (r_out) HIPCHK(ctx, hipMemcpyAsync(r_out, d_r, count * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags_out, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned any = 0;
    for (size_t i = 0; i < count; ++i) any |= flags_out[i];
    if (any & DEC_F_INTERNAL) {
        snprintf(ctx->hip_err, sizeof ctx->hip_err, "big-integer kernel: internal consistency check failed (CRT decryption)");
        return PZ_ERR_HIP;
    }
    return (any & DEC_F_RANGE) ? PZ_ERR_RANGE : PZ_OK;
}
extern "C" int pz_paillier_decrypt_crt(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out,
                                       uint64_t* r_out, uint8_t* flags_out) {
    return decrypt_crt_impl(ctx, sk, count, cts, m_out, r_out, flags_out, 0);
}
extern "C" int pz_paillier_decrypt_crt_dev(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* d_cts, uint64_t* d_m_out,
                                           uint64_t* d_r_out, uint8_t* d_flags_out) {
    return decrypt_crt_impl(ctx, sk, count, d_cts, d_m_out, d_r_out, d_flags_out, 1);
}
