// prime_mont.cuh -- the arithmetic of the prime generation: an integer held by a GROUP of 16 lanes, its carry
// look-ahead over the group's bits of a ballot, and the lane-systolic Montgomery product on three-word columns.  pz_prime.hip builds
// k_prime_mr from it; probe/pz_probe.hip exposes the same functions one at a time (pzp_prime_ops) so that the tests can hold them to
// integers.  Nothing here reads or writes memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t u32;
typedef uint64_t u64;

#define PR_GROUP 16        // lanes per candidate

// ---- a group's integer: lane j of the group holds limbs [j E, j E + E) -----------------------------------------------------------------
template <int E> struct GI {
    u64 v[E];
};
struct GLane {
    unsigned gl;       // lane within the group, 0 .. 15
    unsigned gshift;   // bit of the group's lane 0 in a ballot: 0, 16, 32, 48
};
__device__ __forceinline__ GLane glane() {
    GLane g;
    g.gl = threadIdx.x & 15u;
    g.gshift = threadIdx.x & 48u;
    return g;
}
// the group's 16 bits of a wave-wide ballot
__device__ __forceinline__ u32 grp_ballot(bool p, const GLane& g) { return (u32)(__ballot(p) >> g.gshift) & 0xFFFFu; }
// one-lane shifts inside a row of 16 as DPP moves (row_shl:1 / row_shr:1, bound_ctrl: the lane without a source reads 0)
__device__ __forceinline__ u32 row_down1_32(u32 x) { return __builtin_amdgcn_update_dpp(0u, x, 0x101, 0xf, 0xf, true); }
__device__ __forceinline__ u32 row_up1_32(u32 x) { return __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, true); }
__device__ __forceinline__ u64 row_down1(u64 x) {  // lane j <- lane j + 1 of the group, lane 15 <- 0
    return ((u64)row_down1_32((u32)(x >> 32)) << 32) | row_down1_32((u32)x);
}
__device__ __forceinline__ u64 row_up1(u64 x) {  // lane j <- lane j - 1 of the group, lane 0 <- 0
    return ((u64)row_up1_32((u32)(x >> 32)) << 32) | row_up1_32((u32)x);
}
// limb k of a group's integer in every lane of the group (k is uniform: a loop index)
template <int E> __device__ __forceinline__ u64 grp_limb(const GI<E>& a, unsigned k) {
    u64 x = a.v[0];
#pragma unroll
    for (int e = 1; e < E; ++e) x = (k % E) == (unsigned)e ? a.v[e] : x;
    return __shfl(x, (int)(k / E), PR_GROUP);
}
template <int E> __device__ __forceinline__ GI<E> grp_small(u64 x, const GLane& g) {
    GI<E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) r.v[e] = 0;
    r.v[0] = g.gl == 0 ? x : 0;
    return r;
}
template <int E> __device__ __forceinline__ GI<E> grp_select(bool take_b, const GI<E>& a, const GI<E>& b) {   // by lane mask, as ld_select
    const u64 m = take_b ? ~0ull : 0ull;
    GI<E> r;
#pragma unroll
    for (int e = 0; e < E; ++e) r.v[e] = (a.v[e] & ~m) | (b.v[e] & m);
    return r;
}
template <int E> __device__ __forceinline__ bool grp_eq(const GI<E>& a, const GI<E>& b, const GLane& g) {
    u64 d = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) d |= a.v[e] ^ b.v[e];
    return grp_ballot(d == 0, g) == 0xFFFFu;
}
// the carries (or borrows) into the lanes of a group from per-lane generate / propagate predicates (never both set in one lane): the
// carries of the 17-bit addition (G << 1) + P are exactly the inter-lane ones.  *out: the carry out of lane 15
__device__ __forceinline__ u64 grp_carry_in(bool gen, bool prop, const GLane& g, bool* out) {
    const u32 G = grp_ballot(gen, g), P = grp_ballot(prop, g);
    const u32 s = (G << 1) + P;
    *out = ((s >> 16) & 1u) != 0;
    return ((s ^ P) >> g.gl) & 1u;
}
// d = a - b; returns the borrow out (a < b)
template <int E> __device__ __forceinline__ bool grp_sub(GI<E>& d, const GI<E>& a, const GI<E>& b, const GLane& g) {
    u64 bw = 0, nz = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 t = a.v[e] - b.v[e];
        const u64 b1 = a.v[e] < b.v[e];
        const u64 t2 = t - bw;
        const u64 b2 = t < bw;
        d.v[e] = t2;
        bw = b1 | b2;
        nz |= t2;
    }
    bool out;
    u64 bi = grp_carry_in(bw != 0, nz == 0, g, &out);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 t = d.v[e] - bi;
        bi = d.v[e] < bi;
        d.v[e] = t;
    }
    return out;
}
// x (below 2 c, `top` its bit 64 * 16 E) reduced below c
template <int E> __device__ __forceinline__ GI<E> grp_reduce_once(const GI<E>& x, bool top, const GI<E>& c, const GLane& g) {
    GI<E> d;
    const bool borrow = grp_sub(d, x, c, g);
    return grp_select(top || !borrow, x, d);
}
// 2 x mod c for x < c
template <int E> __device__ __forceinline__ GI<E> grp_double_mod(const GI<E>& x, const GI<E>& c, const GLane& g) {
    const u64 from_below = row_up1(x.v[E - 1] >> 63);
    const bool top = (grp_ballot((x.v[E - 1] >> 63) != 0, g) >> 15) != 0;
    GI<E> y;
#pragma unroll
    for (int e = E - 1; e > 0; --e) y.v[e] = (x.v[e] << 1) | (x.v[e - 1] >> 63);
    y.v[0] = (x.v[0] << 1) | from_below;
    return grp_reduce_once(y, top, c, g);
}

// 64 x 64 -> 128 from four v_mad_u64_u32, as mul64 of pz_bigint.hip does
__device__ __forceinline__ void mul64(u64 x, u64 y, u64& lo, u64& hi) {
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32), y0 = (u32)y, y1 = (u32)(y >> 32);
    const u64 p00 = (u64)x0 * y0;
    const u64 p01 = (u64)x0 * y1 + (p00 >> 32);
    const u64 p10 = (u64)x1 * y0 + (u32)p01;
    hi = (u64)x1 * y1 + (p01 >> 32) + (p10 >> 32);
    lo = (p10 << 32) | (u32)p00;
}
// (lo, hi, ex) += x y: a limb's column as three words, ex a small count
__device__ __forceinline__ void col_mad(u64& lo, u64& hi, u32& ex, u64 x, u64 y) {
    u64 pl, ph;
    mul64(x, y, pl, ph);
    lo += pl;
    const u64 c1 = lo < pl;
    hi += ph;
    const u32 c2 = hi < ph;
    hi += c1;
    const u32 c3 = hi < c1;
    ex += c2 + c3;
}
// Montgomery product a b / R mod c, R = 2^(64 L), for a < c and any b < R; the result is below c.  CIOS over the limbs of b: per step
// every lane adds a_k b_i and c_k m to its columns, limb 0 becomes zero and the columns move one limb down.  The running value stays
// below a + c < 2 c, so after the last step one bit above the group's width is all that can remain.
template <int E> __device__ __forceinline__ GI<E> mont_mul(const GI<E>& a, const GI<E>& b, const GI<E>& c, u64 ninv, unsigned L, const GLane& g) {
    u64 lo[E], hi[E];
    u32 ex[E];
#pragma unroll
    for (int e = 0; e < E; ++e) lo[e] = 0, hi[e] = 0, ex[e] = 0;
    for (unsigned i = 0; i < L; ++i) {
        const u64 bi = grp_limb(b, i);
#pragma unroll
        for (int e = 0; e < E; ++e) col_mad(lo[e], hi[e], ex[e], a.v[e], bi);
        const u64 m = __shfl(lo[0], 0, PR_GROUP) * ninv;
#pragma unroll
        for (int e = 0; e < E; ++e) col_mad(lo[e], hi[e], ex[e], c.v[e], m);
        // one limb down: limb k's (hi, ex) now weigh what limb k + 1's lo weighs, and limb 0's lo is zero
        const u64 next = row_down1(lo[0]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const u64 src = e + 1 < E ? lo[e + 1] : next;
            const u64 t = hi[e] + src;
            hi[e] = (u64)ex[e] + (t < src);
            lo[e] = t;
            ex[e] = 0;
        }
    }
    // resolve: limb k takes limb k - 1's hi (a count of at most 2); the top limb's hi and the carry out are the bit above the width
    const u64 from_below = row_up1(hi[E - 1]);
    const u64 top_hi = __shfl(hi[E - 1], PR_GROUP - 1, PR_GROUP);
    GI<E> r;
    u64 cy = 0;
    bool ones = true;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 inc = e == 0 ? from_below : hi[e - 1];
        const u64 t = lo[e] + inc;
        const u64 c1 = t < inc;
        const u64 t2 = t + cy;
        const u64 c2 = t2 < cy;
        r.v[e] = t2;
        cy = c1 | c2;
        ones = ones && t2 == ~0ull;
    }
    bool out;
    u64 ci = grp_carry_in(cy != 0, ones && cy == 0, g, &out);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 t = r.v[e] + ci;
        ci = t < ci;
        r.v[e] = t;
    }
    return grp_reduce_once(r, out || top_hi != 0, c, g);
}

// a candidate's constants without a division (c odd and at least 3, m0 its limb 0): ninv = -c^-1 mod 2^64, one = R mod c, r2 = R^2 mod c
template <int E> __device__ __forceinline__ void prime_setup(const GI<E>& c, u64 m0, unsigned L, const GLane& g, u64& ninv, GI<E>& one, GI<E>& r2) {
    // -c^-1 mod 2^64: x <- x (2 - c0 x) doubles the correct low bits, and x = c0 is right to 3 bits
    u64 x = m0;
#pragma unroll
    for (int it = 0; it < 5; ++it) x *= 2 - m0 * x;
    ninv = 0 - x;
    // R mod c and R^2 mod c: 64 L doublings of 1 each
    one = grp_small<E>(1, g);
    for (unsigned i = 0; i < 64 * L; ++i) one = grp_double_mod(one, c, g);
    r2 = one;
    for (unsigned i = 0; i < 64 * L; ++i) r2 = grp_double_mod(r2, c, g);
}
