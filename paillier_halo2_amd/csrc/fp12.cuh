// fp12.cuh -- the BN254 tower over fp.cuh's Fq, and G2 on the twist, for the pairing kernels (pz_pairing.hip).
//
// halo2curves' tower (it fixes the GT layout of the ABI):
//   Fq2  = Fq[u]  / (u^2 + 1)
//   Fq6  = Fq2[v] / (v^3 - xi),  xi = 9 + u
//   Fq12 = Fq6[w] / (w^2 - v)    so w^6 = xi, and c_i.c_j of an Fq12 carries w^(i + 2j)
// G2 is the D-type twist y^2 = x^3 + 3/xi over Fq2; (x, y) -> (x w^2, y w^3) maps it into E(Fq12).
// Constants (Frobenius coefficients, 3/xi, the exponents) come from gen_fp12.py -> fp12_gen.cuh.
//
// Values are fp.cuh's lazy representatives in [0, 2p); every routine here takes and returns such values.  Everything is
// passed and returned by value in named fields (no runtime-indexed arrays: those would live in scratch).
#pragma once
#include "fp.cuh"
#include "fp12_gen.cuh"

struct Fq2 {
    Fq c0, c1;
};
struct Fq6 {
    Fq2 c0, c1, c2;
};
struct Fq12 {
    Fq6 c0, c1;
};

// ------------------------------------------------------------------------------------------------ Fq2
__device__ __forceinline__ Fq fq_const(const u32* t) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = t[i];
    return r;
}
__device__ __forceinline__ Fq2 f2_const(const u32* t) { return Fq2{fq_const(t), fq_const(t + 8)}; }
__device__ __forceinline__ Fq2 f2_zero() { return Fq2{fp_zero<FqTag>(), fp_zero<FqTag>()}; }
__device__ __forceinline__ Fq2 f2_one() { return Fq2{fp_one<FqTag>(), fp_zero<FqTag>()}; }
__device__ __forceinline__ Fq2 f2_add(const Fq2& a, const Fq2& b) { return Fq2{fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
__device__ __forceinline__ Fq2 f2_sub(const Fq2& a, const Fq2& b) { return Fq2{fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)}; }
__device__ __forceinline__ Fq2 f2_dbl(const Fq2& a) { return f2_add(a, a); }
__device__ __forceinline__ Fq2 f2_neg(const Fq2& a) { return Fq2{fp_neg(a.c0), fp_neg(a.c1)}; }
__device__ __forceinline__ Fq2 f2_conj(const Fq2& a) { return Fq2{a.c0, fp_neg(a.c1)}; }
__device__ __forceinline__ Fq2 f2_mul_fq(const Fq2& a, const Fq& s) { return Fq2{fp_mul(a.c0, s), fp_mul(a.c1, s)}; }
__device__ __forceinline__ bool f2_is_zero(const Fq2& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
__device__ __forceinline__ bool f2_is_zero_exact(const Fq2& a) { return fp_is_zero_exact(a.c0) && fp_is_zero_exact(a.c1); }
__device__ __forceinline__ bool f2_eq(const Fq2& a, const Fq2& b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }

// Karatsuba: 3 multiplications
__device__ __forceinline__ Fq2 f2_mul(const Fq2& a, const Fq2& b) {
    const Fq t0 = fp_mul(a.c0, b.c0), t1 = fp_mul(a.c1, b.c1);
    const Fq s = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
    return Fq2{fp_sub(t0, t1), fp_sub(fp_sub(s, t0), t1)};
}
// (a0 + a1)(a0 - a1) + 2 a0 a1 u: 2 multiplications
__device__ __forceinline__ Fq2 f2_sqr(const Fq2& a) {
    const Fq t = fp_mul(a.c0, a.c1);
    return Fq2{fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1)), fp_dbl(t)};
}
// a (9 + u) = (9 a0 - a1) + (a0 + 9 a1) u
__device__ __forceinline__ Fq2 f2_mul_xi(const Fq2& a) {
    const Fq2 a8 = f2_dbl(f2_dbl(f2_dbl(a)));
    const Fq2 a9 = f2_add(a8, a);
    return Fq2{fp_sub(a9.c0, a.c1), fp_add(a.c0, a9.c1)};
}
__device__ __forceinline__ Fq2 f2_inv(const Fq2& a) {
    const Fq d = fp_inv(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
    return Fq2{fp_mul(a.c0, d), fp_neg(fp_mul(a.c1, d))};
}

// ------------------------------------------------------------------------------------------------ Fq6
__device__ __forceinline__ Fq6 f6_zero() { return Fq6{f2_zero(), f2_zero(), f2_zero()}; }
__device__ __forceinline__ Fq6 f6_one() { return Fq6{f2_one(), f2_zero(), f2_zero()}; }
__device__ __forceinline__ Fq6 f6_add(const Fq6& a, const Fq6& b) { return Fq6{f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
__device__ __forceinline__ Fq6 f6_sub(const Fq6& a, const Fq6& b) { return Fq6{f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
__device__ __forceinline__ Fq6 f6_neg(const Fq6& a) { return Fq6{f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
// a v = xi a2 + a0 v + a1 v^2
__device__ __forceinline__ Fq6 f6_mul_v(const Fq6& a) { return Fq6{f2_mul_xi(a.c2), a.c0, a.c1}; }

// Karatsuba over Fq2: 6 Fq2 multiplications
__device__ __forceinline__ Fq6 f6_mul(const Fq6& a, const Fq6& b) {
    const Fq2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    const Fq2 s12 = f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), t1), t2);
    const Fq2 s01 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), t0), t1);
    const Fq2 s02 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), t0), t2);
    return Fq6{f2_add(f2_mul_xi(s12), t0), f2_add(s01, f2_mul_xi(t2)), f2_add(s02, t1)};
}
// Chung-Hasan SQR2: 2 Fq2 squarings + 3 Fq2 multiplications
__device__ __forceinline__ Fq6 f6_sqr(const Fq6& a) {
    const Fq2 s0 = f2_sqr(a.c0);
    const Fq2 s1 = f2_dbl(f2_mul(a.c0, a.c1));
    const Fq2 s2 = f2_sqr(f2_add(f2_sub(a.c0, a.c1), a.c2));
    const Fq2 s3 = f2_dbl(f2_mul(a.c1, a.c2));
    const Fq2 s4 = f2_sqr(a.c2);
    return Fq6{f2_add(s0, f2_mul_xi(s3)), f2_add(s1, f2_mul_xi(s4)), f2_sub(f2_sub(f2_add(f2_add(s1, s2), s3), s0), s4)};
}
__device__ __forceinline__ Fq6 f6_inv(const Fq6& a) {
    const Fq2 t0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2 t1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    const Fq2 t2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    const Fq2 den = f2_add(f2_mul(a.c0, t0), f2_mul_xi(f2_add(f2_mul(a.c2, t1), f2_mul(a.c1, t2))));
    const Fq2 di = f2_inv(den);
    return Fq6{f2_mul(t0, di), f2_mul(t1, di), f2_mul(t2, di)};
}

// ------------------------------------------------------------------------------------------------ Fq12
__device__ __forceinline__ Fq12 f12_one() { return Fq12{f6_one(), f6_zero()}; }
__device__ __forceinline__ Fq12 f12_conj(const Fq12& a) { return Fq12{a.c0, f6_neg(a.c1)}; }
// Karatsuba over Fq6: 3 Fq6 multiplications
__device__ __forceinline__ Fq12 f12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    const Fq6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1));
    return Fq12{f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(s, t0), t1)};
}
// complex squaring: (a0 + a1)(a0 + v a1) - t - v t, 2t with t = a0 a1: 2 Fq6 multiplications
__device__ __forceinline__ Fq12 f12_sqr(const Fq12& a) {
    const Fq6 t = f6_mul(a.c0, a.c1);
    const Fq6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return Fq12{f6_sub(f6_sub(s, t), f6_mul_v(t)), f6_add(t, t)};
}
// f * (l0 + l1 w + l3 w^3): the sparse line of a Miller step (l0 at c0.c0, l1 at c1.c0, l3 at c1.c1)
__device__ __forceinline__ Fq12 f12_mul_line(const Fq12& a, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
    // b0 = (l0, 0, 0), b1 = (l1, l3, 0)
    const Fq6 t0 = Fq6{f2_mul(a.c0.c0, l0), f2_mul(a.c0.c1, l0), f2_mul(a.c0.c2, l0)};
    // a1 * (l1 + l3 v): c0 = a0 l1 + xi a2 l3, c1 = a1 l1 + a0 l3, c2 = a2 l1 + a1 l3
    const Fq6 t1 = Fq6{f2_add(f2_mul(a.c1.c0, l1), f2_mul_xi(f2_mul(a.c1.c2, l3))), f2_add(f2_mul(a.c1.c1, l1), f2_mul(a.c1.c0, l3)),
                       f2_add(f2_mul(a.c1.c2, l1), f2_mul(a.c1.c1, l3))};
    // (a0 + a1)(l0 + l1 + l3 v)
    const Fq6 s = f6_add(a.c0, a.c1);
    const Fq2 m0 = f2_add(l0, l1);
    const Fq6 u = Fq6{f2_add(f2_mul(s.c0, m0), f2_mul_xi(f2_mul(s.c2, l3))), f2_add(f2_mul(s.c1, m0), f2_mul(s.c0, l3)),
                      f2_add(f2_mul(s.c2, m0), f2_mul(s.c1, l3))};
    return Fq12{f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(u, t0), t1)};
}
__device__ __forceinline__ Fq12 f12_inv(const Fq12& a) {
    const Fq6 d = f6_inv(f6_sub(f6_sqr(a.c0), f6_mul_v(f6_sqr(a.c1))));
    return Fq12{f6_mul(a.c0, d), f6_neg(f6_mul(a.c1, d))};
}
__device__ __forceinline__ bool f12_is_one(const Fq12& a) {
    const Fq2 one = f2_one();
    return f2_eq(a.c0.c0, one) && f2_is_zero(a.c0.c1) && f2_is_zero(a.c0.c2) && f2_is_zero(a.c1.c0) && f2_is_zero(a.c1.c1) &&
           f2_is_zero(a.c1.c2);
}

// FROB_k_e = xi^(e (p^k - 1)/6) (fp12_gen.cuh)
__device__ __forceinline__ Fq2 frob_const(int k, int e) { return f2_const(PZ_FROB + ((k - 1) * 5 + (e - 1)) * 16); }
// a^(p^k), k = 1, 2, 3: the coefficient of w^e becomes frob_k(c) FROB_k_e (frob_k = conjugation for odd k)
template <int K> __device__ __forceinline__ Fq2 f2_frob(const Fq2& a) { return (K & 1) ? f2_conj(a) : a; }
template <int K> __device__ __forceinline__ Fq12 f12_frob(const Fq12& a) {
    Fq12 r;
    r.c0.c0 = f2_frob<K>(a.c0.c0);
    r.c0.c1 = f2_mul(f2_frob<K>(a.c0.c1), frob_const(K, 2));
    r.c0.c2 = f2_mul(f2_frob<K>(a.c0.c2), frob_const(K, 4));
    r.c1.c0 = f2_mul(f2_frob<K>(a.c1.c0), frob_const(K, 1));
    r.c1.c1 = f2_mul(f2_frob<K>(a.c1.c1), frob_const(K, 3));
    r.c1.c2 = f2_mul(f2_frob<K>(a.c1.c2), frob_const(K, 5));
    return r;
}

// ------------------------------------------------------------------------------------------------ G2 (twist), Jacobian
struct G2Aff {
    Fq2 x, y;
};
struct G2Jac {
    Fq2 x, y, z;   // (X / Z^2, Y / Z^3); z == 0 is the identity
};
// ABI form: 16 u64 words x.c0, x.c1, y.c0, y.c1 (canonical Montgomery), identity = all zero
__device__ __forceinline__ G2Aff g2_load(const uint64_t* p) {
    return G2Aff{Fq2{fp_load<FqTag>(p), fp_load<FqTag>(p + 4)}, Fq2{fp_load<FqTag>(p + 8), fp_load<FqTag>(p + 12)}};
}
__device__ __forceinline__ void g2_store(uint64_t* p, const G2Aff& a) {
    fp_store(p, a.x.c0);
    fp_store(p + 4, a.x.c1);
    fp_store(p + 8, a.y.c0);
    fp_store(p + 12, a.y.c1);
}
__device__ __forceinline__ bool g2_is_inf(const G2Aff& a) { return f2_is_zero_exact(a.x) && f2_is_zero_exact(a.y); }
__device__ __forceinline__ bool fq_is_canonical(const Fq& a) {
    Fq r = a;
    fp_reduce_once(r);
    u32 d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= r.v[i] ^ a.v[i];
    return d == 0;
}
// canonical coordinates on y^2 = x^3 + 3/xi; the identity passes
__device__ __forceinline__ bool g2_on_curve(const G2Aff& a) {
    if (g2_is_inf(a)) return true;
    if (!fq_is_canonical(a.x.c0) || !fq_is_canonical(a.x.c1) || !fq_is_canonical(a.y.c0) || !fq_is_canonical(a.y.c1)) return false;
    const Fq2 rhs = f2_add(f2_mul(f2_sqr(a.x), a.x), f2_const(PZ_TWIST_B));
    return f2_is_zero(f2_sub(f2_sqr(a.y), rhs));
}
// G1 in the ABI's affine form (8 words, (0, 0) = identity): canonical coordinates on y^2 = x^3 + 3
struct G1Pt {
    Fq x, y;
};
__device__ __forceinline__ G1Pt g1_load(const uint64_t* p) { return G1Pt{fp_load<FqTag>(p), fp_load<FqTag>(p + 4)}; }
__device__ __forceinline__ bool g1_is_inf(const G1Pt& a) { return fp_is_zero_exact(a.x) && fp_is_zero_exact(a.y); }
__device__ __forceinline__ bool g1_on_curve(const G1Pt& a) {
    if (g1_is_inf(a)) return true;
    if (!fq_is_canonical(a.x) || !fq_is_canonical(a.y)) return false;
    const Fq one = fp_one<FqTag>();
    const Fq rhs = fp_add(fp_mul(fp_sqr(a.x), a.x), fp_add(fp_dbl(one), one));
    return fp_is_zero(fp_sub(fp_sqr(a.y), rhs));
}

// dbl-2009-l (a = 0)
__device__ __forceinline__ G2Jac g2_dbl(const G2Jac& p) {
    const Fq2 a = f2_sqr(p.x), b = f2_sqr(p.y), c = f2_sqr(b);
    const Fq2 d = f2_dbl(f2_sub(f2_sub(f2_sqr(f2_add(p.x, b)), a), c));
    const Fq2 e = f2_add(f2_dbl(a), a), f = f2_sqr(e);
    const Fq2 x3 = f2_sub(f, f2_dbl(d));
    const Fq2 c8 = f2_dbl(f2_dbl(f2_dbl(c)));
    return G2Jac{x3, f2_sub(f2_mul(e, f2_sub(d, x3)), c8), f2_dbl(f2_mul(p.y, p.z))};
}
// p + q with q affine (not the identity); p may be the identity, equal to q or to -q
__device__ __forceinline__ G2Jac g2_add_mixed(const G2Jac& p, const G2Aff& q) {
    if (f2_is_zero(p.z)) return G2Jac{q.x, q.y, f2_one()};
    // madd-2007-bl
    const Fq2 z1z1 = f2_sqr(p.z);
    const Fq2 u2 = f2_mul(q.x, z1z1), s2 = f2_mul(f2_mul(q.y, p.z), z1z1);
    const Fq2 h = f2_sub(u2, p.x), r = f2_dbl(f2_sub(s2, p.y));
    if (f2_is_zero(h)) {
        if (f2_is_zero(r)) return g2_dbl(p);
        return G2Jac{f2_one(), f2_one(), f2_zero()};
    }
    const Fq2 hh = f2_sqr(h), i = f2_dbl(f2_dbl(hh)), j = f2_mul(h, i), v = f2_mul(p.x, i);
    const Fq2 x3 = f2_sub(f2_sub(f2_sqr(r), j), f2_dbl(v));
    const Fq2 y3 = f2_sub(f2_mul(r, f2_sub(v, x3)), f2_dbl(f2_mul(p.y, j)));
    const Fq2 z3 = f2_sub(f2_sub(f2_sqr(f2_add(p.z, h)), z1z1), hh);
    return G2Jac{x3, y3, z3};
}
__device__ __forceinline__ G2Aff g2_to_affine(const G2Jac& p) {
    if (f2_is_zero(p.z)) return G2Aff{f2_zero(), f2_zero()};
    const Fq2 zi = f2_inv(p.z), zi2 = f2_sqr(zi);
    return G2Aff{f2_mul(p.x, zi2), f2_mul(p.y, f2_mul(zi2, zi))};
}
