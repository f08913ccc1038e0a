// pz_params.hip -- the G2 side of a ParamsKZG file on the device: the 64-byte compressed form of a twist point,
// its decompression (a square root in Fq2) and the twist / subgroup check.  The params object itself is host composition: pz_params.cpp.
//
// G2 point, 64 bytes (halo2curves' G2Compressed [D], the convention of the G1 format of section 15.2): the canonical x.c0 little-endian in
// bytes 0..31, the canonical x.c1 in bytes 32..63, bit 7 of byte 63 = the parity of the canonical y.c0, bit 6 of byte 63 zero (c1 < p < 2^254),
// the identity 64 zero bytes.
//
// One lane per point, workgroups of 64, plain C++ on fp12.cuh's Fq2 / G2Aff / G2Jac: a params file has TWO such points, so nothing here is
// tuned.  The Fq roots are the fixed (p + 1)/4 power (p = 3 mod 4), every candidate accepted only by squaring it; the Fq2 root is the
// complex method over u^2 = -1.  The subgroup check is the double-and-add ladder over the constant r with g2_dbl / g2_add_mixed, whose
// P = +-Q and identity cases it relies on: the last addition of a subgroup point is the cancelling one, a point of small order meets them
// midway.
#include "fp12.cuh"
#include "pz_internal.h"

namespace {

constexpr unsigned GT = 64;

// bit i of a 256-bit constant held in registers (no runtime-indexed array: that would live in scratch)
__device__ __forceinline__ u32 bit_of(const u32 e[8], int i) {
    u32 w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k == (i >> 5)) w = e[k];
    return (w >> (i & 31)) & 1;
}

// a^((p + 1)/4): the square root of a if it has one (p = 3 mod 4); the caller squares it to find out
__device__ __noinline__ Fq fq_sqrt_candidate(const Fq& a) {
    u32 e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // (p + 1) >> 2: p + 1 does not carry out of limb 0 (p[0] = ...47)
        const u32 lo = FieldParams<FqTag>::P(i) + (i == 0 ? 1u : 0u);
        const u32 hi = i < 7 ? FieldParams<FqTag>::P(i + 1) : 0u;
        e[i] = (lo >> 2) | (hi << 30);
    }
    Fq acc = fp_one<FqTag>();
    for (int i = 251; i >= 0; --i) {
        acc = fp_sqr(acc);
        if (bit_of(e, i)) acc = fp_mul(acc, a);
    }
    return acc;
}
__device__ __forceinline__ bool fq_sqrt(const Fq& a, Fq& root) {
    root = fq_sqrt_candidate(a);
    return fp_eq(fp_sqr(root), a);
}

// a square root of a in Fq2 = Fq[u]/(u^2 + 1), false if there is none.  a1 = 0: (sqrt(a0), 0) or (0, sqrt(-a0)) (-1 is not a square).
// Otherwise with N = a0^2 + a1^2 = s^2: t = (a0 +- s)/2 = x0^2, x1 = a1 / (2 x0).
__device__ bool f2_sqrt(const Fq2& a, Fq2& root) {
    Fq c;
    if (fp_is_zero(a.c1)) {
        if (fq_sqrt(a.c0, c)) {
            root = Fq2{c, fp_zero<FqTag>()};
            return true;
        }
        if (fq_sqrt(fp_neg(fp_canon(a.c0)), c)) {
            root = Fq2{fp_zero<FqTag>(), c};
            return true;
        }
        return false;
    }
    Fq s;
    if (!fq_sqrt(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)), s)) return false;
    const Fq half = fq_const(PZ_TWO_INV);
    Fq t = fp_mul(fp_add(a.c0, s), half);
    if (!fq_sqrt(t, c)) {
        t = fp_mul(fp_sub(a.c0, s), half);
        if (!fq_sqrt(t, c)) return false;
    }
    root = Fq2{c, fp_mul(a.c1, fp_inv(fp_dbl(c)))};
    return true;
}

__device__ __forceinline__ void load32w(const uint8_t* p, u32 w[8]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 lo = q[0], hi = q[1];
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
    w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void store32w(uint8_t* p, const u32 w[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// the integer w (below 2^256) as a field element, false if it is not below p
__device__ __forceinline__ bool fq_from_canonical(const u32 w[8], Fq& out) {
    Fq a;
    u32 t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a.v[k] = w[k];
    if (fp_sub_p(t, a) == 0) return false;   // a - p does not borrow
    out = fp_to_mont(a);
    return true;
}
__device__ __forceinline__ u32 fq_parity(const Fq& a) { return fp_canon(fp_from_mont(a)).v[0] & 1u; }

// status: 0 ok, 1 not canonical (c0 >= p or c1 >= p; bit 6 of byte 63 set is such a c1), 2 no point of the twist has this x.  A refused
// point is stored as the identity.  y.c0 = 0: see include/pz.h.
__global__ __launch_bounds__(64) void k_g2_decompress(const uint8_t* __restrict__ bytes, size_t n, uint64_t* __restrict__ points,
                                                      int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * GT + threadIdx.x;
    if (i >= n) return;
    u32 w0[8], w1[8];
    load32w(bytes + 64 * i, w0);
    load32w(bytes + 64 * i + 32, w1);
    const u32 sign = w1[7] >> 31;
    w1[7] &= 0x7fffffffu;
    u32 nz = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) nz |= w0[k] | w1[k];
    G2Aff out{f2_zero(), f2_zero()};
    int st = 0;
    Fq2 x;
    if (!fq_from_canonical(w0, x.c0) || !fq_from_canonical(w1, x.c1)) {
        st = 1;
    } else if (nz | sign) {   // 64 zero bytes are the identity
        const Fq2 rhs = f2_add(f2_mul(f2_sqr(x), x), f2_const(PZ_TWIST_B));
        Fq2 y;
        if (!f2_sqrt(rhs, y) || !f2_eq(f2_sqr(y), rhs)) {
            st = 2;
        } else {
            const Fq y0 = fp_canon(y.c0);
            const bool flip = fp_is_zero_exact(y0) ? fq_parity(y.c1) != 0 : fq_parity(y0) != sign;
            out = G2Aff{x, flip ? f2_neg(Fq2{y0, fp_canon(y.c1)}) : y};
        }
    }
    g2_store(points + 16 * i, out);
    status[i] = st;
}

__global__ __launch_bounds__(64) void k_g2_compress(const uint64_t* __restrict__ points, size_t n, uint8_t* __restrict__ bytes) {
    const size_t i = (size_t)blockIdx.x * GT + threadIdx.x;
    if (i >= n) return;
    const G2Aff q = g2_load(points + 16 * i);
    Fq c0 = fp_zero<FqTag>(), c1 = fp_zero<FqTag>();
    if (!g2_is_inf(q)) {
        c0 = fp_canon(fp_from_mont(q.x.c0));
        c1 = fp_canon(fp_from_mont(q.x.c1));
        c1.v[7] |= fq_parity(q.y.c0) << 31;
    }
    store32w(bytes + 64 * i, c0.v);
    store32w(bytes + 64 * i + 32, c1.v);
}

// status: 0 in the order-r subgroup (the identity included), 1 not canonical, 2 off the twist, 3 on the twist but [r]Q != O
__global__ __launch_bounds__(64) void k_g2_check(const uint64_t* __restrict__ points, size_t n, int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * GT + threadIdx.x;
    if (i >= n) return;
    const G2Aff q = g2_load(points + 16 * i);
    int st;
    if (!fq_is_canonical(q.x.c0) || !fq_is_canonical(q.x.c1) || !fq_is_canonical(q.y.c0) || !fq_is_canonical(q.y.c1)) {
        st = 1;
    } else if (g2_is_inf(q)) {
        st = 0;
    } else if (!g2_on_curve(q)) {
        st = 2;
    } else {
        u32 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = FieldParams<FrTag>::P(k);
        G2Jac acc{f2_one(), f2_one(), f2_zero()};
        for (int b = 253; b >= 0; --b) {
            acc = g2_dbl(acc);
            if (bit_of(e, b)) acc = g2_add_mixed(acc, q);
        }
        st = f2_is_zero(acc.z) ? 0 : 3;
    }
    status[i] = st;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int pz_g2_check_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, int32_t* d_status) {
    if (!ctx || (n && (!d_points || !d_status)) || !aligned16(d_points)) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_g2_check, dim3(pz_div_up(n, GT)), dim3(GT), 0, ctx->stream, d_points, n, d_status);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g2_check(pz_ctx* ctx, const uint64_t* points, size_t n, int32_t* status) {
    if (!ctx || (n && (!points || !status))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dst;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 128, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_A, n * 4, &dst));
    HIPCHK(ctx, hipMemcpyAsync(di, points, n * 128, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(pz_g2_check_dev(ctx, (const uint64_t*)di, n, (int32_t*)dst));
    HIPCHK(ctx, hipMemcpyAsync(status, dst, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

extern "C" int pz_g2_compress(pz_ctx* ctx, const uint64_t* points, size_t n, uint8_t* bytes) {
    if (!ctx || (n && (!points || !bytes))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 128, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 64, &dout));
    HIPCHK(ctx, hipMemcpyAsync(di, points, n * 128, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_compress, dim3(pz_div_up(n, GT)), dim3(GT), 0, ctx->stream, (const uint64_t*)di, n, (uint8_t*)dout);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(bytes, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

extern "C" int pz_g2_decompress(pz_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* points, int32_t* status, uint64_t* n_bad) {
    if (!ctx || (n && (!bytes || !points))) return PZ_ERR_INVALID;
    if (n_bad) *n_bad = 0;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout, *dst;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 64, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 128, &dout));
    PZCHK(pz_ws_get(ctx, WS_IO_A, n * 4, &dst));
    HIPCHK(ctx, hipMemcpyAsync(di, bytes, n * 64, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_decompress, dim3(pz_div_up(n, GT)), dim3(GT), 0, ctx->stream, (const uint8_t*)di, n, (uint64_t*)dout, (int32_t*)dst);
    HIPCHK(ctx, hipGetLastError());
    std::vector<int32_t> st;
    int32_t* hs = status;
    if (!hs) {
        try {
            st.resize(n);
        } catch (...) {
            return PZ_ERR_OOM;
        }
        hs = st.data();
    }
    HIPCHK(ctx, hipMemcpyAsync(points, dout, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hs, dst, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_bad)
        for (size_t i = 0; i < n; ++i) *n_bad += hs[i] != 0;
    return PZ_OK;
}
