// pz_wire.hip -- halo2 wire bytes <-> the ABI's Montgomery words, on the device.
//
// G1 point, 32 bytes (halo2curves' G1Compressed [D]): the canonical x little-endian, bit 7 of byte 31 = parity of the canonical y, bit 6
// of byte 31 zero (x < p < 2^254), the identity 32 zero bytes.  Scalar, 32 bytes: the canonical value below r.
// Proof: the transcript's absorption order -- every commitment but W1 and W2 | pz_proof_evaluate's array without the trailing h(x) |
// W1 | W2 -- against pz_verify_batch's word layout (commitments with W1 and W2 | evaluations with h(x)).
//
// One lane per element, workgroups of 256, 16-byte loads and stores.  The codec of a batch of proofs is ONE LAUNCH PER FAMILY: the point
// kernels and the scalar kernel take a pz_wire_map that says where element i of the launch lies in the byte and the word buffer (the
// plain pz_g1_*compress_dev entry points pass the contiguous map), and k_proof_status folds the element statuses of a proof to its worst.
// Decompression: y = (x^3 + 3)^((p+1)/4) through f29_sqrt_candidate (fp29.cuh), accepted only if y^2 == x^3 + 3.
#include "fp29.cuh"
#include "pz_internal.h"

namespace {

constexpr unsigned WT = 256;

struct Loc {
    size_t wire, word, st;
    bool last;
};
__device__ __forceinline__ Loc locate(const pz_wire_map& m, size_t i, unsigned word_bytes) {
    const size_t p = i / m.per, j = i - p * m.per;
    Loc l;
    l.wire = p * m.wire_stride + (j < m.split ? m.wire_off0 + 32 * j : m.wire_off1 + 32 * (j - m.split));
    l.word = p * m.word_stride + m.word_off + (size_t)word_bytes * j;
    l.st = p * m.st_stride + m.st_off + j;
    l.last = j + 1 == m.per;
    return l;
}
__device__ __forceinline__ void load32(const uint8_t* p, u32 w[8]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 lo = q[0], hi = q[1];
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
    w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void store32(uint8_t* p, const u32 w[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
template <class T> __device__ __forceinline__ bool below_modulus(const u32 w[8]) {
    Fp<T> a;
    u32 t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a.v[k] = w[k];
    return fp_sub_p(t, a) != 0;   // a - p borrows
}

// status: 0 ok, 1 not canonical (x >= p; bit 6 set is such an x), 2 not on the curve.  A refused point is stored as the identity.
__global__ __launch_bounds__(256) void k_g1_decompress(const uint8_t* __restrict__ bytes, size_t n, pz_wire_map m, uint8_t* __restrict__ points,
                                                       int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * WT + threadIdx.x;
    if (i >= n) return;
    const Loc l = locate(m, i, 64);
    u32 w[8];
    load32(bytes + l.wire, w);
    const u32 sign = w[7] >> 31;
    w[7] &= 0x7fffffffu;
    u32 nz = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) nz |= w[k];
    Fq X = fp_zero<FqTag>(), Y = fp_zero<FqTag>();
    int st = 0;
    if (!below_modulus<FqTag>(w)) {
        st = 1;
    } else if (nz | sign) {   // x = 0 with sign 0 is the identity; x = 0 with sign 1 fails below (3 is not a square)
        F29<FqTag> c;
#pragma unroll
        for (int k = 0; k < 9; ++k) c.v[k] = P29<FqTag>::R517(k);
        const F29<FqTag> x256 = f29_mul(f29_unpack<FqTag>(w), c);   // the ABI's form of x
        const F29<FqTag> x261 = f29_to_261(x256);
        const F29<FqTag> one = f29_one<FqTag>();
        const F29<FqTag> rhs = f29_carry(f29_add(f29_mul(f29_sqr(x261), x261), f29_add(one, f29_dbl(one))));   // x^3 + 3, below 5p
        const F29<FqTag> y = f29_sqrt_candidate(rhs);
        const F29<FqTag> y2 = f29_canon<1>(f29_sqr(y)), r = f29_canon<3>(rhs);
        u32 diff = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) diff |= y2.v[k] ^ r.v[k];
        if (diff) {
            st = 2;
        } else {
            F29<FqTag> i1 = f29_zero<FqTag>();
            i1.v[0] = 1;
            const F29<FqTag> yi = f29_canon<1>(f29_mul(y, i1));   // the canonical integer y: its parity is the sign bit
            X = f29_to_fp<1>(x256);
            Y = f29_to_fp<1>(f29_to_256(y));
            if ((yi.v[0] & 1u) != sign) Y = fp_neg(Y);   // 2p - y; fp_store brings it to p - y (y != 0 on this curve)
        }
    }
    fp_store(points + l.word, X);
    fp_store(points + l.word + 32, Y);
    status[l.st] = st;
}

__global__ __launch_bounds__(256) void k_g1_compress(const uint8_t* __restrict__ points, size_t n, pz_wire_map m, uint8_t* __restrict__ bytes) {
    const size_t i = (size_t)blockIdx.x * WT + threadIdx.x;
    if (i >= n) return;
    const Loc l = locate(m, i, 64);
    const Fq X = fp_load<FqTag>(points + l.word), Y = fp_load<FqTag>(points + l.word + 32);
    Fq x = fp_zero<FqTag>();
    if (!(fp_is_zero_exact(X) && fp_is_zero_exact(Y))) {
        x = fp_canon(fp_from_mont(X));
        const Fq y = fp_canon(fp_from_mont(Y));
        x.v[7] |= (y.v[0] & 1u) << 31;
    }
    store32(bytes + l.wire, x.v);
}

// scalars of a launch: decode != 0: bytes -> words with the `>= r` check (status 1, stored as zero); else words -> bytes.  With
// m.skip_last the last element of every proof has no bytes: the h(x) slot, written as zero on decode.
__global__ __launch_bounds__(256) void k_fr_wire(const uint8_t* __restrict__ in, size_t n, pz_wire_map m, int decode, uint8_t* __restrict__ out,
                                                 int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * WT + threadIdx.x;
    if (i >= n) return;
    const Loc l = locate(m, i, 32);
    const bool skip = m.skip_last && l.last;
    if (decode) {
        Fr v = fp_zero<FrTag>();
        int st = 0;
        if (!skip) {
            u32 w[8];
            load32(in + l.wire, w);
            if (below_modulus<FrTag>(w)) {
#pragma unroll
                for (int k = 0; k < 8; ++k) v.v[k] = w[k];
                v = fp_to_mont(v);
            } else {
                st = 1;
            }
        }
        fp_store(out + l.word, v);
        status[l.st] = st;
    } else if (!skip) {
        const Fr c = fp_canon(fp_from_mont(fp_load<FrTag>(in + l.word)));
        store32(out + l.wire, c.v);
    }
}

// one workgroup per proof: out[p] = the worst of its `per` element statuses
__global__ __launch_bounds__(256) void k_proof_status(const int32_t* __restrict__ elem, size_t per, int32_t* __restrict__ out) {
    __shared__ int32_t s[WT];
    const unsigned t = threadIdx.x;
    const int32_t* e = elem + (size_t)blockIdx.x * per;
    int32_t worst = 0;
    for (size_t j = t; j < per; j += WT) worst = max(worst, e[j]);
    s[t] = worst;
    __syncthreads();
    for (unsigned off = WT / 2; off > 0; off >>= 1) {
        if (t < off) s[t] = max(s[t], s[t + off]);
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = s[0];
}

pz_wire_map flat_map(size_t n) {
    pz_wire_map m{};
    m.per = n;
    m.split = n;
    return m;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int pz_wire_proofs_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, int decode, uint8_t* d_bytes, uint64_t* d_words, int32_t* d_elem_status,
                          int32_t* d_status) {
    if (!B) return PZ_OK;
    const size_t n_pt = s.n_own, n_sc = s.n_ev, wire = 32ull * (n_pt + n_sc - 1), words = 64ull * n_pt + 32ull * n_sc;
    pz_wire_map mp{}, ms{};
    mp.per = n_pt;
    mp.split = n_pt - 2;                          // W1 and W2 follow the evaluations on the wire
    mp.wire_stride = ms.wire_stride = wire;
    mp.wire_off1 = 32ull * (n_pt - 2 + n_sc - 1);
    mp.word_stride = ms.word_stride = words;
    mp.st_stride = ms.st_stride = n_pt + n_sc;
    ms.per = ms.split = n_sc;
    ms.wire_off0 = 32ull * (n_pt - 2);
    ms.word_off = 64ull * n_pt;
    ms.st_off = n_pt;
    ms.skip_last = 1;                             // h(x) is not sent
    uint8_t* w8 = (uint8_t*)d_words;
    if (decode) {
        hipLaunchKernelGGL(k_g1_decompress, dim3(pz_div_up(B * n_pt, WT)), dim3(WT), 0, ctx->stream, (const uint8_t*)d_bytes, B * n_pt, mp, w8,
                           d_elem_status);
        hipLaunchKernelGGL(k_fr_wire, dim3(pz_div_up(B * n_sc, WT)), dim3(WT), 0, ctx->stream, (const uint8_t*)d_bytes, B * n_sc, ms, 1, w8,
                           d_elem_status);
        hipLaunchKernelGGL(k_proof_status, dim3((unsigned)B), dim3(WT), 0, ctx->stream, (const int32_t*)d_elem_status, n_pt + n_sc, d_status);
    } else {
        hipLaunchKernelGGL(k_g1_compress, dim3(pz_div_up(B * n_pt, WT)), dim3(WT), 0, ctx->stream, (const uint8_t*)w8, B * n_pt, mp, d_bytes);
        hipLaunchKernelGGL(k_fr_wire, dim3(pz_div_up(B * n_sc, WT)), dim3(WT), 0, ctx->stream, (const uint8_t*)w8, B * n_sc, ms, 0, d_bytes,
                           (int32_t*)nullptr);
    }
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_compress_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, uint8_t* d_bytes) {
    if (!ctx || (n && (!d_points || !d_bytes)) || !aligned16(d_points) || !aligned16(d_bytes)) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_g1_compress, dim3(pz_div_up(n, WT)), dim3(WT), 0, ctx->stream, (const uint8_t*)d_points, n, flat_map(n), d_bytes);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_decompress_dev(pz_ctx* ctx, const uint8_t* d_bytes, size_t n, uint64_t* d_points, int32_t* d_status) {
    if (!ctx || (n && (!d_bytes || !d_points || !d_status)) || !aligned16(d_points) || !aligned16(d_bytes)) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_g1_decompress, dim3(pz_div_up(n, WT)), dim3(WT), 0, ctx->stream, d_bytes, n, flat_map(n), (uint8_t*)d_points, d_status);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_compress(pz_ctx* ctx, const uint64_t* points, size_t n, uint8_t* bytes) {
    if (!ctx || (n && (!points || !bytes))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 64, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 32, &dout));
    HIPCHK(ctx, hipMemcpyAsync(di, points, n * 64, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(pz_g1_compress_dev(ctx, (const uint64_t*)di, n, (uint8_t*)dout));
    HIPCHK(ctx, hipMemcpyAsync(bytes, dout, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

extern "C" int pz_g1_decompress(pz_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* points, int32_t* status, uint64_t* n_bad) {
    if (!ctx || (n && (!bytes || !points))) return PZ_ERR_INVALID;
    if (n_bad) *n_bad = 0;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout, *dst;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 32, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 64, &dout));
    PZCHK(pz_ws_get(ctx, WS_IO_A, n * 4, &dst));
    HIPCHK(ctx, hipMemcpyAsync(di, bytes, n * 32, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(pz_g1_decompress_dev(ctx, (const uint8_t*)di, n, (uint64_t*)dout, (int32_t*)dst));
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
    HIPCHK(ctx, hipMemcpyAsync(points, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hs, dst, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_bad)
        for (size_t i = 0; i < n; ++i) *n_bad += hs[i] != 0;
    return PZ_OK;
}
