// pz_vkgen.hip -- the two kernels keygen_vk needs beyond K1 (csrc/pz_vk_keygen.cpp composes them; halo2's keygen_vk is reached in the
// reference at /root/reference/src/bench.rs:161-175):
//   pz_g1_commit_mask_dev         the commitment of 0 / 1 byte columns (selectors): the plain sum of the Lagrange bases at the set rows,
//                                 without widening the mask to 32-byte scalars and without the Pippenger sort;
//   pz_permutation_sigma_part_dev pz_permutation_sigma_dev for a RANGE of the permutation's columns, so that sigma can be committed tile
//                                 by tile out of one reusable buffer.
#include "ec.cuh"
#include "ec29.cuh"
#include <stdlib.h>

#include "pz_internal.h"

// ------------------------------------------------------------------------------------------------
// mask commitment.  One 256-lane workgroup per (row chunk, column):
//   1. every lane reads 16 mask bytes per pass (one 16-byte load where the column is aligned), coalesced;
//   2. the chunk's set rows are COMPACTED into an LDS list of 16-bit row offsets: a lane's count of set bytes is scanned over the wave
//      with five ballots (one per bit of the count) and popcounts, and the wave takes its place in the list with one LDS atomic -- a
//      selector column is a quarter full, a per-row `if (mask) add` would leave three quarters of every wave waiting;
//   3. lanes stride over the list: dense mixed additions, a table row is loaded for listed rows only;
//   4. a tree over the 256 accumulators in LDS (144 B each, 36 KiB: the list's storage is reused), one XYZZ partial per (column, chunk).
// A second kernel folds a column's partials into one Jacobian point.  The list's order differs from run to run (waves arrive in any
// order); the group element does not.  Bases may repeat or cancel: x29_add_affine / x29_add handle P + P and P - P.
// ------------------------------------------------------------------------------------------------
#define MASK_THREADS 256u
#define MASK_CHUNK_DEFAULT 16384u

__device__ __forceinline__ unsigned mask_bits16(const uint8_t* __restrict__ col, size_t r0, size_t n, bool aligned) {
    unsigned bits = 0;
    if (aligned && r0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(col + r0);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) bits |= ((w[j >> 2] >> (8 * (j & 3))) & 0xffu) ? (1u << j) : 0u;
    } else {
        for (int j = 0; j < 16; ++j)
            if (r0 + j < n && col[r0 + j]) bits |= 1u << j;
    }
    return bits;
}

template <unsigned CH>
__global__ __launch_bounds__(MASK_THREADS) void k_commit_mask(const G1Aff64* __restrict__ table, const uint8_t* __restrict__ mask,
                                                              size_t mask_stride, size_t n, unsigned n_chunks,
                                                              G1X29Raw* __restrict__ partials) {
    constexpr unsigned LIST_BYTES = CH * 2, TREE_BYTES = MASK_THREADS * (unsigned)sizeof(G1X29Raw);
    __shared__ __align__(16) unsigned char s_buf[LIST_BYTES > TREE_BYTES ? LIST_BYTES : TREE_BYTES];
    __shared__ unsigned s_count;
    unsigned short* s_list = reinterpret_cast<unsigned short*>(s_buf);
    G1X29Raw* s_pt = reinterpret_cast<G1X29Raw*>(s_buf);
    const unsigned chunk = blockIdx.x % n_chunks;
    const size_t colx = blockIdx.x / n_chunks;
    const uint8_t* col = mask + colx * mask_stride;
    const size_t base = (size_t)chunk * CH;
    const bool aligned = ((uintptr_t)col & 15u) == 0;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    for (unsigned pass = 0; pass < CH / (MASK_THREADS * 16u); ++pass) {
        const unsigned off = (pass * MASK_THREADS + threadIdx.x) * 16u;   // the lane's 16 rows, relative to the chunk
        const size_t r0 = base + off;
        const unsigned bits = r0 < n ? mask_bits16(col, r0, n, aligned) : 0u;
        const unsigned cnt = __popc(bits);
        // exclusive scan of cnt (0..16) over the wave, bit by bit of the count
        unsigned before = 0, total = 0;
#pragma unroll
        for (unsigned b = 0; b < 5; ++b) {
            const unsigned long long bal = __ballot((cnt >> b) & 1u);
            before += (unsigned)__popcll(bal & lt) << b;
            total += (unsigned)__popcll(bal) << b;
        }
        unsigned wave_base = 0;
        if (lane == 0 && total) wave_base = atomicAdd(&s_count, total);
        wave_base = __shfl(wave_base, 0);
        unsigned pos = wave_base + before;   // < CH: the chunk has CH rows and each is listed at most once
        for (unsigned rest = bits; rest; rest &= rest - 1) s_list[pos++] = (unsigned short)(off + (unsigned)__ffs(rest) - 1u);
    }
    __syncthreads();
    const unsigned count = s_count;
    G1X29 acc = x29_inf();
    for (unsigned i = threadIdx.x; i < count; i += MASK_THREADS) {
        const G1A29 q = a29_load64(table + base + s_list[i]);   // a listed row is below n <= the set's points
        x29_add_affine(acc, q);
    }
    __syncthreads();   // the list is done with: its storage becomes the tree's
    const unsigned live = count < MASK_THREADS ? count : MASK_THREADS;   // lanes at and above it hold the identity
    if (threadIdx.x < live) x29_store_raw(&s_pt[threadIdx.x], acc);
    __syncthreads();
    unsigned top = MASK_THREADS / 2;
    while (top >= live && top > 0) top >>= 1;   // the largest power of two below `live`
    for (unsigned off = top; off > 0; off >>= 1) {
        if (threadIdx.x < off && threadIdx.x + off < live) {
            G1X29 a = x29_load_raw(&s_pt[threadIdx.x]);
            const G1X29 o = x29_load_raw(&s_pt[threadIdx.x + off]);
            x29_add(a, o);
            x29_store_raw(&s_pt[threadIdx.x], a);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) x29_store_raw(partials + colx * n_chunks + chunk, live ? x29_load_raw(&s_pt[0]) : x29_inf());
}

__global__ __launch_bounds__(64) void k_commit_mask_fold(const G1X29Raw* __restrict__ partials, unsigned n_chunks, size_t n_cols,
                                                         G1Jac* __restrict__ out) {
    const size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n_cols) return;
    const G1X29Raw* p = partials + col * n_chunks;
    G1X29 acc = x29_load_raw(p);
    for (unsigned t = 1; t < n_chunks; ++t) {
        const G1X29 o = x29_load_raw(p + t);
        x29_add(acc, o);
    }
    x29_store_jac(out + col, acc);
}

// rows per workgroup: 16384 by default; PZ_MASK_CHUNK = 4096 | 8192 | 16384 | 32768 overrides it (measurements)
static unsigned mask_chunk() {
    const char* e = getenv("PZ_MASK_CHUNK");
    if (e && *e) {
        const unsigned long x = strtoul(e, nullptr, 10);
        if (x == 4096 || x == 8192 || x == 16384 || x == 32768) return (unsigned)x;
    }
    return MASK_CHUNK_DEFAULT;
}

extern "C" int pz_g1_commit_mask_dev(pz_ctx* ctx, const pz_bases* bases, const uint8_t* d_mask, size_t n_cols, size_t n, size_t mask_stride,
                                     uint64_t* d_out_jac) {
    if (!ctx || !bases || (n_cols && (!d_mask || !d_out_jac))) return PZ_ERR_INVALID;
    if (n > bases->n || (n_cols > 1 && mask_stride < n)) return PZ_ERR_INVALID;
    if (n_cols == 0) return PZ_OK;
    PZ_ENTER(ctx);
    const unsigned ch = mask_chunk();
    const size_t chunks = n ? (n + ch - 1) / ch : 1;   // n = 0: one empty chunk per column -> the identity
    if (chunks > 0x10000u) return PZ_ERR_UNSUPPORTED;
    const unsigned n_chunks = (unsigned)chunks;
    size_t group = 0x7fffffffu / n_chunks;   // columns per launch: the grid is one-dimensional
    if (group > n_cols) group = n_cols;
    void* part;
    PZCHK(pz_ws_get(ctx, WS_PARTIALS, group * n_chunks * sizeof(G1X29Raw), &part));
    const G1Aff64* table = (const G1Aff64*)bases->d_table;   // window 0: the points themselves
    for (size_t c0 = 0; c0 < n_cols; c0 += group) {
        const size_t nc = n_cols - c0 < group ? n_cols - c0 : group;
        const dim3 grid((unsigned)(nc * n_chunks));
        const uint8_t* m0 = d_mask + c0 * mask_stride;
#define PZ_MASK_LAUNCH(CH_) \
    hipLaunchKernelGGL(k_commit_mask<CH_>, grid, dim3(MASK_THREADS), 0, ctx->stream, table, m0, mask_stride, n, n_chunks, (G1X29Raw*)part)
        switch (ch) {
            case 4096: PZ_MASK_LAUNCH(4096u); break;
            case 8192: PZ_MASK_LAUNCH(8192u); break;
            case 32768: PZ_MASK_LAUNCH(32768u); break;
            default: PZ_MASK_LAUNCH(16384u); break;
        }
#undef PZ_MASK_LAUNCH
        hipLaunchKernelGGL(k_commit_mask_fold, dim3(pz_div_up(nc, 64)), dim3(64), 0, ctx->stream, (const G1X29Raw*)part, n_chunks, nc,
                           (G1Jac*)d_out_jac + c0);
        HIPCHK(ctx, hipGetLastError());
    }
    return PZ_OK;
}

// ------------------------------------------------------------------------------------------------
// sigma for columns [col_lo, col_lo + n_cols) of an m_total-column permutation: k_perm_sigma of pz_poly.hip over the range's part of
// the maps; images are checked against the WHOLE permutation's m_total x n cells (clamped and reported, as there).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_perm_sigma_part(const u32* __restrict__ map_col, const u32* __restrict__ map_row, size_t n,
                                                         size_t total, unsigned m_total, const Fr* __restrict__ wpow,
                                                         const Fr* __restrict__ dpow, Fr* __restrict__ sigma, size_t stride,
                                                         volatile unsigned* err) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t j = t / n, i = t % n;
    u32 c = map_col[t], r = map_row[t];
    if (c >= m_total || r >= n) {
        *err = 1u;
        c = 0;
        r = 0;
    }
    fp_store(sigma + j * stride + i, fp_mul(fp_load<FrTag>(dpow + c), fp_load<FrTag>(wpow + r)));
}

// the range's columns given by THEIR OWN map arrays (d_mc / d_mr point at the range's first column: n_cols x 2^k entries): what the
// host-pointer keygen_vk uploads tile by tile.  Declared in pz_internal.h.
int pz_permutation_sigma_tile(pz_ctx* ctx, const uint32_t* d_mc, const uint32_t* d_mr, size_t m_total, size_t n_cols, uint32_t k,
                              const uint64_t omega[4], const uint64_t delta[4], uint64_t* d_sigma, size_t sigma_stride) {
    if (!ctx || !d_mc || !d_mr || !omega || !delta || k > 26 || m_total == 0 || m_total > 0xffffffu) return PZ_ERR_INVALID;
    if (n_cols > m_total || (n_cols && !d_sigma)) return PZ_ERR_INVALID;
    const size_t n = (size_t)1 << k;
    if (sigma_stride % 4 || (n_cols > 1 && sigma_stride < 4 * n)) return PZ_ERR_INVALID;
    if (n_cols == 0) return PZ_OK;
    if (n_cols * n > (size_t)0x7fffffffu * 256u) return PZ_ERR_UNSUPPORTED;
    PZ_ENTER(ctx);
    void *wp, *dp;
    PZCHK(pz_get_pow_table(ctx, omega, n, &wp));
    PZCHK(pz_get_pow_table(ctx, delta, m_total, &dp));
    PZCHK(pz_async_err_init(ctx));
    hipLaunchKernelGGL(k_perm_sigma_part, dim3(pz_div_up(n_cols * n, 256)), dim3(256), 0, ctx->stream, d_mc, d_mr, n, n_cols * n,
                       (unsigned)m_total, (const Fr*)wp, (const Fr*)dp, (Fr*)d_sigma, sigma_stride / 4, ctx->async_err_d);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_permutation_sigma_part_dev(pz_ctx* ctx, const uint32_t* d_map_col, const uint32_t* d_map_row, size_t m_total, size_t col_lo,
                                             size_t n_cols, uint32_t k, const uint64_t omega[4], const uint64_t delta[4], uint64_t* d_sigma,
                                             size_t sigma_stride) {
    if (!ctx || !d_map_col || !d_map_row || k > 26 || col_lo > m_total || n_cols > m_total - col_lo) return PZ_ERR_INVALID;
    const size_t off = col_lo << k;
    return pz_permutation_sigma_tile(ctx, d_map_col + off, d_map_row + off, m_total, n_cols, k, omega, delta, d_sigma, sigma_stride);
}
