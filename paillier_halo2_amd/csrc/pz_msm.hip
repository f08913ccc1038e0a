// pz_msm.hip -- K1: BN254 G1 multi-scalar multiplication (== halo2curves best_multiexp, reached
// from /root/reference/src/bench.rs:161-171 through create_proof -> commit_lagrange / commit).
//
// MI355X-first design (not a translation of the CPU bucket loop):
//   * the base set is loaded ONCE into HBM as a window-shifted table T[w][i] = 2^(c*w) * P_i
//     (288 GB of HBM makes nwin x the SRS affordable: 2^17 points x 16 windows = 134 MB), so all
//     Pippenger windows of one MSM share ONE bucket set: no per-window running sums and no serial
//     Horner fold of c*nwin doublings at the end;
//   * scalars -> signed c-bit digits (sign folded into the point), zero digits dropped -- witness
//     columns are mostly short scalars, their cost is proportional to the non-zero digits;
//   * digits are counting-sorted by bucket in HBM (histogram -> scan -> scatter), then one lane
//     owns one bucket chunk and accumulates in XYZZ coordinates with a gather of 64-byte table
//     rows (the table stays Infinity-Cache resident across the columns of a batch); over-full
//     buckets are split into chunks (MsmP::chunk entries at most) so skewed scalars cannot serialise;
//   * sum_b b*B_b by a radix-16 tree of (weighted sum, plain sum) nodes.
// Every kernel takes grid.y = column, so a batch of column commitments is one launch sequence.
//
// Roofline: bounded by 32-bit integer multiply issue (v_mad_u64_u32), NOT by HBM: algorithmic
// traffic is 96 B per (scalar, base) pair; bench.py reports both fractions.
#include "ec.cuh"
#include "ec29.cuh"
#include "ec29_quad.cuh"
#include <math.h>
#include <stdlib.h>

#include "pz_internal.h"

#define MSM_CHUNK_MIN 16u   // chunk = max entries one lane accumulates for one bucket work item (MsmP::chunk,
#define MSM_CHUNK_MAX 256u  // chosen per launch sequence by msm_chunk_for)
#define MSM_HEAVY 24u       // buckets with more chunks than this are folded by a whole workgroup
#define MSM_MEDIUM 1024u    // ... up to this many chunks by a 32-lane group (k_msm_medium_sum), more by a whole workgroup
#define MSM_SLICE_MAX_COLS 8u   // up to this many columns per launch sequence take the bit-sliced reduction (latency), more the radix-16 tree (throughput)

struct MsmP {
    size_t n;          // scalars per column
    size_t n_table;    // points per window row of the table
    unsigned c;        // window bits
    unsigned nwin;     // windows in the table
    unsigned win_lo, win_hi;
    unsigned B;        // buckets = 1 << (c-1)
    size_t cap;        // entry capacity per column = n * (win_hi - win_lo)
    size_t max_items;  // work items per column (upper bound) = B + cap / chunk
    unsigned chunk;    // entries per work item, MSM_CHUNK_MIN..MSM_CHUNK_MAX
    unsigned spt;      // scalars per thread of the sort passes: a slice is SORT_THREADS * spt scalars (msm_spt_for, msm_spt_sparse)
};

// Which scatter runs is decided ON THE DEVICE from the launch's number of non-zero digits (summed by the scan kernels): the
// two-step (coarse + fine, LDS-staged) scatter wins on dense columns -- full-width scalars: 2.6 ms against 6.4 per 256 columns,
// and the accumulation likes its order -- and loses on sparse ones (witness columns: 5.1 ms against 2.2 per 512), and the host
// does not know which kind a launch holds.  All three kernels are launched; the ones not chosen leave at once.
struct ScatterSel {
    const unsigned long long* total;   // non-zero digits of the launch (all columns)
    unsigned long long thr;            // dense if *total >= thr
    volatile unsigned* err;            // set when a sorted-entry position lies outside its list (see scatter_bad): pinned HOST memory
};
// Every position the scatter kernels store to is DERIVED from the histogram pass's counts (bucket offsets + earlier slices'
// counts + a rank), so it is only as good as the agreement between the two passes over the scalars: a caller that overwrites
// the scalars while the call is in flight (the ABI's `_dev` calls are asynchronous), or a defect in a cursor computation, turns
// into stores past the end of the list -- round 3's one memory-access fault was exactly that, an experimental coarse step whose
// cursors over-counted.  Positions are therefore checked against the list they belong to before the
// store (one compare per entry beside an LDS atomic and a 4-byte store), a violation raises a flag in pinned host memory (a plain
// store over the fabric on the error path only: nothing is copied or polled otherwise) and surfaces as PZ_ERR_ASYNC at the
// context's next synchronising entry point; k_msm_accumulate clamps the table row it gathers, so a list with holes cannot send
// a gather outside the table either.
__device__ __noinline__ void scatter_bad(const ScatterSel& s) { *s.err = 1u; }
__device__ __forceinline__ bool scatter_dense(const ScatterSel& s) { return *s.total >= s.thr; }

__device__ __forceinline__ u32 sel8(const u32 s[8], unsigned i) {
    u32 r = s[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) r = (i == (unsigned)k) ? s[k] : r;
    return r;
}

// canonical |k| with sign: k in [0, r) Montgomery -> s = min(k, r-k), neg = (r-k < k)
__device__ __forceinline__ bool scalar_prepare(const Fr& mont, u32 s[8]) {
    Fr k = fp_from_mont(mont);
    Fr t;
    u64 br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u64 d = (u64)FieldParams<FrTag>::P(i) - k.v[i] - br;
        t.v[i] = (u32)d;
        br = (d >> 32) & 1;
    }
    // lexicographic t < k ?
    bool lt = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        if (!decided && t.v[i] != k.v[i]) {
            lt = t.v[i] < k.v[i];
            decided = true;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = lt ? t.v[i] : k.v[i];
    return lt;
}

// signed digit of window w given the running carry: d in (-2^(c-1), 2^(c-1)]
__device__ __forceinline__ int next_digit(const u32 s[8], unsigned w, unsigned c, unsigned& carry) {
    unsigned off = w * c;
    unsigned wi = off >> 5, sh = off & 31;
    u32 lo = wi < 8 ? sel8(s, wi) : 0;
    u32 hi = wi + 1 < 8 ? sel8(s, wi + 1) : 0;
    u64 both = ((u64)hi << 32) | lo;
    unsigned raw = (unsigned)(both >> sh) & ((1u << c) - 1);
    unsigned d = raw + carry;
    if (d > (1u << (c - 1))) {
        carry = 1;
        return (int)d - (int)(1u << c);
    }
    carry = 0;
    return (int)d;
}

// ------------------------------------------------------------------------------------------------
// table build: T[w][i] = 2^(c*w) * P_i, affine
// ------------------------------------------------------------------------------------------------
// Rows are 64-byte affine points like the ABI's, but their coordinates are kept in the 2^261 Montgomery domain of
// fp29.cuh (canonical 256-bit integers): the accumulation kernel unpacks them into 29-bit limbs, nothing else reads them.
__global__ __launch_bounds__(128) void k_build_table(const G1Aff64* __restrict__ bases, G1Aff64* __restrict__ table,
                                                     size_t n, unsigned c, unsigned nwin) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A29 p = a29_load64(bases + i);          // the ABI's 256-domain
    if (!a29_is_inf(p)) {
        p.x = f29_to_261(p.x);
        p.y = f29_to_261(p.y);
        p = a29_canon(p);
    }
    a29_store64(table + i, p);
    G1X29 x = x29_from_affine(p);
    for (unsigned w = 1; w < nwin; ++w) {
        for (unsigned k = 0; k < c; ++k) x = x29_dbl(x);
        const G1A29 a = a29_canon(x29_to_affine(x));
        a29_store64(table + (size_t)w * n + i, a);
        x = x29_from_affine(a);  // back to ZZ = 1
    }
}

// ------------------------------------------------------------------------------------------------
// counting sort of the digits by bucket, LDS-staged.  Scattered global atomics run at ~20 G/s on
// MI355X (one 64-B memory-side request per lane), far below what 50 M digits per column group need,
// so the bucket counters live in LDS: a 1024-thread workgroup owns a slice of SORT_SLICE scalars of
// one column and a private 2^(c-1)-entry counter array (128 KiB at c = 16: one workgroup per CU).
//   pass 1  k_msm_hist    : LDS histogram of the slice's non-zero digits -> slice_hist[col][slice][B]
//   pass 2  k_msm_scan    : per column, bucket totals -> entry offsets, chunk (work item) offsets, and
//                           slice_hist rewritten in place as each slice's start offset per bucket
//   pass 3  k_msm_scatter : slice offsets back into LDS, returning LDS atomics give every digit its
//                           slot; (table index | sign << 31) is written to the sorted entry list
// ------------------------------------------------------------------------------------------------
#define SORT_THREADS 1024u
#ifndef SORT_PER_THREAD
#define SORT_PER_THREAD 8u
#endif
#define SORT_SLICE (SORT_THREADS * SORT_PER_THREAD)
#define SORT_MAXB 32768u

// Workgroup -> (column, slice) for the two sort passes.  Workgroups are dealt round-robin over the 8 XCDs (ids b and b + 8
// share one, MI355X_MICROARCH.md "Workgroup dispatch"), and each XCD has its own L2: with PZ_SORT_XCD all slices of a column
// get ids of one residue mod 8, so the 4-byte entry stores of the scatter pass that fall into the same 128-byte line (same
// bucket, different slices) meet in ONE L2 instead of leaving eight partially written copies of it.  A speed choice only.
#ifndef PZ_SORT_XCD
#define PZ_SORT_XCD 1
#endif
// Fewer than 8 columns keep the plain order: their slices must spread over all XCDs, not fill one.
__device__ __forceinline__ bool sort_block_coords(unsigned n_slices, size_t n_cols, unsigned& slice, size_t& col) {
    if (PZ_SORT_XCD && n_cols >= 8) {
        const unsigned w = blockIdx.x >> 3;
        slice = w % n_slices;
        col = (size_t)(w / n_slices) * 8 + (blockIdx.x & 7u);
    } else {
        slice = blockIdx.x % n_slices;
        col = blockIdx.x / n_slices;
    }
    return col < n_cols;
}
static unsigned sort_grid(unsigned n_slices, size_t n_cols) {
    if (PZ_SORT_XCD && n_cols >= 8) return n_slices * (unsigned)((n_cols + 7) / 8 * 8);
    return n_slices * (unsigned)n_cols;
}

__global__ __launch_bounds__(SORT_THREADS) void k_msm_hist(const Fr* __restrict__ scalars, size_t col_stride, MsmP p,
                                                           u32* __restrict__ slice_hist, unsigned n_slices, size_t n_cols) {
    __shared__ u32 h[SORT_MAXB];
    size_t col;
    unsigned slice;
    if (!sort_block_coords(n_slices, n_cols, slice, col)) return;
    for (unsigned b = threadIdx.x; b < p.B; b += SORT_THREADS) h[b] = 0;
    __syncthreads();
    const size_t base = (size_t)slice * SORT_THREADS * p.spt;
    for (unsigned t = 0; t < p.spt; ++t) {
        const size_t i = base + (size_t)t * SORT_THREADS + threadIdx.x;
        if (i >= p.n) break;
        u32 s[8];
        (void)scalar_prepare(fp_load<FrTag>(scalars + col * col_stride + i), s);
        u32 any = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) any |= s[k];
        if (!any) continue;
        unsigned carry = 0;
        if (p.c == 16) {
            // the production window: digit w is a 16-bit half of limb w/2 -- with the loop unrolled the limb index is
            // a compile-time register, no 8-way select per digit
#pragma unroll
            for (unsigned w = 0; w < 16; ++w) {
                if (w < p.win_hi) {
                    const unsigned d0 = ((s[w >> 1] >> (16 * (w & 1))) & 0xffffu) + carry;
                    carry = d0 > 0x8000u ? 1u : 0u;
                    const unsigned mag = carry ? 0x10000u - d0 : d0;
                    if (w >= p.win_lo && mag != 0) atomicAdd(&h[mag - 1], 1u);
                }
            }
        } else {
            for (unsigned w = 0; w < p.win_hi; ++w) {
                int d = next_digit(s, w, p.c, carry);
                if (w >= p.win_lo && d != 0) atomicAdd(&h[(d < 0 ? -d : d) - 1], 1u);
            }
        }
    }
    __syncthreads();
    u32* out = slice_hist + (col * n_slices + slice) * (size_t)p.B;
    for (unsigned b = threadIdx.x; b < p.B; b += SORT_THREADS) out[b] = h[b];
}

// pass 2a: per (column, bucket): total over the slices; slice_hist rewritten in place as the slice's
// offset RELATIVE to the bucket start (exclusive prefix over slices).  One thread per bucket, coalesced.
__global__ __launch_bounds__(256) void k_msm_totals(u32* __restrict__ slice_hist, unsigned n_slices, MsmP p,
                                                    u32* __restrict__ totals) {
    const size_t col = blockIdx.y;
    const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    u32* sh = slice_hist + col * n_slices * (size_t)p.B + b;
    u32 run = 0;
    unsigned sl = 0;
    for (; sl + 8 <= n_slices; sl += 8) {   // eight loads in flight: a single column is cut into hundreds of slices
        u32 v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) v[k] = sh[(size_t)(sl + k) * p.B];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            sh[(size_t)(sl + k) * p.B] = run;
            run += v[k];
        }
    }
    for (; sl < n_slices; ++sl) {
        const u32 v = sh[(size_t)sl * p.B];
        sh[(size_t)sl * p.B] = run;
        run += v;
    }
    totals[col * p.B + b] = run;
}

#define ITEMS_SOLO 64u   // buckets with more chunks than this get their list entries written by a whole workgroup
// pass 2b: per column exclusive scans of the bucket totals (entry offsets) and of ceil(cnt/CHUNK) (item offsets)
#define SCAN_THREADS 1024
__global__ __launch_bounds__(SCAN_THREADS) void k_msm_scan(const u32* __restrict__ hist, MsmP p, u32* __restrict__ offs,
                                                  u32* __restrict__ items, u32* __restrict__ heavy,
                                                  u32* __restrict__ heavy_cnt, u32* __restrict__ fold_order,
                                                  u32* __restrict__ fold_cnt, u32* __restrict__ item_order,
                                                  u32* __restrict__ item_bucket, unsigned long long* __restrict__ digits_total) {
    __shared__ u32 s_cnt[SCAN_THREADS], s_itm[SCAN_THREADS];
    __shared__ u32 s_heavy;
    __shared__ u32 s_bin[MSM_HEAVY + 1], s_base[MSM_HEAVY + 1];
    __shared__ u32 s_obin[MSM_CHUNK_MAX + 1], s_obase[MSM_CHUNK_MAX + 1];  // work items by chunk size
    if (threadIdx.x == 0) s_heavy = 0;
    if (threadIdx.x <= MSM_HEAVY) s_bin[threadIdx.x] = 0;
    for (unsigned t = threadIdx.x; t <= MSM_CHUNK_MAX; t += blockDim.x) s_obin[t] = 0;
    __syncthreads();
    const size_t col = blockIdx.x;
    const u32* h = hist + col * p.B;
    u32* o = offs + col * (p.B + 1);
    u32* it = items + col * (p.B + 1);
    const unsigned per = (p.B + SCAN_THREADS - 1) / SCAN_THREADS;   // <= 32 (B <= 2^15)
    const unsigned lo = threadIdx.x * per;
    // this thread's bucket totals, all loads in flight at once (a loop that waits for each one costs `per` round trips, twice)
    u32 hv[32];
#pragma unroll
    for (unsigned k = 0; k < 32; ++k) hv[k] = (k < per && lo + k < p.B) ? h[lo + k] : 0u;
    u32 c = 0, m = 0;
#pragma unroll
    for (unsigned k = 0; k < 32; ++k) {
        const unsigned b = lo + k;
        if (k < per && b < p.B) {
            const u32 v = hv[k];
            c += v;
            const u32 ch = (v + p.chunk - 1) / p.chunk;
            m += ch;
            if (ch > MSM_HEAVY) heavy[col * p.B + atomicAdd(&s_heavy, 1u)] = b;
            else if (ch > 1) atomicAdd(&s_bin[ch], 1u);
            if (ch) {  // even split: rem chunks of q+1 entries, ch-rem of q
                const u32 q = v / ch, rem = v % ch;
                if (rem) atomicAdd(&s_obin[q + 1], rem);
                atomicAdd(&s_obin[q], ch - rem);
            }
        }
    }
    s_cnt[threadIdx.x] = c;
    s_itm[threadIdx.x] = m;
    __syncthreads();
    {   // exclusive scan of the per-thread sums over the workgroup: wave scans, then the 16 wave totals
        __shared__ u32 s_wc[SCAN_THREADS / 64], s_wm[SCAN_THREADS / 64];
        const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        u32 ic = c, im = m;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 tc = __shfl_up(ic, off, 64), tm = __shfl_up(im, off, 64);
            if (lane >= (unsigned)off) { ic += tc; im += tm; }
        }
        if (lane == 63) { s_wc[wv] = ic; s_wm[wv] = im; }
        __syncthreads();
        u32 bc = 0, bm = 0;
        for (unsigned k = 0; k < wv; ++k) { bc += s_wc[k]; bm += s_wm[k]; }
        s_cnt[threadIdx.x] = bc + ic - c;
        s_itm[threadIdx.x] = bm + im - m;
        if (threadIdx.x == SCAN_THREADS - 1) {
            o[p.B] = bc + ic;
            it[p.B] = bm + im;
            atomicAdd(digits_total, (unsigned long long)(bc + ic));
        }
    }
    if (threadIdx.x == 0) {
        heavy_cnt[col] = s_heavy;
        // buckets with 2..MSM_HEAVY chunks, ordered by chunk count (largest first): the fold kernel's lanes
        // then run equal trip counts within a wave
        u32 run = 0;
        for (int m2 = (int)MSM_HEAVY; m2 >= 2; --m2) {
            s_base[m2] = run;
            run += s_bin[m2];
            s_bin[m2] = 0;
        }
        fold_cnt[col] = run;
        // work items ordered by chunk size, largest first: the lanes of an accumulation wave then run (nearly)
        // equal trip counts -- real witness columns have most buckets at 1..16 entries
        run = 0;
        for (int sz = (int)p.chunk; sz >= 1; --sz) {
            s_obase[sz] = run;
            run += s_obin[sz];
            s_obin[sz] = 0;
        }
    }
    __syncthreads();
    c = s_cnt[threadIdx.x];
    m = s_itm[threadIdx.x];
#pragma unroll
    for (unsigned k = 0; k < 32; ++k) {
        const unsigned b = lo + k;
        if (k < per && b < p.B) {
            const u32 v = hv[k];
            o[b] = c;
            it[b] = m;
            c += v;
            const u32 ch = (v + p.chunk - 1) / p.chunk;
            m += ch;
            if (ch > 1 && ch <= MSM_HEAVY) fold_order[col * p.B + s_base[ch] + atomicAdd(&s_bin[ch], 1u)] = b;
            if (ch) {
                // where this bucket's work items go in the size-ordered list: its `rem` chunks of q + 1 entries and its
                // ch - rem chunks of q entries (one workgroup per column is parallel enough in a column batch; few columns
                // take k_msm_items_few instead of this kernel)
                const u32 q = v / ch, rem = v % ch;
                const u32 ph = rem ? s_obase[q + 1] + atomicAdd(&s_obin[q + 1], rem) : 0u;
                const u32 pl = s_obase[q] + atomicAdd(&s_obin[q], ch - rem);
                {
                    const u32 item0 = m - ch;
                    u32* ord = item_order + col * p.max_items;
                    u32* obk = item_bucket + col * p.max_items;
                    for (u32 j = 0; j < ch; ++j) {
                        const u32 pos = j < rem ? ph + j : pl + j - rem;
                        ord[pos] = item0 + j;
                        obk[pos] = b;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// pass 3 in two steps: the scatter of DENSE column batches (ScatterSel above; PZ_MSM_SCATTER=one / two force a variant).
// k_msm_scatter keeps 2^15 write frontiers per workgroup open (one per bucket): 2 MB per workgroup, 64 MB per XCD against a
// 4 MB L2, so nearly every 4-byte entry leaves the L2 as its own partial line -- 12.7 GB written per 256-column launch for
// 2.1 GB of entries (profiles/r02_pmc_fetch_write_bench.txt) -- and, the harder floor, 537 M scattered stores cost ~2 ms of
// L2 request rate whatever their bytes.  An MSD split with BOTH steps sorted inside LDS writes runs instead of single entries:
//   k_msm_scatter_coarse : the slice's digits go to the region of their COARSE bucket group (bucket >> 7) of a staging list,
//                          as (bucket & 127) << 25 | sign << 24 | table index
//   k_msm_scatter_fine   : a workgroup per (coarse group, column) sorts the group's entries (32 KB at the production shape)
//                          inside LDS, cursors for the 128 buckets in LDS, and writes whole lines
// Same sorted entry list up to the order inside a bucket, which no consumer depends on.
// Measured per launch (profiles/r03_ab_scatter_two_pass.txt): 256 full-width columns of 2^17: 1.76 + 0.75 ms against 6.43 for the
// single pass (and k_msm_accumulate 0.45 ms faster on this order); 512 witness-like columns: 1.72 + 3.38 against 2.20 -- the
// coarse step costs its rounds whatever the density and the fine step's workgroups find a tenth of the entries.  Hence the
// choice per launch, on the device.
// ------------------------------------------------------------------------------------------------
#define SORT_FINE_LOG 7u
#define SORT_FINE (1u << SORT_FINE_LOG)
#define SORT_COARSE_MAX (SORT_MAXB >> SORT_FINE_LOG)
// The coarse step is LDS-staged as well: a 256-thread workgroup takes its slice in rounds of 256 scalars (<= 4096 entries),
// counting-sorts the round's entries by coarse group inside LDS and writes them out in slot order -- consecutive lanes hit
// consecutive addresses inside a group's run (~16 entries = 64 B on average), so a wave's store instruction touches a handful
// of lines instead of 64.  Three barriers per round; window width 16 only (the digits of a scalar are kept in registers).
#define COARSE_THREADS 256u
#define COARSE_ROUND (COARSE_THREADS * 16u)
// invariants the kernel's packed words rely on: a round holds at most 16 digits of each of its 256 scalars, so a group's count
// in a round (the low half of rb[]) is <= COARSE_ROUND = 4096 < 2^16 and a slot index < COARSE_ROUND always; the group id (high half
// of rb[], the byte in sbin[]) is < SORT_COARSE_MAX = 256; phase 3 hands one counter to each of the COARSE_THREADS threads
static_assert(COARSE_ROUND <= 65536u && SORT_COARSE_MAX <= 256u && SORT_COARSE_MAX == COARSE_THREADS, "k_msm_scatter_coarse packing");
__global__ __launch_bounds__(COARSE_THREADS) void k_msm_scatter_coarse(const Fr* __restrict__ scalars, size_t col_stride, MsmP p,
                                                                       const u32* __restrict__ slice_hist, unsigned n_slices,
                                                                       const u32* __restrict__ offs, u32* __restrict__ staged,
                                                                       size_t n_cols, ScatterSel sel) {
    if (!scatter_dense(sel)) return;
    __shared__ u32 cb[SORT_COARSE_MAX];      // global cursor of every coarse group (position in the column's staging list)
    __shared__ u32 cnt[SORT_COARSE_MAX];     // entries of this round per group
    __shared__ u32 lbase[SORT_COARSE_MAX];   // first LDS slot of the group in this round
    __shared__ u32 gb[SORT_COARSE_MAX];      // global position of LDS slot 0 if it belonged to the group: cursor - lbase
    __shared__ u32 stage[COARSE_ROUND];
    __shared__ unsigned char sbin[COARSE_ROUND];
    __shared__ u32 s_total;
    size_t col;
    unsigned slice;
    if (!sort_block_coords(n_slices, n_cols, slice, col)) return;
    const u32* in = slice_hist + (col * n_slices + slice) * (size_t)p.B;
    const u32* o = offs + col * (p.B + 1);
    const unsigned n_coarse = p.B >> SORT_FINE_LOG;   // <= 256
    if (threadIdx.x < SORT_COARSE_MAX) {
        cb[threadIdx.x] = threadIdx.x < n_coarse ? o[threadIdx.x << SORT_FINE_LOG] : 0u;
        cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    // + the entries earlier slices put into the group: a wave sums 64 consecutive buckets (half a group) per step
    for (unsigned b0 = (threadIdx.x & ~63u); b0 < p.B; b0 += 4 * COARSE_THREADS) {
        u32 v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            const unsigned b = b0 + k * COARSE_THREADS + (threadIdx.x & 63u);
            v[k] = b < p.B ? in[b] : 0u;
        }
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            u32 t = v[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
            const unsigned b = b0 + k * COARSE_THREADS;
            if ((threadIdx.x & 63u) == 0 && b < p.B && t) atomicAdd(&cb[b >> SORT_FINE_LOG], t);
        }
    }
    __syncthreads();
    u32* e = staged + col * p.cap;
    const size_t base = (size_t)slice * SORT_THREADS * p.spt;
    const unsigned rounds = SORT_THREADS * p.spt / COARSE_THREADS;
    // the next round's scalar is requested before this round's stores go out (its latency would otherwise be exposed in every
    // one of the 4 * spt rounds)
    Fr nxt = fp_zero<FrTag>();
    if (base + threadIdx.x < p.n) nxt = fp_load<FrTag>(scalars + col * col_stride + base + threadIdx.x);
    for (unsigned rd = 0; rd < rounds; ++rd) {
        const size_t i = base + (size_t)rd * COARSE_THREADS + threadIdx.x;
        if (base + (size_t)rd * COARSE_THREADS >= p.n) break;   // uniform: the whole round lies beyond the column
        const Fr cur_scalar = nxt;
        // ---- phase 1: digits of this thread's scalar, rank of each inside its group (LDS counters)
        u32 ev[16], rb[16];
#pragma unroll
        for (unsigned w = 0; w < 16; ++w) rb[w] = 0xffffffffu;
        if (i < p.n) {
            u32 s[8];
            const bool neg = scalar_prepare(cur_scalar, s);
            unsigned carry = 0;
#pragma unroll
            for (unsigned w = 0; w < 16; ++w) {
                if (w < p.win_hi) {
                    const unsigned d0 = ((s[w >> 1] >> (16 * (w & 1))) & 0xffffu) + carry;
                    carry = d0 > 0x8000u ? 1u : 0u;
                    const unsigned mag = carry ? 0x10000u - d0 : d0;
                    if (w >= p.win_lo && mag != 0) {
                        const unsigned bkt = mag - 1, grp = bkt >> SORT_FINE_LOG;
                        const bool sgn = neg != (carry != 0);
                        ev[w] = (u32)((size_t)w * p.n_table + i) | (sgn ? 0x01000000u : 0u) | ((bkt & (SORT_FINE - 1)) << 25);
                        rb[w] = atomicAdd(&cnt[grp], 1u) | (grp << 16);
                    }
                }
            }
        }
        __syncthreads();
        // ---- phase 2: exclusive scan of the 256 counters by the first wave
        if (threadIdx.x < 64) {
            const unsigned c0 = cnt[4 * threadIdx.x], c1 = cnt[4 * threadIdx.x + 1], c2 = cnt[4 * threadIdx.x + 2], c3 = cnt[4 * threadIdx.x + 3];
            const unsigned sum = c0 + c1 + c2 + c3;
            unsigned incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off, 64);
                if ((int)threadIdx.x >= off) incl += t;
            }
            const unsigned excl = incl - sum;
            lbase[4 * threadIdx.x] = excl;
            lbase[4 * threadIdx.x + 1] = excl + c0;
            lbase[4 * threadIdx.x + 2] = excl + c0 + c1;
            lbase[4 * threadIdx.x + 3] = excl + c0 + c1 + c2;
            if (threadIdx.x == 63) s_total = incl;
        }
        __syncthreads();
        // ---- phase 3: cursors, placement into the staging array
        {
            const unsigned g = cb[threadIdx.x], c = cnt[threadIdx.x];
            gb[threadIdx.x] = g - lbase[threadIdx.x];
            cb[threadIdx.x] = g + c;
            cnt[threadIdx.x] = 0;
        }
#pragma unroll
        for (unsigned w = 0; w < 16; ++w) {
            if (rb[w] != 0xffffffffu) {
                const unsigned grp = rb[w] >> 16, slot = lbase[grp] + (rb[w] & 0xffffu);
                stage[slot] = ev[w];
                sbin[slot] = (unsigned char)grp;
            }
        }
        __syncthreads();
        // ---- phase 4: out in slot order (coalesced inside every group's run)
        {
            const size_t in_ = i + COARSE_THREADS;
            if (rd + 1 < rounds && in_ < p.n) nxt = fp_load<FrTag>(scalars + col * col_stride + in_);
        }
        const unsigned total = s_total;
        for (unsigned sl = threadIdx.x; sl < total; sl += COARSE_THREADS) {
            const u32 pos = gb[sbin[sl]] + sl;
            if (pos < p.cap) e[pos] = stage[sl];
            else scatter_bad(sel);
        }
    }
}

// Scattered 4-byte stores are bound by the L2's request rate, not by bytes (537 M stores of a 256-column launch: ~2 ms at best,
// measured 3.5 ms), so a group that fits the staging array is sorted INSIDE LDS and leaves as whole lines; a larger group
// (skewed columns) takes the direct path.
#define FINE_LDS_ENTRIES 12288u   // 48 KB: three workgroups per CU
#define FINE_THREADS 512u        // x 8 loads in flight per thread: ~48 KB outstanding per CU
__global__ __launch_bounds__(FINE_THREADS) void k_msm_scatter_fine(MsmP p, const u32* __restrict__ offs, const u32* __restrict__ staged,
                                                          u32* __restrict__ entries, ScatterSel sel) {
    if (!scatter_dense(sel)) return;
    __shared__ u32 cur[SORT_FINE + 1];
    __shared__ u32 buf[FINE_LDS_ENTRIES];
    const size_t col = blockIdx.y;
    const u32* o = offs + col * (p.B + 1) + ((size_t)blockIdx.x << SORT_FINE_LOG);
    if (threadIdx.x <= SORT_FINE) cur[threadIdx.x] = o[threadIdx.x];
    __syncthreads();
    const u32 lo = cur[0], hi = cur[SORT_FINE];   // the group's region; cur[SORT_FINE] is never advanced
    __syncthreads();
    const u32* src = staged + col * p.cap;
    u32* dst = entries + col * p.cap;
    const bool in_lds = hi - lo <= FINE_LDS_ENTRIES;
    for (u32 j0 = lo + threadIdx.x; j0 < hi; j0 += 8 * FINE_THREADS) {
        u32 v[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const u32 j = j0 + k * FINE_THREADS;
            v[k] = j < hi ? src[j] : 0xffffffffu;
        }
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            if (j0 + k * FINE_THREADS < hi) {
                const u32 pos = atomicAdd(&cur[v[k] >> 25], 1u);
                const u32 e = (v[k] & 0x00ffffffu) | ((v[k] & 0x01000000u) << 7);
                if (pos >= hi) scatter_bad(sel);   // beyond the group's region (pos >= lo always: cursors start at bucket offsets)
                else if (in_lds) buf[pos - lo] = e;
                else dst[pos] = e;
            }
        }
    }
    if (!in_lds) return;
    __syncthreads();
    for (u32 j = threadIdx.x; j < hi - lo; j += FINE_THREADS) dst[lo + j] = buf[j];
}

// ------------------------------------------------------------------------------------------------
// FEW columns (one large MSM, a rank's share of it: nc <= MSM_SLICE_MAX_COLS): k_msm_scan's single workgroup per column is the
// whole chip's critical path there (114 us for 2^15 buckets: strided global accesses from one CU, a few LDS counters every
// thread adds to).  The same offsets, item counts and size-ordered work item list from two kernels with a thread per bucket:
//   k_msm_totals_few : k_msm_totals + per 256-bucket block: entry sum, item sum, items by chunk size (257 bins)
//   k_msm_items_few  : block prefix from the block sums, in-block scans, list positions = [sizes larger] + [same size in
//                      earlier blocks] + [rank inside the block]; writes offs / items / item_order / item_bucket
// No heavy / fold lists: the fold kernels of this path look at every bucket themselves (k_msm_fold_few).
// ------------------------------------------------------------------------------------------------
#define FEW_BINS (MSM_CHUNK_MAX + 1u)
__device__ __forceinline__ u32 block_sum_256(u32 v, u32* s_tmp) {   // sum over the 256 threads of a workgroup (s_tmp: 4 words)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}

__global__ __launch_bounds__(256) void k_msm_totals_few(u32* __restrict__ slice_hist, unsigned n_slices, MsmP p,
                                                        u32* __restrict__ totals, u32* __restrict__ blk_cnt,
                                                        u32* __restrict__ blk_itm, u32* __restrict__ blk_bins) {
    __shared__ u32 s_bin[FEW_BINS];
    __shared__ u32 s_tmp[4];
    const size_t col = blockIdx.y;
    const unsigned nblk = gridDim.x;
    const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned t = threadIdx.x; t < FEW_BINS; t += blockDim.x) s_bin[t] = 0;
    u32 run = 0;
    if (b < p.B) {
        u32* sh = slice_hist + col * n_slices * (size_t)p.B + b;
        unsigned sl = 0;
        for (; sl + 8 <= n_slices; sl += 8) {   // eight loads in flight: a single column is cut into hundreds of slices
            u32 v[8];
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) v[k] = sh[(size_t)(sl + k) * p.B];
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) {
                sh[(size_t)(sl + k) * p.B] = run;
                run += v[k];
            }
        }
        for (; sl < n_slices; ++sl) {
            const u32 v = sh[(size_t)sl * p.B];
            sh[(size_t)sl * p.B] = run;
            run += v;
        }
        totals[col * p.B + b] = run;
    }
    __syncthreads();
    const u32 ch = (run + p.chunk - 1) / p.chunk;
    if (ch) {   // even split: rem chunks of q + 1 entries, ch - rem of q
        const u32 q = run / ch, rem = run % ch;
        if (rem) atomicAdd(&s_bin[q + 1], rem);
        atomicAdd(&s_bin[q], ch - rem);
    }
    const u32 sc = block_sum_256(run, s_tmp);
    const u32 sm = block_sum_256(ch, s_tmp);
    if (threadIdx.x == 0) {
        blk_cnt[col * nblk + blockIdx.x] = sc;
        blk_itm[col * nblk + blockIdx.x] = sm;
    }
    __syncthreads();
    u32* bo = blk_bins + (col * nblk + blockIdx.x) * (size_t)FEW_BINS;
    for (unsigned t = threadIdx.x; t < FEW_BINS; t += blockDim.x) bo[t] = s_bin[t];
}

__global__ __launch_bounds__(256) void k_msm_items_few(MsmP p, const u32* __restrict__ totals, const u32* __restrict__ blk_cnt,
                                                       const u32* __restrict__ blk_itm, const u32* __restrict__ blk_bins,
                                                       u32* __restrict__ offs, u32* __restrict__ items,
                                                       u32* __restrict__ item_order, u32* __restrict__ item_bucket,
                                                       unsigned long long* __restrict__ digits_total) {
    __shared__ u32 s_pos[FEW_BINS], s_tot[FEW_BINS], s_rank[FEW_BINS];
    __shared__ u32 s_tmp[4], s_wc[4], s_wm[4];
    __shared__ u32 s_big[256];
    __shared__ u32 s_nbig;
    const size_t col = blockIdx.y;
    const unsigned nblk = gridDim.x, blk = blockIdx.x;
    const unsigned b = blk * blockDim.x + threadIdx.x;
    if (threadIdx.x == 0) s_nbig = 0;
    // entries / items in the blocks before this one
    u32 pc = 0, pm = 0;
    for (unsigned i = threadIdx.x; i < blk; i += blockDim.x) {
        pc += blk_cnt[col * nblk + i];
        pm += blk_itm[col * nblk + i];
    }
    pc = block_sum_256(pc, s_tmp);
    pm = block_sum_256(pm, s_tmp);
    // list positions by chunk size: items of a larger size come first, then the same size in earlier blocks
    for (unsigned sz = threadIdx.x; sz < FEW_BINS; sz += blockDim.x) {
        u32 tot = 0, pre = 0;
        const u32* bb = blk_bins + col * nblk * (size_t)FEW_BINS + sz;
        unsigned i = 0;
        for (; i + 8 <= nblk; i += 8) {
            u32 v[8];
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) v[k] = bb[(size_t)(i + k) * FEW_BINS];
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) {
                tot += v[k];
                if (i + k < blk) pre += v[k];
            }
        }
        for (; i < nblk; ++i) {
            const u32 v = bb[(size_t)i * FEW_BINS];
            tot += v;
            if (i < blk) pre += v;
        }
        s_tot[sz] = tot;
        s_pos[sz] = pre;
        s_rank[sz] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int sz = (int)MSM_CHUNK_MAX; sz >= 1; --sz) {
            s_pos[sz] += run;
            run += s_tot[sz];
        }
    }
    // in-block exclusive scans of the bucket totals and chunk counts
    const u32 v = b < p.B ? totals[col * p.B + b] : 0u;
    const u32 ch = (v + p.chunk - 1) / p.chunk;
    u32 ic = v, im = ch;
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 tc = __shfl_up(ic, off, 64), tm = __shfl_up(im, off, 64);
        if (lane >= (unsigned)off) { ic += tc; im += tm; }
    }
    if (lane == 63) { s_wc[wv] = ic; s_wm[wv] = im; }
    __syncthreads();
    u32 bc = 0, bm = 0;
    for (unsigned k = 0; k < wv; ++k) { bc += s_wc[k]; bm += s_wm[k]; }
    const u32 o_b = pc + bc + ic - v, it_b = pm + bm + im - ch;
    u32* o = offs + col * (p.B + 1);
    u32* it = items + col * (p.B + 1);
    if (b < p.B) {
        o[b] = o_b;
        it[b] = it_b;
        if (b == p.B - 1) {
            o[p.B] = o_b + v;
            it[p.B] = it_b + ch;
            atomicAdd(digits_total, (unsigned long long)(o_b + v));
        }
    }
    u32* ord = item_order + col * p.max_items;
    u32* obk = item_bucket + col * p.max_items;
    u32 ph = 0, pl = 0, rem = 0;
    if (ch) {
        const u32 q = v / ch;
        rem = v % ch;
        if (rem) ph = s_pos[q + 1] + atomicAdd(&s_rank[q + 1], rem);
        pl = s_pos[q] + atomicAdd(&s_rank[q], ch - rem);
        if (ch > ITEMS_SOLO) {
            s_big[atomicAdd(&s_nbig, 1u)] = threadIdx.x;
        } else {
            for (u32 j = 0; j < ch; ++j) {
                const u32 pos = j < rem ? ph + j : pl + j - rem;
                ord[pos] = it_b + j;
                obk[pos] = b;
            }
        }
    }
    // buckets with many chunks: their list entries are written by the whole workgroup (parameters through LDS)
    __shared__ u32 s_par[256][5];
    if (ch > ITEMS_SOLO) {
        s_par[threadIdx.x][0] = ch; s_par[threadIdx.x][1] = rem; s_par[threadIdx.x][2] = ph; s_par[threadIdx.x][3] = pl; s_par[threadIdx.x][4] = it_b;
    }
    __syncthreads();
    for (unsigned k = 0; k < s_nbig; ++k) {
        const unsigned tt = s_big[k];
        const u32 ch2 = s_par[tt][0], rem2 = s_par[tt][1], ph2 = s_par[tt][2], pl2 = s_par[tt][3], it2 = s_par[tt][4];
        for (u32 j = threadIdx.x; j < ch2; j += blockDim.x) {
            const u32 pos = j < rem2 ? ph2 + j : pl2 + j - rem2;
            ord[pos] = it2 + j;
            obk[pos] = blk * blockDim.x + tt;
        }
    }
}

__global__ __launch_bounds__(SORT_THREADS) void k_msm_scatter(const Fr* __restrict__ scalars, size_t col_stride, MsmP p,
                                                              const u32* __restrict__ slice_hist, unsigned n_slices,
                                                              const u32* __restrict__ offs, u32* __restrict__ entries, size_t n_cols,
                                                              ScatterSel sel) {
    if (scatter_dense(sel)) return;   // the two-step kernels take this launch
    __shared__ u32 h[SORT_MAXB];
    size_t col;
    unsigned slice;
    if (!sort_block_coords(n_slices, n_cols, slice, col)) return;
    // slice_hist == nullptr: the column is ONE slice (sparse launches, msm_spt_sparse) -- every slice offset is zero, k_msm_totals
    // did not run and the histogram still holds counts: the cursors are the bucket offsets themselves
    const bool sliced = slice_hist != nullptr;
    const u32* in = sliced ? slice_hist + (col * n_slices + slice) * (size_t)p.B : offs;
    const u32* o = offs + col * (p.B + 1);
    // eight buckets per thread in flight (a plain loop waited for each pair of loads: 32 round trips per workgroup, the
    // whole cost of the pass for a single column cut into many slices)
    for (unsigned b0 = threadIdx.x; b0 < p.B; b0 += 8 * SORT_THREADS) {
        u32 va[8], vb[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const unsigned b = b0 + k * SORT_THREADS, bc = b < p.B ? b : p.B - 1;
            va[k] = o[bc];
            vb[k] = sliced ? in[bc] : 0u;
        }
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const unsigned b = b0 + k * SORT_THREADS;
            if (b < p.B) h[b] = va[k] + vb[k];
        }
    }
    __syncthreads();
    u32* e = entries + col * p.cap;
    const size_t base = (size_t)slice * SORT_THREADS * p.spt;
    for (unsigned t = 0; t < p.spt; ++t) {
        const size_t i = base + (size_t)t * SORT_THREADS + threadIdx.x;
        if (i >= p.n) break;
        u32 s[8];
        const bool neg = scalar_prepare(fp_load<FrTag>(scalars + col * col_stride + i), s);
        u32 any = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) any |= s[k];
        if (!any) continue;
        unsigned carry = 0;
        if (p.c == 16) {
#pragma unroll
            for (unsigned w = 0; w < 16; ++w) {
                if (w < p.win_hi) {
                    const unsigned d0 = ((s[w >> 1] >> (16 * (w & 1))) & 0xffffu) + carry;
                    carry = d0 > 0x8000u ? 1u : 0u;
                    const unsigned mag = carry ? 0x10000u - d0 : d0;
                    if (w >= p.win_lo && mag != 0) {
                        const u32 pos = atomicAdd(&h[mag - 1], 1u);
                        const bool sgn = neg != (carry != 0);
                        if (pos < p.cap) e[pos] = (u32)((size_t)w * p.n_table + i) | (sgn ? 0x80000000u : 0u);
                        else scatter_bad(sel);
                    }
                }
            }
        } else {
            for (unsigned w = 0; w < p.win_hi; ++w) {
                int d = next_digit(s, w, p.c, carry);
                if (w >= p.win_lo && d != 0) {
                    const unsigned b = (d < 0 ? -d : d) - 1;
                    const u32 pos = atomicAdd(&h[b], 1u);
                    const bool sgn = neg != (d < 0);
                    if (pos < p.cap) e[pos] = (u32)((size_t)w * p.n_table + i) | (sgn ? 0x80000000u : 0u);
                    else scatter_bad(sel);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bucket accumulation: one lane per (bucket, chunk) work item
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_msm_accumulate(const G1Aff64* __restrict__ table, MsmP p,
                                                        const u32* __restrict__ offs, const u32* __restrict__ items,
                                                        const u32* __restrict__ item_order,
                                                        const u32* __restrict__ item_bucket,
                                                        const u32* __restrict__ entries, G1X29Raw* __restrict__ partials) {
    // grid.x = column, grid.y = block of ranks: workgroups are dispatched x-fastest, so the largest items of EVERY
    // column start first and the chip always holds work of one size class (with the column in grid.y, each column's
    // few long items pinned its ~128 resident workgroups and the columns went through 8 at a time)
    const size_t col = blockIdx.x;
    const u32* it = items + col * (p.B + 1);
    const u32 total = it[p.B];
    const u32 rank = blockIdx.y * blockDim.x + threadIdx.x;
    if (rank >= total) return;
    const u32 item = item_order[col * p.max_items + rank];   // chunk-size order (scan kernel)
    const unsigned b = item_bucket[col * p.max_items + rank];
    const u32* o = offs + col * (p.B + 1);
    // the bucket's entries are split EVENLY over its chunks (sizes differ by at most one)
    const u32 cnt = o[b + 1] - o[b], nch = it[b + 1] - it[b], j = item - it[b];
    const u32 q = cnt / nch, rem = cnt % nch;
    const u32 start = o[b] + j * q + (j < rem ? j : rem);
    const u32 end = start + q + (j < rem ? 1u : 0u);
    const u32* e = entries + col * p.cap;
    const u32 last_row = (u32)((size_t)p.nwin * p.n_table - 1);   // the gather never leaves the table, whatever the list holds
    G1X29 acc = x29_inf();
    for (u32 k = start; k < end; ++k) {
        u32 ent = e[k];
        const u32 row = ent & 0x7fffffffu;
        G1A29 q = a29_load64(table + (row < last_row ? row : last_row));
        if ((ent & 0x80000000u) && !a29_is_inf(q)) q.y = a29_neg_y(q.y);
        x29_add_affine(acc, q);
    }
    x29_store_raw(partials + col * p.max_items + item, acc);
}

// A bucket with more than MsmP::chunk entries owns several consecutive partials; its sum is left in the
// first one.  Ordinary buckets (<= MSM_HEAVY chunks): one lane each, a short serial fold -- uniform
// columns (every bucket ~4 chunks) keep a wave's lanes on the same trip count.  Heavy buckets (short
// scalars put half of their signed-digit carries into the single bucket "digit 1", tens of thousands of
// entries) are listed by the scan kernel and folded by a whole workgroup each: strided serial sums,
// then an LDS tree.
__global__ __launch_bounds__(256) void k_msm_bucket_sum(MsmP p, const u32* __restrict__ items,
                                                        const u32* __restrict__ fold_order,
                                                        const u32* __restrict__ fold_cnt, G1X29Raw* __restrict__ partials) {
    const size_t col = blockIdx.x;  // as in k_msm_accumulate: rank blocks of all columns together
    const unsigned r = blockIdx.y * blockDim.x + threadIdx.x;
    if (r >= fold_cnt[col]) return;
    const unsigned b = fold_order[col * p.B + r];
    const u32* it = items + col * (p.B + 1);
    const u32 first = it[b], m = it[b + 1] - first;
    G1X29Raw* pc = partials + col * p.max_items + first;
    G1X29 acc = x29_load_raw(pc);
    for (u32 t = 1; t < m; ++t) {
        G1X29 o = x29_load_raw(pc + t);
        x29_add(acc, o);
    }
    x29_store_raw(pc, acc);
}

__global__ __launch_bounds__(256) void k_msm_heavy_sum(MsmP p, const u32* __restrict__ items,
                                                       const u32* __restrict__ heavy, const u32* __restrict__ heavy_cnt,
                                                       G1X29Raw* __restrict__ partials) {
    __shared__ G1X29Raw s_pt[256];
    const size_t col = blockIdx.y;
    const u32 nh = heavy_cnt[col];
    const u32* it = items + col * (p.B + 1);
    for (u32 k = blockIdx.x; k < nh; k += gridDim.x) {
        const u32 b = heavy[col * p.B + k];
        const u32 first = it[b], m = it[b + 1] - first;
        if (m <= MSM_MEDIUM) continue;   // k_msm_medium_sum's (block-uniform branch)
        G1X29Raw* pc = partials + col * p.max_items + first;
        G1X29 acc = x29_inf();
        for (u32 t = threadIdx.x; t < m; t += blockDim.x) {
            G1X29 o = x29_load_raw(pc + t);
            x29_add(acc, o);
        }
        x29_store_raw(&s_pt[threadIdx.x], acc);
        __syncthreads();
        // tree over the lanes that hold something: depth log2(min(m, 256)) additions, not always 8
        unsigned top = 128;
        while (top >= m && top > 0) top >>= 1;   // largest power of two below m (m > MSM_HEAVY >= 2)
        for (unsigned off = top; off > 0; off >>= 1) {
            if (threadIdx.x < off && threadIdx.x + off < (m < 256u ? m : 256u)) {
                G1X29 a = x29_load_raw(&s_pt[threadIdx.x]);
                G1X29 o = x29_load_raw(&s_pt[threadIdx.x + off]);
                x29_add(a, o);
                x29_store_raw(&s_pt[threadIdx.x], a);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) x29_store_raw(pc, x29_load_raw(&s_pt[0]));
        __syncthreads();
    }
}

// Buckets of MSM_HEAVY < m <= MSM_MEDIUM chunks: a 32-lane group each (eight buckets per workgroup at a time).  One large
// MSM makes EVERY bucket such a bucket (2^22 points: 2^15 buckets of 32 chunks): a whole workgroup per bucket left 7/8 of
// its lanes idle through an 8-level tree and cost 2.5 ms whatever the MSM's size.
__global__ __launch_bounds__(256) void k_msm_medium_sum(MsmP p, const u32* __restrict__ items,
                                                        const u32* __restrict__ heavy, const u32* __restrict__ heavy_cnt,
                                                        G1X29Raw* __restrict__ partials) {
    __shared__ G1X29Raw s_pt[256];
    const size_t col = blockIdx.y;
    const u32 nh = heavy_cnt[col];
    const u32* it = items + col * (p.B + 1);
    const unsigned g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const u32 rounds = (nh + gridDim.x * 8 - 1) / (gridDim.x * 8);
    for (u32 r = 0; r < rounds; ++r) {
        const u32 k = (r * gridDim.x + blockIdx.x) * 8 + g;
        u32 first = 0, m = 0;
        if (k < nh) {
            const u32 b = heavy[col * p.B + k];
            first = it[b];
            m = it[b + 1] - first;
            if (m > MSM_MEDIUM) m = 0;   // k_msm_heavy_sum's
        }
        G1X29Raw* pc = partials + col * p.max_items + first;
        G1X29 acc = x29_inf();
        for (u32 t = l; t < m; t += 32) {
            G1X29 o = x29_load_raw(pc + t);
            x29_add(acc, o);
        }
        x29_store_raw(&s_pt[threadIdx.x], acc);
        __syncthreads();
        for (unsigned off = 16; off > 0; off >>= 1) {
            if (l < off && l + off < m) {
                G1X29 a = x29_load_raw(&s_pt[threadIdx.x]);
                G1X29 o = x29_load_raw(&s_pt[threadIdx.x + off]);
                x29_add(a, o);
                x29_store_raw(&s_pt[threadIdx.x], a);
            }
            __syncthreads();
        }
        if (l == 0 && m) x29_store_raw(pc, x29_load_raw(&s_pt[threadIdx.x]));
        __syncthreads();
    }
}

// FEW columns: the bucket folds without the scan kernel's lists.  Every addition of a fold is ~6 us of dependent latency on a
// nearly empty chip, so a bucket's partial sums are folded by a GROUP of G lanes: strided serial sums, then a log2(G)-level
// tree through LDS.  Launched twice: G = 4 for buckets of 2 .. MSM_FEW_SMALL chunks (uniform scalars: 8 - 9 chunks per bucket,
// depth 2 + 2 additions), G = 32 for MSM_FEW_SMALL + 1 .. MSM_MEDIUM; longer buckets are found and folded by whole workgroups
// in k_msm_heavy_few.  All groups of a workgroup run the same number of rounds (256 / G buckets per workgroup and round).
#define MSM_FEW_SMALL 32u
__global__ __launch_bounds__(256) void k_msm_fold_few(MsmP p, const u32* __restrict__ items, G1X29Raw* __restrict__ partials,
                                                      unsigned logG, unsigned m_lo, unsigned m_hi) {
    __shared__ G1X29Raw s_pt[256];
    const size_t col = blockIdx.y;
    const u32* it = items + col * (p.B + 1);
    const unsigned G = 1u << logG, gpw = 256u >> logG;   // lanes per group, groups per workgroup
    const unsigned g = threadIdx.x >> logG, l = threadIdx.x & (G - 1);
    const unsigned per_round = gridDim.x * gpw;
    const u32 rounds = (p.B + per_round - 1) / per_round;
    for (u32 r = 0; r < rounds; ++r) {
        const u32 b = (r * gridDim.x + blockIdx.x) * gpw + g;
        u32 first = 0, m = 0;
        if (b < p.B) {
            first = it[b];
            m = it[b + 1] - first;
            if (m <= m_lo || m > m_hi) m = 0;
        }
        if (!__syncthreads_or(m != 0)) continue;   // nothing to fold in this round (block-uniform)
        G1X29Raw* pc = partials + col * p.max_items + first;
        if (logG == 2) {
            // a quad per bucket: its four lanes walk the partial sums TOGETHER, each addition split over them (ec29_quad.cuh:
            // 4 product latencies per addition instead of 14); the next partial is in flight while the current one is added
            if (m) {
                G1X29 acc = x29_load_raw(pc);
                G1X29 nxt = x29_load_raw(pc + 1);
                for (u32 t = 1; t < m; ++t) {
                    const G1X29 cur = nxt;
                    if (t + 1 < m) nxt = x29_load_raw(pc + t + 1);
                    x29_add_quad(acc, cur);
                }
                if (l == 0) x29_store_raw(pc, acc);
            }
            continue;
        }
        G1X29 acc = x29_inf();
        for (u32 t = l; t < m; t += G) {
            G1X29 o = x29_load_raw(pc + t);
            x29_add(acc, o);
        }
        x29_store_raw(&s_pt[threadIdx.x], acc);
        __syncthreads();
        for (unsigned off = G >> 1; off > 0; off >>= 1) {
            if (l < off && l + off < m) {
                G1X29 a = x29_load_raw(&s_pt[threadIdx.x]);
                G1X29 o = x29_load_raw(&s_pt[threadIdx.x + off]);
                x29_add(a, o);
                x29_store_raw(&s_pt[threadIdx.x], a);
            }
            __syncthreads();
        }
        if (l == 0 && m) x29_store_raw(pc, x29_load_raw(&s_pt[threadIdx.x]));
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_msm_heavy_few(MsmP p, const u32* __restrict__ items, G1X29Raw* __restrict__ partials) {
    __shared__ G1X29Raw s_pt[256];
    __shared__ u32 s_list[256];
    __shared__ u32 s_n;
    const size_t col = blockIdx.y;
    const u32* it = items + col * (p.B + 1);
    for (unsigned b0 = blockIdx.x * 256u; b0 < p.B; b0 += gridDim.x * 256u) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const unsigned bq = b0 + threadIdx.x;
        if (bq < p.B && it[bq + 1] - it[bq] > MSM_MEDIUM) s_list[atomicAdd(&s_n, 1u)] = bq;
        __syncthreads();
        const unsigned nl = s_n;
        for (unsigned k = 0; k < nl; ++k) {
            const u32 b = s_list[k];
            const u32 first = it[b], m = it[b + 1] - first;
            G1X29Raw* pc = partials + col * p.max_items + first;
            G1X29 acc = x29_inf();
            for (u32 t = threadIdx.x; t < m; t += blockDim.x) {
                G1X29 o = x29_load_raw(pc + t);
                x29_add(acc, o);
            }
            x29_store_raw(&s_pt[threadIdx.x], acc);
            __syncthreads();
            for (unsigned off = 128; off > 0; off >>= 1) {
                if (threadIdx.x < off) {
                    G1X29 a = x29_load_raw(&s_pt[threadIdx.x]);
                    G1X29 o = x29_load_raw(&s_pt[threadIdx.x + off]);
                    x29_add(a, o);
                    x29_store_raw(&s_pt[threadIdx.x], a);
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) x29_store_raw(pc, x29_load_raw(&s_pt[0]));
            __syncthreads();
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// sum_b (b+1) * B_b  as a tree of nodes {V = weighted sum with local weights 1.., S = plain sum}
// ------------------------------------------------------------------------------------------------
struct alignas(16) MsmNode {
    G1X29Raw V, S;
};

// level 1: node t covers buckets [t*m, (t+1)*m)
__global__ __launch_bounds__(128) void k_msm_reduce_l1(MsmP p, unsigned m, const u32* __restrict__ items,
                                                       const G1X29Raw* __restrict__ partials, MsmNode* __restrict__ nodes) {
    const size_t col = blockIdx.y;
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned nn = p.B / m;
    if (t >= nn) return;
    const u32* it = items + col * (p.B + 1);
    const G1X29Raw* pc = partials + col * p.max_items;
    G1X29 run = x29_inf(), acc = x29_inf();
    for (unsigned j = m; j-- > 0;) {
        unsigned b = t * m + j;
        u32 a = it[b], z = it[b + 1];
        if (z > a) {  // merged: the bucket's sum sits in its first partial
            G1X29 v = x29_load_raw(pc + a);
            x29_add(run, v);
        }
        x29_add(acc, run);
    }
    MsmNode* o = nodes + col * nn + t;
    x29_store_raw(&o->V, acc);
    x29_store_raw(&o->S, run);
}

// Upper levels with every addition done by a QUAD of lanes (ec29_quad.cuh): a lane-serial combine is a chain of ~50 dependent
// additions of 14 dependent products each on a handful of nodes -- latency-bound -- and a quad's addition is 4 products deep:
// 470 -> 240 us per launch (profiles/r03_ab_tree_quad_vs_lane.txt).  Level 1 stays lane-serial (k_msm_reduce_l1: 8 waves per SIMD
// of nodes, throughput-bound, skips empty buckets: 2.23 ms against 3.48 with quads).  The arms that lost those A/Bs -- quad level 1,
// lane combine, the wave-scan level 1 of north_star's wording -- are kept as source under profiles/probes/r03_retired_arms/.
__global__ __launch_bounds__(256) void k_msm_combine_quad(unsigned n_in, unsigned m, unsigned log_w,
                                                          const MsmNode* __restrict__ in, MsmNode* __restrict__ out) {
    const size_t col = blockIdx.y;
    const unsigned t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const unsigned n_out = n_in / m;
    if (t >= n_out) return;
    const MsmNode* c = in + col * n_in + (size_t)t * m;
    G1X29 run = x29_inf(), acc = x29_inf();
    for (unsigned k = m; k-- > 1;) {
        const G1X29 s = x29_load_raw(&c[k].S);
        x29_add_quad(run, s);
        x29_add_quad(acc, run);
    }
    for (unsigned k = 0; k < log_w; ++k) acc = x29_dbl_quad(acc);
    const G1X29 s0 = x29_load_raw(&c[0].S);
    x29_add_quad(run, s0);
    for (unsigned k = 0; k < m; ++k) {
        const G1X29 v = x29_load_raw(&c[k].V);
        x29_add_quad(acc, v);
    }
    if ((threadIdx.x & 3u) == 0) {
        MsmNode* o = out + col * n_out + t;
        x29_store_raw(&o->V, acc);
        x29_store_raw(&o->S, run);
    }
}

// ------------------------------------------------------------------------------------------------
// The same sum for FEW columns (one large MSM, a single best_multiexp call of the drop-in binding), where the radix-16
// tree above is pure latency: its lanes chain ~50 dependent point additions per level (1.4 ms for one column whatever
// its size).  Bit-sliced instead:  sum_b w_b B_b = sum_j 2^j T_j  with  T_j = sum of the buckets whose weight w_b = b + 1
// has bit j set -- c subset sums, each a fully parallel tree reduction (depth log2 B additions instead of ~150), then
// a pairwise Horner fold of the c slices (depth log2 c).
//   k_msm_slice_partial : block of 256 weights -> its subset sums for the low eight bits + its plain sum (LDS trees)
//   k_msm_slice_reduce  : the blocks' sums of (column, bit j) -> T_j (LDS tree)
//   k_msm_slice_horner  : U = T_0 + 2 T_1, ...; then pairs of pairs with 2, 4, 8 doublings: one workgroup per column
// ------------------------------------------------------------------------------------------------
// sum of the first n entries of s_pt (n a power of two <= 256, 256 threads) into s_pt[0]: pairwise tree, every addition done by a
// QUAD (ec29_quad.cuh) -- 64 additions per round, ~4 product latencies each
__device__ __forceinline__ void lds_tree_sum_quad(G1X29Raw* s_pt, unsigned n) {
    const unsigned quad = threadIdx.x >> 2;
    for (unsigned off = n >> 1; off > 0; off >>= 1) {
        __syncthreads();
        for (unsigned node = quad; node < off; node += 64) {   // the same trip count for the four lanes of a quad
            G1X29 a = x29_load_raw(&s_pt[node]);
            const G1X29 o = x29_load_raw(&s_pt[node + off]);
            x29_add_quad(a, o);
            if ((threadIdx.x & 3u) == 0) x29_store_raw(&s_pt[node], a);
        }
    }
    __syncthreads();
}

// Blocks are cut by WEIGHT, w = 256 blk + t (w = 0 has no bucket; bucket b has weight b + 1), so that the bits of w split
// cleanly: bits 0..7 are bits of t -- within a block exactly half of the t have bit y -- and bits >= 8 are bits of blk -- a
// block is in such a slice with ALL its buckets or with none.  Per block therefore NINE half-size subset sums of 128 leaves:
//   slot y < 8: the block's buckets whose t has bit y;  slot 8: those whose t has bit 7 CLEAR
// (slot 7 + slot 8 = the block's plain sum, which serves every high bit): 9 * 127 additions instead of 16 * 255, and with
// 18 KB of LDS per workgroup all blocks x slots of a column are resident at once (one round instead of 1161 / 1024).
#define SLICE_SLOTS 9u
__global__ __launch_bounds__(256) void k_msm_slice_partial(MsmP p, const u32* __restrict__ items,
                                                           const G1X29Raw* __restrict__ partials, unsigned nblk,
                                                           G1X29Raw* __restrict__ slice_part) {
    __shared__ G1X29Raw s_pt[128];
    const size_t col = blockIdx.z;
    const unsigned y = blockIdx.y, blk = blockIdx.x;
    const u32* it = items + col * (p.B + 1);
    if (threadIdx.x < 128) {
        const unsigned i = threadIdx.x, yy = y < 8 ? y : 7u;
        // the i-th t with bit yy set (slots 0..7) or clear (slot 8)
        const unsigned t = ((i >> yy) << (yy + 1)) | (y < 8 ? (1u << yy) : 0u) | (i & ((1u << yy) - 1u));
        const unsigned w = blk * 256u + t;
        G1X29 v = x29_inf();
        if (w >= 1 && w <= p.B) {
            const u32 a = it[w - 1], z = it[w];
            if (z > a) v = x29_load_raw(partials + col * p.max_items + a);
        }
        x29_store_raw(&s_pt[i], v);
    }
    lds_tree_sum_quad(s_pt, 128);
    if (threadIdx.x == 0) slice_part[(col * SLICE_SLOTS + y) * nblk + blk] = s_pt[0];
}

// T_j of one column: bit j < 8 -> the blocks' slot-j sums; bit j >= 8 -> slots 7 and 8 (together a block's plain sum) of the
// blocks whose index has bit j - 8: at most 2 * 64 values for B <= 2^15, a tree of 128
__global__ __launch_bounds__(256) void k_msm_slice_reduce(MsmP p, unsigned nblk, const G1X29Raw* __restrict__ slice_part,
                                                          G1X29Raw* __restrict__ slices) {
    __shared__ G1X29Raw s_pt[256];
    const size_t col = blockIdx.y;
    const unsigned j = blockIdx.x;
    const G1X29Raw* base = slice_part + col * SLICE_SLOTS * (size_t)nblk;
    G1X29 acc = x29_inf();
    unsigned count;
    if (j < 8) {
        count = nblk;
        for (unsigned t = threadIdx.x; t < nblk; t += 256) {
            G1X29 o = x29_load_raw(base + (size_t)j * nblk + t);
            x29_add(acc, o);
        }
    } else {
        const unsigned s_ = j - 8;
        // blocks with bit s_ of their index: the k-th is k with a one inserted at bit s_; two values (slots 7, 8) per block
        const unsigned n_sel = (nblk + (1u << s_)) >> (s_ + 1) << s_;   // upper bound on such blocks below nblk (exact or + partial run)
        count = 2 * n_sel;
        for (unsigned t = threadIdx.x; t < count; t += 256) {
            const unsigned k = t >> 1;
            const unsigned blk = ((k >> s_) << (s_ + 1)) | (1u << s_) | (k & ((1u << s_) - 1u));
            if (blk < nblk) {
                G1X29 o = x29_load_raw(base + (size_t)(7 + (t & 1u)) * nblk + blk);
                x29_add(acc, o);
            }
        }
    }
    x29_store_raw(&s_pt[threadIdx.x], acc);
    unsigned n = 1;
    while (n < count && n < 256) n <<= 1;   // only the levels that hold something
    lds_tree_sum_quad(s_pt, n);
    if (threadIdx.x == 0) slices[col * 16 + j] = s_pt[0];
}

// sum_j 2^j T_j for c <= 16 slices: four pairwise levels, level l combining neighbours with 2^l doublings; every pair is a quad's
__global__ __launch_bounds__(64) void k_msm_slice_horner(MsmP p, const G1X29Raw* __restrict__ slices, G1Jac* __restrict__ out) {
    __shared__ G1X29Raw s_pt[16];
    const size_t col = blockIdx.x;
    if (threadIdx.x < 16) {
        G1X29 v = threadIdx.x < p.c ? x29_load_raw(slices + col * 16 + threadIdx.x) : x29_inf();
        x29_store_raw(&s_pt[threadIdx.x], v);
    }
    const unsigned quad = threadIdx.x >> 2;
    for (unsigned l = 0; l < 4; ++l) {
        __syncthreads();
        const unsigned stride = 1u << l;
        if (quad < (8u >> l)) {
            const unsigned i = quad * 2 * stride;
            G1X29 hi = x29_load_raw(&s_pt[i + stride]);
            for (unsigned k = 0; k < stride; ++k) hi = x29_dbl_quad(hi);
            G1X29 lo = x29_load_raw(&s_pt[i]);
            x29_add_quad(lo, hi);
            if ((threadIdx.x & 3u) == 0) x29_store_raw(&s_pt[i], lo);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) x29_store_jac(out + col, x29_load_raw(&s_pt[0]));
}

__global__ void k_msm_emit(const MsmNode* __restrict__ nodes, size_t n_cols, G1Jac* __restrict__ out) {
    size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n_cols) return;
    x29_store_jac(out + col, x29_load_raw(&nodes[col].V));
}

// small utilities -------------------------------------------------------------------------------
__global__ void k_g1_sum(const G1Jac* __restrict__ in, size_t n, G1Jac* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    G1X29 acc = x29_inf();
    for (size_t i = 0; i < n; ++i) {
        G1X29 x = x29_load_jac(in + i);
        x29_add(acc, x);
    }
    x29_store_jac(out, acc);
}

__global__ void k_g1_normalize(const G1Jac* __restrict__ in, size_t n, G1Aff64* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A29 a = x29_to_affine(x29_load_jac(in + i));
    if (!a29_is_inf(a)) {   // back to the ABI's 256-domain
        a.x = f29_to_256(a.x);
        a.y = f29_to_256(a.y);
    }
    a29_store64(out + i, a);
}

// out[i] = [k_i] G, G = (1, 2); plain double-and-add over the canonical scalar bits
__global__ __launch_bounds__(128) void k_fixed_base_mul(const Fr* __restrict__ scalars, size_t n,
                                                        G1Aff64* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr k = fp_from_mont(fp_load<FrTag>(scalars + i));
    G1A29 g;
    g.x = f29_one<FqTag>();
    g.y = f29_canon<1>(f29_dbl(g.x));
    G1X29 acc = x29_inf();
    for (int bit = 253; bit >= 0; --bit) {
        acc = x29_dbl(acc);
        u32 w = sel8(k.v, (unsigned)bit >> 5);
        if ((w >> (bit & 31)) & 1) x29_add_affine(acc, g);
    }
    G1A29 a = x29_to_affine(acc);
    if (!a29_is_inf(a)) {
        a.x = f29_to_256(a.x);
        a.y = f29_to_256(a.y);
    }
    a29_store64(out + i, a);
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static size_t pz_msm_ws_gib() {
    static size_t v = 0;
    if (!v) {
        const char* e = getenv("PZ_MSM_WS_GIB");
        long g = e ? atol(e) : 48;
        v = g < 1 ? 1 : (size_t)g;
    }
    return v;
}

static unsigned default_window_bits(size_t n) {
    if (n <= 1u << 8) return 9;
    if (n <= 1u << 11) return 11;
    if (n <= 1u << 14) return 13;
    return 16;
}

extern "C" int pz_bases_load_g1(pz_ctx* ctx, const uint64_t* bases_affine, size_t n_points, int on_device,
                                uint32_t window_bits, pz_bases** out) {
    if (!ctx || !out || !bases_affine || n_points == 0) return PZ_ERR_INVALID;
    *out = nullptr;
    unsigned c = window_bits ? window_bits : default_window_bits(n_points);
    if (c < 4 || c > 16) return PZ_ERR_INVALID;
    unsigned nwin = 253 / c + 1;
    if ((uint64_t)nwin * n_points >= (1ull << 31)) return PZ_ERR_UNSUPPORTED;
    PZ_ENTER(ctx);
    pz_bases* b = new pz_bases();
    b->n = n_points;
    b->c = c;
    b->nwin = nwin;
    b->device = ctx->device;
    hipError_t e = pz_hip_malloc(ctx, &b->d_table, (size_t)nwin * n_points * 64);
    if (e != hipSuccess) {
        delete b;
        return pz_hip_fail(ctx, e, "hipMalloc(table)");
    }
    const void* d_src = bases_affine;
    if (!on_device) {
        void* stage;
        int rc = pz_ws_get(ctx, WS_IO_A, n_points * 64, &stage);
        if (rc != PZ_OK) { (void)pz_hip_free(b->d_table); delete b; return rc; }
        e = hipMemcpyAsync(stage, bases_affine, n_points * 64, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { (void)pz_hip_free(b->d_table); delete b; return pz_hip_fail(ctx, e, "memcpy bases"); }
        d_src = stage;
    }
    hipLaunchKernelGGL(k_build_table, dim3(pz_div_up(n_points, 128)), dim3(128), 0, ctx->stream,
                       (const G1Aff64*)d_src, (G1Aff64*)b->d_table, n_points, c, nwin);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)pz_hip_free(b->d_table); delete b; return pz_hip_fail(ctx, e, "k_build_table"); }
    *out = b;
    return PZ_OK;
}

extern "C" int pz_srs_load_g1(pz_ctx* ctx, uint32_t k, const uint64_t* bases_affine, int lagrange, pz_bases** out) {
    if (k > 26) return PZ_ERR_INVALID;
    int rc = pz_bases_load_g1(ctx, bases_affine, (size_t)1 << k, 0, 0, out);
    if (rc == PZ_OK) (*out)->lagrange = lagrange;
    return rc;
}

extern "C" int pz_bases_free(pz_ctx* ctx, pz_bases* b) {
    if (!b) return PZ_OK;
    if (ctx) {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (b->d_table) (void)pz_hip_free(b->d_table);
    delete b;
    return PZ_OK;
}

extern "C" int pz_bases_info(const pz_bases* b, size_t* n_points, uint32_t* window_bits, uint32_t* n_windows) {
    if (!b) return PZ_ERR_INVALID;
    if (n_points) *n_points = b->n;
    if (window_bits) *window_bits = b->c;
    if (n_windows) *n_windows = b->nwin;
    return PZ_OK;
}

// Work items are handed to lanes in chunk-size order, so a wave's lanes run equal trip counts whatever the
// chunk bound is; the bound only has to leave enough items to fill the chip (>= ~2^18 lanes per launch)
// and keep a single skewed bucket from serialising.  Larger chunks mean fewer partial sums to write and fold.
static unsigned msm_chunk_for(size_t n_cols, size_t digits_per_col, unsigned window_bits) {
    static int env = -1;
    if (env < 0) {
        const char* e = getenv("PZ_MSM_CHUNK");
        env = e ? atoi(e) : 0;
    }
    if (env >= (int)MSM_CHUNK_MIN && env <= (int)MSM_CHUNK_MAX) return (unsigned)env;
    if (n_cols <= MSM_SLICE_MAX_COLS) {
        // one large MSM (or a rank's share of it): every bucket holds many entries, and the chunk trades the accumulation's load
        // balance (flat below a knee, rising above it) against the partial sums the folds must add up (falling with the chunk).
        // Measured optimum ([r4], bench.py --workload msm22 --emulate-world 8 with PZ_MSM_CHUNK): 96 at 2048 entries per bucket (one
        // 2^22-point MSM: 6.33 ms against 6.93 with the 2^18-lane rule's 256), 24-28 at 256 per bucket (a 2^19-point share: 1.00 ms
        // against 1.01) -- chunk = 0.79 * (entries per bucket)^0.63 passes through both
        const double per_bucket = (double)digits_per_col / (double)((size_t)1 << (window_bits - 1));
        double ch = 0.79 * pow(per_bucket, 0.63);
        // in steps of 32 (16 below 24): the window split's shares measured 15 % slower at 24 / 26 than at 32
        unsigned c32 = ch < 24.0 ? MSM_CHUNK_MIN : 32u * (unsigned)((ch + 16.0) / 32.0);
        if (c32 > MSM_CHUNK_MAX) c32 = MSM_CHUNK_MAX;
        return c32;
    }
    const size_t want = (n_cols * digits_per_col) >> 18;   // >= 2^18 lanes: four waves per SIMD
    unsigned chunk = MSM_CHUNK_MIN;
    while (chunk < MSM_CHUNK_MAX && chunk * 2 <= want) chunk *= 2;
    return chunk;
}

// Scalars per thread of the sort passes.  A slice costs its workgroup ~0.4 MB of fixed traffic (zeroing / loading / storing
// the 2^15 bucket counters), so slices are as large as SORT_PER_THREAD allows -- unless that leaves too few workgroups: a single
// 2^19-point column in 64 slices kept 3/4 of the chip idle through both passes.  How few is too few was measured on that
// column (a rank's share of c4; hist + totals + scatter): 512 workgroups 206 us, 256: 178, 128: 163 -- the fixed traffic of the
// extra slices costs more than the idle CUs.  Column batches have thousands of slices either way.
static unsigned msm_spt_for(size_t n_cols, size_t n) {
    const size_t min_wg = n_cols <= MSM_SLICE_MAX_COLS ? 128 : 512;
    unsigned spt = SORT_PER_THREAD;
    while (spt > 1 && n_cols * pz_div_up(n, (size_t)SORT_THREADS * spt) < min_wg) spt >>= 1;
    return spt;
}

// ... of a column batch the caller declared SPARSE (pz_msm_g1_dev_ex: witness-like columns of short scalars).  Such a column
// leaves ~24 000 entries, so the fixed traffic above IS the sort (640 KB of counters against 512 KB of
// scalars per 8192-scalar slice), and the single-pass scatter's write frontier, which made larger slices slower on full-width
// columns, is short.  A slice grows up to MSM_SPARSE_SLICE scalars (PZ_MSM_SPARSE_SLICE overrides, for the A/B) -- the whole
// column where it fits: then k_msm_totals is not launched at all -- while the launch keeps the 512 workgroups of msm_spt_for.
// Measured on the 3034 advice columns of a c2 proof (profiles/sparse_sort_slice_ab.txt; hist .. scatter): 8192: 21.3 ms,
// 32768: 17.9, the whole column of 2^17: 18.0 (device-chosen scatter and 8192, the launches without a hint: 23.7) -- beyond
// 32768 the bookkeeping saved is small against a workgroup that walks 128 scalars per thread with four waves per SIMD.
#ifndef MSM_SPARSE_SLICE
#define MSM_SPARSE_SLICE (1u << 15)
#endif
static unsigned msm_spt_sparse(size_t n_cols, size_t n) {
    static long env = -1;
    if (env < 0) {
        const char* e = getenv("PZ_MSM_SPARSE_SLICE");
        env = e ? atol(e) : 0;
    }
    const size_t slice = env >= (long)SORT_SLICE && env <= (1l << 24) ? (size_t)env : (size_t)MSM_SPARSE_SLICE;
    unsigned spt = SORT_PER_THREAD;
    while ((size_t)SORT_THREADS * spt * 2 <= slice && (size_t)SORT_THREADS * spt < n) spt <<= 1;   // no larger than the column needs
    while (spt > 1 && n_cols * pz_div_up(n, (size_t)SORT_THREADS * spt) < 512) spt >>= 1;
    return spt;
}

static int msm_group(pz_ctx* ctx, const pz_bases* bases, const Fr* d_scalars, size_t nc, size_t n, size_t cs,
                     unsigned win_lo, unsigned win_hi, unsigned chunk, int density, G1Jac* d_out) {
    MsmP p;
    p.n = n;
    p.n_table = bases->n;
    p.c = bases->c;
    p.nwin = bases->nwin;
    p.win_lo = win_lo;
    p.win_hi = win_hi;
    p.B = 1u << (bases->c - 1);
    p.cap = n * (size_t)(win_hi - win_lo);
    p.chunk = chunk;
    if (p.B + n * (size_t)(win_hi - win_lo) / chunk > 65535u * 256u) return PZ_ERR_CAPACITY;  // grid.y of k_msm_accumulate
    p.max_items = p.B + p.cap / chunk;
    void *hist, *offs, *heavy, *items, *entries, *partials, *na, *nb, *totals, *fold, *iord;
    // PZ_MSM_SCATTER=one / two force the single-pass / the two-step scatter (A/B); default: chosen on the device per launch
    static int scatter_mode = -1;   // 0 auto, 1 one, 2 two
    if (scatter_mode < 0) {
        const char* e = getenv("PZ_MSM_SCATTER");
        scatter_mode = (e && !strcmp(e, "one")) ? 1 : (e && !strcmp(e, "two")) ? 2 : 0;
    }
    // the caller's density hint (pz_msm_g1_dev_ex) picks launches and slice sizes of a COLUMN BATCH, never results: either scatter
    // sorts any column, a wrong hint only costs time.  The few-column path and a forced variant (above) ignore it.
    const bool batch = nc > MSM_SLICE_MAX_COLS;
    const bool hint_sparse = batch && scatter_mode == 0 && density == PZ_MSM_SPARSE;
    const bool hint_dense = batch && scatter_mode == 0 && density == PZ_MSM_DENSE;
    p.spt = hint_sparse ? msm_spt_sparse(nc, n) : msm_spt_for(nc, n);
    const unsigned n_slices = pz_div_up(n, (size_t)SORT_THREADS * p.spt);
    // a sparse column in ONE slice: its histogram is the column's totals and every slice offset is zero -- no k_msm_totals
    const bool one_slice = hint_sparse && n_slices == 1;
    PZCHK(pz_ws_get(ctx, WS_HIST, nc * (size_t)n_slices * p.B * 4, &hist));
    PZCHK(pz_ws_get(ctx, WS_CURSOR, nc * (size_t)(p.B + 1) * 4, &heavy));
    // few columns: k_msm_totals_few / k_msm_items_few instead of k_msm_totals / k_msm_scan (one workgroup per column)
    const bool split_items = nc <= MSM_SLICE_MAX_COLS;
    const unsigned nblk_few = pz_div_up(p.B, 256);
    // bucket totals | (few columns) per 256-bucket block: entry sums, item sums, items by chunk size
    PZCHK(pz_ws_get(ctx, WS_TOTALS, nc * ((size_t)p.B + (split_items ? (size_t)nblk_few * (2 + FEW_BINS) : 0)) * 4, &totals));
    u32* blk_cnt = (u32*)totals + nc * (size_t)p.B;
    u32* blk_itm = blk_cnt + nc * (size_t)nblk_few;
    u32* blk_bins = blk_itm + nc * (size_t)nblk_few;
    u32* heavy_cnt = (u32*)heavy + nc * (size_t)p.B;
    PZCHK(pz_ws_get(ctx, WS_MISC, nc * (size_t)(p.B + 1) * 4, &fold));
    u32* fold_cnt = (u32*)fold + nc * (size_t)p.B;
    PZCHK(pz_ws_get(ctx, WS_ORDER, nc * p.max_items * 8, &iord));
    u32* item_order = (u32*)iord;
    u32* item_bucket = (u32*)iord + nc * p.max_items;
    PZCHK(pz_ws_get(ctx, WS_OFFS, nc * (p.B + 1) * 4, &offs));
    PZCHK(pz_ws_get(ctx, WS_ITEMS, nc * (p.B + 1) * 4, &items));
    PZCHK(pz_ws_get(ctx, WS_ENTRIES, nc * p.cap * 4 + 16, &entries));
    // the staged entry holds a 24-bit table index; a few columns have too few slices for the 256-thread coarse step (a rank's
    // 2^19-point share of c4: 110 + 41 us against 111 for the single pass) unless forced
    const bool two_pass = scatter_mode != 1 && !hint_sparse && p.c == 16 && (size_t)p.nwin * p.n_table <= ((size_t)1 << 24) &&
                          (nc > MSM_SLICE_MAX_COLS || scatter_mode == 2);
    {
        const size_t part_bytes = nc * p.max_items * sizeof(G1X29Raw), stage_bytes = two_pass ? nc * p.cap * 4 + 16 : 0;
        PZCHK(pz_ws_get(ctx, WS_PARTIALS, part_bytes > stage_bytes ? part_bytes : stage_bytes, &partials));
    }
    // radix of the reduction tree
    const unsigned m1 = p.B >= 16 ? 16 : p.B;
    unsigned n_nodes = p.B / m1;
    PZCHK(pz_ws_get(ctx, WS_NODES_A, nc * (size_t)n_nodes * sizeof(MsmNode), &na));
    PZCHK(pz_ws_get(ctx, WS_NODES_B, nc * (size_t)(n_nodes / 2 + 1) * sizeof(MsmNode), &nb));
    hipStream_t st = ctx->stream;
    pz_timer tall(ctx, PZ_T_MSM_ALL);
    dim3 gs(sort_grid(n_slices, nc));
    void* dsel;
    PZCHK(pz_ws_get(ctx, WS_SEL, 8, &dsel));
    HIPCHK(ctx, hipMemsetAsync(dsel, 0, 8, st));
    PZCHK(pz_async_err_init(ctx));
    {
        pz_timer tsort(ctx, PZ_T_MSM_SORT);
        hipLaunchKernelGGL(k_msm_hist, gs, dim3(SORT_THREADS), 0, st, d_scalars, cs, p, (u32*)hist, n_slices, nc);
        if (split_items) {
            // few columns: offsets, item counts and the size-ordered list from two bucket-parallel kernels (no single-workgroup scan)
            hipLaunchKernelGGL(k_msm_totals_few, dim3(nblk_few, (unsigned)nc), dim3(256), 0, st, (u32*)hist, n_slices, p, (u32*)totals,
                               blk_cnt, blk_itm, blk_bins);
            hipLaunchKernelGGL(k_msm_items_few, dim3(nblk_few, (unsigned)nc), dim3(256), 0, st, p, (const u32*)totals, (const u32*)blk_cnt,
                               (const u32*)blk_itm, (const u32*)blk_bins, (u32*)offs, (u32*)items, item_order, item_bucket,
                               (unsigned long long*)dsel);
        } else {
            if (!one_slice)
                hipLaunchKernelGGL(k_msm_totals, dim3(pz_div_up(p.B, 256), (unsigned)nc), dim3(256), 0, st, (u32*)hist, n_slices, p,
                                   (u32*)totals);
            hipLaunchKernelGGL(k_msm_scan, dim3((unsigned)nc), dim3(SCAN_THREADS), 0, st, (const u32*)(one_slice ? hist : totals), p,
                               (u32*)offs, (u32*)items, (u32*)heavy, heavy_cnt, (u32*)fold, fold_cnt, item_order, item_bucket,
                               (unsigned long long*)dsel);
        }
        // dense launch (>= 0.4 of the digits non-zero: full-width scalars) -> two-step; sparse (witness columns) -> single pass.
        // With a hint only the hinted variant is queued, and thr makes it take the launch whatever the digit total is.
        ScatterSel sel;
        sel.total = (const unsigned long long*)dsel;
        sel.thr = !two_pass ? ~0ull : (scatter_mode == 2 || hint_dense) ? 0ull : (unsigned long long)(0.4 * (double)nc * (double)p.cap);
        sel.err = ctx->async_err_d;
        if (two_pass) {
            // the staging list lives in the partial sums' buffer: k_msm_accumulate writes those after the list is consumed
            hipLaunchKernelGGL(k_msm_scatter_coarse, gs, dim3(COARSE_THREADS), 0, st, d_scalars, cs, p, (const u32*)hist, n_slices,
                               (const u32*)offs, (u32*)partials, nc, sel);
            hipLaunchKernelGGL(k_msm_scatter_fine, dim3(p.B >> SORT_FINE_LOG, (unsigned)nc), dim3(FINE_THREADS), 0, st, p, (const u32*)offs,
                               (const u32*)partials, (u32*)entries, sel);
        }
        if (!two_pass || (scatter_mode != 2 && !hint_dense))
            hipLaunchKernelGGL(k_msm_scatter, gs, dim3(SORT_THREADS), 0, st, d_scalars, cs, p, one_slice ? (const u32*)nullptr : (const u32*)hist,
                               n_slices, (const u32*)offs, (u32*)entries, nc, sel);
    }
    {
        pz_timer tacc(ctx, PZ_T_MSM_ACC);
        hipLaunchKernelGGL(k_msm_accumulate, dim3((unsigned)nc, pz_div_up(p.max_items, 256)), dim3(256), 0, st,
                           (const G1Aff64*)bases->d_table, p, (const u32*)offs, (const u32*)items,
                           (const u32*)item_order, (const u32*)item_bucket, (const u32*)entries, (G1X29Raw*)partials);
    }
    pz_timer ttree(ctx, PZ_T_MSM_TREE);
    if (split_items) {
        // 4-lane groups: 64 buckets per workgroup; 32-lane groups: 8 per workgroup and round (rounds without work cost one barrier)
        const unsigned gx4 = pz_div_up(p.B, 64), gx32 = p.B / 8 < 2048u ? (p.B / 8 ? p.B / 8 : 1u) : 2048u;
        hipLaunchKernelGGL(k_msm_fold_few, dim3(gx4, (unsigned)nc), dim3(256), 0, st, p, (const u32*)items, (G1X29Raw*)partials, 2u, 1u, MSM_FEW_SMALL);
        hipLaunchKernelGGL(k_msm_fold_few, dim3(gx32, (unsigned)nc), dim3(256), 0, st, p, (const u32*)items, (G1X29Raw*)partials, 5u, MSM_FEW_SMALL,
                           MSM_MEDIUM);
        hipLaunchKernelGGL(k_msm_heavy_few, dim3(p.B / 256 < 64u ? (p.B / 256 ? p.B / 256 : 1u) : 64u, (unsigned)nc), dim3(256), 0, st, p,
                           (const u32*)items, (G1X29Raw*)partials);
    } else {
    hipLaunchKernelGGL(k_msm_bucket_sum, dim3((unsigned)nc, pz_div_up(p.B, 256)), dim3(256), 0, st, p, (const u32*)items,
                       (const u32*)fold, (const u32*)fold_cnt, (G1X29Raw*)partials);
    // heavy buckets are few per column in a column batch, but a single large MSM makes every bucket heavy:
    // size grid.x so the launch has ~8k workgroups either way (workgroups beyond the list exit at once)
    unsigned hx = (unsigned)(8192 / nc);
    if (hx < 4) hx = 4;   // column batches have a handful of heavy buckets per column at most; empty blocks still cost ~50 ns
    if (hx > p.B) hx = p.B;
    hipLaunchKernelGGL(k_msm_heavy_sum, dim3(hx, (unsigned)nc), dim3(256), 0, st, p, (const u32*)items, (const u32*)heavy,
                       (const u32*)heavy_cnt, (G1X29Raw*)partials);
    hipLaunchKernelGGL(k_msm_medium_sum, dim3(hx, (unsigned)nc), dim3(256), 0, st, p, (const u32*)items, (const u32*)heavy,
                       (const u32*)heavy_cnt, (G1X29Raw*)partials);
    }
    if (nc <= MSM_SLICE_MAX_COLS) {
        // few columns: bit-sliced parallel reduction (depth ~ log2 B + log2 c point additions)
        const unsigned nblk = (p.B >> 8) + 1;   // blocks by weight: w = 256 blk + t, 1 <= w <= B
        void *sp, *sl;
        PZCHK(pz_ws_get(ctx, WS_NODES_A, nc * (size_t)SLICE_SLOTS * nblk * sizeof(G1X29Raw), &sp));
        PZCHK(pz_ws_get(ctx, WS_NODES_B, nc * 16 * sizeof(G1X29Raw), &sl));
        hipLaunchKernelGGL(k_msm_slice_partial, dim3(nblk, SLICE_SLOTS, (unsigned)nc), dim3(256), 0, st, p, (const u32*)items,
                           (const G1X29Raw*)partials, nblk, (G1X29Raw*)sp);
        hipLaunchKernelGGL(k_msm_slice_reduce, dim3(p.c, (unsigned)nc), dim3(256), 0, st, p, nblk, (const G1X29Raw*)sp, (G1X29Raw*)sl);
        hipLaunchKernelGGL(k_msm_slice_horner, dim3((unsigned)nc), dim3(64), 0, st, p, (const G1X29Raw*)sl, d_out);
        HIPCHK(ctx, hipGetLastError());
        return PZ_OK;
    }
    hipLaunchKernelGGL(k_msm_reduce_l1, dim3(pz_div_up(n_nodes, 128), (unsigned)nc), dim3(128), 0, st, p, m1,
                       (const u32*)items, (const G1X29Raw*)partials, (MsmNode*)na);
    const unsigned m1_used = m1;
    MsmNode* cur = (MsmNode*)na;
    MsmNode* nxt = (MsmNode*)nb;
    unsigned log_w = 0;
    for (unsigned t = m1_used; t > 1; t >>= 1) ++log_w;
    while (n_nodes > 1) {
        unsigned m = n_nodes >= 16 ? 16 : n_nodes;
        hipLaunchKernelGGL(k_msm_combine_quad, dim3(pz_div_up((size_t)(n_nodes / m) * 4, 256), (unsigned)nc), dim3(256), 0, st, n_nodes, m,
                           log_w, (const MsmNode*)cur, nxt);
        n_nodes /= m;
        for (unsigned t = m; t > 1; t >>= 1) ++log_w;
        MsmNode* tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    hipLaunchKernelGGL(k_msm_emit, dim3(pz_div_up(nc, 64)), dim3(64), 0, st, (const MsmNode*)cur, nc, d_out);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_msm_g1_dev(pz_ctx* ctx, const pz_bases* bases, const uint64_t* d_scalars, size_t n_cols, size_t n,
                             size_t col_stride, uint32_t win_lo, uint32_t win_hi, uint64_t* d_out_jac) {
    return pz_msm_g1_dev_ex(ctx, bases, d_scalars, n_cols, n, col_stride, win_lo, win_hi, PZ_MSM_AUTO, d_out_jac);
}

extern "C" int pz_msm_g1_dev_ex(pz_ctx* ctx, const pz_bases* bases, const uint64_t* d_scalars, size_t n_cols, size_t n,
                                size_t col_stride, uint32_t win_lo, uint32_t win_hi, int density, uint64_t* d_out_jac) {
    if (!ctx || !bases || (n_cols && (!d_scalars || !d_out_jac))) return PZ_ERR_INVALID;
    if (density != PZ_MSM_AUTO && density != PZ_MSM_SPARSE && density != PZ_MSM_DENSE) return PZ_ERR_INVALID;
    if (n > bases->n || win_lo > win_hi || win_hi > bases->nwin) return PZ_ERR_INVALID;
    if (col_stride % 4 || (n_cols > 1 && col_stride < 4 * n)) return PZ_ERR_INVALID;
    if (n_cols == 0) return PZ_OK;
    PZ_ENTER(ctx);
    if (n == 0 || win_lo == win_hi) {
        // empty sum: identity for every column
        size_t nn = n_cols;
        void* z;
        PZCHK(pz_ws_get(ctx, WS_NODES_A, nn * sizeof(MsmNode), &z));
        HIPCHK(ctx, hipMemsetAsync(z, 0, nn * sizeof(MsmNode), ctx->stream));  // ZZ = 0 -> identity
        hipLaunchKernelGGL(k_msm_emit, dim3(pz_div_up(nn, 64)), dim3(64), 0, ctx->stream, (const MsmNode*)z, nn,
                           (G1Jac*)d_out_jac);
        HIPCHK(ctx, hipGetLastError());
        return PZ_OK;
    }
    const size_t cs = col_stride / 4;
    // column groups: bound the sorted-entry workspace (4 B per digit) to ~1 GiB, grid.y to 65535
    const size_t digits = n * (size_t)(win_hi - win_lo);
    const unsigned chunk = msm_chunk_for(n_cols, digits, bases->c);
    const size_t part_col = (digits / chunk) * sizeof(G1X29Raw);   // shared with the two-pass scatter's staging list (4 B per digit)
    size_t per_col = digits * 4 + (part_col > digits * 4 ? part_col : digits * 4) + (digits / chunk) * 8 +
                     (size_t)(1u << (bases->c - 1)) * (180 + 4 * (size_t)pz_div_up(n, (size_t)SORT_THREADS * msm_spt_for(1, n)));   // spt of the smallest group (a halved group recomputes it): an upper bound on the slices
    // group size: sized for 288 GB of HBM -- by default up to 48 GiB of sort / partial-sum workspace per launch
    // sequence (PZ_MSM_WS_GIB overrides), so the latency-bound tree levels are paid once per ~2000 columns
    size_t ws_budget = pz_msm_ws_gib() << 30;
    {
        // never plan for more than half of what is free (plus what this context already holds).  The query is cached: between
        // two launch sequences it left the GPU idle for ~0.3 ms
        if (ctx->mem_avail == 0 || ++ctx->mem_avail_age >= 64) {
            const size_t free_b = pz_mem_free_bytes(ctx);   // (the driver's figure + the free part of the context's arena)
            if (free_b) {
                size_t held = 0;
                for (int i = 0; i < WS_COUNT; ++i) held += ctx->ws[i].cap;
                ctx->mem_avail = (free_b + held) / 2;
                ctx->mem_avail_age = 0;
            }
        }
        if (ctx->mem_avail && ws_budget > ctx->mem_avail) ws_budget = ctx->mem_avail;
    }
    size_t group = ws_budget / per_col;
    if (group == 0) group = 1;
    if (group > n_cols) group = n_cols;
    if (group > 4096) group = 4096;
    if (density == PZ_MSM_SPARSE && group > MSM_SLICE_MAX_COLS) {
        // a sparse batch has no staging list and the slices msm_spt_sparse gives a group of this size (a larger group has no
        // more of them per column): size the group again from that.  A smaller last group may hold more slices per column, by
        // the 512-workgroup rule at most ~1024 histograms (128 MB) in all.
        const size_t slices = pz_div_up(n, (size_t)SORT_THREADS * msm_spt_sparse(group, n));
        per_col = digits * 4 + part_col + (digits / chunk) * 8 + (size_t)(1u << (bases->c - 1)) * (180 + 4 * slices);
        group = ws_budget / per_col;
        if (group > n_cols) group = n_cols;
        if (group > 4096) group = 4096;
    }
    for (size_t c0 = 0; c0 < n_cols;) {
        const size_t nc = n_cols - c0 < group ? n_cols - c0 : group;
        const int rc = msm_group(ctx, bases, (const Fr*)d_scalars + c0 * cs, nc, n, cs, win_lo, win_hi, chunk, density, (G1Jac*)d_out_jac + c0);
        if (rc == PZ_ERR_OOM && group > 1) {
            // the cached free-memory figure was stale (someone else allocated since): halve the group, ask again next call
            ctx->mem_avail = 0;
            (void)hipGetLastError();
            group = (group + 1) / 2;
            continue;
        }
        PZCHK(rc);
        c0 += nc;
    }
    return PZ_OK;
}

extern "C" int pz_msm_g1_batch(pz_ctx* ctx, const pz_bases* bases, const uint64_t* const* scalar_cols, size_t n_cols,
                               size_t n, uint64_t* out_jac) {
    if (!ctx || !bases || (n_cols && (!scalar_cols || !out_jac))) return PZ_ERR_INVALID;
    if (n > bases->n) return PZ_ERR_INVALID;
    if (n_cols == 0) return PZ_OK;
    PZ_ENTER(ctx);
    const size_t bytes = n * 32;
    for (size_t j = 0; j < n_cols; ++j)
        if (!scalar_cols[j] && n) return PZ_ERR_INVALID;
    // column groups through two staging buffers: the upload of group g+1 (io_h2d) runs under the kernels of group g.  Group
    // sizes ramp up 128 MiB, 256 MiB, ... to 1 GiB: only the first, small upload is exposed, and the later launch sequences
    // are wide enough (256 columns at 2^17) for the reduction tree's fixed latency to vanish
    const size_t g_min = bytes ? (((size_t)1 << 27) / bytes ? ((size_t)1 << 27) / bytes : 1) : n_cols;
    size_t g_max = bytes ? (((size_t)1 << 30) / bytes ? ((size_t)1 << 30) / bytes : 1) : n_cols;
    if (g_max > n_cols) g_max = n_cols;
    void *d_s, *d_o;
    PZCHK(pz_ws_get(ctx, WS_IO_B, 2 * g_max * bytes + 32, &d_s));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n_cols * 96, &d_o));
    PZCHK(pz_io_init(ctx));
    hipEvent_t* ev_in = ctx->io_ev;        // [2] group uploaded
    hipEvent_t* ev_done = ctx->io_ev + 2;  // [2] group consumed by its kernels
    int rc = PZ_OK;
    size_t g = 0, group = g_min < g_max ? g_min : g_max;
    for (size_t c0 = 0; c0 < n_cols && rc == PZ_OK; ++g) {
        const size_t nc = n_cols - c0 < group ? n_cols - c0 : group;
        const unsigned b = (unsigned)(g & 1);
        char* buf = (char*)d_s + b * g_max * bytes;
        hipError_t e = hipSuccess;
        if (g >= 2) e = hipStreamWaitEvent(ctx->io_h2d, ev_done[b], 0);
        for (size_t j = 0; j < nc && e == hipSuccess && bytes; ++j)
            e = hipMemcpyAsync(buf + j * bytes, scalar_cols[c0 + j], bytes, hipMemcpyHostToDevice, ctx->io_h2d);
        if (e == hipSuccess) e = hipEventRecord(ev_in[b], ctx->io_h2d);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ev_in[b], 0);
        if (e != hipSuccess) { rc = pz_hip_fail(ctx, e, "pz_msm_g1_batch: upload"); break; }
        rc = pz_msm_g1_dev(ctx, bases, (const uint64_t*)buf, nc, n, 4 * n, 0, bases->nwin, (uint64_t*)d_o + c0 * 12);
        if (rc == PZ_OK && (e = hipEventRecord(ev_done[b], ctx->stream)) != hipSuccess) rc = pz_hip_fail(ctx, e, "pz_msm_g1_batch: event");
        c0 += nc;
        group = group * 2 < g_max ? group * 2 : g_max;
    }
    if (rc == PZ_OK) {
        hipError_t e = hipMemcpyAsync(out_jac, d_o, n_cols * 96, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = pz_hip_fail(ctx, e, "pz_msm_g1_batch: download");
    }
    // the host buffers belong to the caller again when this returns, whatever happened
    hipError_t e1 = hipStreamSynchronize(ctx->io_h2d), e2 = hipStreamSynchronize(ctx->stream);
    if (rc == PZ_OK && (e1 != hipSuccess || e2 != hipSuccess)) rc = pz_hip_fail(ctx, e1 != hipSuccess ? e1 : e2, "pz_msm_g1_batch: synchronize");
    if (rc == PZ_OK) rc = pz_check_async(ctx);
    return rc;
}

extern "C" int pz_msm_g1(pz_ctx* ctx, const pz_bases* bases, const uint64_t* scalars, size_t n, uint64_t out_jac[12]) {
    if (n && !scalars) return PZ_ERR_INVALID;
    const uint64_t* cols[1] = {scalars};
    return pz_msm_g1_batch(ctx, bases, cols, 1, n, out_jac);
}

extern "C" int pz_g1_sum(pz_ctx* ctx, const uint64_t* jac, size_t n, uint64_t out_jac[12]) {
    if (!ctx || !out_jac || (n && !jac)) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    void* d;
    PZCHK(pz_ws_get(ctx, WS_IO_C, (n + 1) * 96, &d));
    if (n) HIPCHK(ctx, hipMemcpyAsync((char*)d + 96, jac, n * 96, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(64), 0, ctx->stream, (const G1Jac*)((char*)d + 96), n, (G1Jac*)d);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_jac, d, 96, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

// device-resident form: the fold of the all-gathered per-rank partial points, no host hop (n is the world size)
// One MSM over several contexts (devices) from ONE host thread: pz_msm_g1_dev only queues work, so the shares run side by side on
// their devices; the downloads (one synchronisation per context, in rank order) and the fold follow.
extern "C" int pz_msm_g1_multi(pz_ctx* const* ctxs, const pz_bases* const* bases, const uint64_t* const* d_scalars, const size_t* n_per_ctx,
                               size_t n_ctx, int split_points, uint64_t out_jac[12]) {
    if (!ctxs || !bases || !d_scalars || !n_per_ctx || !out_jac || n_ctx == 0 || n_ctx > 1024) return PZ_ERR_INVALID;
    for (size_t r = 0; r < n_ctx; ++r) {
        if (!ctxs[r] || (n_per_ctx[r] && (!bases[r] || !d_scalars[r]))) return PZ_ERR_INVALID;
        if (n_per_ctx[r] && bases[r]->device != ctxs[r]->device) return PZ_ERR_INVALID;
        if (!split_points && (n_per_ctx[r] != n_per_ctx[0] || !bases[r] || bases[r]->nwin != bases[0]->nwin || bases[r]->c != bases[0]->c))
            return PZ_ERR_INVALID;   // the window split needs every context to hold the same scalars and the same table shape
    }
    std::vector<uint64_t> parts(n_ctx * 12, 0);
    std::vector<void*> d_part(n_ctx, nullptr);
    for (size_t r = 0; r < n_ctx; ++r) {
        pz_ctx* c = ctxs[r];
        PZ_ENTER(c);   // (recursive: the entry points below take it again)
        PZCHK(pz_ws_get(c, WS_MULTI, 96, &d_part[r]));
        uint32_t lo = 0, hi = n_per_ctx[r] ? bases[r]->nwin : 0;
        if (!split_points && n_per_ctx[r]) {
            lo = (uint32_t)(r * bases[r]->nwin / n_ctx);
            hi = (uint32_t)((r + 1) * bases[r]->nwin / n_ctx);
        }
        if (n_per_ctx[r] == 0 || lo == hi) {
            HIPCHK(c, hipMemsetAsync(d_part[r], 0, 96, c->stream));   // Jacobian identity (z = 0): an empty share
            continue;
        }
        PZCHK(pz_msm_g1_dev(c, bases[r], d_scalars[r], 1, n_per_ctx[r], 4 * n_per_ctx[r], lo, hi, (uint64_t*)d_part[r]));
    }
    for (size_t r = 0; r < n_ctx; ++r) PZCHK(pz_download(ctxs[r], &parts[12 * r], d_part[r], 96));   // rank order == the fixed fold order
    return pz_g1_sum(ctxs[0], parts.data(), n_ctx, out_jac);
}

extern "C" int pz_g1_sum_dev(pz_ctx* ctx, const uint64_t* d_jac, size_t n, uint64_t* d_out_jac) {
    if (!ctx || !d_out_jac || (n && !d_jac)) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(64), 0, ctx->stream, (const G1Jac*)d_jac, n, (G1Jac*)d_out_jac);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_normalize(pz_ctx* ctx, const uint64_t* jac, size_t n, uint64_t* aff) {
    if (!ctx || (n && (!jac || !aff))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 96, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 64, &dout));
    HIPCHK(ctx, hipMemcpyAsync(di, jac, n * 96, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g1_normalize, dim3(pz_div_up(n, 64)), dim3(64), 0, ctx->stream, (const G1Jac*)di, n,
                       (G1Aff64*)dout);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(aff, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

// ------------------------------------------------------------------------------------------------
// G1 radix-2 inverse FFT: the Lagrange-basis SRS g_lagrange from the monomial g of a params file WITHOUT the toxic
// scalar -- what halo2's ParamsKZG::setup / read path does with best_fft over G1Projective (SURVEY.md section 8f rank 2;
// reached from /root/reference/src/bench.rs:161-171 through gen_srs):
//   g_lagrange[i] = (1/n) sum_j omega^(-i j) g[j]
// The butterflies are those of the field transform, with the twiddle product a 254-bit scalar multiplication (double-and-
// add in XYZZ).  DIT over a bit-reversed XYZZ image in HBM, one launch per stage, one lane per butterfly.  A one-time cost
// per SRS: (k + 1) * 2^(k-1) scalar multiplications (~0.1 s at k = 17).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ G1X29 x29_scalar_mul(const G1X29& pt, const u32 k[8]) {
    G1X29 acc = x29_inf();
    bool started = false;   // skip the leading zero bits (wave-uniform only when every lane agrees: plain branch)
    for (int bit = 253; bit >= 0; --bit) {
        if (started) acc = x29_dbl(acc);
        if ((sel8(k, (unsigned)bit >> 5) >> (bit & 31)) & 1u) {
            x29_add(acc, pt);
            started = true;
        }
    }
    return acc;
}
__device__ __forceinline__ G1X29 x29_neg(const G1X29& p) {
    G1X29 r = p;
    if (!x29_is_inf(p)) r.y = f29_carry(f29_neg<4, 31>(p.y));   // value < 4p, limbs back below 2^29 + 8
    return r;
}

// load: A[bitrev(i)] = [scale] g[i]   (scale = 1/n as a canonical integer)
__global__ __launch_bounds__(128) void k_gfft_load(const G1Aff64* __restrict__ g, G1X29Raw* __restrict__ A, unsigned log_n, Fr scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    G1A29 p = a29_load64(g + i);
    G1X29 x = x29_inf();
    if (!a29_is_inf(p)) {
        p.x = f29_to_261(p.x);
        p.y = f29_to_261(p.y);
        const Fr kc = fp_from_mont(scale);
        x = x29_scalar_mul(x29_from_affine(a29_canon(p)), kc.v);
    }
    const size_t r = log_n ? (size_t)(__brev((unsigned)i) >> (32 - log_n)) : 0;
    x29_store_raw(A + r, x);
}
// one DIT stage: pairs (i0, i0 + half), twiddle tw[pos << (log_n - s - 1)]
__global__ __launch_bounds__(128) void k_gfft_stage(G1X29Raw* __restrict__ A, const Fr* __restrict__ tw, unsigned log_n, unsigned s) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >> (log_n - 1)) return;
    const size_t half = (size_t)1 << s, pos = t & (half - 1), i0 = ((t >> s) << (s + 1)) + pos, i1 = i0 + half;
    const G1X29 u = x29_load_raw(A + i0);
    G1X29 v = x29_load_raw(A + i1);
    if (pos) {
        const Fr w = fp_from_mont(fp_load<FrTag>(tw + (pos << (log_n - s - 1))));
        v = x29_scalar_mul(v, w.v);
    }
    G1X29 a = u, b = u;
    x29_add(a, v);
    const G1X29 nv = x29_neg(v);
    x29_add(b, nv);
    x29_store_raw(A + i0, a);
    x29_store_raw(A + i1, b);
}
__global__ __launch_bounds__(128) void k_gfft_store(const G1X29Raw* __restrict__ A, G1Aff64* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A29 a = x29_to_affine(x29_load_raw(A + i));
    if (!a29_is_inf(a)) {
        a.x = f29_to_256(a.x);
        a.y = f29_to_256(a.y);
    }
    a29_store64(out + i, a);
}

extern "C" int pz_srs_lagrange_from_monomial_dev(pz_ctx* ctx, uint32_t k, const uint64_t omega_inv[4], const uint64_t n_inv[4],
                                                 const uint64_t* d_g, uint64_t* d_g_lagrange) {
    if (!ctx || !omega_inv || !n_inv || !d_g || !d_g_lagrange || k > 26) return PZ_ERR_INVALID;
    PZ_ENTER(ctx);
    const size_t n = (size_t)1 << k;
    void *tw, *A;
    PZCHK(pz_get_pow_table(ctx, omega_inv, n, &tw));
    PZCHK(pz_ws_get(ctx, WS_PARTIALS, n * sizeof(G1X29Raw), &A));
    Fr sc;
    memcpy(sc.v, n_inv, 32);
    hipLaunchKernelGGL(k_gfft_load, dim3(pz_div_up(n, 128)), dim3(128), 0, ctx->stream, (const G1Aff64*)d_g, (G1X29Raw*)A, (unsigned)k, sc);
    for (unsigned s2 = 0; s2 < k; ++s2)
        hipLaunchKernelGGL(k_gfft_stage, dim3(pz_div_up(n / 2, 128)), dim3(128), 0, ctx->stream, (G1X29Raw*)A, (const Fr*)tw, (unsigned)k, s2);
    hipLaunchKernelGGL(k_gfft_store, dim3(pz_div_up(n, 128)), dim3(128), 0, ctx->stream, (const G1X29Raw*)A, (G1Aff64*)d_g_lagrange, n);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

// on-curve check of affine points (identity (0,0) accepted): the is_on_curve assertion of halo2curves' read_raw
__device__ __forceinline__ bool g1_point_ok(const G1Affine& p) {
    if (aff_is_inf(p)) return true;
    // coordinates must be canonical (< p) and satisfy y^2 = x^3 + 3
    Fq three = fp_add(fp_add(fp_one<FqTag>(), fp_one<FqTag>()), fp_one<FqTag>());
    Fq rhs = fp_add(fp_mul(fp_sqr(p.x), p.x), three);
    Fq rx = p.x, ry = p.y;
    fp_reduce_once(rx);
    fp_reduce_once(ry);
    bool canon = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) canon = canon && rx.v[k] == p.x.v[k] && ry.v[k] == p.y.v[k];
    Fq d = fp_sub(fp_sqr(p.y), rhs);
    return canon && fp_is_zero(d);
}

__global__ __launch_bounds__(256) void k_g1_check(const G1Affine* __restrict__ pts, size_t n, unsigned long long* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!g1_point_ok(aff_load(pts + i))) atomicAdd(bad, 1ull);
}

// the same predicate over n points in groups of `group` consecutive ones: flags[i / group] becomes 1 if point i fails
__global__ __launch_bounds__(256) void k_g1_check_groups(const G1Affine* __restrict__ pts, size_t n, size_t group, int32_t* __restrict__ flags) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!g1_point_ok(aff_load(pts + i))) atomicOr(flags + i / group, 1);
}

int pz_g1_check_groups_launch(pz_ctx* ctx, const uint64_t* d_points, size_t n_groups, size_t group, int32_t* d_flags) {
    const size_t n = n_groups * group;
    if (!n) return PZ_OK;
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, n_groups * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_g1_check_groups, dim3(pz_div_up(n, 256)), dim3(256), 0, ctx->stream, (const G1Affine*)d_points, n, group, d_flags);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_check_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, uint64_t* n_bad) {
    if (!ctx || !n_bad || (n && !d_points)) return PZ_ERR_INVALID;
    *n_bad = 0;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void* cnt;
    PZCHK(pz_ws_get(ctx, WS_MISC, 8, &cnt));
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_g1_check, dim3(pz_div_up(n, 256)), dim3(256), 0, ctx->stream, (const G1Affine*)d_points, n,
                       (unsigned long long*)cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(n_bad, cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}

extern "C" int pz_g1_fixed_base_mul_dev(pz_ctx* ctx, const uint64_t* d_scalars, size_t n, uint64_t* d_out_affine) {
    if (!ctx || (n && (!d_scalars || !d_out_affine))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    hipLaunchKernelGGL(k_fixed_base_mul, dim3(pz_div_up(n, 128)), dim3(128), 0, ctx->stream, (const Fr*)d_scalars, n,
                       (G1Aff64*)d_out_affine);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}

extern "C" int pz_g1_fixed_base_mul(pz_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_affine) {
    if (!ctx || (n && (!scalars || !out_affine))) return PZ_ERR_INVALID;
    if (!n) return PZ_OK;
    PZ_ENTER(ctx);
    void *di, *dout;
    PZCHK(pz_ws_get(ctx, WS_IO_B, n * 32, &di));
    PZCHK(pz_ws_get(ctx, WS_IO_C, n * 64, &dout));
    HIPCHK(ctx, hipMemcpyAsync(di, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(pz_g1_fixed_base_mul_dev(ctx, (const uint64_t*)di, n, (uint64_t*)dout));
    HIPCHK(ctx, hipMemcpyAsync(out_affine, dout, n * 64, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
