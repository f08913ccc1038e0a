// pz_prime.hip -- prime generation for Paillier keys: a batched Miller-Rabin test in which every candidate is its own
// modulus (k_prime_mr), a trial-division sieve over a window of candidates start + stride i (k_prime_residues, k_prime_mark) and the
// search that joins them (pz_prime_search).
// The group arithmetic itself (GI, grp_*, mont_mul, prime_setup) is prime_mont.cuh, shared with the probe library.
//
// Mapping to CDNA4.  The K3 arithmetic of pz_bigint.hip gives one wavefront to one integer of 64 or 128 limbs and reduces by Barrett under
// ONE modulus whose reciprocal costs a division; a 1024-bit candidate would idle three quarters of its lanes and pay that division per
// candidate.  Here a candidate is held by a GROUP of 16 lanes -- one DPP row, so the one-limb shift of the systolic product is a row
// shift -- and a wavefront holds four candidates; lane j of a group holds limbs [j E, j E + E): E = 1 up to 16 limbs, E = 2 up to 32.
// Products are Montgomery products with R = 2^(64 limbs): a lane-systolic CIOS of `limbs` outer steps (so a product costs
// limbs x 16 E limb products per group, not the K3 capacity), every limb's column kept as (lo, hi, ex) words so that no carry crosses
// a lane inside the loop; the carries are resolved once per product by a look-ahead over the group's 16 bits of a ballot.  The
// candidate's constants need no division: -c^-1 mod 2^64 by Newton steps, R mod c and R^2 mod c by 128 limbs doublings mod c.
//
// Constant time.  Candidates that turn out prime are key material.  In k_prime_mr no branch and no address depends on a candidate: the
// loops run over `limbs` and `rounds` (launch arguments), every group -- one beyond `count` or one whose candidate is even or below 3
// runs on the value 3 -- executes the same instructions, exponent bits and conditional subtractions act through lane masks, and the
// verdict is a predicate accumulated per group.  What a group's lanes compare against positions is s, the number of trailing zero
// bits of c - 1, and nothing else.  The sieve is NOT constant time in the window's start (it steps through multiples).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "prime_mont.cuh"
#include "pz_internal.h"

#define PR_BLOCK 256       // 4 wavefronts, 16 candidates
#define PR_MAX_LIMBS 32
#define PR_MAX_COUNT 65536
#define PR_MAX_ROUNDS 64
#define PR_MAX_WINDOW (1u << 20)
#define PR_MAX_WANT 64
#define PR_SIEVE_PRIMES 6541   // the odd primes below 2^16
#define PR_SEG 4096            // offsets one thread of k_prime_mark walks

// ---- k_prime_mr: batched Miller-Rabin, one group of 16 lanes per candidate (semantics: pz.h pz_bigint_is_prime) --------------------------
template <int E> __global__ __launch_bounds__(PR_BLOCK) void k_prime_mr(const u64* __restrict__ cands, unsigned L, unsigned count,
                                                                         const u64* __restrict__ bases, unsigned rounds,
                                                                         uint8_t* __restrict__ flags, u32* __restrict__ witness) {
    const GLane g = glane();
    const unsigned j = blockIdx.x * (PR_BLOCK / PR_GROUP) + threadIdx.x / PR_GROUP;
    const bool live = j < count;
    GI<E> c;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned k = g.gl * E + e;
        c.v[e] = (live && k < L) ? cands[(size_t)j * L + k] : 0;
    }
    // classify without a branch: a candidate that is even or below 3 (and a group beyond count) runs on 3
    u64 hi_or = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) hi_or |= (g.gl * E + e) == 0 ? 0 : c.v[e];
    const bool wide = grp_ballot(hi_or != 0, g) != 0;
    const u64 c0 = __shfl(c.v[0], 0, PR_GROUP);
    const bool is_two = !wide && c0 == 2;
    const bool tested = live && (c0 & 1) != 0 && (wide || c0 != 1);
    c = grp_select(!tested, c, grp_small<E>(3, g));
    const u64 m0 = tested ? c0 : 3;
    u64 ninv;
    GI<E> one, r2;
    prime_setup(c, m0, L, g, ninv, one, r2);
    GI<E> mone;
    (void)grp_sub(mone, c, one, g);   // c - 1 in Montgomery form
    // c - 1 = d 2^s: the exponent's words are c's with bit 0 cleared; s from the lowest set bit
    GI<E> ex = c;
    ex.v[0] &= g.gl == 0 ? ~1ull : ~0ull;
    unsigned s = 0xFFFFu;
#pragma unroll
    for (int e = E - 1; e >= 0; --e) {
        const unsigned tz = 64 * (g.gl * E + e) + (unsigned)__builtin_ctzll(ex.v[e] | (1ull << 63));
        s = ex.v[e] != 0 ? tz : s;
    }
    for (int off = 8; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)s, off, PR_GROUP);
        s = o < s ? o : s;
    }
    const GI<E> zero = grp_small<E>(0, g);
    unsigned first_fail = rounds;
    for (unsigned k = rounds; k-- > 0;) {
        // a = bases[k] mod c in Montgomery form: the base is the operand whose limbs are scanned, so it need not be below c
        const GI<E> am = mont_mul(r2, grp_small<E>(bases[k], g), c, ninv, L, g);
        bool pass = grp_eq(am, zero, g) || grp_eq(am, one, g) || grp_eq(am, mone, g);
        // left to right over all 64 L bits of c - 1 from 1: after bit `pos` the accumulator is a^((c - 1) >> pos)
        GI<E> acc = one;
        for (unsigned w = L; w-- > 0;) {
            const u64 word = grp_limb(ex, w);
            for (unsigned b = 64; b-- > 0;) {
                const unsigned pos = 64 * w + b;
                acc = mont_mul(acc, acc, c, ninv, L, g);
                const GI<E> t = mont_mul(acc, am, c, ninv, L, g);
                acc = grp_select(((word >> b) & 1) != 0, acc, t);
                const bool is_one = grp_eq(acc, one, g), is_mone = grp_eq(acc, mone, g);
                pass = pass || (pos == s && (is_one || is_mone)) || (pos < s && pos >= 1 && is_mone);
            }
        }
        first_fail = pass ? first_fail : k;
    }
    if (live && g.gl == 0) {
        witness[j] = tested ? first_fail : 0xFFFFFFFFu;
        flags[j] = tested ? (first_fail == rounds) : is_two;
    }
}

// ---- the sieve --------------------------------------------------------------------------------------------------------------------------
// res[i] = start mod primes[i]: Horner over 32-bit halves from the top, r < 2^16 so (r << 32 | half) stays inside 64 bits
__global__ void k_prime_residues(const u64* __restrict__ start, unsigned L, const u32* __restrict__ primes, unsigned n_primes,
                                 u32* __restrict__ res) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_primes) return;
    const u64 p = primes[i];
    u64 r = 0;
    for (unsigned k = L; k-- > 0;) {
        const u64 w = start[k];
        r = ((r << 32) | (w >> 32)) % p;
        r = ((r << 32) | (w & 0xFFFFFFFFull)) % p;
    }
    res[i] = (u32)r;
}
// mask[i] <- 0 where primes[t] divides c_i = start + stride i (and, in safe mode, where c_i = 1 mod primes[t], so that the prime
// divides (c_i - 1) / 2).  Thread (t, segment): the multiples inside its PR_SEG offsets.  The mask is set to 1 beforehand; every store
// writes the same 0, so their order does not matter
__global__ void k_prime_mark(const u32* __restrict__ primes, const u32* __restrict__ res, unsigned n_primes, unsigned stride, unsigned safe,
                             unsigned window, uint8_t* __restrict__ mask) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_primes) return;
    const unsigned lo = blockIdx.y * PR_SEG, hi = min(window, lo + PR_SEG);
    const u32 p = primes[t], r = res[t];
    const u32 half = (p + 1) / 2;                                     // 2^-1 mod p
    const u32 inv = stride == 2 ? half : (u32)(((u64)half * half) % p);   // stride^-1 mod p
    for (unsigned target = 0; target <= safe; ++target) {
        // the first i with r + stride i = target (mod p)
        const u32 i0 = (u32)(((u64)((target + p - r) % p) * inv) % p);
        unsigned i = lo <= i0 ? i0 : i0 + ((lo - i0 + p - 1) / p) * p;
        for (; i < hi; i += p) mask[i] = 0;
    }
}
// cands[j] = start + stride offs[j], or half of that (rounded down) where halve is set: the (c - 1) / 2 of an odd c
__global__ void k_prime_candidates(const u64* __restrict__ start, unsigned L, unsigned stride, const u32* __restrict__ offs, unsigned n,
                                   unsigned halve, u64* __restrict__ cands) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    u64 carry = (u64)stride * offs[j];
    u64 prev = 0;
    for (unsigned k = 0; k < L; ++k) {
        const u64 w = start[k] + carry;
        carry = w < carry;
        if (halve) {
            if (k > 0) cands[(size_t)j * L + k - 1] = (prev >> 1) | (w << 63);
            prev = w;
        } else {
            cands[(size_t)j * L + k] = w;
        }
    }
    if (halve) cands[(size_t)j * L + L - 1] = prev >> 1;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static int mr_launch(pz_ctx* ctx, uint32_t limbs, size_t count, const u64* d_cands, uint32_t rounds, const u64* d_bases, uint8_t* d_flags,
                     u32* d_wit) {
    pz_timer tm(ctx, PZ_T_TRACE);
    const dim3 grid((unsigned)((count + PR_BLOCK / PR_GROUP - 1) / (PR_BLOCK / PR_GROUP))), block(PR_BLOCK);
    if (limbs <= 16) hipLaunchKernelGGL(k_prime_mr<1>, grid, block, 0, ctx->stream, d_cands, limbs, (unsigned)count, d_bases, rounds, d_flags, d_wit);
    else hipLaunchKernelGGL(k_prime_mr<2>, grid, block, 0, ctx->stream, d_cands, limbs, (unsigned)count, d_bases, rounds, d_flags, d_wit);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
static int mr_args_check(const pz_ctx* ctx, uint32_t limbs, uint32_t rounds, const uint64_t* bases) {
    if (!ctx || !bases || limbs == 0 || rounds < 1 || rounds > PR_MAX_ROUNDS) return PZ_ERR_INVALID;
    for (uint32_t k = 0; k < rounds; ++k)
        if (bases[k] < 2) return PZ_ERR_INVALID;
    return limbs > PR_MAX_LIMBS ? PZ_ERR_UNSUPPORTED : PZ_OK;
}
// the epilogue of a call that staged candidates: the staging is overwritten and the stream drained whatever the run returned
static int prime_wipe_and_sync(pz_ctx* ctx, int rc, void* d, size_t bytes, void* d2 = nullptr, size_t bytes2 = 0) {
    hipError_t e = hipMemsetAsync(d, 0, bytes, ctx->stream);
    if (e == hipSuccess && d2) e = hipMemsetAsync(d2, 0, bytes2, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (rc != PZ_OK) return rc;
    HIPCHK(ctx, e);
    return PZ_OK;
}

static int is_prime_impl(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* cands, uint32_t rounds, const uint64_t* bases,
                         uint8_t* flags_out, uint32_t* witness_out, int on_device) {
    if (!cands || !flags_out || !witness_out || count < 1 || count > PR_MAX_COUNT) return PZ_ERR_INVALID;
    PZCHK(mr_args_check(ctx, limbs, rounds, bases));
    PZ_ENTER(ctx);
    const size_t cb = up256(count * limbs * 8), bb = up256(PR_MAX_ROUNDS * 8), wb = up256(count * 4), fb = up256(count);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_PRIME_MR, bb + (on_device ? 0 : cb + wb + fb), &ws));
    u64* d_bases = (u64*)ws;
    PZCHK(pz_upload_small_async(ctx, d_bases, bases, rounds * 8));
    if (on_device) return mr_launch(ctx, limbs, count, cands, rounds, d_bases, flags_out, witness_out);
    u64* d_c = (u64*)((char*)ws + bb);
    u32* d_wit = (u32*)((char*)d_c + cb);
    uint8_t* d_flags = (uint8_t*)d_wit + wb;
    auto run = [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(d_c, cands, count * limbs * 8, hipMemcpyHostToDevice, ctx->stream));
        PZCHK(mr_launch(ctx, limbs, count, d_c, rounds, d_bases, d_flags, d_wit));
        HIPCHK(ctx, hipMemcpyAsync(witness_out, d_wit, count * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(flags_out, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
        return PZ_OK;
    };
    return prime_wipe_and_sync(ctx, run(), d_c, cb + wb + fb);
}
extern "C" int pz_bigint_is_prime(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* cands, uint32_t rounds, const uint64_t* bases,
                                  uint8_t* flags_out, uint32_t* witness_out) {
    return is_prime_impl(ctx, limbs, count, cands, rounds, bases, flags_out, witness_out, 0);
}
extern "C" int pz_bigint_is_prime_dev(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* d_cands, uint32_t rounds,
                                      const uint64_t* bases, uint8_t* d_flags_out, uint32_t* d_witness_out) {
    return is_prime_impl(ctx, limbs, count, d_cands, rounds, bases, d_flags_out, d_witness_out, 1);
}

// the odd primes below 2^16 on the device, built and uploaded at the context's first use
static int sieve_table(pz_ctx* ctx, const u32** d_out) {
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_PRIME_TAB, PR_SIEVE_PRIMES * 4, &ws));
    if (!ctx->prime_table_ready) {
        std::vector<uint8_t> comp(1u << 16, 0);
        std::vector<u32> primes;
        for (u32 p = 3; p < (1u << 16); p += 2) {
            if (comp[p]) continue;
            primes.push_back(p);
            for (u32 q = p * p; q < (1u << 16) && p < 256; q += 2 * p) comp[q] = 1;
        }
        if (primes.size() != PR_SIEVE_PRIMES) return PZ_ERR_INTERNAL;
        HIPCHK(ctx, hipMemcpyAsync(ws, primes.data(), PR_SIEVE_PRIMES * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->prime_table_ready = true;
    }
    *d_out = (const u32*)ws;
    return PZ_OK;
}
static int sieve_args_check(const pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe) {
    if (!ctx || !start || limbs == 0 || window < 1 || window > PR_MAX_WINDOW || safe > 1) return PZ_ERR_INVALID;
    if (limbs > PR_MAX_LIMBS) return PZ_ERR_UNSUPPORTED;
    bool wide = (start[0] >> 32) != 0;
    for (uint32_t k = 1; k < limbs; ++k) wide = wide || start[k] != 0;
    if (!wide || (start[0] & (safe ? 3 : 1)) != (safe ? 3u : 1u)) return PZ_ERR_INVALID;
    // start + stride (window - 1) must fit `limbs` words
    u64 carry = (u64)(safe ? 4 : 2) * (window - 1);
    for (uint32_t k = 0; k < limbs; ++k) {
        const u64 w = start[k] + carry;
        carry = w < carry;
    }
    return carry ? PZ_ERR_RANGE : PZ_OK;
}
// the device side of a sieve: d_start (limbs words, already there), d_res (PR_SIEVE_PRIMES words), d_mask (window bytes)
static int sieve_launch(pz_ctx* ctx, uint32_t limbs, const u64* d_start, size_t window, uint32_t safe, u32* d_res, uint8_t* d_mask) {
    const u32* d_primes;
    PZCHK(sieve_table(ctx, &d_primes));
    HIPCHK(ctx, hipMemsetAsync(d_mask, 1, window, ctx->stream));
    const unsigned tb = 256, nb = (PR_SIEVE_PRIMES + tb - 1) / tb;
    hipLaunchKernelGGL(k_prime_residues, dim3(nb), dim3(tb), 0, ctx->stream, d_start, limbs, d_primes, (unsigned)PR_SIEVE_PRIMES, d_res);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_prime_mark, dim3(nb, (unsigned)((window + PR_SEG - 1) / PR_SEG)), dim3(tb), 0, ctx->stream, d_primes, d_res,
                       (unsigned)PR_SIEVE_PRIMES, safe ? 4u : 2u, safe, (unsigned)window, d_mask);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
// the sieve workspace: start | residues | mask
struct SieveBufs {
    u64* d_start;
    u32* d_res;
    uint8_t* d_mask;
    size_t bytes;
};
static int sieve_bufs(pz_ctx* ctx, uint32_t limbs, size_t window, SieveBufs* b) {
    const size_t sb = up256((size_t)limbs * 8), rb = up256(PR_SIEVE_PRIMES * 4);
    void* ws;
    b->bytes = sb + rb + up256(window);
    PZCHK(pz_ws_get(ctx, WS_PRIME_SIEVE, b->bytes, &ws));
    b->d_start = (u64*)ws;
    b->d_res = (u32*)((char*)ws + sb);
    b->d_mask = (uint8_t*)ws + sb + rb;
    return PZ_OK;
}
extern "C" int pz_prime_sieve(pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe, uint8_t* mask_out) {
    if (!mask_out) return PZ_ERR_INVALID;
    PZCHK(sieve_args_check(ctx, limbs, start, window, safe));
    PZ_ENTER(ctx);
    SieveBufs b;
    PZCHK(sieve_bufs(ctx, limbs, window, &b));
    auto run = [&]() -> int {
        HIPCHK(ctx, hipMemcpyAsync(b.d_start, start, (size_t)limbs * 8, hipMemcpyHostToDevice, ctx->stream));
        PZCHK(sieve_launch(ctx, limbs, b.d_start, window, safe, b.d_res, b.d_mask));
        HIPCHK(ctx, hipMemcpyAsync(mask_out, b.d_mask, window, hipMemcpyDeviceToHost, ctx->stream));
        return PZ_OK;
    };
    return prime_wipe_and_sync(ctx, run(), b.d_start, b.bytes);
}

// the search's Miller-Rabin staging: bases | offsets | candidates | witness | flags, for batches of at most `cap` candidates
struct SearchBufs {
    u64* d_bases;
    u32* d_offs;
    u64* d_cands;
    u32* d_wit;
    uint8_t* d_flags;
    char* secret;   // from the offsets on
    size_t secret_bytes;
};
// flags of one Miller-Rabin pass over the candidates start + stride offs[j] (halve: over their (c - 1) / 2), appended after `at` candidates
// already staged; the launch covers offs.size() candidates
static int search_stage(pz_ctx* ctx, uint32_t limbs, const u64* d_start, uint32_t stride, const SearchBufs& b, const std::vector<u32>& offs,
                        unsigned halve, size_t at) {
    const size_t n = offs.size();
    HIPCHK(ctx, hipMemcpyAsync(b.d_offs + at, offs.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_prime_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_start, limbs, stride, b.d_offs + at,
                       (unsigned)n, halve, b.d_cands + at * limbs);
    HIPCHK(ctx, hipGetLastError());
    return PZ_OK;
}
static int search_flags(pz_ctx* ctx, uint32_t limbs, const SearchBufs& b, size_t n, uint32_t rounds, const u64* d_bases,
                        std::vector<uint8_t>& flags) {
    flags.resize(n);
    PZCHK(mr_launch(ctx, limbs, n, b.d_cands, rounds, d_bases, b.d_flags, b.d_wit));
    HIPCHK(ctx, hipMemcpyAsync(flags.data(), b.d_flags, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PZ_OK;
}
static int search_run(pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe, uint32_t rounds,
                      const uint64_t* bases, uint32_t want, uint32_t* offsets_out, uint32_t* found_out, size_t* survivors_out,
                      const SieveBufs& sv, const SearchBufs& b, size_t cap) {
    const uint32_t stride = safe ? 4 : 2;
    HIPCHK(ctx, hipMemcpyAsync(sv.d_start, start, (size_t)limbs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b.d_bases, bases, rounds * 8, hipMemcpyHostToDevice, ctx->stream));
    PZCHK(sieve_launch(ctx, limbs, sv.d_start, window, safe, sv.d_res, sv.d_mask));
    std::vector<uint8_t> mask(window), flags;
    HIPCHK(ctx, hipMemcpyAsync(mask.data(), sv.d_mask, window, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<u32> surv;
    for (size_t i = 0; i < window; ++i)
        if (mask[i]) surv.push_back((u32)i);
    if (survivors_out) *survivors_out = surv.size();
    uint32_t found = 0;
    // survivors in ascending batches; inside a batch the first round alone thins the candidates (and, in safe mode, their halves) before
    // the remaining rounds run on what is left: round 0 is one of the rounds, so nothing that passes them all is lost
    for (size_t at = 0; at < surv.size() && found < want; at += cap) {
        std::vector<u32> live(surv.begin() + at, surv.begin() + std::min(surv.size(), at + cap)), keep;
        for (unsigned halve = 0; halve <= safe && !live.empty(); ++halve) {
            PZCHK(search_stage(ctx, limbs, sv.d_start, stride, b, live, halve, 0));
            PZCHK(search_flags(ctx, limbs, b, live.size(), 1, b.d_bases, flags));
            keep.clear();
            for (size_t j = 0; j < live.size(); ++j)
                if (flags[j]) keep.push_back(live[j]);
            live.swap(keep);
        }
        if (rounds > 1 && !live.empty()) {
            // candidates, then their halves behind them: the staging holds two batches
            PZCHK(search_stage(ctx, limbs, sv.d_start, stride, b, live, 0, 0));
            if (safe) PZCHK(search_stage(ctx, limbs, sv.d_start, stride, b, live, 1, live.size()));
            PZCHK(search_flags(ctx, limbs, b, live.size() * (1 + safe), rounds - 1, b.d_bases + 1, flags));
            keep.clear();
            for (size_t j = 0; j < live.size(); ++j)
                if (flags[j] && (!safe || flags[live.size() + j])) keep.push_back(live[j]);
            live.swap(keep);
        }
        for (size_t j = 0; j < live.size() && found < want; ++j) offsets_out[found++] = live[j];
    }
    *found_out = found;
    std::fill(mask.begin(), mask.end(), 0);
    std::fill(surv.begin(), surv.end(), 0);
    return PZ_OK;
}
extern "C" int pz_prime_search(pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe, uint32_t rounds,
                               const uint64_t* bases, uint32_t want, uint32_t* offsets_out, uint32_t* found_out, size_t* survivors_out) {
    if (!offsets_out || !found_out || want < 1 || want > PR_MAX_WANT) return PZ_ERR_INVALID;
    PZCHK(mr_args_check(ctx, limbs, rounds, bases));
    PZCHK(sieve_args_check(ctx, limbs, start, window, safe));
    PZ_ENTER(ctx);
    SieveBufs sv;
    PZCHK(sieve_bufs(ctx, limbs, window, &sv));
    // a batch: a safe prime wants about a thousand survivors tested, a plain one a few dozen.  Twice the batch is staged at most
    // (candidates and their halves in the last pass)
    const size_t cap = safe ? 4096 : 1024;
    const size_t bb = up256(PR_MAX_ROUNDS * 8), ob = up256(2 * cap * 4), cb = up256(2 * cap * limbs * 8), wb = up256(2 * cap * 4), fb = up256(2 * cap);
    void* ws;
    PZCHK(pz_ws_get(ctx, WS_PRIME_MR, bb + ob + cb + wb + fb, &ws));
    SearchBufs b;
    b.d_bases = (u64*)ws;
    b.secret = (char*)ws + bb;
    b.secret_bytes = ob + cb + wb + fb;
    b.d_offs = (u32*)b.secret;
    b.d_cands = (u64*)(b.secret + ob);
    b.d_wit = (u32*)(b.secret + ob + cb);
    b.d_flags = (uint8_t*)(b.secret + ob + cb + wb);
    *found_out = 0;
    const int rc = search_run(ctx, limbs, start, window, safe, rounds, bases, want, offsets_out, found_out, survivors_out, sv, b, cap);
    return prime_wipe_and_sync(ctx, rc, sv.d_start, sv.bytes, b.secret, b.secret_bytes);
}
