/* pz.h -- C ABI of the MI355X-native (gfx950, hand-written HIP) hot path of the
 * Paillier-in-Halo2 prover.  This header is the whole drop-in boundary: plain pointers and sizes,
 * no C++/torch types.  Library: paillier_halo2_amd/csrc/libpz_hip.so.
 *
 * The reference (aerius-labs/paillier-halo2) is a plain Rust library with no FFI seam of its own
 * (src/lib.rs:1-2); every entry point below names the reference call site / dependency routine it
 * replaces.  INTEGRATION.md shows the Rust `extern "C"` stub a maintainer adds for each.
 *
 * Conventions (all functions):
 *   - return 0 (PZ_OK) on success, a negative pz_status on error; never throw, never abort, no
 *     callbacks; there is NO CPU fallback -- without a usable gfx950 device pz_init fails.
 *   - field elements: 4 x u64 little-endian limbs in MONTGOMERY form (R = 2^256), exactly the
 *     in-memory layout of halo2curves Fr / Fq.  G1Affine = {x, y} (64 B), identity = all-zero.
 *     G1 Jacobian = {x, y, z} (96 B), identity z = 0 (returned as (0, R, 0)).
 *   - big integers: little-endian u64 limb arrays (limb 0 least significant), i.e. the limb order
 *     of AssignedBigUint::limbs() at limb_bits = 64 (paillier.rs:22-30).
 *   - "host" pointers are ordinary process memory; "_dev" entry points take device pointers
 *     (hipMalloc / torch tensor data_ptr) valid on the context's device and run asynchronously on
 *     the context's stream (pz_set_stream); host-pointer entry points synchronise before returning.
 *   - every field element / coordinate handed to the library must be CANONICAL (an integer below the modulus in
 *     Montgomery form), as halo2curves guarantees for Fr / Fq values; limbs in [p, 2^256) are not reduced on entry
 *     and give undefined (silently wrong) results.  pz_g1_check_dev validates points on request.
 *   - pz_set_stream orders the new stream after the work already queued on the previous one (event wait), so cached
 *     tables / workspaces stay consistent; the caller still orders its OWN buffers between streams.
 *   - a pz_ctx is bound to ONE device (one process per GPU, ranks joined by RCCL above this ABI);
 *     distinct contexts may be used concurrently; one context is serialised INTERNALLY (a recursive mutex held for
 *     the duration of every entry point), and entry points call hipSetDevice themselves, so they may be called
 *     from any thread -- e.g. halo2's rayon workers reaching a patched best_multiexp with one shared context.
 */
#ifndef PZ_H
#define PZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pz_ctx pz_ctx;
typedef struct pz_bases pz_bases;

enum pz_status {
    PZ_OK = 0,
    PZ_ERR_INVALID = -1,      /* null pointer, bad size, log_n out of range ...            */
    PZ_ERR_HIP = -2,          /* a HIP runtime call failed (see pz_last_hip_error)          */
    PZ_ERR_NO_DEVICE = -3,    /* no gfx950 device visible                                   */
    PZ_ERR_OOM = -4,          /* device allocation failed                                   */
    PZ_ERR_ZERO_MODULUS = -5, /* mul_mod / pow_mod with modulus 0 (reference: BigUint % 0 panics, paillier.rs:91) */
    PZ_ERR_RANGE = -6,        /* quotient does not fit the limb count the circuit assigns it (unsatisfiable in the reference) */
    PZ_ERR_UNSUPPORTED = -7,  /* n_devices != 1, limb count not a supported size ...         */
    PZ_ERR_CAPACITY = -8,     /* caller-provided output capacity too small                  */
    PZ_ERR_MESSAGE_RANGE = -9,/* uniform-shape circuit: a message does not fit the m_bits the circuit decomposes */
    PZ_ERR_ASYNC = -10        /* reported by a synchronising entry point (pz_sync, pz_download, the host-pointer MSM calls): an
                                 earlier asynchronous pz_msm_g1* call found its scalars changed while it ran, or
                                 pz_permutation_sigma_dev found an image outside its m x n cells; the outputs of that call are
                                 invalid (no out-of-bounds access took place: positions are checked on the device) */
    ,
    PZ_ERR_INTERNAL = -11     /* a device-side wait ran into its bound.  Only source today: K3 (pz_paillier_trace / pz_paillier_encrypt*):
                                 a chain is worked by two workgroups, and a multiplier workgroup waits for each square its squarer
                                 publishes; that wait is bounded (2^27 polls, tens of seconds) so that every wave has an exit whatever
                                 happens to the other workgroup.  For the caller: the call has returned cleanly, c_out / result /
                                 n_steps of the affected chains were NOT written and their step records are incomplete -- discard all
                                 outputs of the call; the context and its device memory are intact and the same call may simply be
                                 repeated.  It does not occur in normal operation (roles are handed out by arrival, so a multiplier's
                                 squarer has always started before it; see csrc/pz_bigint.hip k_pow_mod_chain); it is the defined
                                 outcome if the device stops scheduling a started workgroup. */
};

/* ---------------------------------------------------------------------------------------------
 * context
 * ------------------------------------------------------------------------------------------- */
/* n_devices must be 1; device_ids[0] is the HIP device ordinal (NULL -> device 0). */
int pz_init(int n_devices, const int* device_ids, pz_ctx** out);
int pz_free(pz_ctx* ctx);
const char* pz_strerror(int status);
/* last HIP error string recorded by this context (empty string if none) */
const char* pz_last_hip_error(const pz_ctx* ctx);
/* stream used by the _dev entry points (NULL = the context's own stream). */
int pz_set_stream(pz_ctx* ctx, void* hip_stream);
int pz_sync(pz_ctx* ctx);
/* explicit ABI version, bumped whenever an entry point below is added, removed or changes meaning (measurement probes are
 * not part of this ABI: they live in libpz_probe.so).  A binding compares it with the PZ_ABI_VERSION it was built against. */
#define PZ_ABI_VERSION 7
int pz_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * device memory -- for a host that owns no HIP runtime of its own (the reference's Rust prover behind this FFI; the C++
 * driver in paillier_halo2_amd/host/prove_c2.cpp).  The `_dev` entry points take these pointers as they are, so a proof's
 * columns can stay in HBM from K4 through K1 and K2 (patch points C / D of INTEGRATION.md: bench.rs:161-171's create_proof).
 * ------------------------------------------------------------------------------------------- */
/* (a request that does not fit makes the library give back what it holds as caches -- cached blocks, then the grow-only sort / partial-sum
 * workspaces of pz_msm_g1*, which the next MSM sizes anew for what is free then -- before it returns PZ_ERR_OOM) */
int pz_dev_alloc(pz_ctx* ctx, size_t bytes, void** d_out);
/* block cache of pz_dev_alloc / pz_dev_free (off by default: max_bytes = 0): freed blocks of 32 MiB and more are KEPT by the context, up
 * to max_bytes in all, and handed to the next pz_dev_alloc of that size (or up to an eighth smaller) instead of going back to the driver.
 * For a caller that proves message after message of the reference's circuit -- a new 116-GB proving key each (paillier.rs:50-55 makes
 * every message its own circuit) -- the driver's allocation cost (seconds per key) is then paid once: pz_pk_create / pz_pk_free allocate
 * through these functions, with column counts rounded up to 64 so that keys of nearly equal shape ask for identical sizes.  Lowering the
 * limit releases what exceeds it; the library releases the cache itself when one of its own allocations runs out of memory. */
int pz_dev_cache_limit(pz_ctx* ctx, size_t max_bytes);
/* the ARENA: one block of `bytes` reserved from the driver NOW, out of which this context's later allocations are carved -- pz_dev_alloc and
 * every buffer the library allocates for itself on this context (workspaces, tables, pz_load_bases*, pz_circuit_structure_dev's arrays and
 * temporaries, a proving key).  Freed blocks go back to the arena and coalesce; a request the arena cannot serve falls through to the
 * driver (and the block cache above).  For the caller pz_dev_cache_limit was made for, at the sizes where the cache stops helping: at
 * config c5 (3072-bit n, k = 19; bench.rs:161-171's keygen + proof per run) a step holds 250 GB, the cache has to be released between a
 * key and the next structure's temporaries, and half of an 11-s step was driver allocation calls; from an arena the same step makes none.
 * Blocks are 4 KiB-granular and NOT zeroed.  A block may be freed through any context.  bytes = 0 releases the arena (also pz_free does);
 * one that still holds live blocks -- PZ_ERR_INVALID -- is detached from the context and stays reserved until the last of them is freed.
 * Size it from pz_dev_mem_info (leave a few GiB to the runtime).  PZ_DEV_ARENA_POISON=1 in the environment fills the arena, and every
 * block again when it is freed, with 0xA5 (tests). */
int pz_dev_arena(pz_ctx* ctx, size_t bytes);
/* out: arena bytes, bytes in live blocks, the peak of that, the largest free hole, requests served, requests it could not serve (all 0
 * without an arena) */
int pz_dev_arena_info(pz_ctx* ctx, uint64_t out[6]);
/* the driver's free / total device memory (hipMemGetInfo; waits for the device's queued work on ROCm).  Either pointer may be NULL */
int pz_dev_mem_info(pz_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
/* waits for the context's queued work, then frees */
int pz_dev_free(pz_ctx* ctx, void* d);
/* host -> device on the context's stream; returns when the host buffer may be reused */
int pz_upload(pz_ctx* ctx, void* d_dst, const void* src, size_t bytes);
/* device -> host on the context's stream; returns when the data has arrived (everything queued before it has run) */
int pz_download(pz_ctx* ctx, void* dst, const void* d_src, size_t bytes);
/* asynchronous fill on the context's stream */
int pz_dev_memset(pz_ctx* ctx, void* d_dst, int byte_value, size_t bytes);
/* asynchronous device -> device copy on the context's stream (e.g. a column's Lagrange values into the buffer its coefficient
 * form is computed in) */
int pz_dev_copy(pz_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* the same for `rows` runs of `width` bytes, the runs dst_pitch / src_pitch bytes apart (a prover fills the blinding rows at the end
 * of every column of a proof from one staged block of random elements) */
int pz_dev_copy_2d(pz_ctx* ctx, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch, size_t width, size_t rows);
/* order two contexts of one device: everything queued on `producer`'s stream so far happens before whatever `waiter` queues
 * from now on (an event wait, no host synchronisation) */
int pz_ctx_wait(pz_ctx* waiter, pz_ctx* producer);

/* ---------------------------------------------------------------------------------------------
 * K1 -- G1 multi-scalar multiplication.  Replaces halo2curves `best_multiexp(coeffs, bases)`
 * reached from /root/reference/src/bench.rs:161-171 (bench_builder -> create_proof ->
 * ParamsKZG::commit_lagrange / commit).  The VALUE (the group element) equals best_multiexp's;
 * the Jacobian representative is not unique, compare after pz_g1_normalize (halo2 itself writes
 * commitments to the transcript in affine form after batch_normalize).
 * ------------------------------------------------------------------------------------------- */
/* Upload 2^k affine bases (host) and build the device-resident window-shifted table
 * T[w][i] = 2^(c*w) * P_i.  `lagrange` only labels the set (g vs g_lagrange of ParamsKZG).
 * window_bits = 0 picks the default for k. */
int pz_srs_load_g1(pz_ctx* ctx, uint32_t k, const uint64_t* bases_affine, int lagrange, pz_bases** out);
/* general form: n_points need not be a power of two; bases may already be on the device. */
int pz_bases_load_g1(pz_ctx* ctx, const uint64_t* bases_affine, size_t n_points, int on_device,
                     uint32_t window_bits, pz_bases** out);
int pz_bases_free(pz_ctx* ctx, pz_bases* bases);
/* window parameters of a loaded set: c = window bits, n_windows = floor(253/c)+1 */
int pz_bases_info(const pz_bases* bases, size_t* n_points, uint32_t* window_bits, uint32_t* n_windows);

/* == best_multiexp(scalars[0..n], bases[0..n]);  n <= n_points.  Host pointers. */
int pz_msm_g1(pz_ctx* ctx, const pz_bases* bases, const uint64_t* scalars, size_t n, uint64_t out_jac[12]);
/* n_cols column commitments against the same bases (commit_lagrange per advice column).  Host pointers (pageable or
 * page-locked); the columns are streamed through device staging buffers in groups, uploads on a copy stream of the
 * library's own beside the kernels of the previous group; the call returns when out_jac is complete. */
int pz_msm_g1_batch(pz_ctx* ctx, const pz_bases* bases, const uint64_t* const* scalar_cols, size_t n_cols,
                    size_t n, uint64_t* out_jac /* n_cols x 12 */);
/* device-resident form: scalars = n_cols columns, column j at d_scalars + j*col_stride (in u64
 * units, >= 4*n); result n_cols x 12 u64 on the device.  Only Pippenger windows
 * [win_lo, win_hi) are accumulated (pass 0, n_windows for the full MSM) -- the multi-GPU split of
 * one large MSM gives each rank a disjoint window range and sums the partial points. */
int pz_msm_g1_dev(pz_ctx* ctx, const pz_bases* bases, const uint64_t* d_scalars, size_t n_cols, size_t n,
                  size_t col_stride, uint32_t win_lo, uint32_t win_hi, uint64_t* d_out_jac);
/* pz_msm_g1_dev with a DENSITY HINT for a batch of columns (more than 8 per call; fewer ignore it).  The digit sort has a
 * variant for columns of short scalars (witness cells: few non-zero digits) and one for full-width scalars; without a hint
 * (PZ_MSM_AUTO == pz_msm_g1_dev) both are queued and the device picks one per launch from the number of non-zero digits.  A
 * caller that knows what its columns hold says so: PZ_MSM_SPARSE queues the single-pass scatter alone and sorts in
 * column-sized slices, PZ_MSM_DENSE queues the two-step scatter alone.  The hint chooses launches and sizes, never results:
 * the group element is the same under every hint (compare after pz_g1_normalize), a wrong hint only costs time.  Any other
 * value of `density` is PZ_ERR_INVALID. */
#define PZ_MSM_AUTO 0
#define PZ_MSM_SPARSE 1
#define PZ_MSM_DENSE 2
int pz_msm_g1_dev_ex(pz_ctx* ctx, const pz_bases* bases, const uint64_t* d_scalars, size_t n_cols, size_t n,
                     size_t col_stride, uint32_t win_lo, uint32_t win_hi, int density, uint64_t* d_out_jac);
/* sum of n Jacobian points (host in/out): the fixed-order fold of per-rank partial MSMs. */
int pz_g1_sum(pz_ctx* ctx, const uint64_t* jac /* n x 12 */, size_t n, uint64_t out_jac[12]);
/* device form: d_jac (n x 12) and d_out_jac (12) are device pointers; asynchronous on the context's stream.  d_out_jac
 * must not alias d_jac.  Used after the all-gather of the sharded MSM: every rank folds the same points in rank order. */
int pz_g1_sum_dev(pz_ctx* ctx, const uint64_t* d_jac, size_t n, uint64_t* d_out_jac);
/* ONE multi-scalar multiplication over n_ctx contexts -- one per GPU of a node (several on one device work too) -- in one call:
 * north_star's "disjoint Pippenger windows of one large MSM sharded across the GPUs, partial sums folded" for a single-process host.
 *   split_points == 0: context r accumulates windows [r W / n_ctx, (r + 1) W / n_ctx) of ALL n_per_ctx[r] (== n) scalars; it holds all
 *                      scalars (d_scalars[r]) and a table of all bases (bases[r], the same window width everywhere);
 *   split_points != 0: context r takes its own point range: d_scalars[r] holds its n_per_ctx[r] scalars, bases[r] its n_per_ctx[r]
 *                      bases (SURVEY 8e's alternative: 1 / n_ctx of the table memory and scalar reads per GPU).
 * Every context's share is queued on its own stream (the call does not serialise them), the 96-byte partial points are then read
 * back in rank order and folded on ctxs[0] in that fixed order.  Blocks until out_jac is there.  d_scalars[r] / bases[r] belong to
 * ctxs[r]'s device.  Across PROCESSES (one per GPU) the same is pz_msm_g1_dev + an exchange of the partials + pz_g1_sum[_dev]. */
int pz_msm_g1_multi(pz_ctx* const* ctxs, const pz_bases* const* bases, const uint64_t* const* d_scalars, const size_t* n_per_ctx,
                    size_t n_ctx, int split_points, uint64_t out_jac[12]);
/* Jacobian -> affine for n points (host in/out): `batch_normalize`. */
int pz_g1_normalize(pz_ctx* ctx, const uint64_t* jac /* n x 12 */, size_t n, uint64_t* aff /* n x 8 */);
/* out[i] = [scalars[i]] * G1 generator, affine; scalars are Fr Montgomery (host in/out).  This is
 * the fixed-base multiplication `ParamsKZG::setup` uses for g[i] = [s^i]G; also used to build
 * synthetic base sets with known discrete logs. */
int pz_g1_fixed_base_mul(pz_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_affine /* n x 8 */);
/* device form of the same; out_affine is a device pointer */
int pz_g1_fixed_base_mul_dev(pz_ctx* ctx, const uint64_t* d_scalars, size_t n, uint64_t* d_out_affine);

/* Commitment of BYTE MASKS (csrc/pz_vkgen.hip): d_out_jac[col] = sum of P_i over the rows i < n where d_mask[col * mask_stride + i] != 0
 * (any non-zero byte counts, as in pz_fr_from_mask_dev) -- commit_lagrange of a selector column, which halo2's Assembly holds as 0 / 1
 * bytes, without widening it to 32-byte scalars and without the Pippenger sort: the set rows of a row chunk are compacted into a list
 * and added as they are.  The group element equals pz_msm_g1_dev of the pz_fr_from_mask_dev columns (compare after pz_g1_normalize);
 * repeated and cancelling bases are handled.  n <= n_points of the set; mask_stride in bytes, >= n; n_cols x 12 words out.  Device
 * pointers, asynchronous on the context's stream. */
int pz_g1_commit_mask_dev(pz_ctx* ctx, const pz_bases* bases, const uint8_t* d_mask, size_t n_cols, size_t n, size_t mask_stride,
                          uint64_t* d_out_jac);

/* ---------------------------------------------------------------------------------------------
 * K2 -- radix-2 NTT over Fr.  Replaces halo2curves `best_fft(a, omega, log_n)` reached from the
 * same call site through halo2-axiom EvaluationDomain::{ifft, fft, coeff_to_extended,
 * extended_to_coeff}:  a[k] <- sum_j a[j] * omega^(j k), natural order in and out, in place.
 * ------------------------------------------------------------------------------------------- */
int pz_ntt_fr(pz_ctx* ctx, uint64_t* a /* 2^log_n x 4 */, const uint64_t omega[4], uint32_t log_n);
/* n_cols transforms in place in HOST memory: column groups are uploaded, transformed and downloaded concurrently (two copy
 * streams of the library's own + the context's stream); the call returns when every column is back. */
int pz_ntt_fr_batch(pz_ctx* ctx, uint64_t* const* cols, size_t n_cols, const uint64_t omega[4], uint32_t log_n);
/* device-resident, n_cols columns at d_a + j*col_stride (u64 units).  Optional fused steps
 * (either may be NULL):
 *   pre_coset_g : a[i] *= g^i before the transform (distribute_powers of coeff_to_extended)
 *   post_scale  : a[k] *= s   after  the transform (the 1/n `ifft_divisor`)            */
int pz_ntt_fr_dev(pz_ctx* ctx, uint64_t* d_a, size_t n_cols, size_t col_stride, const uint64_t omega[4],
                  uint32_t log_n, const uint64_t* pre_coset_g, const uint64_t* post_scale);
/* the same out of place: column j is read at d_in + j*in_stride and its transform written at d_out + j*out_stride (d_in is not
 * modified; d_out == d_in with equal strides is pz_ntt_fr_dev).  lagrange_to_coeff of a committed column: the Lagrange values
 * stay where the commitment kernel reads them, the coefficient form gets its own buffer. */
int pz_ntt_fr_to_dev(pz_ctx* ctx, const uint64_t* d_in, size_t in_stride, uint64_t* d_out, size_t out_stride, size_t n_cols,
                     const uint64_t omega[4], uint32_t log_n, const uint64_t* pre_coset_g, const uint64_t* post_scale);

/* coeff_to_extended in one call (n = 2^log_n coefficients per column -> 2^log_e * n evaluations on the coset):
 *   d_ext[col][2^log_e * q + r] = sum_i d_coeff[col][i] * scale * coset_gens[r]^i * omega_n^(i q)
 * coset_gens (host, 2^log_e x 4 limbs, Montgomery) = g * omega_ext^r; omega_n = omega_ext^(2^log_e) generates the
 * 2^log_n domain; scale may be NULL (1) -- pass the 1/n ifft divisor here when d_coeff still carries it.
 * log_n <= 18, log_e <= 3.  Equals zero-extending to 2^(log_n+log_e), distribute_powers(g) and best_fft(omega_ext). */
int pz_ntt_fr_extend_dev(pz_ctx* ctx, const uint64_t* d_coeff, size_t n_cols, size_t in_stride, uint64_t* d_ext,
                         size_t out_stride, uint32_t log_n, uint32_t log_e, const uint64_t omega_n[4],
                         const uint64_t* coset_gens, const uint64_t* scale);
/* in-place representation change of n Fr elements on the device: to_mont != 0: canonical little-endian
 * integers (must be < r) -> Montgomery form (Fr::from_raw); else Montgomery -> canonical (to_repr). */
/* Lagrange values -> coefficients (in place: lagrange_to_coeff = best_fft(omega_n^-1), then * n_inv) AND -> the extended
 * coset values of pz_ntt_fr_extend_dev, in one call: the final pass of the inverse transform is fused with the first pass
 * of the 2^log_e forward transforms, so the coefficients are written once and never read back (10 <= log_n <= 18; other
 * sizes run the two transforms back to back).  Results are identical to pz_ntt_fr_dev + pz_ntt_fr_extend_dev. */
int pz_ntt_fr_coeff_extend_dev(pz_ctx* ctx, uint64_t* d_values, size_t n_cols, size_t col_stride, uint64_t* d_ext,
                               size_t out_stride, uint32_t log_n, uint32_t log_e, const uint64_t omega_n[4],
                               const uint64_t omega_n_inv[4], const uint64_t n_inv[4], const uint64_t* coset_gens);
int pz_fr_convert_dev(pz_ctx* ctx, uint64_t* d_a, size_t n, int to_mont);
/* a byte mask -> field elements: d_out[i] = d_mask[i] != 0 ? 1 : 0 (Montgomery form), n elements, both on the device.  How selectors --
 * 0 / 1 bytes in halo2's Assembly -- become Lagrange-form fixed columns without crossing PCIe as 32-byte elements (keygen). */
int pz_fr_from_mask_dev(pz_ctx* ctx, const uint8_t* d_mask, size_t n, uint64_t* d_out);

/* ---------------------------------------------------------------------------------------------
 * K3 -- big-integer witness generation for g^m * r^n mod n^2.  Replaces the native
 * (num-bigint) part of biguint-halo2's BigUintChip::{mul_mod, pow_mod_fixed_exp}
 * (call sites /root/reference/src/paillier.rs:51,55,57,81) and paillier_enc_native /
 * paillier_add_native (paillier.rs:87-97).
 * A "step" is one mul_mod: (a, b, q, r) with a*b = q*modulus + r, 0 <= r < modulus, each `limbs`
 * u64 limbs, laid out a|b|q|r (4*limbs u64 per step).
 * ------------------------------------------------------------------------------------------- */
/* one mul_mod witness (PaillierChip::add's single step, paillier.rs:81) */
int pz_mul_mod(pz_ctx* ctx, uint32_t limbs, const uint64_t* a, const uint64_t* b, const uint64_t* modulus,
               uint64_t* q, uint64_t* r);
/* pow_mod_fixed_exp step trace: acc = 1, sq = base; for each bit of exp LSB->MSB: emit
 * (sq,sq,q,sq') ; if bit: emit (acc,sq_old,q,acc').  steps_out has room for *n_steps steps on
 * entry (needs bits(exp) + popcount(exp)); on return *n_steps = steps written. result = acc. */
int pz_paillier_trace(pz_ctx* ctx, uint32_t limbs_n2, const uint64_t* n2, const uint64_t* base, const uint64_t* exp,
                      uint32_t exp_limbs, uint64_t* steps_out, size_t* n_steps, uint64_t* result);
/* whole PaillierChip::encrypt witness (paillier.rs:32-60) for `batch` independent instances:
 * per instance n, g, m, r are limbs_n limbs (limbs_n2 = 2*limbs_n); n2 = n*n is formed on the
 * device; the g^m and r^n chains of every instance run concurrently; then c = gm*rn mod n2.
 * steps_out: per instance `steps_cap` steps (layout as above): first the g^m trace, then the r^n
 * trace, then the final mul_mod.  n_steps_g / n_steps_r (per instance) receive the trace lengths.
 * c_out: batch x 2*limbs_n limbs.  steps_out may be NULL (values only: the paillier_enc_native use). */
int pz_paillier_encrypt(pz_ctx* ctx, uint32_t limbs_n, size_t batch, const uint64_t* n, const uint64_t* g,
                        const uint64_t* m, const uint64_t* r, uint64_t* steps_out, size_t steps_cap,
                        uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out);
/* device-resident output form used by the prover pipeline (steps stay in HBM for K4) */
int pz_paillier_encrypt_dev(pz_ctx* ctx, uint32_t limbs_n, size_t batch, const uint64_t* n, const uint64_t* g,
                            const uint64_t* m, const uint64_t* r, uint64_t* d_steps_out, size_t steps_cap,
                            uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out);

/* Uniform-shape variant (NOT the reference's circuit): g^m as BigUintChip::pow_mod over exactly
 * m_bits in-circuit exponent bits -- per bit the step (acc, sq) [kept only if the bit is set: select] then the step (sq, sq)
 * -- so n_steps_g = 2 * m_bits for every message and one vk / pk serves every proof of a key.  r^n and the final mul_mod as
 * above.  PZ_ERR_MESSAGE_RANGE if a message does not fit m_bits.  Same buffer conventions as pz_paillier_encrypt[_dev]. */
int pz_paillier_encrypt_uniform(pz_ctx* ctx, uint32_t limbs_n, size_t batch, uint32_t m_bits, const uint64_t* n, const uint64_t* g,
                                const uint64_t* m, const uint64_t* r, uint64_t* steps_out, size_t steps_cap, uint32_t* n_steps_g,
                                uint32_t* n_steps_r, uint64_t* c_out);
int pz_paillier_encrypt_uniform_dev(pz_ctx* ctx, uint32_t limbs_n, size_t batch, uint32_t m_bits, const uint64_t* n,
                                    const uint64_t* g, const uint64_t* m, const uint64_t* r, uint64_t* d_steps_out, size_t steps_cap,
                                    uint32_t* n_steps_g, uint32_t* n_steps_r, uint64_t* c_out);

/* Tally: C = c_1 * ... * c_count mod n^2, PaillierChip::add (paillier.rs:62-85) folded over `count` FULL-WIDTH ciphertexts
 * (2*limbs_n limbs each, cts = count x 2*limbs_n words) as a product tree, 2 <= count <= 65536 (else PZ_ERR_INVALID):
 *   cur = [c_1 .. c_count]; while len(cur) > 1: nxt = [mul_mod(cur[2j], cur[2j+1]) for j < len(cur)/2], an odd last element is
 *   carried up without a product; cur = nxt.
 * The count - 1 records a|b|q|r are numbered in the order this loop creates them (level-major); c_out = the root.  n^2 is formed
 * on the device; one launch per level on the context's stream, no host synchronisation between levels.  steps_out (steps_cap >=
 * count - 1 records, else PZ_ERR_CAPACITY) may be NULL: the value only.  A ciphertext >= n^2 is PZ_ERR_RANGE (the chain kernel's
 * range bit: the circuit's r < n^2 check of such a value cannot hold), n = 0 is PZ_ERR_ZERO_MODULUS.  Same host / device split and
 * buffer conventions as pz_paillier_encrypt[_dev]. */
int pz_paillier_tally(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, uint64_t* steps_out,
                      size_t steps_cap, uint64_t* c_out);
int pz_paillier_tally_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, uint64_t* d_steps_out,
                          size_t steps_cap, uint64_t* c_out);

/* Weighted tally: C = c_1^w_1 * ... * c_count^w_count mod n^2 = Enc(sum w_i m_i), Paillier's scalar homomorphism folded into the tally.
 * 1 <= count <= 65536, 1 <= w_bits <= 64 (else PZ_ERR_INVALID); weights = count 64-bit words (HOST), each below 2^w_bits (else
 * PZ_ERR_MESSAGE_RANGE, checked before any launch); cts as pz_paillier_tally.
 *   power_i = BigUintChip::pow_mod(c_i, w_i) over EXACTLY w_bits in-circuit bits, LSB first (the uniform schedule of
 *   pz_paillier_encrypt_uniform's g^m): per bit the step (acc, sq) then the step (sq, sq), acc takes the product only where the bit is
 *   set; acc starts at 1, sq at c_i.  The trailing square of every chain is kept: it is the dependency's pow_mod as it stands.
 *   Then the product tree of pz_paillier_tally over power_1 .. power_count (count = 1: no tree, C = power_1).
 * Records a|b|q|r: first the chains' 2 * count * w_bits, chain-major (chain i, bit j at 2 (i w_bits + j) and the next), then the
 * tree's count - 1 in level-major order; c_out = the root.  One team per chain (one launch for all chains: no workgroup waits on
 * another), one launch per tree level, all on the context's stream without host synchronisation in between; n^2 and its Barrett
 * constants are formed once.  steps_out (steps_cap >= 2 count w_bits + count - 1 records, else PZ_ERR_CAPACITY) may be NULL: the value
 * only.  A ciphertext >= n^2 is PZ_ERR_RANGE, n = 0 is PZ_ERR_ZERO_MODULUS.  Same host / device split and buffer conventions as
 * pz_paillier_tally[_dev].  (PZ_ABI_VERSION stays 7: these are additions, nothing existing changes.) */
int pz_paillier_wtally(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t w_bits, const uint64_t* n, const uint64_t* cts,
                       const uint64_t* weights, uint64_t* steps_out, size_t steps_cap, uint64_t* c_out);
int pz_paillier_wtally_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t w_bits, const uint64_t* n, const uint64_t* cts,
                           const uint64_t* weights, uint64_t* d_steps_out, size_t steps_cap, uint64_t* c_out);

/* Ballot: c_i = g^m_i * r_i^n mod n^2 for i = 1..count under ONE key (n, g) -- the values of circuit kind 6 ("ballot": every c_i holds
 * a message below 2^m_bits, and for count >= 2 the messages add up to a public S).  1 <= count <= 1024,
 * 1 <= m_bits <= 64 (else PZ_ERR_INVALID); n, g: limbs_n words each; ms = count 64-bit words, ONE per message; rs = count x limbs_n
 * words; c_out = count x 2*limbs_n words (all HOST).  Per entry, in this order:
 *   gm_i = BigUintChip::pow_mod(g, m_i) over EXACTLY m_bits in-circuit bits, LSB first (pz_paillier_wtally's chain on the base g): per
 *   bit the step (acc, sq) then the step (sq, sq), acc takes the product only where the bit is set; the trailing square is kept;
 *   rn_i = pow_mod_fixed_exp(r_i, n): per bit of n, LSB first, the step (cur, cur), then on a set bit the step (acc, cur) -- nr =
 *   bits(n) + popcount(n) steps, the same for every entry (n is public: its bits shape the circuit, as in pz_paillier_encrypt);
 *   the step (gm_i, rn_i), whose remainder is c_i.
 * Records a|b|q|r of 2*limbs_n words per field, ciphertext-major: entry i at records i * (2 m_bits + nr + 1) and on.  *n_steps_r (may
 * be NULL) = nr, ONE value.  steps_out (steps_cap >= count * (2 m_bits + nr + 1) records, else PZ_ERR_CAPACITY) may be NULL: the
 * values only.  Refusals, in this order: a null pointer, limbs_n = 0, count or m_bits out of range: PZ_ERR_INVALID; 2*limbs_n > 128:
 * PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; a message >= 2^m_bits: PZ_ERR_MESSAGE_RANGE; n = 0: PZ_ERR_ZERO_MODULUS --
 * all before any launch.  r_i is not compared with n and r_i = 0 is not refused (neither does the circuit: kind 2's property).
 * One team per ciphertext, ONE launch for all entries, no workgroup waits on another; n^2 and its Barrett constants are formed once.
 * The messages and the r_i are secrets: a message's bit reaches the accumulator as a lane-wise mask, no branch or address depends on
 * m_i or r_i (the value-dependent trip count of mul_mod's Barrett correction remains, as in every K3 entry point), and the staged
 * copies of ms and rs (host form: of the records too) in the context's workspace are overwritten before the call returns.
 * _dev: d_steps_out is a DEVICE buffer; everything else as above.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_ballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, const uint64_t* n, const uint64_t* g,
                       const uint64_t* ms, const uint64_t* rs, uint64_t* steps_out, size_t steps_cap, uint32_t* n_steps_r, uint64_t* c_out);
int pz_paillier_ballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, const uint64_t* n, const uint64_t* g,
                           const uint64_t* ms, const uint64_t* rs, uint64_t* d_steps_out, size_t steps_cap, uint32_t* n_steps_r,
                           uint64_t* c_out);

/* Short-randomness ballot (Damgard-Jurik-Nielsen encryption, "DJN mode"): c_i = g^m_i * hs^s_i mod n^2 for i = 1..count under ONE key
 * (n, g, hs), hs = h^n mod n^2 with h = -x^2 mod n for a random unit x (keys.djn_generator, pz::djn_generator) -- an ordinary Paillier
 * ciphertext with r_i = h^s_i mod n, which tally, weighted tally, mix, decrypt, partial and combine take unchanged (DESIGN.md section
 * 15.18).  Security rests on the short-exponent assumption in <hs>: s_bits is the caller's, customarily at least twice the security
 * level, and has no default.  1 <= count <= 1024, 1 <= m_bits <= 64, 1 <= s_bits <= 128*limbs_n (else PZ_ERR_INVALID); n, g: limbs_n
 * words each; hs: 2*limbs_n words; ms = count 64-bit words, ONE per message; ss = count x ceil(s_bits/64) words; c_out = count x
 * 2*limbs_n words (all HOST).  Per entry, in this order:
 *   gm_i = BigUintChip::pow_mod(g, m_i) over EXACTLY m_bits in-circuit bits, LSB first (pz_paillier_ballot's g-chain): per bit the
 *   step (acc, sq) then the step (sq, sq), acc takes the product only where the bit is set; the trailing square is kept;
 *   hss_i = BigUintChip::pow_mod(hs, s_i) over EXACTLY s_bits bits in the same schedule (pz_paillier_partial's chain on the base hs);
 *   the step (gm_i, hss_i), whose remainder is c_i.
 * Records a|b|q|r of 2*limbs_n words per field, ciphertext-major: entry i at records i * (2 m_bits + 2 s_bits + 1) and on; n is not
 * in the count.  steps_out (steps_cap >= count * (2 m_bits + 2 s_bits + 1) records, else PZ_ERR_CAPACITY) may be NULL: the values only.
 * Refusals, in this order: a null pointer, limbs_n = 0, count, m_bits or s_bits out of range: PZ_ERR_INVALID; 2*limbs_n > 128:
 * PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; a message >= 2^m_bits or an s_i >= 2^s_bits: PZ_ERR_MESSAGE_RANGE; n = 0:
 * PZ_ERR_ZERO_MODULUS -- all before any launch.  An hs >= n^2: PZ_ERR_RANGE (found by the kernel, which then writes nothing; the status
 * is read before anything is copied out).  No output buffer is written on a refusal.  hs = 0 is not refused here
 * (verifier.public_inputs("sballot") refuses it).
 * One team per ciphertext runs both chains and the product, ONE launch for all entries, no workgroup waits on another; n^2 and its
 * Barrett constants are formed once.  The messages and the s_i are SECRET: bit t of s_i is read from word t / 64, an address that
 * depends on t alone, and reaches the accumulator as a lane-wise mask; no branch or address depends on m_i or s_i (the value-dependent
 * trip count of mul_mod's Barrett correction remains, as in every K3 entry point), and the staged copies of ms and ss (host form: of
 * the records too) in the context's workspace are overwritten before the call returns.
 * _dev: d_steps_out is a DEVICE buffer; everything else as above.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_sballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                        const uint64_t* g, const uint64_t* hs, const uint64_t* ms, const uint64_t* ss, uint64_t* steps_out,
                        size_t steps_cap, uint64_t* c_out);
int pz_paillier_sballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                            const uint64_t* g, const uint64_t* hs, const uint64_t* ms, const uint64_t* ss, uint64_t* d_steps_out,
                            size_t steps_cap, uint64_t* c_out);

/* Packed ballot: K = slots choices in ONE ciphertext, c_i = (prod_j G_j^v_ij) * hs^s_i mod n^2 for i =
 * 1..count under ONE key (n, hs) and the public slot bases G_j = g^(2^(j w)) mod n^2, j = 0..K-1 (keys.pballot_bases, pz::pballot_bases:
 * read from ONE pz_paillier_trace) -- an ordinary short-randomness ciphertext of M_i = sum_j v_ij 2^(j w), which tally, weighted tally,
 * mix, decrypt, partial and combine take unchanged; the homomorphic product adds every slot at once (keys.pballot_capacity states how
 * many ballots a slot holds before it carries).  Neither g nor w is an argument: the bases carry both.  1 <= count <= 1024, 1 <= slots
 * <= 64, count * slots <= 1024, 1 <= m_bits <= 64, 1 <= s_bits <= 128*limbs_n (else PZ_ERR_INVALID); n: limbs_n words; hs: 2*limbs_n
 * words; gs = slots x 2*limbs_n words; vs = count x slots 64-bit words, ONE per value, ciphertext-major; ss = count x ceil(s_bits/64)
 * words; c_out = count x 2*limbs_n words (all HOST).  Per entry, in this order:
 *   for j = 0..K-1, P_j = BigUintChip::pow_mod(G_j, v_ij) over EXACTLY m_bits in-circuit bits, LSB first (pz_paillier_sballot's
 *   g-chain on the base G_j): per bit the step (acc, sq) then the step (sq, sq); the trailing square is kept;
 *   hss_i = BigUintChip::pow_mod(hs, s_i) over EXACTLY s_bits bits in the same schedule;
 *   the folds (P_0, P_1) -> t_1, (t_1, P_2) -> t_2, .., (t_{K-1}, hss_i) -> c_i (with K = 1 the one step (P_0, hss_i)).
 * Records a|b|q|r of 2*limbs_n words per field, ciphertext-major: entry i at records i * per and on, per = 2 m_bits K + 2 s_bits + K --
 * slot j's chain at 2 m_bits j, the hs-chain at 2 m_bits K, the K folds last.  With K = 1 and G_0 = g this is pz_paillier_sballot's
 * entry bit for bit.  steps_out (steps_cap >= count * per records, else PZ_ERR_CAPACITY) may be NULL: the values only.
 * Refusals, in this order: a null pointer, limbs_n = 0, count, slots, count * slots, m_bits or s_bits out of range: PZ_ERR_INVALID;
 * 2*limbs_n > 128: PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; a value >= 2^m_bits or an s_i >= 2^s_bits:
 * PZ_ERR_MESSAGE_RANGE; n = 0: PZ_ERR_ZERO_MODULUS -- all before any launch.  An hs or any G_j >= n^2: PZ_ERR_RANGE (found by the kernel,
 * which then writes nothing; the status is read before anything is copied out).  No output buffer is written on a refusal.
 * One team per ciphertext runs its K slot chains, its hs-chain and the folds, ONE launch for all entries, no workgroup waits on another;
 * n^2 and its Barrett constants are formed once.  The values and the s_i are SECRET: v_ij is read from word i K + j and bit t of s_i
 * from word t / 64, addresses that depend on loop counters alone, and both reach their accumulators as a lane-wise mask; no branch or
 * address depends on them (the value-dependent trip count of mul_mod's Barrett correction remains, as in every K3 entry point), and
 * the staged copies of vs and ss (host form: of the records too) in the context's workspace are overwritten before the call returns.
 * _dev: d_steps_out is a DEVICE buffer; everything else as above.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_pballot(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t slots, uint32_t m_bits, uint32_t s_bits, const uint64_t* n,
                        const uint64_t* hs, const uint64_t* gs, const uint64_t* vs, const uint64_t* ss, uint64_t* steps_out,
                        size_t steps_cap, uint64_t* c_out);
int pz_paillier_pballot_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t slots, uint32_t m_bits, uint32_t s_bits,
                            const uint64_t* n, const uint64_t* hs, const uint64_t* gs, const uint64_t* vs, const uint64_t* ss,
                            uint64_t* d_steps_out, size_t steps_cap, uint64_t* c_out);

/* The mix: a verifiable shuffle's values.  A mixer takes c_1 .. c_K under the key n and publishes
 * c'_i = c_perm(i) * r_i^n mod n^2: the same plaintexts, re-randomised, in an order nobody else can follow.  K = count is a power of two
 * in 1 .. 1024; n: limbs_n words; cts = count x 2*limbs_n words; rs = count x limbs_n words; mixed_out = count x 2*limbs_n words (HOST).
 * The permutation arrives as the switch bits of a Benes network over the K positions (pz_mix_route makes them from perm):
 *   d = log2 K, 2d - 1 layers l = 0 .. 2d - 2 (none for K = 1); layer l acts on bit beta(l) = l for l < d and 2d - 2 - l above;
 *   switch s of a layer is the s-th position j, ascending, with bit beta clear, its partner j' = j | 2^beta; with bit b the switch
 *   leaves out[j] = b ? in[j'] : in[j] and out[j'] = b ? in[j] : in[j'].  Values stay in place: no wire shuffle between layers.
 *   bits: (2d - 1) * K / 2 bytes, layer-major, each 0 or 1 (may be NULL for K = 1).  ANY bits give SOME permutation.
 * routes_out (may be NULL): every layer's outputs, routes[l][position][2*limbs_n], (2d - 1) * K * 2*limbs_n words.  steps_out
 * (steps_cap >= count * (nr + 1) records, else PZ_ERR_CAPACITY; may be NULL: the values only): records a|b|q|r of 2*limbs_n words per
 * field, output-major -- output i's nr = bits(n) + popcount(n) records of pow_mod_fixed_exp(r_i, n) (per bit of n, LSB first, the step
 * (cur, cur), then on a set bit the step (acc, cur): pz_paillier_ballot's r-chain), then the step (d_i, rn_i), d_i the last layer's
 * value at position i (c_1 for K = 1), whose remainder is c'_i.
 * Refusals, in this order: a null pointer, limbs_n = 0, a count that is no power of two in 1 .. 1024: PZ_ERR_INVALID; 2*limbs_n > 128:
 * PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; a bit byte above 1: PZ_ERR_MESSAGE_RANGE; n = 0: PZ_ERR_ZERO_MODULUS -- all
 * before any launch.  A c_j >= n^2: PZ_ERR_RANGE (found by the kernel).  No output buffer is written on a refusal.  r_i is not compared
 * with n and r_i = 0 is not refused (c'_i = 0 then: verifier.public_inputs("mix") refuses such a list).
 * One launch per layer over its K / 2 switches, then ONE launch of K teams for the r^n chains and products; no workgroup waits on
 * another; n^2 and its Barrett constants are formed once.  The bits, the r_i and the route layers are SECRET: a switch reads both
 * inputs and writes both outputs under a lane-wise mask made from its bit, no address or branch depends on a bit or on r_i (the
 * value-dependent trip count of mul_mod's Barrett correction remains, as in every K3 entry point), and the staged bits and r_i (host
 * form: the staged routes and records too) in the context's workspace are overwritten before the call returns.
 * _dev: d_routes_out and d_steps_out are DEVICE buffers (either may be NULL; the kernels have written them by the time a c_j >= n^2
 * is reported); everything else as above.
 *   pz_mix_route   host logic, no context: the switch bits of perm (perm[i] = the index of the input that output position i
 *       receives), by the looping algorithm; bits_out: (2d - 1) * K / 2 bytes (may be NULL for K = 1).  A count that is no power of
 *       two in 1 .. 1024, a perm that is no permutation of 0 .. K - 1, a null pointer: PZ_ERR_INVALID, bits_out untouched.  Its working
 *       memory is overwritten before it returns.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_mix(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, const uint8_t* bits,
                    const uint64_t* rs, uint64_t* routes_out, uint64_t* steps_out, size_t steps_cap, uint64_t* mixed_out);
int pz_paillier_mix_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, const uint64_t* n, const uint64_t* cts, const uint8_t* bits,
                        const uint64_t* rs, uint64_t* d_routes_out, uint64_t* d_steps_out, size_t steps_cap, uint64_t* mixed_out);
int pz_mix_route(size_t count, const uint32_t* perm, uint8_t* bits_out);

/* The short-randomness mix: a mixer of an election that casts short-randomness ballots publishes
 * c'_i = c_perm(i) * hs^s_i mod n^2 under the key (n, hs), hs = h^n mod n^2 (keys.djn_generator) -- pz_paillier_mix with every r_i^n
 * chain of bits(n) + popcount(n) steps replaced by an hs^s_i chain of 2 s_bits steps over a SHORT secret s_i.  c'_i holds what
 * c_perm(i) holds only if hs is an n-th residue: that is the key authority's to show (circuit kind 5, or kind 7 and a combiner), not
 * this call's.  Hiding rests on the short-exponent assumption in <hs>: s_bits is the caller's and has no default.  K = count is a power
 * of two in 1 .. 1024, 1 <= s_bits <= 128*limbs_n; n: limbs_n words; hs: 2*limbs_n words; cts = count x 2*limbs_n words; ss = count x
 * ceil(s_bits/64) words, as pz_paillier_sballot takes them; bits, routes_out, mixed_out exactly as pz_paillier_mix (HOST).
 * The network is pz_paillier_mix's, launched as it launches it: on the same cts and bits the route layers are the same words.
 * steps_out (steps_cap >= count * (2 s_bits + 1) records, else PZ_ERR_CAPACITY; may be NULL: the values only): records a|b|q|r of
 * 2*limbs_n words per field, output-major -- output i's 2 s_bits records of BigUintChip::pow_mod(hs, s_i) over EXACTLY s_bits bits,
 * LSB first (per bit the step (acc, sq) then the step (sq, sq), acc takes the product only where the bit is set; the trailing square
 * is kept: pz_paillier_partial's and pz_paillier_sballot's chain), then the step (d_i, hss_i), d_i the last layer's value at position
 * i (c_1 for K = 1), whose remainder is c'_i.
 * Refusals, in this order: a null pointer (bits and routes_out may be NULL for K = 1), limbs_n = 0, a count that is no power of two in
 * 1 .. 1024, s_bits out of range: PZ_ERR_INVALID; 2*limbs_n > 128: PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; a bit byte
 * above 1 or an s_i >= 2^s_bits: PZ_ERR_MESSAGE_RANGE; n = 0: PZ_ERR_ZERO_MODULUS -- all before any launch.  An hs >= n^2 or a c_j >=
 * n^2: PZ_ERR_RANGE (found by the kernel; the status is read before anything is copied out).  No output buffer is written on a
 * refusal.  hs = 0 and s_i = 0 are not refused (verifier.public_inputs("smix") refuses hs = 0 and an output 0).
 * One launch per layer over its K / 2 switches, then ONE launch of K teams for the chains and products; no workgroup waits on
 * another; n^2 and its Barrett constants are formed once.  The bits, the s_i and the route layers are SECRET: a switch reads both
 * inputs and writes both outputs under a lane-wise mask made from its bit, bit t of s_i is read from word t / 64, an address that
 * depends on t alone, and reaches the accumulator as a lane-wise mask; no address or branch depends on a bit or on s_i (the
 * value-dependent trip count of mul_mod's Barrett correction remains, as in every K3 entry point), and the staged bits and s_i (host
 * form: the staged routes and records too) in the context's workspace are overwritten before the call returns.
 * _dev: d_routes_out and d_steps_out are DEVICE buffers (either may be NULL; the kernels have written them by the time a c_j >= n^2
 * is reported) and stay the caller's to overwrite; everything else as above.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_smix(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t s_bits, const uint64_t* n, const uint64_t* hs,
                     const uint64_t* cts, const uint8_t* bits, const uint64_t* ss, uint64_t* routes_out, uint64_t* steps_out,
                     size_t steps_cap, uint64_t* mixed_out);
int pz_paillier_smix_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t s_bits, const uint64_t* n, const uint64_t* hs,
                         const uint64_t* cts, const uint8_t* bits, const uint64_t* ss, uint64_t* d_routes_out, uint64_t* d_steps_out,
                         size_t steps_cap, uint64_t* mixed_out);

/* Decryption with randomness recovery, for the key holder.  The secret key is a handle: n, g, lambda and d = n^-1 mod lambda
 * (HOST words, limbs_n each; d is the caller's -- paillier_halo2_amd/keys.py::secret_from_primes computes it).
 *   pz_paillier_sk_create  forms n^2 and the Barrett constants of n^2 and of n once, derives on the device x = L(g^lambda mod n^2),
 *       mu = x^(lambda-1) mod n and ginv = (g mod n)^(lambda-1) mod n (both orders divide lambda: no inversion routine), and checks
 *       g^lambda mod n^2 = 1 (mod n), x mu = 1 (mod n), n d = 1 (mod lambda) and 0 < d < lambda < n: anything else is PZ_ERR_INVALID
 *       (lambda + 1, d + 1, g = 1 ...).  n = 0: PZ_ERR_ZERO_MODULUS; 2 * limbs_n > 128: PZ_ERR_UNSUPPORTED.  Synchronises.  The staging
 *       copies of lambda - 1 and x in the shared workspaces are overwritten before it returns.
 *   pz_paillier_sk_params  mu and ginv (HOST, limbs_n words each), for tests and bindings.
 *   pz_paillier_sk_free    overwrites the handle's device memory (lambda, d, mu) in stream order, then releases it.  NULL is PZ_OK.
 *   pz_paillier_decrypt    1 <= count <= 65536 (else PZ_ERR_INVALID) ciphertexts of 2 * limbs_n words (HOST).  Per ciphertext
 *       u = c^lambda mod n^2; flags_out[i] bit 0 is set if u mod n != 1 (c is no unit: its m and r are written as zero), else
 *       m = floor(u / n) mu mod n and, if r_out is not NULL, r = ((c mod n) ginv^m)^d mod n with c = g^m r^n mod n^2 (an r >= n used at
 *       encryption comes back reduced mod n: it encrypts to the same c).  A c >= n^2 sets bit 1 of its flag, zeros its outputs and
 *       makes the call PZ_ERR_RANGE (the other entries are still written).  m_out, r_out: count x limbs_n words; flags_out: count
 *       bytes.  One launch per power over all ciphertexts (c^lambda; ginv^m, skipped when ginv = 1; the d-th power), a fixed-window
 *       schedule set by limbs_n and the bit length of n alone, the table entry chosen by reading all of them under a mask.
 *   pz_paillier_decrypt_dev  the same with DEVICE pointers, asynchronous on the context's stream: it returns once the launches are
 *       queued, and what the host form reports as PZ_ERR_RANGE is bit 1 of an entry's flag here. */
typedef struct pz_paillier_sk pz_paillier_sk;
int pz_paillier_sk_create(pz_ctx* ctx, uint32_t limbs_n, const uint64_t* n, const uint64_t* g, const uint64_t* lambda,
                          const uint64_t* d, pz_paillier_sk** out);
int pz_paillier_sk_params(const pz_paillier_sk* sk, uint64_t* mu_out, uint64_t* ginv_out);
int pz_paillier_sk_free(pz_ctx* ctx, pz_paillier_sk* sk);
int pz_paillier_decrypt(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out, uint64_t* r_out,
                        uint8_t* flags_out);
int pz_paillier_decrypt_dev(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* d_cts, uint64_t* d_m_out,
                            uint64_t* d_r_out, uint8_t* d_flags_out);

/* Decryption by the CRT: the same m, r, flags and return codes from half-length powers mod p^2 and q^2.
 *   pz_paillier_sk_create_crt  everything pz_paillier_sk_create does, through the same code (the lambda path of the handle is the
 *       same), then the CRT part in the handle's one device block, from p and q (HOST, limbs_n words each): the Barrett constants of
 *       p^2, q^2, p, q, p - 1, q - 1; h_P = (L_P(g^(P-1) mod P^2))^-1 mod P, qinv = q^-1 mod p, d_P = d mod (P - 1), ginv mod P.  All of
 *       it is derived on the device; the inverses are powers (h_P = x_P^(P-2) mod P, qinv = (q mod p)^(p-2) mod p).  Refused: a null
 *       pointer, p or q even or below 3, p q != n (checked on the device), x_P h_P != 1 (mod P) or q qinv != 1 (mod p) -- which a
 *       composite "prime" fails -- PZ_ERR_INVALID; p^2 or q^2 beyond limbs_n words PZ_ERR_UNSUPPORTED (the rule that makes every
 *       quotient fit; the primes need not be of equal length; every balanced key passes).  Primality itself is NOT tested:
 *       pz_bigint_is_prime is there for the caller.  p and q may come in either order.  Synchronises.  The staged copies of p, q,
 *       p - 1, p - 2 ... on the host and in the shared workspace are overwritten on every path out; pz_paillier_sk_free overwrites
 *       the whole block.
 *   pz_paillier_sk_has_crt  1 if the handle holds a CRT part, else 0 (NULL: 0).
 *   pz_paillier_decrypt_crt, pz_paillier_decrypt_crt_dev  the arguments, results, flags, return codes and count bounds of
 *       pz_paillier_decrypt[_dev], bit for bit; a handle without a CRT part is PZ_ERR_INVALID.  (pz_paillier_decrypt[_dev] never takes
 *       this path.)  Launches: the split c mod P^2 at the capacity of n^2, one power launch over both sides of every ciphertext
 *       (2 count teams at 64 limbs whatever the key size, exponent P - 1, the fixed-window schedule of pz_paillier_decrypt over the bit
 *       length of P), Garner; for r one more power launch (ginv mod P to m mod (P - 1), skipped when ginv = 1, and the d_P-th power,
 *       back to back in one team) and one more Garner.  No instruction stream or address depends on p, q, h_P, qinv, d_P or on any
 *       intermediate; the bit lengths of p and q are the key's public shape.  What stays value-dependent is mul_mod's Barrett
 *       correction count, as in every K3 entry point -- here it also runs under the SECRET moduli p^2, q^2, p, q, p - 1, q - 1.
 *       The workspace intermediates (c mod P^2 -- one of them factors n --, the side results, m mod (P - 1), c mod P) are
 *       overwritten before the host form returns, on every path, and in stream order behind the last kernel in the _dev form.
 * (PZ_ABI_VERSION stays 7: additions.) */
int pz_paillier_sk_create_crt(pz_ctx* ctx, uint32_t limbs_n, const uint64_t* n, const uint64_t* g, const uint64_t* lambda,
                              const uint64_t* d, const uint64_t* p, const uint64_t* q, pz_paillier_sk** out);
int pz_paillier_sk_has_crt(const pz_paillier_sk* sk);
int pz_paillier_decrypt_crt(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* cts, uint64_t* m_out, uint64_t* r_out,
                            uint8_t* flags_out);
int pz_paillier_decrypt_crt_dev(pz_ctx* ctx, const pz_paillier_sk* sk, size_t count, const uint64_t* d_cts, uint64_t* d_m_out,
                                uint64_t* d_r_out, uint8_t* d_flags_out);

/* T-of-T threshold decryption.  A dealer splits theta = lambda (lambda^-1 mod n) additively into T shares
 * (paillier_halo2_amd/keys.py::deal_shares, PaillierChip::deal_shares); the public threshold key holds n, g, a base v, h_i = v^theta_i
 * mod n^2 and mu2 = (2a)^-1 mod n with 1 + a n = g^theta mod n^2.  Nothing below ever sees lambda.
 *   pz_paillier_partial   one trustee's partial decryptions of `count` ciphertexts (1 .. 1024, else PZ_ERR_INVALID) under its share
 *       theta < 2^e_bits, 1 <= e_bits <= 128 limbs_n (else PZ_ERR_INVALID): h = v^theta and u_j = (c_j^2)^theta mod n^2.  n: limbs_n
 *       words; v, theta, every c_j, h_out and every u_j: 2*limbs_n words (all HOST).  Chain 0 is BigUintChip::pow_mod(v, theta), chain
 *       j = 1 .. count is pow_mod(s_j, theta) with s_j = c_j^2 mod n^2, each over EXACTLY e_bits bits, LSB first (pz_paillier_wtally's
 *       chain): per bit the step (acc, sq) then the step (sq, sq), acc takes the product only where the bit is set; the trailing square
 *       is kept.  Records a|b|q|r of 2*limbs_n words per field: first the `count` squaring records (c_j, c_j, q, s_j), then chain i
 *       (0 .. count) at records count + i 2 e_bits and on -- count + (count + 1) 2 e_bits in all (steps_cap below that: PZ_ERR_CAPACITY;
 *       steps_out may be NULL: the values only).  Refusals, in this order and all before any launch: a null pointer, limbs_n = 0, count
 *       or e_bits out of range: PZ_ERR_INVALID; 2*limbs_n > 128: PZ_ERR_UNSUPPORTED; a short steps_cap: PZ_ERR_CAPACITY; theta >=
 *       2^e_bits: PZ_ERR_MESSAGE_RANGE; n = 0: PZ_ERR_ZERO_MODULUS.  A v or c_j >= n^2 is PZ_ERR_RANGE (found on the device).
 *       One team per chain, ONE launch of count + 1 teams (a team squares its own ciphertext first), no workgroup waits on another; n^2
 *       and its Barrett constants are formed once.  theta is a SECRET: bit t is read from word t / 64, an address that depends on t
 *       alone, and reaches the accumulator as a lane-wise mask; no branch or trip count depends on it (the value-dependent trip count of
 *       mul_mod's Barrett correction remains, as in every K3 entry point); the staged copy of theta (host form: of the records too) in
 *       the context's workspace is overwritten before the call returns.
 *   pz_paillier_partial_dev   d_steps_out is a DEVICE buffer; everything else as above.
 *   pz_paillier_combine   m_j = L(U_j) mu2 mod n with U_j = prod_i u_ij mod n^2 over the `trustees` (1 .. 256) partials of each of `count`
 *       (1 .. 1024) ciphertexts; partials trustee-major (trustees x count x 2*limbs_n words), n and mu2 limbs_n words, m_out count x
 *       limbs_n words, flags_out count bytes (all HOST).  Flag bit 0: U mod n != 1 (the partials do not belong together; the entry's m is
 *       zero); bit 1: a partial >= n^2 (m zero; the call returns PZ_ERR_RANGE after writing every entry).  One team per ciphertext, one
 *       launch.  Nothing here is secret.
 *   pz_paillier_combine_dev   d_partials, d_m_out and d_flags_out are DEVICE buffers (n and mu2 stay HOST words); the work is queued on
 *       the context's stream and the call returns without waiting: the flags are the caller's to read.  (PZ_ABI_VERSION stays 7:
 *       additions.) */
int pz_paillier_partial(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t e_bits, const uint64_t* n, const uint64_t* v,
                        const uint64_t* theta, const uint64_t* cts, uint64_t* steps_out, size_t steps_cap, uint64_t* h_out, uint64_t* u_out);
int pz_paillier_partial_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, uint32_t e_bits, const uint64_t* n, const uint64_t* v,
                            const uint64_t* theta, const uint64_t* cts, uint64_t* d_steps_out, size_t steps_cap, uint64_t* h_out,
                            uint64_t* u_out);
int pz_paillier_combine(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t trustees, const uint64_t* n, const uint64_t* mu2,
                        const uint64_t* partials, uint64_t* m_out, uint8_t* flags_out);
int pz_paillier_combine_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t trustees, const uint64_t* n, const uint64_t* mu2,
                            const uint64_t* d_partials, uint64_t* d_m_out, uint8_t* d_flags_out);

/* t-of-T threshold decryption with Shamir shares.  A dealer shares theta by a polynomial f of degree t - 1
 * over Z_(n lambda), f(0) = theta, trustee i holds s_i = f(i) (paillier_halo2_amd/keys.py::deal_shamir, pz::deal_shamir); the trustees
 * open exactly as above (pz_paillier_partial, circuit kind 7: a share is a number below n lambda either way).  Any t of them combine:
 * with Delta = T! and the integers mu_i = Delta prod_{j in S, j != i} j / (j - i), A = prod_{mu_i > 0} u_i^mu_i and B = prod_{mu_i < 0}
 * u_i^|mu_i| satisfy A = B (1 + x n) mod n^2, so x = ((A - B mod n^2) / n) (B mod n)^-1 mod n and m = x mu2 mod n with the key's
 * mu2 = (2 a Delta)^-1 mod n: no inverse mod n^2, one inverse of an n-sized value mod n.
 *   pz_bigint_mod_inverse   inv_j = x_j^-1 mod `mod` for `count` (1 .. 65536) values of `limbs` words under ONE odd modulus (mod: limbs
 *       words; xs, inv_out: count x limbs words; flags_out: count bytes; all HOST).  Refusals, in this order and all before any launch:
 *       a null pointer, limbs = 0, count out of range: PZ_ERR_INVALID; limbs > 128: PZ_ERR_UNSUPPORTED; mod = 0: PZ_ERR_ZERO_MODULUS;
 *       mod even or mod = 1: PZ_ERR_INVALID.  flags_out[j] bit 0: gcd(x_j, mod) != 1 (x_j = 0 included), the output is zero; bit 1:
 *       x_j >= mod, the output is zero and the call returns PZ_ERR_RANGE after writing every entry; bit 2: the iteration bound ran out
 *       (cannot happen for an odd modulus; PZ_ERR_HIP).  The result is canonical, in [0, mod).  One wavefront per value runs a
 *       right-shift binary extended Euclid of at most 2 bitlen(mod) + 4 steps, a bound taken from the modulus alone.  Nothing here is
 *       secret: branches and trip counts follow the operands.
 *   pz_bigint_mod_inverse_dev   d_xs, d_inv_out and d_flags_out are DEVICE buffers (mod stays HOST words); the work is queued on the
 *       context's stream and the call returns without waiting: the flags are the caller's to read.
 *   pz_paillier_combine_t   the combiner for `members` (1 .. 256) partials of each of `count` (1 .. 1024) ciphertexts.  partials
 *       member-major (members x count x 2*limbs_n words), as pz_paillier_combine has them; exps: members x exp_words (1 .. 64) words, the
 *       magnitudes |mu_i|; neg: one sign byte (0 or 1) per member; n and mu2 limbs_n words; m_out count x limbs_n words; flags_out count
 *       bytes (all HOST).  Refusals, in this order and all before any launch: a null pointer, limbs_n = 0, count, members or exp_words
 *       out of range: PZ_ERR_INVALID; 2*limbs_n > 128: PZ_ERR_UNSUPPORTED; n = 0: PZ_ERR_ZERO_MODULUS; a zero exponent: PZ_ERR_INVALID;
 *       a sign byte > 1: PZ_ERR_INVALID.  n must be odd (an even n ends in flag bit 2).  Flag bit 0: A mod n != B mod n (the partials
 *       do not belong together or are too few; m zero); bit 1: a partial >= n^2 (m zero; PZ_ERR_RANGE after writing every entry); bit
 *       2: an internal check failed (PZ_ERR_HIP); bit 3: B mod n is not a unit (m zero).  With every exponent 1, no negative sign and a
 *       T-of-T key's mu2 this is pz_paillier_combine, bit for bit.  One team per ciphertext, one launch; A and B are interleaved
 *       (Straus) chains over the longest exponent's bits.  Nothing here is secret.
 *   pz_paillier_combine_t_dev   d_partials, d_m_out and d_flags_out are DEVICE buffers (n, mu2, exps and neg stay HOST); asynchronous
 *       on the context's stream.
 *   pz_shamir_lagrange   host logic, no context: for the `members` (1 .. trustees) distinct ids (1 .. trustees <= 256) of a combination,
 *       |mu_i| into exps_out (members x exp_words words, in the order of ids) and its sign into neg_out (1: negative).  Anything else:
 *       PZ_ERR_INVALID.  *words_needed (may be NULL) receives the words of the longest magnitude; exp_words below that: PZ_ERR_CAPACITY
 *       with nothing written to exps_out.  |mu_i| < (T!)^2 < 2^3368: 64 words always suffice.  (PZ_ABI_VERSION stays 7: additions.) */
int pz_bigint_mod_inverse(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* mod, const uint64_t* xs, uint64_t* inv_out,
                          uint8_t* flags_out);
int pz_bigint_mod_inverse_dev(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* mod, const uint64_t* d_xs, uint64_t* d_inv_out,
                              uint8_t* d_flags_out);
int pz_paillier_combine_t(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2,
                          const uint64_t* exps, uint32_t exp_words, const uint8_t* neg, const uint64_t* partials, uint64_t* m_out,
                          uint8_t* flags_out);
int pz_paillier_combine_t_dev(pz_ctx* ctx, uint32_t limbs_n, size_t count, size_t members, const uint64_t* n, const uint64_t* mu2,
                              const uint64_t* exps, uint32_t exp_words, const uint8_t* neg, const uint64_t* d_partials, uint64_t* d_m_out,
                              uint8_t* d_flags_out);
int pz_shamir_lagrange(uint32_t trustees, size_t members, const uint32_t* ids, uint64_t* exps_out, uint32_t exp_words, uint8_t* neg_out,
                       uint32_t* words_needed);

/* Prime generation for Paillier keys: what keys.secret_from_primes / deal_shares / deal_shamir and the C++ dealers
 * take as arguments.  Every candidate is its own odd modulus: 16 lanes hold one candidate (four per wavefront), products are Montgomery
 * products of `limbs` outer steps, and a candidate's constants come from Newton steps and doublings, never from a division.
 *   pz_bigint_is_prime   Miller-Rabin on `count` (1 .. 65536) candidates of `limbs` (1 .. 32) words over `rounds` (1 .. 64) bases shared by
 *       all candidates (cands: count x limbs words; bases: rounds words, each >= 2; flags_out: count bytes; witness_out: count words; all
 *       HOST).  Refusals, in this order and all before any launch: a null pointer, limbs = 0, count or rounds out of range, a base < 2:
 *       PZ_ERR_INVALID; limbs > 32: PZ_ERR_UNSUPPORTED.  c < 2 or an even c > 2: flag 0, witness 0xFFFFFFFF; c = 2: flag 1, witness
 *       0xFFFFFFFF.  Otherwise, with c - 1 = d 2^s and a = bases[k] mod c, round k passes if a is 0, 1 or c - 1, else if a^d is 1 or c - 1,
 *       else if one of the next s - 1 squarings gives c - 1.  witness_out[j] is the index of the first round that fails, or `rounds` if
 *       none does; flags_out[j] = 1 iff witness_out[j] = rounds.  Candidates may be SECRET (a prime found is key material): no branch and
 *       no address of the kernel depends on a candidate -- every group runs all 64 limbs exponent bits of every round, the bits act
 *       through lane masks and the verdict is a predicate; the device staging is overwritten before the call returns.
 *   pz_bigint_is_prime_dev   d_cands, d_flags_out and d_witness_out are DEVICE buffers (bases stay HOST words); the work is queued on the
 *       context's stream and the call returns without waiting.
 *   pz_prime_sieve   the trial-division sieve alone over the `window` (1 .. 2^20) candidates c_i = start + stride i: mask_out[i] = 1 iff no
 *       odd prime p below 2^16 (6541 of them) divides c_i and -- with safe = 1 -- none divides (c_i - 1) / 2, i.e. c_i != 1 mod p.  safe = 0:
 *       stride 2, start odd; safe = 1: stride 4, start = 3 mod 4.  start: limbs words, mask_out: window bytes (HOST).  Refusals, in this
 *       order and all before any launch: a null pointer, limbs = 0, window out of range, safe > 1: PZ_ERR_INVALID; limbs > 32:
 *       PZ_ERR_UNSUPPORTED; start below 2^32 (so that no candidate is a sieve prime) or of the wrong residue: PZ_ERR_INVALID;
 *       start + stride (window - 1) does not fit limbs words: PZ_ERR_RANGE.  Not constant time in start.
 *   pz_prime_search   the `want` (1 .. 64) smallest offsets i of that window whose c_i survives the sieve and passes all `rounds` rounds of
 *       pz_bigint_is_prime over `bases` -- and, with safe = 1, whose (c_i - 1) / 2 passes them too -- ascending in offsets_out (want
 *       words); *found_out may be less than want, and an empty result is PZ_OK with *found_out = 0.  *survivors_out (may be NULL) receives
 *       the sieve's survivor count.  Refusals: those of the two calls above, a null offsets_out or found_out and want out of range
 *       (PZ_ERR_INVALID) first.  Survivors are tested in ascending batches, round 0 before the others, until want are found.  Every device
 *       buffer that held the start, residues, survivors or candidates is overwritten before the call returns.  (PZ_ABI_VERSION stays 7:
 *       additions.) */
int pz_bigint_is_prime(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* cands, uint32_t rounds, const uint64_t* bases,
                       uint8_t* flags_out, uint32_t* witness_out);
int pz_bigint_is_prime_dev(pz_ctx* ctx, uint32_t limbs, size_t count, const uint64_t* d_cands, uint32_t rounds, const uint64_t* bases,
                           uint8_t* d_flags_out, uint32_t* d_witness_out);
int pz_prime_sieve(pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe, uint8_t* mask_out);
int pz_prime_search(pz_ctx* ctx, uint32_t limbs, const uint64_t* start, size_t window, uint32_t safe, uint32_t rounds,
                    const uint64_t* bases, uint32_t want, uint32_t* offsets_out, uint32_t* found_out, size_t* survivors_out);

/* ---------------------------------------------------------------------------------------------
 * K4 -- expansion of a step trace into advice-column cells (Fr Montgomery, 32 B each), i.e. the
 * values halo2-lib's Context would hold after BigUintChip emitted the constraints of every
 * mul_mod (limb convolutions, range-check digit splits, carry chains).  Replaces the cell pushes
 * behind the dependency call sites paillier.rs:39-57, bench.rs:44-74.  Layout: DESIGN.md section 4.
 * ------------------------------------------------------------------------------------------- */
/* `limbs` = the circuit's limbs per big integer, each `limb_bits` wide (16..90: the reference uses 64 in
 * bench.rs:140 / paillier.rs:116 and 88 in its add test, paillier.rs:186-187).  Step records stay what K3 emits:
 * little-endian 64-bit words, words = ceil(limbs * limb_bits / 64) per big integer (== limbs at limb_bits 64);
 * K4 re-cuts them into limb_bits-wide limbs.  PZ_ERR_UNSUPPORTED outside 2*limb_bits + log2(limbs) + 3 <= 192. */
/* cells one mul_mod step expands to, for the given shape */
int pz_witness_cells_per_step(uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits, size_t* advice_cells,
                              size_t* lookup_cells);
/* d_steps: n_steps steps on the device (a|b|q|r, `words` 64-bit words each), d_modulus: `words` words on
 * the device; writes n_steps*advice_cells Fr elements to d_advice and n_steps*lookup_cells to
 * d_lookup (either may be NULL to skip). */
int pz_witness_expand_dev(pz_ctx* ctx, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits,
                          const uint64_t* d_steps, size_t n_steps, const uint64_t* d_modulus, uint64_t* d_advice,
                          uint64_t* d_lookup);

/* The WHOLE circuit's cell stream, operation by operation in the drivers' call order (bench.rs:33-75 paillier_enc_test,
 * kind = 0; bench.rs:77-117 paillier_enc_add_test, kind = 1): assign_integer of n, g, m|c1, r|c2; square + refresh of n
 * (paillier.rs:39-45 / 69-75); load_zero; for encrypt both pow_mod_fixed_exp chains (assign_constant(1), load_zero, their
 * mul_mod steps); the final mul_mod; assign_integer(res, 2*enc_bits); assert_equal_fresh.  Layout and per-operation cell
 * patterns: paillier_halo2_amd/layout.py::circuit_cells, DESIGN.md section 4 (dependency-derived, SURVEY tag [D]).
 * kind = 2: the uniform-shape encrypt circuit of pz_paillier_encrypt_uniform (g^m as pow_mod: num_to_bits of m's limbs, per
 * bit mul_mod + limb-wise select + square_mod; n_steps_g = 2 * limbs_n * limb_bits).
 * kind = 3: the tally of B = n_steps_g + 1 ciphertexts (pz_paillier_tally), n_steps_r = 0 (anything else: PZ_ERR_INVALID):
 * assign_integer(n); assign_integer(c_i, 2*enc_bits) for i = 1..B; square + refresh of n, once; the B - 1 mul_mod blocks of the
 * product tree in record order; assign_integer(res, 2*enc_bits); assert_equal_fresh(root, res).  No load_zero, no g, no pow_mod
 * constants.
 * kind = 4: the weighted tally (pz_paillier_wtally) of B = n_steps_r + 1 ciphertexts with W = n_steps_g / (2 B) bits per weight
 * (n_steps_g must be a multiple of 2 B and W in 1 .. 64, else PZ_ERR_INVALID): assign_integer(n); assign_integer(c_i, 2*enc_bits) for
 * i = 1..B; load_witness(w_i) for i = 1..B (B consecutive cells, no gate); square + refresh of n, once; per ciphertext
 * assign_constant(1), load_zero, num_to_bits(w_i, W) (7 W - 2 cells, tied to the load_witness cell) and W blocks of mul_mod(acc, sq),
 * limb-wise select, square_mod(sq); the B - 1 mul_mod blocks of the tree over the powers; assign_integer(res); assert_equal_fresh.
 * kind = 5: "decrypt" -- kind 2's circuit cell for cell from the same records (x = the plaintext m, y = the recovered randomness r of
 * pz_paillier_decrypt); its STATEMENT alone differs (pz_circuit_public_cells: n | g | m | c).  Accepted wherever kind 2 is:
 * pz_circuit_cells, pz_circuit_expand[_cols]_dev, pz_circuit_public_cells, pz_circuit_structure_dev (exp_g ignored, exp_r = n). */
int pz_circuit_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g,
                     size_t n_steps_r, size_t* advice_cells, size_t* lookup_cells);
/* inputs (HOST): n | g | x | y as ceil(limbs_n*limb_bits/64) 64-bit words each, then res as ceil(2*limbs_n*limb_bits/64)
 * words.  d_steps (device): the n_steps_g + n_steps_r + 1 step records K3 produced (add: one record); the circuit's
 * result c is the last record's remainder.  kind 3: inputs = n | c_1 .. c_B | res, ceil(limbs_n*limb_bits/64) words, then B times
 * ceil(2*limbs_n*limb_bits/64), then as many for res; d_steps holds EXACTLY B - 1 = n_steps_g records, the fields a|b|q|r of
 * ceil(2*limbs_n*limb_bits/64) words each.  pz_paillier_tally_dev writes fields of 2*ceil(limbs_n*limb_bits/64) words: the same where
 * 64 divides limbs_n*limb_bits (every 64-bit-limb shape), so its device buffer is passed as it stands; otherwise (264-bit n in 88-bit
 * limbs: 10 words against 9) the records are REPACKED to this width first, as host/paillier_chip.hpp's tally does.  The host inputs
 * of a large tally (B ciphertexts) are staged through pinned memory that grows to their size.  kind 4: inputs = n | c_1 .. c_B |
 * w_1 .. w_B | res with ONE 64-bit word per weight (a weight >= 2^W: PZ_ERR_MESSAGE_RANGE); d_steps holds the 2 B W chain records, then
 * the B - 1 tree records (pz_paillier_wtally_dev's order; repacked like kind 3's where the widths differ).  d_modulus: n^2 (device).
 * d_lookup may be NULL.
 * rows / col_stride cut the streams into the circuit's columns: cell c goes to column c / rows, row c % rows, columns
 * col_stride elements apart (rows = 2^k - blinding rows, col_stride = 2^k: every column is then a 2^k-row Lagrange vector
 * the commitment, product and NTT entry points take as it stands; rows above `rows` are not written).  0, 0 = dense. */
int pz_circuit_expand_dev(pz_ctx* ctx, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits,
                          const uint64_t* inputs, const uint64_t* d_steps, size_t n_steps_g, size_t n_steps_r,
                          const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride);

/* Circuit kind 6, "ballot" (DESIGN.md section 15.10): under the key (n, g) the K = count ciphertexts c_1 .. c_K (1 .. 1024) each encrypt a
 * value m_i < 2^b, b = m_bits (1 .. 64), and for K >= 2 their sum is the public S.  Its shape is K, b and the records of ONE r^n chain
 * (n_steps_r = bits(n) + popcount(n) >= 1), which do not fit n_steps_g / n_steps_r: the by-kind entry points refuse kind 6 and these take
 * the three numbers (anything out of range: PZ_ERR_INVALID).  The stream, in emission order: assign_integer(n), assign_integer(g);
 * load_witness(m_1 .. m_K) (K consecutive cells, no gate); for K >= 2 FlexGate::sum(m_1 .. m_K) = m_1 | 1 | m_2 | s_2 | 1 | m_3 | s_3 | ..
 * (1 + 3 (K - 1) cells, gate windows every 3 cells, the last s is S); assign_integer(r_i) for i = 1..K; square + refresh of n, once;
 * load_zero; per ciphertext pow_mod(g_ext, m_i) over exactly b bits (assign_constant(1), load_zero, num_to_bits(m_i, b) of 7 b - 2 cells
 * tied to the load_witness cell, then b blocks of mul_mod(acc, sq), limb-wise select, square_mod(sq): kind 4's chain with the trailing
 * square), pow_mod_fixed_exp(r_i_ext, n) ([1, 0], then the n_steps_r mul_mod blocks) and mul_mod(gm_i, rn_i); then per ciphertext
 * assign_integer(res_i, 2*enc_bits) and assert_equal_fresh(c_i, res_i).  The circuit neither compares r_i with n nor refuses r_i = 0.
 *   pz_ballot_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_ballot_expand_dev    the values.  inputs (HOST): n | g (ceil(limbs_n*limb_bits/64) words each) | m_1 .. m_K (ONE word each; a
 *       message >= 2^b: PZ_ERR_MESSAGE_RANGE) | r_1 .. r_K (as n) | res_1 .. res_K (ceil(2*limbs_n*limb_bits/64) words each).  d_steps
 *       (device): the K (2 b + n_steps_r + 1) records of pz_paillier_ballot_dev, ciphertext-major, fields of ceil(2*limbs_n*limb_bits/64)
 *       words (repacked first where that differs from 2*ceil(limbs_n*limb_bits/64), as for kinds 3 and 4).  d_modulus: n^2 (device).
 *       rows / col_stride as pz_circuit_expand_dev.
 *   pz_ballot_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_ballot_public_cells  the stream indices of the exposed cells in statement order: n | g | c_1 | .. | c_K (the limb cells of n's,
 *       g's and every res_i's assign_integer) and, for K >= 2, S (the sum's last cell): n_public = 2 limbs_n + K 2 limbs_n + (K >= 2). */
int pz_ballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_r,
                    size_t* advice_cells, size_t* lookup_cells);
int pz_ballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                         size_t n_steps_r, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice,
                         uint64_t* d_lookup, size_t rows, size_t col_stride);
int pz_ballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                              size_t n_steps_r, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                              uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts, size_t n_adv_cols, size_t max_rows,
                              size_t lookup_rows, size_t col_stride);
int pz_ballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, size_t n_steps_r,
                           uint64_t* cells_out, size_t capacity, size_t* n_public);

/* Circuit kind 7, "partial" (DESIGN.md section 15.11): one trustee's partial decryptions of K = count ciphertexts (1 .. 1024) under the
 * public threshold key's base v and its own h: there is ONE theta < 2^(2 enc_bits) with h = v^theta and u_j = (c_j^2)^theta mod n^2 for
 * every j.  Its shape is K and the key size alone; the by-kind entry points refuse kind 7 and these take `count` (out of range:
 * PZ_ERR_INVALID).  The stream, in emission order: assign_integer(n); assign_integer of v, theta, c_1 .. c_K at full width (2 limbs_n
 * limbs); square + refresh of n, once; load_zero; pow_mod(v, theta) exactly as kind 2 emits pow_mod -- [1, 0], then per limb of theta
 * num_to_bits(limb, limb_bits) and that limb's blocks of mul_mod(acc, sq), limb-wise select, square_mod(sq) --; per ciphertext
 * mul_mod(c_j, c_j) and pow_mod(s_j, theta) the same way; then assign_integer(h) + assert_equal_fresh, and the same for every u_j.  The
 * circuit compares nothing with n^2: a verifier refuses v, h, c_j or u_j >= n^2 outside it.
 *   pz_partial_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_partial_expand_dev    the values.  inputs (HOST): n (ceil(limbs_n*limb_bits/64) words) | v | theta | c_1 .. c_K | h | u_1 .. u_K
 *       (ceil(2*limbs_n*limb_bits/64) words each; theta >= 2^(2*limbs_n*limb_bits): PZ_ERR_MESSAGE_RANGE).  d_steps (device): the
 *       K + (K + 1) 2 E records of pz_paillier_partial_dev with e_bits = E = 2*limbs_n*limb_bits, as they are, fields of
 *       ceil(2*limbs_n*limb_bits/64) words (repacked first where that differs from 2*ceil(limbs_n*limb_bits/64), as for kinds 3, 4 and
 *       6).  d_modulus: n^2 (device).  rows / col_stride as pz_circuit_expand_dev.
 *   pz_partial_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_partial_public_cells  the stream indices of the exposed cells in statement order: n | v | h | c_1 | u_1 | .. | c_K | u_K (the limb
 *       cells of the assign_integer of each): n_public = limbs_n + (2 + 2 K) 2 limbs_n. */
int pz_partial_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t* advice_cells, size_t* lookup_cells);
int pz_partial_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, const uint64_t* inputs,
                          const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows,
                          size_t col_stride);
int pz_partial_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, const uint64_t* inputs,
                               const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup,
                               const uint64_t* d_col_starts, size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride);
int pz_partial_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint64_t* cells_out, size_t capacity,
                            size_t* n_public);

/* Circuit kind 8, "mix" (DESIGN.md section 15.17): the list c'_1 .. c'_K is a re-randomised permutation of the list c_1 .. c_K under the
 * key n -- there are a permutation pi and r_i with c'_i = c_pi(i) r_i^n mod n^2 for every i.  K = count is a power of two in 1 .. 1024.
 * Its shape is K and the records of ONE r^n chain (n_steps_r = bits(n) + popcount(n) >= 1); the by-kind entry points refuse kind 8 and
 * these take the two numbers (anything out of range: PZ_ERR_INVALID).  The stream, in emission order: assign_integer(n);
 * assign_integer(c_j) at full width (2 limbs_n limbs) for j = 1 .. K; assign_integer(r_i) for i = 1 .. K; square + refresh of n, once;
 * load_zero; the Benes network of pz_paillier_mix layer by layer and switch by switch -- assert_bit of the switch's bit ([0, b, b, b]),
 * then per limb t select(in[j'][t], in[j][t], b) and select(in[j][t], in[j'][t], b), 8 cells each with gate windows at 0 and 4: 4 + 16
 * * 2 limbs_n cells a switch --; per output [1, 0], the n_steps_r mul_mod blocks of pow_mod_fixed_exp(r_i extended by the load_zero
 * cell, n) and mul_mod(d_i, rn_i); then per output assign_integer(c'_i) at full width and assert_equal_fresh.  The selects' sel cells
 * are tied to their switch's bit cell, their operands to the limb cells they read (layer 0: the assigned c_j; above: the previous
 * layer's outputs), the final block's operands to the last layer's outputs and the chain's result, each assert_equal_fresh's bit to
 * the constant 1: whatever the bits, a network of conditional swaps under bits in {0, 1} is SOME permutation.  The circuit neither
 * compares r_i with n nor refuses r_i = 0, and K is a power of two (DESIGN.md section 15.17 lists what is absent).
 *   pz_mix_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_mix_expand_dev    the values.  inputs (HOST): n (ceil(limbs_n*limb_bits/64) words) | c_1 .. c_K (ceil(2*limbs_n*limb_bits/64)
 *       words each) | r_1 .. r_K (as n) | res_1 .. res_K (as the c_j).  bits (HOST): the switch bytes as pz_paillier_mix took them (a
 *       byte above 1: PZ_ERR_MESSAGE_RANGE; may be NULL for K = 1).  d_routes, d_steps (device): the route layers and the K (n_steps_r +
 *       1) records of pz_paillier_mix_dev AS THEY ARE, fields of 2*ceil(limbs_n*limb_bits/64) words (where that differs from
 *       ceil(2*limbs_n*limb_bits/64) the records are repacked on the device first; d_routes may be NULL for K = 1).  d_modulus: n^2
 *       (device).  rows / col_stride as pz_circuit_expand_dev.
 *   pz_mix_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_mix_public_cells  the stream indices of the exposed cells in statement order: n | c_1 | .. | c_K | c'_1 | .. | c'_K (the limb cells
 *       of the assign_integer of each): n_public = limbs_n + 2 K 2 limbs_n. */
int pz_mix_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r, size_t* advice_cells,
                 size_t* lookup_cells);
int pz_mix_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                      const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                      const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride);
int pz_mix_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r,
                           const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                           const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                           size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride);
int pz_mix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, size_t n_steps_r, uint64_t* cells_out,
                        size_t capacity, size_t* n_public);

/* Circuit kind 9, "sballot" (DESIGN.md section 15.18): under the key (n, g, hs) the K = count ciphertexts c_1 .. c_K (1 .. 1024) are
 * short-randomness ballots c_i = g^m_i hs^s_i mod n^2 with m_i < 2^b, b = m_bits (1 .. 64), and s_i < 2^s_bits, s_bits = s_limbs *
 * limb_bits with 1 <= s_limbs <= 2*limbs_n, and for K >= 2 the m_i add up to the public S.  Its shape is (K, b, s_limbs) and the key
 * SIZE: no bit of n shapes it, so one proving and verifying key serves every election of a size.  The by-kind entry points refuse
 * kind 9 and these take the three numbers (anything out of range: PZ_ERR_INVALID).  The stream, in emission order:
 * assign_integer(n), assign_integer(g), assign_integer(hs, 2*enc_bits); load_witness(m_1 .. m_K); for K >= 2 FlexGate::sum as in kind
 * 6; assign_integer(s_i, s_bits) for i = 1..K (s_limbs limbs each); square + refresh of n, once; load_zero; per ciphertext
 * pow_mod(g_ext, m_i) over exactly b bits exactly as kind 6 ([1, 0], num_to_bits(m_i, b), b blocks of mul_mod(acc, sq), limb-wise
 * select, square_mod(sq)), then pow_mod(hs, s_i) exactly as kind 7 emits a chain ([1, 0], then per limb of s_i num_to_bits(limb,
 * limb_bits) and that limb's blocks), then mul_mod(gm_i, hss_i); then per ciphertext assign_integer(res_i, 2*enc_bits) and
 * assert_equal_fresh(c_i, res_i).  The circuit compares nothing with n^2 and does not refuse hs = 0 (verifier.public_inputs does).
 *   pz_sballot_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_sballot_expand_dev    the values.  inputs (HOST): n | g (ceil(limbs_n*limb_bits/64) words each) | hs (ceil(2*limbs_n*limb_bits/64)
 *       words) | m_1 .. m_K (ONE word each; a message >= 2^b: PZ_ERR_MESSAGE_RANGE) | s_1 .. s_K (ceil(s_bits/64) words each; an s_i >=
 *       2^s_bits: PZ_ERR_MESSAGE_RANGE) | res_1 .. res_K (as hs).  d_steps (device): the K (2 b + 2 s_bits + 1) records of
 *       pz_paillier_sballot_dev AS THEY ARE, fields of 2*ceil(limbs_n*limb_bits/64) words (where that differs from
 *       ceil(2*limbs_n*limb_bits/64) the records are repacked on the device first).  d_modulus: n^2 (device).  rows / col_stride as
 *       pz_circuit_expand_dev.
 *   pz_sballot_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_sballot_public_cells  the stream indices of the exposed cells in statement order: n | g | hs | c_1 | .. | c_K (the limb cells of
 *       n's, g's, hs's and every res_i's assign_integer) and, for K >= 2, S (the sum's last cell): n_public = 2 limbs_n + (K + 1) 2
 *       limbs_n + (K >= 2). */
int pz_sballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, uint32_t s_limbs,
                     size_t* advice_cells, size_t* lookup_cells);
int pz_sballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                          uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus, uint64_t* d_advice,
                          uint64_t* d_lookup, size_t rows, size_t col_stride);
int pz_sballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits,
                               uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                               uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts, size_t n_adv_cols, size_t max_rows,
                               size_t lookup_rows, size_t col_stride);
int pz_sballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t m_bits, uint32_t s_limbs,
                            uint64_t* cells_out, size_t capacity, size_t* n_public);

/* Circuit kind 10, "smix" (DESIGN.md section 15.20): the list c'_1 .. c'_K is a re-randomised permutation of the list c_1 .. c_K under
 * the key (n, hs) -- there are a permutation pi and s_i < 2^s_bits with c'_i = c_pi(i) hs^s_i mod n^2 for every i.  K = count is a power
 * of two in 1 .. 1024, s_bits = s_limbs * limb_bits with 1 <= s_limbs <= 2*limbs_n.  Its shape is (K, s_limbs) and the key SIZE: no bit
 * of n shapes it, so one proving and verifying key serves every election of a size.  The by-kind entry points refuse kind 10 and these
 * take the two numbers (anything out of range: PZ_ERR_INVALID).  The stream, in emission order: assign_integer(n); assign_integer(hs,
 * 2*enc_bits); assign_integer(c_j, 2*enc_bits) for j = 1 .. K; assign_integer(s_i, s_bits) for i = 1 .. K (s_limbs limbs each); square
 * + refresh of n, once; load_zero (kept although nothing is extended by it: kinds 7, 8 and 9 emit it there); the Benes network exactly
 * as kind 8 -- per switch [0, b, b, b], then per limb the two 8-cell selects with gate windows at 0 and 4 --; per output [1, 0],
 * pow_mod(hs, s_i) exactly as kind 9 emits its hs-chain (per limb of s_i num_to_bits(limb, limb_bits) and that limb's blocks) and
 * mul_mod(d_i, hss_i); then per output assign_integer(c'_i, 2*enc_bits) and assert_equal_fresh.  The selects' sel cells are tied to
 * their switch's bit cell, their operands to the limb cells they read (layer 0: the assigned c_j; above: the previous layer's
 * outputs), every hs-chain's first sq to assign_integer(hs)'s limb cells (all K chains run on ONE public base), every chain's
 * num_to_bits accumulators to assign_integer(s_i)'s limb cells, the final block's operands to the last layer's outputs (K = 1: c_1's
 * limbs) and the chain's last select outputs, its result to the assert_equal_fresh against c'_i, each assert_equal_fresh's bit to the
 * constant 1.  The circuit compares nothing with n^2 and refuses neither hs = 0 nor s_i = 0 (verifier.public_inputs does the former).
 *   pz_smix_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_smix_expand_dev    the values.  inputs (HOST): n (ceil(limbs_n*limb_bits/64) words) | hs (ceil(2*limbs_n*limb_bits/64) words) |
 *       c_1 .. c_K (as hs) | s_1 .. s_K (ceil(s_bits/64) words each; an s_i >= 2^s_bits: PZ_ERR_MESSAGE_RANGE) | res_1 .. res_K (as hs).
 *       bits (HOST): the switch bytes as pz_paillier_smix took them (a byte above 1: PZ_ERR_MESSAGE_RANGE; may be NULL for K = 1).
 *       d_routes, d_steps (device): the route layers and the K (2 s_bits + 1) records of pz_paillier_smix_dev AS THEY ARE, fields of
 *       2*ceil(limbs_n*limb_bits/64) words (where that differs from ceil(2*limbs_n*limb_bits/64) they are repacked on the device
 *       first; d_routes may be NULL for K = 1).  d_modulus: n^2 (device).  rows / col_stride as pz_circuit_expand_dev.
 *   pz_smix_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_smix_public_cells  the stream indices of the exposed cells in statement order: n | hs | c_1 | .. | c_K | c'_1 | .. | c'_K (the
 *       limb cells of the assign_integer of each): n_public = limbs_n + 2 limbs_n + 2 K 2 limbs_n. */
int pz_smix_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs, size_t* advice_cells,
                  size_t* lookup_cells);
int pz_smix_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                       const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                       const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride);
int pz_smix_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs,
                            const uint64_t* inputs, const uint8_t* bits, const uint64_t* d_routes, const uint64_t* d_steps,
                            const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                            size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride);
int pz_smix_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t s_limbs, uint64_t* cells_out,
                         size_t capacity, size_t* n_public);

/* Circuit kind 11, "pballot" (DESIGN.md section 15.21): under the key (n, hs) and the public slot bases G_0 .. G_{K-1}, K = slots (1 ..
 * 64), the R = count ciphertexts c_1 .. c_R (1 .. 1024, R K <= 1024) are packed ballots c_i = (prod_j G_j^v_ij) hs^s_i mod n^2 with every
 * v_ij < 2^b, b = m_bits (1 .. 64), and s_i < 2^s_bits, s_bits = s_limbs * limb_bits with 1 <= s_limbs <= 2*limbs_n, and for K >= 2 the
 * values of ciphertext i add up to the public S_i.  Its shape is (R, K, b, s_limbs) and the key SIZE: neither n, g nor the slot width
 * shapes it, so one proving and verifying key serves every election of a size; the verifier derives G_j = g^(2^(j w)) mod n^2 itself
 * (verifier.public_inputs).  The by-kind entry points refuse kind 11 and these take the four numbers (anything out of range:
 * PZ_ERR_INVALID).  The stream, in emission order: assign_integer(n), assign_integer(hs, 2*enc_bits), assign_integer(G_j, 2*enc_bits)
 * for j = 0..K-1; load_witness of the R K values, ciphertext-major; for K >= 2 one FlexGate::sum per ciphertext over its K cells;
 * assign_integer(s_i, s_bits) for i = 1..R; square + refresh of n, once; load_zero; per ciphertext, per slot [1, 0], num_to_bits(v_ij,
 * b) and b blocks of mul_mod(acc, sq), limb-wise select, square_mod(sq) exactly as kind 6's g-chain with the first sq G_j's limb cells,
 * then pow_mod(hs, s_i) exactly as kind 9, then the K fold blocks mul_mod(P_0, P_1), mul_mod(t_1, P_2), .., mul_mod(t_{K-1}, hss_i);
 * then per ciphertext assign_integer(res_i, 2*enc_bits) and assert_equal_fresh(c_i, res_i).  With K = 1 and G_0 = g the computation is
 * kind 9's for one ciphertext (g then stands at full width and in hs's place in the order).  The circuit compares nothing with n^2.
 *   pz_pballot_cells         the stream's advice / lookup cell counts (host logic).
 *   pz_pballot_expand_dev    the values.  inputs (HOST): n (ceil(limbs_n*limb_bits/64) words) | hs | G_0 .. G_{K-1}
 *       (ceil(2*limbs_n*limb_bits/64) words each) | v_11 .. v_RK (ONE word each, ciphertext-major; a value >= 2^b:
 *       PZ_ERR_MESSAGE_RANGE) | s_1 .. s_R (ceil(s_bits/64) words each; an s_i >= 2^s_bits: PZ_ERR_MESSAGE_RANGE) | res_1 .. res_R (as hs).
 *       d_steps (device): the R (2 b K + 2 s_bits + K) records of pz_paillier_pballot_dev AS THEY ARE, fields of
 *       2*ceil(limbs_n*limb_bits/64) words (where that differs from ceil(2*limbs_n*limb_bits/64) the records are repacked on the device
 *       first).  d_modulus: n^2 (device).  rows / col_stride as pz_circuit_expand_dev.
 *   pz_pballot_expand_cols_dev  the same with the advice cells in break-point columns, as pz_circuit_expand_cols_dev.
 *   pz_pballot_public_cells  the stream indices of the exposed cells in statement order: n | hs | G_0 | .. | G_{K-1} | c_1 | .. | c_R
 *       (the limb cells of n's, hs's, every G_j's and every res_i's assign_integer) and, for K >= 2, S_1 .. S_R (each sum's last
 *       cell): n_public = limbs_n + 2 limbs_n (1 + K + R) + (K >= 2) R. */
int pz_pballot_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots, uint32_t m_bits,
                     uint32_t s_limbs, size_t* advice_cells, size_t* lookup_cells);
int pz_pballot_expand_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots,
                          uint32_t m_bits, uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps, const uint64_t* d_modulus,
                          uint64_t* d_advice, uint64_t* d_lookup, size_t rows, size_t col_stride);
int pz_pballot_expand_cols_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots,
                               uint32_t m_bits, uint32_t s_limbs, const uint64_t* inputs, const uint64_t* d_steps,
                               const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                               size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride);
int pz_pballot_public_cells(uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t count, uint32_t slots, uint32_t m_bits,
                            uint32_t s_limbs, uint64_t* cells_out, size_t capacity, size_t* n_public);

/* The same stream with the ADVICE cells in halo2-lib's break-point column layout -- what the dependency's assign_with_constraints
 * [D] does with the Context's cell list when it fills the basic-gate columns (reached from bench.rs:161-171 through keygen /
 * create_proof -> synthesize): a 4-cell gate never straddles two columns; the column ends where one would, and the cell it ends
 * with is written AGAIN as row 0 of the next column (the two copies are tied by an equality constraint of the circuit).
 *   pz_circuit_break_points (host, no device work): from the selector mask of the stream (gate_mask[i] != 0 where a gate window
 *   starts at cell i) and max_rows (usable rows of a column) -> starts[j] = the stream index of column j's row 0, j < *n_cols, and
 *   starts[*n_cols] = n_cells.  starts_out may be NULL (count only); PZ_ERR_CAPACITY if capacity < *n_cols + 1; PZ_ERR_UNSUPPORTED if
 *   two gates overlap by other than three cells at a break (the dependency asserts the same).
 *   pz_circuit_expand_cols_dev: as pz_circuit_expand_dev, the advice stream placed by d_col_starts (DEVICE array of n_adv_cols + 1
 *   entries as above), columns col_stride elements apart; the lookup stream is cut plainly into columns of lookup_rows cells.
 *   Column j's rows above starts[j + 1] - starts[j] are not written. */
int pz_circuit_break_points(const uint8_t* gate_mask, size_t n_cells, size_t max_rows, uint64_t* starts_out, size_t capacity,
                            size_t* n_cols);
int pz_circuit_expand_cols_dev(pz_ctx* ctx, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits,
                               const uint64_t* inputs, const uint64_t* d_steps, size_t n_steps_g, size_t n_steps_r,
                               const uint64_t* d_modulus, uint64_t* d_advice, uint64_t* d_lookup, const uint64_t* d_col_starts,
                               size_t n_adv_cols, size_t max_rows, size_t lookup_rows, size_t col_stride);

/* RefreshAux::new(limb_bits, l, r).increased_limbs_vec (paillier.rs:40-44): the number of further limbs each product limb's
 * maximal value spills into; *n_out entries (= the refreshed integer's limb count) are written. */
int pz_refresh_aux(uint32_t limb_bits, uint32_t num_limbs_l, uint32_t num_limbs_r, uint8_t* increased_limbs,
                   uint32_t capacity, uint32_t* n_out);
/* cells ONE chip operation pushes -- the terms pz_circuit_cells sums; op: 0 assign_integer(limbs), 1 square(limbs),
 * 2 refresh (limbs x limbs product), 3 load_zero / load_constant, 4 mul_mod(limbs), 5 assert_equal_fresh(limbs). */
int pz_op_cells(int op, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits, size_t* advice_cells, size_t* lookup_cells);

/* host-pointer form: steps / modulus / outputs in process memory (n_steps*advice_cells and n_steps*lookup_cells Fr
 * elements; either output may be NULL); synchronises before returning. */
int pz_witness_expand(pz_ctx* ctx, uint32_t limbs, uint32_t limb_bits, uint32_t lookup_bits, const uint64_t* steps,
                      size_t n_steps, const uint64_t* modulus, uint64_t* advice_out, uint64_t* lookup_out);

/* ---------------------------------------------------------------------------------------------
 * "next" rows, built on the kernels above
 * ------------------------------------------------------------------------------------------- */
/* ParamsKZG::setup with a known toxic scalar s (what halo2-lib's gen_srs does with its seeded rng; reached from
 * /root/reference/src/bench.rs:161-171): d_g[i] = [s^i] G, d_g_lagrange[i] = [L_i(s)] G over the 2^k domain
 * generated by omega (L_i(s) = (s^n - 1) omega^i / (n (s - omega^i))).  Either output may be NULL.  s, omega: Fr
 * Montgomery (host); outputs: device, 2^k affine points each.  s must not lie in the domain (PZ_ERR_INVALID). */
int pz_srs_setup_g1_dev(pz_ctx* ctx, uint32_t k, const uint64_t s[4], const uint64_t omega[4], uint64_t* d_g,
                        uint64_t* d_g_lagrange);
/* The Lagrange-basis SRS from the monomial one WITHOUT the toxic scalar (what ParamsKZG does with a params file's `g`):
 * d_g_lagrange[i] = (1/n) sum_j omega^(-i j) d_g[j], a radix-2 inverse FFT over G1 (the twiddle product is a scalar
 * multiplication).  d_g, d_g_lagrange: 2^k affine points on the device (may not alias); omega_inv, n_inv: Fr Montgomery
 * (host).  One-time cost per SRS, (k + 1) 2^(k-1) scalar multiplications. */
int pz_srs_lagrange_from_monomial_dev(pz_ctx* ctx, uint32_t k, const uint64_t omega_inv[4], const uint64_t n_inv[4],
                                      const uint64_t* d_g, uint64_t* d_g_lagrange);
/* keygen, permutation polynomials (halo2 permutation::keygen::Assembly::build_pk): d_sigma[j][i] = delta^(d_map_col[j*n+i]) *
 * omega^(d_map_row[j*n+i]) over the 2^k domain, n = 2^k, for m columns -- (map_col, map_row) is the cell the copy-constraint
 * cycle maps (j, i) to (circuit structure, supplied by the caller: device arrays of m * n u32 each).  ONE call covers the whole
 * permutation: every image must lie inside the m x n cells of the call (an image outside is clamped on the device and the next
 * synchronising entry point returns PZ_ERR_ASYNC). */
int pz_permutation_sigma_dev(pz_ctx* ctx, const uint32_t* d_map_col, const uint32_t* d_map_row, size_t m, uint32_t k,
                             const uint64_t omega[4], const uint64_t delta[4], uint64_t* d_sigma, size_t sigma_stride);
/* the same for the columns [col_lo, col_lo + n_cols) of an m_total-column permutation, written to d_sigma + (j - col_lo) * sigma_stride:
 * sigma in tiles through one reusable buffer (pz_vk_keygen*).  d_map_col / d_map_row are those of the WHOLE permutation (m_total * 2^k
 * entries each); images are checked against its m_total x 2^k cells, clamped and reported as PZ_ERR_ASYNC exactly as above. */
int pz_permutation_sigma_part_dev(pz_ctx* ctx, const uint32_t* d_map_col, const uint32_t* d_map_row, size_t m_total, size_t col_lo,
                                  size_t n_cols, uint32_t k, const uint64_t omega[4], const uint64_t delta[4], uint64_t* d_sigma,
                                  size_t sigma_stride);
/* keygen_vk + keygen_pk for n_cols Lagrange-form fixed columns (selectors, constants, table, sigma) on the device: their
 * commitments (commit_lagrange, n_cols x 12), then IN PLACE their coefficient form, and (d_ext != NULL) their values on the
 * extended coset (as pz_ntt_fr_extend_dev) -- the proving key's polynomials, resident in HBM for every later proof.
 * Reached in the reference through bench.rs:161-175 (keygen_vk / keygen_pk inside bench_builder). */
int pz_keygen_columns_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, uint64_t* d_cols, size_t n_cols, size_t col_stride,
                          uint32_t k, uint32_t log_e, const uint64_t omega_n[4], const uint64_t omega_n_inv[4],
                          const uint64_t n_inv[4], const uint64_t* coset_gens, uint64_t* d_commit_jac, uint64_t* d_ext,
                          size_t ext_stride);
/* on-curve validation of n affine points on the device (y^2 = x^3 + 3, canonical coordinates, identity (0,0)
 * accepted): *n_bad = number of points that fail.  The check halo2curves' read_raw performs when ParamsKZG::read
 * loads a `params/kzg_bn254_{k}.srs` file (paillier_halo2_amd/srs.py reads that format). */
int pz_g1_check_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, uint64_t* n_bad);
/* BN254 pairing (the verifier's side of ParamsKZG; csrc/pz_pairing.hip).  halo2curves' tower: Fq2 = Fq[u]/(u^2 + 1),
 * Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq12 = Fq6[w]/(w^2 - v); G2 on the D-type twist y^2 = x^3 + 3/(9 + u) over Fq2.
 * G2 affine points: 16 words x.c0, x.c1, y.c0, y.c1 (4 Montgomery words each, ParamsKZG RawBytes), identity = all zero.
 * G1: the affine form above (8 words, (0, 0) = identity).  GT: 48 words, Fq12 c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1.
 * e(P, Q) = f_{6x+2,Q}(P) l_{[6x+2]Q,pi(Q)}(P) l_{..,-pi^2(Q)}(P), raised to exactly (p^12 - 1)/r; a pair with an identity
 * contributes 1.  The device entry points are asynchronous on the context's stream. */
/* halo2curves' G2 generator */
int pz_g2_generator(uint64_t out[16]);
/* d_out[i] = [s_i] Q_i for n G2 points (on the twist; the result is undefined otherwise); scalars Fr Montgomery (4 words) */
int pz_g2_mul_dev(pz_ctx* ctx, const uint64_t* d_g2, const uint64_t* d_scalars, size_t n, uint64_t* d_out);
/* d_gt[i] = e(P_i, Q_i); all 48 words zero (not a GT element) if P_i or Q_i is off its curve or not canonical */
int pz_pairing_dev(pz_ctx* ctx, const uint64_t* d_g1, const uint64_t* d_g2, size_t n, uint64_t* d_gt);
/* n_checks products of pairs_per_check pairings (check i takes pairs i * pairs_per_check + j): d_ok[i] = 1 if
 * prod_j e(P_ij, Q_ij) == 1, 0 if not, -1 if any input of that check is off its curve or not canonical.  No subgroup check. */
int pz_pairing_check_dev(pz_ctx* ctx, const uint64_t* d_g1, const uint64_t* d_g2, size_t n_checks, uint32_t pairs_per_check,
                         int32_t* d_ok);
/* The device batch verifier (csrc/pz_verify.hip + pz_verify.cpp): halo2's KZG / SHPLONK verify_proof for the proofs of pz_proof_*, a
 * batch at a time, with the same verdicts as paillier_halo2_amd/verifier.py::verify_batch.  No toxic scalar: the last step is
 * pz_pairing_check_dev.
 * pz_vk_create   the verifier's side of a key and its params, copied to the device once: the key's commitments fixed_affine
 *                ((n_adv + 2) x 8, pz_pk_commitments' first array) and sigma_affine (m x 8, m = n_adv + n_lk + 1), g[0] of the params (8),
 *                g2 and s_g2 (16 each, ParamsKZG RawBytes).  PZ_ERR_INVALID if g2 or s_g2 is zero, g[0] is the identity, n_adv or n_lk
 *                is 0, k is outside 4..24 or blinding_factors + 2 > 2^k.  The key holds device memory of `ctx` (which must outlive it).
 * pz_vk_info     a proof's words: commitment_words = 8 x (n_adv + 4 n_lk + n_sets + 6), evals_words = pz_pk_info's.
 * pz_verify_batch  proofs: n_proofs x (commitment_words + evals_words) host words, each proof what the stepper hands back, in its phase
 *                order: the commitments advice | lookup advice | A' | S' | permutation products | lookup products | random | h_0..h_2 |
 *                W1 | W2, then pz_proof_evaluate's array (the constants row and the trailing h(x) included).  Proof i's transcript seed is
 *                seeds[seed_offsets[i] .. seed_offsets[i + 1]) (n_proofs + 1 offsets; the caller's bytes, as prove_connected's 8-byte
 *                little-endian index).  verdicts[i] = 1 if h(x) (x^n - 1) equals the constraint expression, the proof states that h(x),
 *                evaluations are canonical and the opening's pairing check holds, else 0; *all_ok = every verdict is 1.
 *                The words come unchecked, and pz_verify_batch is never laxer than pz_verify_batch_bytes: every commitment of a proof
 *                must be the identity (0, 0) or have canonical coordinates (below p) on the curve -- pz_g1_check_dev's rule, the wire
 *                decoder's statuses 1 and 2, pz_pairing_check_dev's -1, halo2's `read` -- or that proof alone gets verdict 0 (one launch
 *                over the batch's commitments before the fold; the other proofs are judged without it).
 *                One fold with random weights (OS randomness) and one 2-pair check decide an all-good batch; otherwise (or when ab_affine
 *                is asked for) n_proofs independent checks in one pz_pairing_check_dev launch give the verdicts.  Optional (NULL
 *                allowed): h_evals n x 4 (the h(x) each proof implies, Montgomery), ab_affine n x 16 (each proof's SHPLONK points A then
 *                B, unweighted).  A batch with bad proofs is PZ_OK; errors are malformed arguments and device failures only.  Host
 *                pointers; synchronises.
 * pz_vk_free     releases the key. */
typedef struct pz_vk pz_vk;
int pz_vk_create(pz_ctx* ctx, uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, const uint64_t* fixed_affine,
                 const uint64_t* sigma_affine, const uint64_t g0_affine[8], const uint64_t g2[16], const uint64_t s_g2[16], pz_vk** out);
int pz_vk_info(const pz_vk* vk, size_t* commitment_words, size_t* evals_words);
int pz_verify_batch(pz_vk* vk, const uint64_t* proofs, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                    int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok);
int pz_vk_free(pz_vk* vk);
/* keygen_vk (csrc/pz_vk_keygen.cpp): the key's commitments from the circuit STRUCTURE alone -- halo2's keygen_vk, which the
 * reference reaches at bench.rs:161-175 -- for a party that only verifies and will not trust a key file: no proving key is built, no transform
 * runs, nothing stays resident.  Inputs as pz_pk_create[_dev] takes them (selectors u8 [n_adv][2^k], constants n_constants x 4 canonical words
 * (host), map_col / map_row u32 [m][2^k], m = n_adv + n_lk + 1; the table column is 0 .. 2^lookup_bits - 1); outputs as pz_pk_commitments
 * writes them (fixed_affine (n_adv + 2) x 8, sigma_affine m x 8, HOST), word for word what a key of pz_pk_create gives, so they go straight
 * into pz_vk_create.  Selectors: pz_g1_commit_mask_dev; the constants and table columns: one small MSM; sigma: tiles of `tile` columns (0 = 64)
 * through one buffer, pz_permutation_sigma_part_dev + pz_msm_g1_dev.  Device memory beyond the caller's arrays is O(tile 2^k) (at config c2,
 * tile 64: 0.3 GB against the proving key's 116 + 30).  n_adv, n_lk >= 1; lookup_bits < k; 4 <= k <= 24; the bases cover 2^k points; an
 * image outside the m x 2^k cells: PZ_ERR_ASYNC.  Synchronises.
 * pz_vk_keygen_dev  selectors / map_col / map_row on the device (pz_circuit_structure_dev's arrays, or uploaded by the caller): only read.
 * pz_vk_keygen      the same three in HOST memory, uploaded tile by tile. */
int pz_vk_keygen_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                     const uint8_t* d_selectors, const uint64_t* constants, size_t n_constants, const uint32_t* d_map_col,
                     const uint32_t* d_map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine);
int pz_vk_keygen(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                 const uint8_t* selectors, const uint64_t* constants, size_t n_constants, const uint32_t* map_col, const uint32_t* map_row,
                 size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine);
/* halo2 wire bytes (csrc/pz_wire.hip): what gen_proof returns and check_proof takes in the reference (bench.rs:173-178,
 * a Vec<u8>), decoded and encoded on the device.  All integers little-endian.
 *   G1 point, 32 bytes (halo2curves' G1Compressed [D]): the canonical (non-Montgomery) x; bit 7 of byte 31 = the parity of the canonical y;
 *     bit 6 of byte 31 is 0 (x < p < 2^254); the identity is 32 zero bytes.  Decoding: y = (x^3 + 3)^((p+1)/4), accepted only if
 *     y^2 = x^3 + 3, negated to the stated parity.  status: 0 ok, 1 not canonical (x >= p), 2 not on the curve; a refused point is written
 *     as the identity.  No subgroup check (cofactor 1).
 *   scalar, 32 bytes: the canonical value; a value >= r is refused (status 1).
 *   proof: the transcript's absorption order -- the commitments of pz_verify_batch's layout WITHOUT W1 and W2 | pz_proof_evaluate's array
 *     WITHOUT the trailing h(x) (halo2 does not send it; the verifier computes it) | W1 | W2:
 *     32 x (commitment_words / 8 + evals_words / 4 - 1) bytes.
 * pz_g1_compress_dev / pz_g1_decompress_dev   n points, device pointers (16-byte aligned), asynchronous on the context's stream.
 * pz_g1_compress / pz_g1_decompress           host pointers, synchronise.  status (n) and n_bad (points with a status other than 0) may be NULL.
 * pz_proof_wire_bytes     a proof's size on the wire.
 * pz_proof_encode         n_proofs proofs in pz_verify_batch's word layout -> wire bytes (the h(x) slot is dropped).  Host pointers.
 * pz_proof_decode         the reverse; the h(x) slot is written as zero; status[i] = the worst status of proof i's elements (its words are
 *                         defined -- refused elements zero -- but must not be used when status[i] != 0).  Host pointers.
 * pz_verify_batch_bytes   pz_verify_batch on n_proofs x pz_proof_wire_bytes bytes: the same verdicts as pz_verify_batch gives for the decoded
 *                         proofs, but for the "proof states h(x)" test, which does not apply.  A proof that does not decode gets verdict 0
 *                         (h_evals / ab_affine rows zero), the call stays PZ_OK, its points never reach the MSM and the other proofs are
 *                         judged as if it were absent.  Every commitment that reaches the MSM is on the curve by construction. */
int pz_g1_compress_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, uint8_t* d_bytes);
int pz_g1_decompress_dev(pz_ctx* ctx, const uint8_t* d_bytes, size_t n, uint64_t* d_points, int32_t* d_status);
int pz_g1_compress(pz_ctx* ctx, const uint64_t* points, size_t n, uint8_t* bytes);
int pz_g1_decompress(pz_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* points, int32_t* status, uint64_t* n_bad);
int pz_proof_wire_bytes(const pz_vk* vk, size_t* bytes);
int pz_proof_encode(pz_vk* vk, const uint64_t* proofs_words, size_t n_proofs, uint8_t* out_bytes);
int pz_proof_decode(pz_vk* vk, const uint8_t* bytes, size_t n_proofs, uint64_t* out_words, int32_t* status);
int pz_verify_batch_bytes(pz_vk* vk, const uint8_t* bytes, size_t n_proofs, const uint8_t* seeds, const size_t* seed_offsets,
                          int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok);
/* ParamsKZG files through the library (csrc/pz_params.hip + pz_params.cpp): halo2's ParamsKZG::{read_custom,
 * write_custom, downsize} (the reference reaches them through gen_srs, bench.rs:161-171), every point decoded and checked on the device,
 * plus a check that g, g_lagrange, g2 and s_g2 belong to ONE structured reference string.
 *   G2 point, 64 bytes (halo2curves' G2Compressed [D], the convention of the G1 format above): bytes 0..31 the canonical x.c0, bytes 32..63
 *     the canonical x.c1, both little-endian; bit 7 of byte 63 = the parity of the canonical y.c0; bit 6 of byte 63 is 0; the identity is 64
 *     zero bytes.  Decoding: y = sqrt(x^3 + 3/(9 + u)) in Fq2 (the complex method over the (p+1)/4 root of Fq), accepted only if
 *     y^2 equals it, negated to the stated parity.  status: 0 ok, 1 not canonical (c0 >= p or c1 >= p), 2 no twist point has this x; a
 *     refused point is written as the identity.  y.c0 = 0: the two roots (0, +-y.c1) share the parity 0 and the format cannot tell them
 *     apart; compression writes the bit 0, and decompression returns the root whose canonical y.c1 is EVEN whatever the bit says, so such
 *     a point with an odd y.c1 comes back negated (no such point is known in the order-r subgroup; a file that holds one is refused by
 *     pz_params_check's relation checks, not silently accepted).  No subgroup check in the codec: that is pz_g2_check.
 *   pz_g2_check[_dev]  one status per point (16 words, int32): 0 in the order-r subgroup (the identity included), 1 not canonical, 2 off
 *     the twist, 3 on the twist but [r]Q != O -- the twist's cofactor 2p - r is not 1 (it has the factors 10069 and 5864401), which is why
 *     pz_pairing_check_dev's "no subgroup check" needs this in front of it for untrusted G2 input.  _dev: device pointers (16-byte
 *     aligned), asynchronous; the others take host pointers and synchronise.  status / n_bad of pz_g2_decompress may be NULL.
 *   file layouts (halo2's write_custom): u32 k | g[2^k] | g_lagrange[2^k] | g2 | s_g2, little-endian.  PZ_SERDE_RAW and
 *     PZ_SERDE_RAW_UNCHECKED: points are this ABI's words (64 B G1, 128 B G2); PZ_SERDE_PROCESSED: the compressed forms (32 B, 64 B).
 *   pz_params_file_bytes   the size of a file for k (1..28) in a format; no device work.
 *   pz_params_decode   host bytes (may be a memory-mapped file) -> a params object on the device.  The G1 sections are uploaded in chunks
 *     of a fixed number of points (PZ_PARAMS_CHUNK in the environment overrides it: tests) -- compressed points through ONE staging buffer
 *     of a chunk, raw points straight to their place -- so a k = 26 file never has a second copy on the device.  PROCESSED and RAW check
 *     every G1 point (its decompression status / pz_g1_check_dev) and that both G2 points are canonical and on the twist; any bad point:
 *     PZ_ERR_INVALID, *n_bad (may be NULL) = their number, no object (halo2 panics there).  RAW_UNCHECKED checks sizes only.  A len that
 *     is not pz_params_file_bytes of the header's k, or a k outside 1..28: PZ_ERR_INVALID (*n_bad = 0).
 *   pz_params_from_dev  the same object from points already on the device (what pz_srs_setup_g1_dev and pz_g2_mul_dev produce): d_g and
 *     d_g_lagrange (2^k affine points each) are COPIED; d_g_lagrange = NULL derives it (pz_srs_lagrange_from_monomial_dev).  g2, s_g2: host.
 *   pz_params_info     k, g[0] (8 words), g2 and s_g2 (16 each): exactly what pz_vk_create takes.  Any output may be NULL.
 *   pz_params_points   device pointers of g and g_lagrange, owned by the object (either may be NULL).
 *   pz_params_bases    the window table of g (lagrange = 0) or g_lagrange (!= 0), built on the first request and owned by the object (do
 *     not pz_bases_free it): MSMs over it equal those over pz_srs_load_g1 of the same points.
 *   pz_params_encode   the object -> file bytes (host); PZ_ERR_CAPACITY if capacity < pz_params_file_bytes.  RAW_UNCHECKED writes what RAW
 *     writes.
 *   pz_params_downsize ParamsKZG::downsize: k_new <= k (else PZ_ERR_INVALID); g truncated, g_lagrange recomputed on the device for the
 *     smaller domain, the G2 pair kept.  A new object.
 *   pz_params_check    PZ_OK whatever the verdict (errors are device failures only).  *failed, bits:
 *       PZ_PARAMS_BAD_G1        some point of g or g_lagrange is not canonical or off the curve
 *       PZ_PARAMS_BAD_G2        g2 or s_g2 has a pz_g2_check status other than 0, or is the identity
 *       PZ_PARAMS_BAD_G0        g[0] is the identity
 *       PZ_PARAMS_BAD_POWERS    g is not a geometric sequence g[i+1] = [s] g[i] for the s of the G2 pair (s_g2 = [s] g2)
 *       PZ_PARAMS_BAD_LAGRANGE  g_lagrange is not the Lagrange form of g over the 2^k domain
 *     The three point checks always run.  POWERS and LAGRANGE run only if all three passed -- no unchecked point reaches an MSM or the
 *     pairing -- and otherwise their bits are set in *skipped (may be NULL).  POWERS: with rho from OS randomness ONE 2-column MSM over g,
 *     A = sum_{i<n-1} rho^i g[i] and -B = -sum_{i<n-1} rho^i g[i+1], then e(A, s_g2) e(-B, g2) == 1 (pz_pairing_check_dev).  LAGRANGE: with
 *     tau, v_i = tau^i: MSM(g_lagrange, v) == MSM(g, iNTT(v)) after normalisation.  Each errs with probability about n / r.
 *     What it does NOT prove: that nobody knows s.  A string that passes is well-formed for SOME s; whether that s was destroyed is a
 *     matter of the ceremony that made the file, which no computation on the file can show. */
typedef struct pz_params pz_params;
#define PZ_SERDE_PROCESSED 0
#define PZ_SERDE_RAW 1
#define PZ_SERDE_RAW_UNCHECKED 2
#define PZ_PARAMS_BAD_G1 1u
#define PZ_PARAMS_BAD_G2 2u
#define PZ_PARAMS_BAD_G0 4u
#define PZ_PARAMS_BAD_POWERS 8u
#define PZ_PARAMS_BAD_LAGRANGE 16u
int pz_g2_compress(pz_ctx* ctx, const uint64_t* points, size_t n, uint8_t* bytes);
int pz_g2_decompress(pz_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* points, int32_t* status, uint64_t* n_bad);
int pz_g2_check_dev(pz_ctx* ctx, const uint64_t* d_points, size_t n, int32_t* d_status);
int pz_g2_check(pz_ctx* ctx, const uint64_t* points, size_t n, int32_t* status);
int pz_params_file_bytes(uint32_t k, int format, size_t* bytes);
int pz_params_decode(pz_ctx* ctx, const uint8_t* bytes, size_t len, int format, pz_params** out, uint64_t* n_bad);
int pz_params_from_dev(pz_ctx* ctx, uint32_t k, const uint64_t* d_g, const uint64_t* d_g_lagrange, const uint64_t g2[16],
                       const uint64_t s_g2[16], pz_params** out);
int pz_params_info(const pz_params* params, uint32_t* k, uint64_t g0_affine[8], uint64_t g2[16], uint64_t s_g2[16]);
int pz_params_points(const pz_params* params, const uint64_t** d_g, const uint64_t** d_g_lagrange);
int pz_params_bases(pz_params* params, int lagrange, const pz_bases** bases);
int pz_params_encode(const pz_params* params, int format, uint8_t* out, size_t capacity);
int pz_params_downsize(const pz_params* params, uint32_t k_new, pz_params** out);
int pz_params_check(pz_params* params, uint32_t* failed, uint32_t* skipped);
int pz_params_free(pz_params* params);
/* evaluation of n_cols coefficient-form polynomials (n coefficients each, device) at the point x:
 * d_out[col] = sum_i d_coeffs[col][i] * x^i   (the evals phase of create_proof / eval_polynomial). */
int pz_poly_eval_dev(pz_ctx* ctx, const uint64_t* d_coeffs, size_t n_cols, size_t col_stride, size_t n,
                     const uint64_t x[4], uint64_t* d_out);
/* the same at 1..4 points in one pass over the coefficients (a polynomial's rotation set x, omega x, ...):
 * xs = n_points x 4 words, d_out[col][point].  Identical values to n_points calls of pz_poly_eval_dev. */
int pz_poly_eval_multi_dev(pz_ctx* ctx, const uint64_t* d_coeffs, size_t n_cols, size_t col_stride, size_t n,
                           const uint64_t* xs, uint32_t n_points, uint64_t* d_out);

/* The prover steps between the commitments and the NTTs (in the reference all of
 * them run inside create_proof, reached from /root/reference/src/bench.rs:161-171).  Device pointers throughout, field
 * elements Fr Montgomery, strides in uint64_t units; challenges / constants are host pointers to one element.
 * Precondition checked on entry: the challenges beta, gamma, delta, y handed to pz_permutation_product_sets_dev and the three
 * pz_quotient_*_dev functions must be canonical (below r) -- they are converted on the host into the limb form the kernels
 * keep in scalar registers; a non-canonical word returns PZ_ERR_INVALID (it is not reduced). */
/* halo2 BatchInvert: d_a[i] <- 1 / d_a[i] in place, zeros stay zero. */
int pz_fr_batch_invert_dev(pz_ctx* ctx, uint64_t* d_a, size_t n);
/* running product: d_z[0] = z0, d_z[i+1] = d_z[i] * d_a[i] for i < n-1 (n outputs; d_z may alias d_a). */
int pz_fr_prefix_product_dev(pz_ctx* ctx, const uint64_t* d_a, size_t n, const uint64_t z0[4], uint64_t* d_z);
/* permutation::Argument::commit for one chunk of m columns over the 2^log_n domain generated by omega:
 *   d_z[0] = z0,  d_z[i+1] = d_z[i] * prod_{j<m} (v_j[i] + beta*delta_start*delta^j*omega^i + gamma)
 *                                              / (v_j[i] + beta*sigma_j[i] + gamma)
 * v_j = d_cols + j*col_stride (Lagrange values), sigma_j = d_sigma + j*sigma_stride (permutation polynomial values).
 * delta_start = delta^(index of the chunk's first column).  Blinding rows are the caller's business. */
int pz_permutation_product_dev(pz_ctx* ctx, const uint64_t* d_cols, size_t col_stride, const uint64_t* d_sigma,
                               size_t sigma_stride, size_t m, uint32_t log_n, const uint64_t omega[4],
                               const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_start[4],
                               const uint64_t delta[4], const uint64_t z0[4], uint64_t* d_z);
/* all sets of the permutation argument in one call: m columns in chunks of chunk_len (set j = columns
 * [j*chunk_len, ...), delta powers continuing across sets); d_z[0][0] = 1 and d_z[j][0] = d_z[j-1][usable_rows], as
 * halo2 chains them.  Per batch of sets: the terms stored once, a prefix scan of the numerators and a suffix scan of the
 * denominators, one inversion per set; the chaining value enters a set's scan as its start value (a zero denominator inverts to
 * zero, as in pz_fr_batch_invert_dev).  The environment variable PZ_PERM_SET_BATCH caps the sets per batch (tests). */
int pz_permutation_product_sets_dev(pz_ctx* ctx, const uint64_t* d_cols, size_t col_stride, const uint64_t* d_sigma,
                                    size_t sigma_stride, size_t m, uint32_t chunk_len, uint32_t log_n, size_t usable_rows,
                                    const uint64_t omega[4], const uint64_t beta[4], const uint64_t gamma[4],
                                    const uint64_t delta[4], uint64_t* d_z, size_t z_stride);
/* lookup::prover permute_expression_pair for halo2-lib's range-check lookups: every input column (values in
 * [0, 2^value_bits), value_bits <= 24) against the shared table column, over the first `rows` (usable) rows:
 *   d_perm_inputs[col] = the input column sorted ascending;
 *   d_perm_tables[col][i] = d_perm_inputs[col][i] where a run of equal inputs starts, otherwise the left-over table
 *   values in ascending order (halo2's BTreeMap order).
 * PZ_ERR_RANGE if a value is not a canonical integer below 2^value_bits or an input value does not occur in the
 * table (the reference's prover fails there: the lookup is unsatisfiable).  Rows >= `rows` are not written. */
int pz_lookup_permute_dev(pz_ctx* ctx, const uint64_t* d_inputs, size_t n_cols, size_t col_stride,
                          const uint64_t* d_table, size_t rows, uint32_t value_bits, uint64_t* d_perm_inputs,
                          uint64_t* d_perm_tables, size_t out_stride);
/* lookup grand products, n_lookups of them against one table column (z0 the same for all, normally 1):
 *   d_z[k][0] = z0, d_z[k][i+1] = d_z[k][i] * (A_k[i]+beta)(S[i]+gamma) / ((A'_k[i]+beta)(S'_k[i]+gamma)).
 * One batched inversion and one batched scan for all of them. */
int pz_lookup_product_dev(pz_ctx* ctx, const uint64_t* d_inputs, size_t input_stride, const uint64_t* d_table,
                          const uint64_t* d_perm_inputs, size_t perm_input_stride, const uint64_t* d_perm_tables,
                          size_t perm_table_stride, size_t n_lookups, size_t n, const uint64_t beta[4],
                          const uint64_t gamma[4], const uint64_t z0[4], uint64_t* d_z, size_t z_stride);
/* evaluate_h, custom-gate part, for halo2-lib's vertical gate on the extended domain of 2^log_ext points:
 *   for each column j in order:  d_h[i] = d_h[i]*y + sel_j[i] * (a_j[i] + a_j[i+s]*a_j[i+2s] - a_j[i+3s]),
 * indices mod 2^log_ext, s = rot_step = 2^(log_ext - k) (one row of the 2^k domain).  d_h is read and written. */
int pz_quotient_gate_dev(pz_ctx* ctx, const uint64_t* d_adv_ext, size_t adv_stride, const uint64_t* d_sel_ext,
                         size_t sel_stride, size_t n_cols, uint32_t log_ext, uint32_t rot_step, const uint64_t y[4],
                         uint64_t* d_h);
/* evaluate_h, permutation argument (halo2 plonk/evaluation.rs "Permutations"): m_total columns in n_sets chunks of
 * chunk_len, all arrays on the extended domain of 2^log_ext points X_i = coset_g * omega_ext^i, one domain row =
 * rot_step indices, last_rotation = blinding_factors + 1 rows.  In halo2's order, each folded as h = h*y + term:
 *   l0 (1 - z_0);  l_last (z_last^2 - z_last);  for j > 0: l0 (z_j - z_{j-1}(omega^-last_rotation X));
 *   for every set: l_active ( z_j(omega X) prod_c (v_c + beta sigma_c + gamma) - z_j(X) prod_c (v_c + delta^c beta X + gamma) ).
 * omega_ext must be a PRIMITIVE 2^log_ext-th root of unity (log_ext >= 1): rows i and i + 2^(log_ext-1) are evaluated together and
 * share the identity term through X_{i + N/2} = -X_i.  All challenges canonical (below r), Montgomery form. */
int pz_quotient_permutation_dev(pz_ctx* ctx, const uint64_t* d_cols_ext, size_t col_stride, const uint64_t* d_sigma_ext,
                                size_t sigma_stride, const uint64_t* d_z_ext, size_t z_stride, uint32_t n_sets,
                                uint32_t chunk_len, uint32_t m_total, uint32_t log_ext, uint32_t rot_step,
                                uint32_t last_rotation, const uint64_t* d_l0, const uint64_t* d_l_last,
                                const uint64_t* d_l_active, const uint64_t beta[4], const uint64_t gamma[4],
                                const uint64_t delta[4], const uint64_t coset_g[4], const uint64_t omega_ext[4],
                                const uint64_t y[4], uint64_t* d_h);
/* the same for a RANGE of sets, so that the prover can stream tiles of extended columns through it (evaluate_h never needs all
 * columns on the extended domain at once): this call adds the product lines of sets [set_lo, set_lo + n_sets) of n_sets_total;
 * d_cols_ext / d_sigma_ext point at the call's first column (= column set_lo * chunk_len of the argument) and m_cols counts the call's
 * columns (n_sets * chunk_len, fewer only when the call ends with the argument's last set); d_z_ext holds ALL n_sets_total products.
 * head != 0: the boundary and chaining lines (l0 (1 - z_0), l_last (z_last^2 - z_last), l0 (z_j - z_{j-1}(omega^-last X))) are added
 * first -- pass it with the first range only.  Calls in increasing set order give the value of one pz_quotient_permutation_dev. */
int pz_quotient_permutation_part_dev(pz_ctx* ctx, const uint64_t* d_cols_ext, size_t col_stride, const uint64_t* d_sigma_ext,
                                     size_t sigma_stride, const uint64_t* d_z_ext, size_t z_stride, uint32_t n_sets_total,
                                     uint32_t set_lo, uint32_t n_sets, uint32_t chunk_len, uint32_t m_cols, int head, uint32_t log_ext,
                                     uint32_t rot_step, uint32_t last_rotation, const uint64_t* d_l0, const uint64_t* d_l_last,
                                     const uint64_t* d_l_active, const uint64_t beta[4], const uint64_t gamma[4],
                                     const uint64_t delta[4], const uint64_t coset_g[4], const uint64_t omega_ext[4],
                                     const uint64_t y[4], uint64_t* d_h);
/* evaluate_h, lookup arguments (n_lookups of them against one table column), per lookup in halo2's order:
 *   l0 (1 - z);  l_last (z^2 - z);  l_active ( z(omega X)(a' + beta)(s' + gamma) - z(X)(a + beta)(s + gamma) );
 *   l0 (a' - s');  l_active (a' - s')(a' - a'(omega^-1 X)). */
int pz_quotient_lookup_dev(pz_ctx* ctx, const uint64_t* d_input_ext, size_t input_stride, const uint64_t* d_table_ext,
                           const uint64_t* d_perm_input_ext, size_t perm_input_stride, const uint64_t* d_perm_table_ext,
                           size_t perm_table_stride, const uint64_t* d_z_ext, size_t z_stride, uint32_t n_lookups,
                           uint32_t log_ext, uint32_t rot_step, const uint64_t* d_l0, const uint64_t* d_l_last,
                           const uint64_t* d_l_active, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4],
                           uint64_t* d_h);
/* The SPLIT forms of the two line kernels (the prover's two-coset quotient).  The lines that carry l_active
 * times a grand product's recurrence -- the product line of every permutation set, the third line of every lookup -- go to a second
 * accumulator d_h_d WITHOUT the factor l_active; d_h_low takes the remaining lines.  Both accumulators step through the powers of y
 * the unsplit form steps through, so d_h_low + l_active * d_h_d equals the unsplit d_h point for point, call by call.  Arguments as
 * in pz_quotient_permutation_part_dev / pz_quotient_lookup_dev (the permutation form reads no l_active row); d_h_low and d_h_d are
 * distinct arrays of 2^log_ext elements, both read and written. */
int pz_quotient_permutation_split_dev(pz_ctx* ctx, const uint64_t* d_cols_ext, size_t col_stride, const uint64_t* d_sigma_ext,
                                      size_t sigma_stride, const uint64_t* d_z_ext, size_t z_stride, uint32_t n_sets_total,
                                      uint32_t set_lo, uint32_t n_sets, uint32_t chunk_len, uint32_t m_cols, int head, uint32_t log_ext,
                                      uint32_t rot_step, uint32_t last_rotation, const uint64_t* d_l0, const uint64_t* d_l_last,
                                      const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4],
                                      const uint64_t coset_g[4], const uint64_t omega_ext[4], const uint64_t y[4], uint64_t* d_h_low,
                                      uint64_t* d_h_d);
int pz_quotient_lookup_split_dev(pz_ctx* ctx, const uint64_t* d_input_ext, size_t input_stride, const uint64_t* d_table_ext,
                                 const uint64_t* d_perm_input_ext, size_t perm_input_stride, const uint64_t* d_perm_table_ext,
                                 size_t perm_table_stride, const uint64_t* d_z_ext, size_t z_stride, uint32_t n_lookups,
                                 uint32_t log_ext, uint32_t rot_step, const uint64_t* d_l0, const uint64_t* d_l_last,
                                 const uint64_t* d_l_active, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4],
                                 uint64_t* d_h_low, uint64_t* d_h_d);
/* The values of that second accumulator on the domain H itself, from the LAGRANGE forms (no transform; call it before they become
 * coefficients):  d_out[i] = sum_j y^(S-1-j + 5 n_lookups) D_j(omega^i) + sum_l y^(5 (n_lookups-1-l) + 2) D^lk_l(omega^i) for the rows
 * row_lo <= i < 2^log_n, zero below row_lo, with S = ceil(m / chunk_len),
 *   D_j  = z_j(omega X) prod_c (v_c + beta sigma_c + gamma) - z_j(X) prod_c (v_c + beta delta^c X + gamma)   (c over set j's columns),
 *   D^lk = z(omega X)(a' + beta)(s' + gamma) - z(X)(a + beta)(s + gamma);
 * row 2^log_n - 1 reads z(omega^0).  With row_lo = the usable rows these are ALL the non-zero values of D on H: on the active rows
 * the recurrence that built the products makes every D_j and D^lk vanish.  One lane per (set or lookup, row): the cost of
 * 2^log_n - row_lo rows (at most 65535).  d_cols / d_sigma: [m][2^log_n], d_z: [S][..], the lookup arrays [n_lookups][..], d_table one
 * column (all NULL-able when n_lookups = 0); strides in 64-bit words; challenges canonical, Montgomery form. */
int pz_quotient_d_rows_dev(pz_ctx* ctx, const uint64_t* d_cols, size_t col_stride, const uint64_t* d_sigma, size_t sigma_stride,
                           const uint64_t* d_z, size_t z_stride, uint32_t m, uint32_t chunk_len, const uint64_t* d_input,
                           size_t input_stride, const uint64_t* d_table, const uint64_t* d_perm_input, size_t perm_input_stride,
                           const uint64_t* d_perm_table, size_t perm_table_stride, const uint64_t* d_zl, size_t zl_stride,
                           uint32_t n_lookups, uint32_t log_n, size_t row_lo, const uint64_t omega[4], const uint64_t beta[4],
                           const uint64_t gamma[4], const uint64_t delta[4], const uint64_t y[4], uint64_t* d_out);
/* d_out[col][i] = d_a[col][i] * d_row[i], i < n (a column times a row of values on the same points, e.g. the accumulator above
 * times l_active); d_out may be d_a. */
int pz_fr_mul_row_dev(pz_ctx* ctx, const uint64_t* d_a, size_t n_cols, size_t col_stride, size_t n, const uint64_t* d_row,
                      uint64_t* d_out, size_t out_stride);
/* division by the vanishing polynomial on the extended coset: d_h[i] /= (coset_g * omega_ext^i)^(2^log_n) - 1,
 * i < 2^(log_n + log_e) (the divisor takes 2^log_e distinct values; log_e = 0: the points are ONE coset of the 2^log_n-th roots and
 * the divisor is the constant coset_g^n - 1 -- the prover evaluates a quotient of degree < 3n on three such cosets instead of halo2's
 * 4n-point coset, paillier_halo2_amd/prover.py). */
int pz_quotient_finish_dev(pz_ctx* ctx, uint64_t* d_h, uint32_t log_n, uint32_t log_e, const uint64_t coset_g[4],
                           const uint64_t omega_ext[4]);
/* d_a[col][i] *= c * g^i, i < n (distribute_powers; with g = 1/coset_g the un-scaling step of extended_to_coeff).
 * c may be NULL (= 1). */
int pz_fr_distribute_powers_dev(pz_ctx* ctx, uint64_t* d_a, size_t n_cols, size_t col_stride, size_t n,
                                const uint64_t g[4], const uint64_t c[4]);
/* random linear combination of n_cols polynomials (n elements each): d_out[i] = sum_j v^(n_cols-1-j) * p_j[i], computed
 * as acc = acc*v + p_j over the columns; accumulate != 0 starts from the current d_out (continuing a Horner fold
 * across calls).  The polynomial folding step of the multiopen argument, before pz_poly_div_linear_dev. */
int pz_fr_lincomb_dev(pz_ctx* ctx, const uint64_t* d_polys, size_t n_cols, size_t col_stride, size_t n,
                      const uint64_t v[4], uint64_t* d_out, int accumulate);
/* kate_division: d_q[col] = (p_col(X) - p_col(x)) / (X - x) for n-coefficient polynomials: n-1 coefficients, the
 * n-th slot is written as zero (d_q may alias d_coeffs). */
int pz_poly_div_linear_dev(pz_ctx* ctx, const uint64_t* d_coeffs, size_t n_cols, size_t col_stride, size_t n,
                           const uint64_t x[4], uint64_t* d_q, size_t q_stride);

/* SHPLONK multi-point opening (halo2 multiopen::shplonk::prover, the last step of create_proof; SURVEY.md section 8f
 * rank 3).  Queries are grouped by rotation set: set k opens set_n_polys[k] coefficient-form polynomials (device
 * pointers, n coefficients each, listed set after set in d_polys) at set_n_points[k] points given as indices into
 * `points` (host, n_points_total x 4 limbs; the union of all sets' points, no duplicates).  evals (host): for each set,
 * for each of its polynomials, its value at each of the set's points.  y, v, u: the transcript's challenges (host).
 *   begin : d_h = sum_k v^k (sum_j y^j P_kj - R_k) / Z_{S_k}   (n coefficients; commit it, hash it, draw u)
 *   finish: d_h2 = (sum_k v^k z_k (sum_j y^j P_kj - R_k(u)) - Z_T(u) h) / (X - u) / z_0,  z_k = Z_{T \ S_k}(u);
 *           frees the state.  d_h2 may not alias d_h.
 * At most 16 sets, 8 points per set, 32 points overall; one opening in flight per context (the state lives in the context's
 * workspace). */
typedef struct pz_shplonk pz_shplonk;
int pz_shplonk_begin_dev(pz_ctx* ctx, size_t n, uint32_t n_sets, const uint32_t* set_n_polys, const uint64_t* const* d_polys,
                         const uint32_t* set_n_points, const uint32_t* point_idx, uint32_t n_points_total, const uint64_t* points,
                         const uint64_t* evals, const uint64_t y[4], const uint64_t v[4], uint64_t* d_h, pz_shplonk** state);
int pz_shplonk_finish_dev(pz_ctx* ctx, pz_shplonk* state, const uint64_t u[4], const uint64_t* d_h, uint64_t* d_h2);
int pz_shplonk_free(pz_ctx* ctx, pz_shplonk* state);

/* ---------------------------------------------------------------------------------------------
 * Patch point D as entry points: keygen and create_proof, one call per transcript round.
 * Replaces, for halo2-lib circuits (one gate q (a + b c - d) per advice column, range-check lookups of lookup-enabled advice columns
 * against one table column, a permutation over [advice | lookup advice | constants]): halo2-axiom's keygen_vk / keygen_pk /
 * create_proof as reached from /root/reference/src/bench.rs:161-171 (bench_builder -> keygen -> gen_proof).  The composition is the
 * one of paillier_halo2_amd/host/create_proof.hpp (the code tests/cpp/prove_connected runs; the quotient on three cosets of <omega_n>:
 * DESIGN.md section 6.3); the transcript stays with the caller: every phase returns what must be absorbed (affine points of 8 words,
 * evaluations of 4 words, all Montgomery) and takes the challenges squeezed after it (Montgomery representatives below r, else
 * PZ_ERR_INVALID).  The circuit STRUCTURE is an input of keygen, as it is of halo2's: selector positions, the constants column, and
 * the copy constraints as a permutation map (cell (c, r) of the permutation's columns -> (map_col, map_row); identity where
 * unconstrained) over m = n_adv + n_lk + 1 columns; the lookup table is 0 .. 2^lookup_bits - 1.  chunk = 2 (cs.degree() = 4).
 *
 * pz_pk_create   selectors: u8 [n_adv][2^k]; constants: n_constants x 4 words, canonical integers (NOT Montgomery), row order;
 *                map_col / map_row: u32 [m][2^k] (all host).  Builds and keeps RESIDENT the commitments, the coefficient forms and the
 *                extended forms of the fixed and sigma columns, l_0 / l_last / l_active, and one proof's workspace (at config c2:
 *                116 + 30 GB).  n_adv, n_lk >= 1; lookup_bits < k.  tile: columns extended per step of the quotient (even; 64).  The key holds device memory of `ctx`
 *                (which must outlive it) and serves ONE proof at a time.  The selectors are uploaded as bytes and become field elements on
 *                the device (pz_fr_from_mask_dev); the host arrays are not referenced after the call returns.
 *                ext_resident_cols: PZ_PK_EXT_ALL = the extended-coset forms of every selector and sigma column stay resident (halo2's
 *                ProvingKey: fixed_cosets / permutation.cosets); a number R = the STREAMED proving key: only selector j / sigma j with j < R
 *                keep them, the others are re-extended from their coefficient forms per tile inside pz_proof_quotient (+ one transform per
 *                such column, three cosets, per proof) -- the memory plan of shapes whose extended key does not fit (BASELINE config c5:
 *                3072-bit n, k = 19: 239 GB; R = 0 there).  The proof does not depend on R, byte for byte.
 * pz_pk_create_dev  the same with selectors / map_col / map_row ALREADY ON THE DEVICE (device pointers of `ctx`'s device: a structure
 *                generated there -- pz_circuit_structure_dev -- or uploaded by the caller): nothing of them crosses PCIe or is copied on the
 *                host; they are only read during the call.  constants stay a (small) host array.
 * pz_pk_info     n_fixed = n_adv + 2 (selectors | constants | table); blinding_words = 64-bit words of caller randomness one proof
 *                consumes; evals_words = length of pz_proof_evaluate's output.
 * pz_pk_commitments  the verifying key's commitments: n_fixed x 8 and m x 8 words.
 *
 * pz_proof_begin d_cols: device, [m][2^k] elements: the advice then the lookup-advice columns as pz_circuit_expand_cols_dev wrote
 *                them (rows >= max_rows zero); the last column and the blinding rows are filled here; CONSUMED (ends in coefficient
 *                form).  blinding: n_blinding >= blinding_words random words (host) -- a production prover hands over OS randomness; the
 *                elements are drawn uniformly below r by rejection (254-bit candidates), blinding_words includes the margin.  The
 *                deterministic stream from `seed` (tests, benches: NOT zero-knowledge) must be asked for explicitly: blinding = NULL
 *                AND n_blinding = PZ_BLINDING_SEEDED_TEST_STREAM; NULL with any other count is PZ_ERR_INVALID.
 *                -> advice_affine: (n_adv + n_lk) x 8.                                            [transcript: ... -> theta]
 * pz_proof_lookups       -> n_lk x 8 each (permuted inputs A', permuted tables S')                 [-> beta, gamma]
 * pz_proof_products      -> n_sets x 8 (permutation products), n_lk x 8 (lookup products), 8 (the vanishing argument's random
 *                        polynomial)                                                              [-> y]
 * pz_proof_quotient      -> 3 x 8: the quotient's pieces h_0, h_1, h_2                             [-> x]
 * pz_proof_evaluate      -> evals_words words: for each family in this order, for each of its polynomials, its values at the
 *                        family's points (indices into {x, wx, w^2 x, w^3 x, w^-(blinding_factors+1) x, w^-1 x}):
 *                        advice n_adv {0,1,2,3} | lookup advice then the constants column n_lk + 1 {0} | fixed n_fixed {0} |
 *                        sigma m {0} | permutation products n_sets {0,1,4} | lookup products n_lk {0,1} | A' n_lk {0,5} |
 *                        S' n_lk {0} | random 1 {0} | h_0 + x^n h_1 + x^2n h_2 1 {0} (the verifier computes the last itself:
 *                        not absorbed)                                                            [-> SHPLONK's y, v]
 * pz_proof_open_begin    -> 8: SHPLONK's first commitment                                          [-> u]
 * pz_proof_open_finish   -> 8: the second; quotient_degree_ok = 0 if the quotient's degree exceeds 3n - 4 (an unsatisfied
 *                        witness: the proof will not verify).
 * Phases out of order return PZ_ERR_INVALID; after any error only pz_proof_free is valid.  pz_proof_free releases the key's
 * workspace for the next proof; pz_pk_free refuses (PZ_ERR_INVALID) while a proof is open.
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * The circuit STRUCTURE of the reference's drivers, generated on the device (csrc/pz_structure.hip) -- what halo2's keygen extracts by
 * synthesising paillier_enc_test / paillier_enc_add_test (/root/reference/src/bench.rs:33-117) once: selector positions, the
 * copy-constraint permutation, the constants column, the break-point column layout.  It depends on the shape only: key size, limb
 * width, lookup bits and the BITS of the two fixed exponents (paillier.rs:50-55 hands m and n to pow_mod_fixed_exp), so with the
 * reference's circuit every new message needs a new structure and a new key:  pz_circuit_structure_dev -> pz_pk_create_dev ->
 * pz_structure_free -> proofs.  The compiled counterpart of paillier_halo2_amd/circuit_structure.py, equal to it array for array.
 * kind: 0 encrypt (exp_g = the message m, exp_r = the modulus n: ceil(limbs_n * limb_bits / 64) words each; only their bits are used), 1 add (no exponents),
 * 2 the uniform-shape encrypt circuit (exp_g ignored: one structure for every message of a key).  limb_bits 16..90, lookup_bits < k.
 * minimum_rows: the argument of the tester's calculate_params -- it fixes the NUMBER of advice / lookup-advice columns as
 * ceil(cells / (2^k - minimum_rows)) (20 on the reference's bench path, 9 under MockProver); columns are FILLED to
 * max_rows = 2^k - (blinding_factors + 3) (halo2-lib's FlexGateConfig::max_rows [D]).  PZ_ERR_UNSUPPORTED beyond 2^31 cells.
 * pz_structure_info: n_adv configured advice columns of which n_adv_filled hold cells; n_lk; max_rows; the counts K4 needs
 * (n_steps_g, n_steps_r) and the stream's sizes.
 * pz_structure_arrays: DEVICE pointers d_selectors u8 [n_adv][2^k], d_map_col / d_map_row u32 [m][2^k] (m = n_adv + n_lk + 1),
 * d_col_starts u64 [n_adv + 1] (what pz_circuit_expand_cols_dev takes); HOST pointers constants (n_constants x 4 words, canonical)
 * and col_starts_host.  All owned by the structure, valid until pz_structure_free.  Any output may be NULL.
 * pz_circuit_structure_tally_dev: the structure of the tally circuit (kind 3 of pz_circuit_cells) of `count` ciphertexts, 2 <= count <=
 * 65536 (else PZ_ERR_INVALID): its shape is count and the key size alone, so there are no exponents.  Block t's operand limbs are tied to
 * the remainder cells of the block that produced them or to the limb cells of assign_integer(c_i), by the product tree of
 * pz_paillier_tally.  An ordinary pz_structure (n_steps_g = count - 1, n_steps_r = 0): pz_structure_expose, pz_pk_create[_pub]_dev,
 * pz_vk_keygen[_pub]_dev and the pz_proof_* stepper take it as it is.
 * pz_circuit_structure_wtally_dev: the structure of the weighted tally (kind 4) of `count` ciphertexts (1 .. 65536) and w_bits (1 .. 64)
 * bits per weight: its shape is count, w_bits and the key size alone -- ONE key serves every weight vector and every set of ciphertexts.
 * The weight's load_witness cell is tied to its chain's num_to_bits accumulator, a chain's first sq to assign_integer(c_i)'s limbs, the
 * tree's leaves to the chains' last select outputs.  An ordinary pz_structure (n_steps_g = 2 count w_bits, n_steps_r = count - 1).
 * pz_circuit_structure_ballot_dev: the structure of the ballot (kind 6, pz_ballot_cells) of `count` ciphertexts (1 .. 1024) and m_bits
 * (1 .. 64) bits per message under the key whose modulus is exp_r (ceil(limbs_n * limb_bits / 64) words: its bits shape every r^n chain,
 * as in kind 2): ONE key serves every ballot of an election.  A message's load_witness cell is tied to its chain's num_to_bits
 * accumulator and to its operand in the sum, every g-chain's first sq to assign_integer(g)'s limbs extended by the load_zero cell, every
 * r-chain's base to assign_integer(r_i)'s, the final block's operands to the chains' results, each assert_equal_fresh's bit to the
 * constant 1.  An ordinary pz_structure (n_steps_g = 2 m_bits, n_steps_r = the records of ONE r^n chain); pz_structure_expose works on it
 * (statement: pz_ballot_public_cells).
 * pz_circuit_structure_partial_dev: the structure of a trustee's partial decryptions (kind 7, pz_partial_cells) of `count` ciphertexts
 * (1 .. 1024): ONE key serves every trustee and every set of ciphertexts of that count.  Every chain's num_to_bits accumulators are
 * tied to assign_integer(theta)'s limb cells, chain 0's first sq to assign_integer(v)'s, each squaring block's two operands to
 * assign_integer(c_j)'s, chain j's first sq to that block's remainder, each chain's last select outputs to the assert_equal_fresh against
 * h / u_j, each assert_equal_fresh's bit to the constant 1.  An ordinary pz_structure (n_steps_g = the 2 E records of ONE chain,
 * n_steps_r = 0); pz_structure_expose works on it (statement: pz_partial_public_cells).
 * pz_circuit_structure_mix_dev: the structure of the mix (kind 8, pz_mix_cells) of `count` = 2^d ciphertexts (1 .. 1024) under the key
 * whose modulus is exp_r (ceil(limbs_n * limb_bits / 64) words: its bits shape every r^n chain): ONE key serves every mixer of an
 * election.  Every select's sel cell is tied to its switch's bit cell, its operands to the limb cells they read, every r-chain's base
 * to assign_integer(r_i)'s limbs extended by the load_zero cell, the final block's operands to the last layer's outputs and the
 * chain's result, each assert_equal_fresh's bit to the constant 1.  An ordinary pz_structure (n_steps_g = 0, n_steps_r = the records
 * of ONE r^n chain); pz_structure_expose works on it (statement: pz_mix_public_cells).
 * pz_circuit_structure_sballot_dev: the structure of the short-randomness ballot (kind 9, pz_sballot_cells) of `count` ciphertexts
 * (1 .. 1024), m_bits (1 .. 64) bits per message and exponents of s_limbs (1 .. 2 limbs_n) limbs.  It takes NO exponent: nothing of
 * the key but its size shapes the circuit, and ONE key serves every election of a size (count, m_bits, s_limbs, limbs_n).  Every
 * hs-chain's num_to_bits accumulators are tied to assign_integer(s_i)'s limb cells, every hs-chain's first sq to assign_integer(hs)'s
 * limbs (all K chains run on ONE base), a message's load_witness cell to its chain's num_to_bits accumulator and to its operand in the
 * sum, every g-chain's first sq to assign_integer(g)'s limbs extended by the load_zero cell, the final block's operands to the
 * g-chain's and the hs-chain's last select outputs, its result to the assert_equal_fresh against res_i, each assert_equal_fresh's bit
 * to the constant 1.  An ordinary pz_structure (n_steps_g = 2 m_bits, n_steps_r = the 2 s_limbs limb_bits records of ONE hs-chain);
 * pz_structure_expose works on it (statement: pz_sballot_public_cells).
 * pz_circuit_structure_smix_dev: the structure of the short-randomness mix (kind 10, pz_smix_cells) of `count` = 2^d ciphertexts (1 ..
 * 1024) with exponents of s_limbs (1 .. 2 limbs_n) limbs.  It takes NO exponent: nothing of the key but its size shapes the circuit, and
 * ONE key serves every mixer of every election of a size (count, s_limbs, limbs_n).  Kind 8's network walk composed with kind 9's chain
 * walk: every select's sel cell is tied to its switch's bit cell, its operands to the limb cells they read, every hs-chain's first sq
 * to assign_integer(hs)'s limbs, every chain's num_to_bits accumulators to assign_integer(s_i)'s limb cells, the final block's
 * operands to the last layer's outputs and the chain's last select outputs, its result to the assert_equal_fresh against c'_i, each
 * assert_equal_fresh's bit to the constant 1.  An ordinary pz_structure (n_steps_g = 0, n_steps_r = the 2 s_limbs limb_bits records of
 * ONE hs-chain); pz_structure_expose works on it (statement: pz_smix_public_cells).
 * pz_circuit_structure_pballot_dev: the structure of the packed ballot (kind 11, pz_pballot_cells) of `count` ciphertexts (1 .. 1024) of
 * `slots` values (1 .. 64, count * slots <= 1024) of m_bits (1 .. 64) bits with exponents of s_limbs (1 .. 2 limbs_n) limbs.  It takes
 * NO exponent and no slot width: ONE key serves every election of a size (count, slots, m_bits, s_limbs, limbs_n).  The copy
 * constraints carry the claim: slot j's first sq is tied to assign_integer(G_j)'s limb cells for EVERY ciphertext (what binds a slot to
 * its base), every hs-chain's first sq to assign_integer(hs)'s limbs, a value's load_witness cell to its chain's num_to_bits
 * accumulator and to its operand in its ciphertext's sum, every hs-chain's num_to_bits accumulators to assign_integer(s_i)'s limb
 * cells, every fold's operands to the last select outputs of the chain or the remainder of the fold they name, the last fold's result
 * to the assert_equal_fresh against res_i, each assert_equal_fresh's bit to the constant 1.  An ordinary pz_structure (n_steps_g = 2
 * m_bits, n_steps_r = the 2 s_limbs limb_bits records of ONE hs-chain); pz_structure_expose works on it (statement:
 * pz_pballot_public_cells).
 * ------------------------------------------------------------------------------------------- */
typedef struct pz_structure pz_structure;
int pz_circuit_structure_dev(pz_ctx* ctx, int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k,
                             const uint64_t* exp_g, const uint64_t* exp_r, size_t minimum_rows, uint32_t blinding_factors,
                             pz_structure** out);
int pz_circuit_structure_tally_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                   size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_wtally_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                    uint32_t w_bits, size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_ballot_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                    uint32_t m_bits, const uint64_t* exp_r, size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_mix_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                 const uint64_t* exp_r, size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_partial_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                     size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_sballot_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                     uint32_t m_bits, uint32_t s_limbs, size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_smix_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                  uint32_t s_limbs, size_t minimum_rows, uint32_t blinding_factors, pz_structure** out);
int pz_circuit_structure_pballot_dev(pz_ctx* ctx, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, uint32_t k, size_t count,
                                     uint32_t slots, uint32_t m_bits, uint32_t s_limbs, size_t minimum_rows, uint32_t blinding_factors,
                                     pz_structure** out);
int pz_structure_info(const pz_structure* st, size_t* n_adv, size_t* n_adv_filled, size_t* n_lk, size_t* max_rows, size_t* n_constants,
                      size_t* n_cells, size_t* n_lookups, size_t* n_steps_g, size_t* n_steps_r);
int pz_structure_arrays(const pz_structure* st, const uint8_t** d_selectors, const uint32_t** d_map_col, const uint32_t** d_map_row,
                        const uint64_t** d_col_starts, const uint64_t** constants, const uint64_t** col_starts_host);
int pz_structure_free(pz_structure* st);

typedef struct pz_pk pz_pk;
typedef struct pz_proof pz_proof;
#define PZ_BLINDING_SEEDED_TEST_STREAM (~(size_t)0)
#define PZ_PK_EXT_ALL (~(size_t)0)
int pz_pk_create(pz_ctx* ctx, const pz_bases* bases_lagrange, const pz_bases* bases_monomial, uint32_t k, uint32_t lookup_bits,
                 uint32_t blinding_factors, size_t max_rows, size_t n_adv, size_t n_lk, const uint8_t* selectors,
                 const uint64_t* constants, size_t n_constants, const uint32_t* map_col, const uint32_t* map_row, size_t tile,
                 size_t ext_resident_cols, pz_pk** out);
int pz_pk_create_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, const pz_bases* bases_monomial, uint32_t k, uint32_t lookup_bits,
                     uint32_t blinding_factors, size_t max_rows, size_t n_adv, size_t n_lk, const uint8_t* d_selectors,
                     const uint64_t* constants, size_t n_constants, const uint32_t* d_map_col, const uint32_t* d_map_row, size_t tile,
                     size_t ext_resident_cols, pz_pk** out);
int pz_pk_info(const pz_pk* pk, size_t* n_fixed, size_t* n_perm_cols, size_t* n_sets, size_t* blinding_words, size_t* evals_words);
int pz_pk_commitments(const pz_pk* pk, uint64_t* fixed_affine, uint64_t* sigma_affine);
int pz_pk_free(pz_pk* pk);
int pz_proof_begin(pz_pk* pk, uint64_t* d_cols, uint64_t seed, const uint64_t* blinding, size_t n_blinding, pz_proof** out,
                   uint64_t* advice_affine);
int pz_proof_lookups(pz_proof* proof, const uint64_t theta[4], uint64_t* perm_inputs_affine, uint64_t* perm_tables_affine);
int pz_proof_products(pz_proof* proof, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* perm_z_affine,
                      uint64_t* lookup_z_affine, uint64_t* random_affine);
int pz_proof_quotient(pz_proof* proof, const uint64_t y[4], uint64_t* h_affine);
int pz_proof_evaluate(pz_proof* proof, const uint64_t x[4], uint64_t* evals);
int pz_proof_open_begin(pz_proof* proof, const uint64_t y[4], const uint64_t v[4], uint64_t* w1_affine);
int pz_proof_open_finish(pz_proof* proof, const uint64_t u[4], uint64_t* w2_affine, int* quotient_degree_ok);
int pz_proof_free(pz_proof* proof);

/* ---------------------------------------------------------------------------------------------
 * PUBLIC INPUTS (csrc/pz_public.hip): one optional instance column, n_instance in {0, 1} -- halo2-lib's
 * assigned_instances / num_instance_columns [D], which the reference's drivers leave at zero, as every entry point above does.  With it a
 * proof states that a GIVEN ciphertext c is the encryption under a GIVEN key (n, g), not only that some witness fits the shape.
 *   - the instance column is the LAST column of the permutation, [advice | lookup advice | constants | instance], m' = m + 1 columns,
 *     n_sets = ceil(m' / 2); the indices and delta powers of the other columns do not move.  Row i < n_public holds public value i, every
 *     other row is zero, the blinding rows included (halo2 does not blind instance columns).  n_public <= max_rows.
 *   - it is neither committed nor opened: a proof grows by one sigma evaluation and, when m' is odd, one permutation product.  The
 *     verifier computes inst(x) = sum_{i < n_public} v_i l_i(x), l_i(x) = (x^n - 1)/n omega^i / (x - omega^i), itself and uses it as the
 *     last permuted value; a challenge x with x^n = 1 gives verdict 0.
 *   - transcript: the n_public values are absorbed as scalars (Montgomery words, like every other scalar) after the caller's seed and
 *     before the first advice commitment; with no instance column nothing is absorbed and every existing transcript is unchanged.
 *   - exposed values: little-endian limbs of limb_bits, n[limbs_n] | g[limbs_n] | c[2 limbs_n] for kind 0 and 2,
 *     n | g | c1[limbs_n] | c2[limbs_n] | c[2 limbs_n] for kind 1 (add); m and r stay private.  Kind 3 (tally of B = n_steps_g + 1):
 *     n[limbs_n] | c_1[2 limbs_n] | .. | c_B[2 limbs_n] | C[2 limbs_n].  Kind 4 (weighted tally of B = n_steps_r + 1): n | c_1 | .. | c_B |
 *     w_1 | .. | w_B | C, a weight being ONE value (its load_witness cell), n_public = limbs_n + (B + 1) 2 limbs_n + B.  (Kind 0 bakes the message's bits into the
 *     key's shape -- the reference's property; kind 2, the uniform-shape circuit, is the zero-knowledge statement.)
 *     Kind 5 (decrypt): n[limbs_n] | g[limbs_n] | m[limbs_n] | c[2 limbs_n], n_public = 5 limbs_n -- "c decrypts to m": there is an r with
 *     c = g^m r^n mod n^2.  The circuit does not compare m with n: the verifier must, on the two public values (m >= n says nothing).
 * pz_circuit_public_cells  host only: the stream indices of the exposed advice cells in that order (arguments as pz_circuit_cells).
 *                cells_out may be NULL (count only); PZ_ERR_CAPACITY if capacity < *n_public.
 * pz_structure_expose      adds the column to a structure: the exposed cells' (column, row) through the break-point table, the instance
 *                cells inserted into their copy cycles ON THE DEVICE (each the greatest cell of its class: the class's last cell maps to
 *                it, it maps to the class's first; the n_public rows are grouped by class with one host sort, so a tally's tens of
 *                thousands of cells cost O(n_public log n_public)), d_map_col / d_map_row regrown to [m + 1][2^k] -- pz_structure_arrays
 *                returns the new ones, the earlier pointers are dead.  Selectors and everything else are untouched.  Once per structure.
 *                PZ_ERR_UNSUPPORTED if n_public exceeds max_rows, the column's usable rows (a tally of too many ciphertexts for this k).
 * pz_structure_public      n_instance, n_public and the DEVICE arrays d_cell_col / d_cell_row (u32, n_public each; NULL before expose).
 * pz_public_gather_dev     out_words (HOST, n_public x 4 canonical words) = the exposed cells of a witness column block d_cols (columns
 *                col_stride words apart, Montgomery): a prover reads the statement off its own witness.  Synchronises.  col_stride must be a
 *                multiple of 4 and d_cols 16-byte aligned (PZ_ERR_INVALID otherwise).  The cell arrays are TRUSTED: every (column, row) must
 *                lie inside the caller's column block (pz_structure_public's arrays do, for a block of n_adv columns of 2^k rows); they are
 *                not checked against it.
 * pz_instance_eval_dev     the verifier's kernel on its own: d_out[p] = inst_p(x_p) for n_proofs proofs; d_instances n_proofs x n_public x 4
 *                canonical words, d_x / d_out n_proofs x 4 Montgomery words, omega the 2^k-th root, n_inv = 1 / 2^k (host, Montgomery).  One
 *                field inversion per 1024 terms (batch inversion across a workgroup).  d_flags[p] (int32): bit 0 x_p lies on the domain
 *                (a zero denominator, or x^n = 1), bit 1 a value >= r; d_out[p] is then meaningless.  Any n_public from 0 to 2^k.
 *                Asynchronous on the context's stream.
 * pz_pk_create_pub[_dev], pz_vk_keygen_pub[_dev], pz_vk_create_pub   the entry points above with n_instance and n_public; maps and
 *                sigma_affine have m + n_instance columns; n_instance = 0 (then n_public must be 0) IS the old entry point.
 *                pz_pk_info, pz_vk_info, pz_proof_wire_bytes, pz_proof_encode / _decode follow the key's m' and n_sets.
 * pz_proof_begin_pub       pz_proof_begin plus instances (n_public x 4 canonical words, host): d_cols is [m'][2^k]; the constants column
 *                AND the instance column are filled here.  A value >= r or a wrong n_public: PZ_ERR_INVALID.
 * pz_verify_batch_pub, pz_verify_batch_bytes_pub   instances: n_proofs x n_public x 4 canonical words (host).  A value >= r gives verdict
 *                0 for that proof; the others are judged without it.
 * An OLD entry point (pz_proof_begin, pz_verify_batch, pz_verify_batch_bytes) on a key with an instance column, or a wrong n_public:
 * PZ_ERR_INVALID.
 * ------------------------------------------------------------------------------------------- */
int pz_circuit_public_cells(int kind, uint32_t limbs_n, uint32_t limb_bits, uint32_t lookup_bits, size_t n_steps_g, size_t n_steps_r,
                            uint64_t* cells_out, size_t capacity, size_t* n_public);
int pz_structure_expose(pz_structure* st);
int pz_structure_public(const pz_structure* st, size_t* n_instance, size_t* n_public, const uint32_t** d_cell_col, const uint32_t** d_cell_row);
int pz_public_gather_dev(pz_ctx* ctx, const uint64_t* d_cols, size_t col_stride, const uint32_t* d_cell_col, const uint32_t* d_cell_row,
                         size_t n_public, uint64_t* out_words);
int pz_instance_eval_dev(pz_ctx* ctx, uint32_t k, const uint64_t omega[4], const uint64_t n_inv[4], const uint64_t* d_instances,
                         size_t n_public, size_t n_proofs, const uint64_t* d_x, uint64_t* d_out, int32_t* d_flags);
int pz_pk_create_pub(pz_ctx* ctx, const pz_bases* bases_lagrange, const pz_bases* bases_monomial, uint32_t k, uint32_t lookup_bits,
                     uint32_t blinding_factors, size_t max_rows, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                     const uint8_t* selectors, const uint64_t* constants, size_t n_constants, const uint32_t* map_col, const uint32_t* map_row,
                     size_t tile, size_t ext_resident_cols, pz_pk** out);
int pz_pk_create_pub_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, const pz_bases* bases_monomial, uint32_t k, uint32_t lookup_bits,
                         uint32_t blinding_factors, size_t max_rows, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                         const uint8_t* d_selectors, const uint64_t* constants, size_t n_constants, const uint32_t* d_map_col,
                         const uint32_t* d_map_row, size_t tile, size_t ext_resident_cols, pz_pk** out);
int pz_vk_keygen_pub_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                         size_t n_instance, size_t n_public, const uint8_t* d_selectors, const uint64_t* constants, size_t n_constants,
                         const uint32_t* d_map_col, const uint32_t* d_map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine);
int pz_vk_keygen_pub(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                     size_t n_instance, size_t n_public, const uint8_t* selectors, const uint64_t* constants, size_t n_constants,
                     const uint32_t* map_col, const uint32_t* map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine);
int pz_vk_create_pub(pz_ctx* ctx, uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                     const uint64_t* fixed_affine, const uint64_t* sigma_affine, const uint64_t g0_affine[8], const uint64_t g2[16],
                     const uint64_t s_g2[16], pz_vk** out);
int pz_proof_begin_pub(pz_pk* pk, uint64_t* d_cols, uint64_t seed, const uint64_t* blinding, size_t n_blinding, const uint64_t* instances,
                       size_t n_public, pz_proof** out, uint64_t* advice_affine);
int pz_verify_batch_pub(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint64_t* proofs, size_t n_proofs, const uint8_t* seeds,
                        const size_t* seed_offsets, int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine, int* all_ok);
int pz_verify_batch_bytes_pub(pz_vk* vk, const uint64_t* instances, size_t n_public, const uint8_t* bytes, size_t n_proofs,
                              const uint8_t* seeds, const size_t* seed_offsets, int32_t* verdicts, uint64_t* h_evals, uint64_t* ab_affine,
                              int* all_ok);

/* ---------------------------------------------------------------------------------------------
 * KEY BINDING (host/key_digest.hpp): the verifying key's digest at the head of the Fiat-Shamir transcript, where
 * halo2 absorbs vk.transcript_repr.  Opt-in: without it every transcript starts from the caller's seed alone and every proof, key and file
 * is byte for byte what it was.
 *   D = BLAKE2b-512, personalisation the 16 bytes "PZ-Key-Digest-v1", over six little-endian u64 -- k, blinding_factors, n_adv, n_lk,
 *   n_instance, n_public -- then fixed_affine ((n_adv + 2) x 8 words) and sigma_affine ((n_adv + n_lk + 1 + n_instance) x 8 words), both as
 *   pz_pk_commitments, pz_vk_keygen* and pz_vk_create[_pub] carry them (Montgomery words, little-endian).  lookup_bits is pinned by the table
 *   column's commitment; the params are not part of it.  A BOUND transcript is the unbound one with D || seed for its seed bytes.
 * pz_key_digest   host only: no context, no device.  n_instance = 0 with n_public != 0, or a null pointer: PZ_ERR_INVALID.
 * pz_pk_digest, pz_vk_digest   the key's D, computed on the first request and kept in the object.  The prover stepper (pz_proof_*) never
 *                 sees the transcript: its caller asks pz_pk_digest and seeds with D || seed.
 * pz_vk_bind      on != 0: pz_verify_batch, pz_verify_batch_pub, pz_verify_batch_bytes and pz_verify_batch_bytes_pub replay every proof from
 *                 D || seed; 0 (the default of a new key): from the seed alone.  A proof made one way does not verify the other way
 *                 (verdict 0, not an error).
 * pz_vk_is_bound  *on = 1 or 0.
 * ------------------------------------------------------------------------------------------- */
int pz_key_digest(uint32_t k, uint32_t blinding_factors, size_t n_adv, size_t n_lk, size_t n_instance, size_t n_public,
                  const uint64_t* fixed_affine, const uint64_t* sigma_affine, uint8_t out[64]);
int pz_pk_digest(const pz_pk* pk, uint8_t out[64]);
int pz_vk_digest(const pz_vk* vk, uint8_t out[64]);
int pz_vk_bind(pz_vk* vk, int on);
int pz_vk_is_bound(const pz_vk* vk, int* on);

/* ---------------------------------------------------------------------------------------------
 * measurement helpers (used by bench.py; not part of the reference surface).  Issue-rate microbenchmarks: libpz_probe.so.
 * ------------------------------------------------------------------------------------------- */
/* HIP-event timing of the dominant kernel on the context's stream: accumulated since the last
 * reset, for kernel class `which` (0 = MSM bucket accumulation, 1 = NTT passes, 2 = modexp trace,
 * 3 = witness expand, 4 = MSM whole pipeline, 5 = MSM digit sort (histogram, scans, scatter), 6 = MSM bucket folds and
 * reduction tree).  Enabled by pz_timing_enable(ctx, 1). */
int pz_timing_enable(pz_ctx* ctx, int on);
int pz_timing_reset(pz_ctx* ctx);
int pz_timing_get(pz_ctx* ctx, int which, double* total_ms, uint64_t* launches);
#ifdef __cplusplus
}
#endif
#endif /* PZ_H */
