// pz_internal.h -- shared host-side plumbing of libpz_hip.so (context, workspaces, error handling,
// HIP-event timing).  Not part of the ABI; the ABI is include/pz.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/pz.h"

enum { PZ_T_MSM_ACC = 0, PZ_T_NTT = 1, PZ_T_TRACE = 2, PZ_T_EXPAND = 3, PZ_T_MSM_ALL = 4, PZ_T_MSM_SORT = 5, PZ_T_MSM_TREE = 6, PZ_T_COUNT = 7 };

struct pz_pow_table {   // cached table init * base^i, i < n  (twiddles omega^i, coset powers s*g^i)
    uint64_t base[4];
    uint64_t init[4];
    size_t n;
    size_t cap;         // entries the buffer holds (>= n: an evicted table's buffer is reused)
    void* d;            // cap x 32 B
    void* d_raw = nullptr;   // the same entries as constant pairs (c, floor(c 2^261 / p)), 18 x 29-bit limbs = 72 B each, built on demand for the K2 kernels
    bool raw_valid = false;
    uint64_t stamp;     // last use (LRU: per-proof challenge points would otherwise grow the cache without bound)
};

struct pz_ext_table {   // packed [2^e][n] pre-scale tables of pz_ntt_fr_extend_dev, keyed by its parameters
    std::vector<uint64_t> key;
    void* d;       // constant pairs, 72 B per entry: [2^e][n][18] u32
};

struct pz_wsbuf {
    void* d = nullptr;
    size_t cap = 0;
};

enum { WS_HIST = 0, WS_OFFS, WS_CURSOR, WS_ITEMS, WS_ENTRIES, WS_PARTIALS, WS_NODES_A, WS_NODES_B, WS_NTT_TMP,
       WS_IO_A, WS_IO_B, WS_IO_C, WS_BIG_A, WS_BIG_B, WS_BIG_C, WS_MISC, WS_TOTALS, WS_ORDER, WS_SH_C, WS_SH_SMALL, WS_ROWC, WS_SEL, WS_K3, WS_MULTI, WS_PAIR, WS_PRIME_TAB, WS_PRIME_SIEVE, WS_PRIME_MR, WS_COUNT };

struct pz_event_pair {
    hipEvent_t a, b;
};

#define PZ_IO_EVENTS 10
struct pz_arena;
struct pz_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    char hip_err[256] = {0};
    pz_wsbuf ws[WS_COUNT];
    std::vector<pz_pow_table> pow_tables;
    uint64_t pow_clock = 0;
    std::vector<pz_ext_table> ext_tables;
    bool timing = false;
    std::vector<pz_event_pair> ev[PZ_T_COUNT];
    size_t ev_used[PZ_T_COUNT] = {0};
    double ev_ms[PZ_T_COUNT] = {0};
    uint64_t ev_n[PZ_T_COUNT] = {0};
    int cu_count = 256;
    size_t mem_avail = 0;      // (free + held) / 2 as last queried by pz_msm_g1_dev; hipMemGetInfo drains the queue on ROCm,
    unsigned mem_avail_age = 0; // so it is asked again only every 64 calls
    // host-pointer entry points (pz_msm_g1_batch, pz_ntt_fr_batch): copy engines of their own, so that the PCIe transfers
    // of the next / previous column group run beside the kernels of the current one (pz_io_init creates them on first use)
    hipStream_t io_h2d = nullptr, io_d2h = nullptr;
    hipEvent_t io_ev[PZ_IO_EVENTS] = {};
    // small pinned staging blocks for host arguments of asynchronous entry points (pz_upload_small_async): a ring of four, a
    // slot is reused only after the copy recorded on it has completed
    void* stage_h[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t stage_cap[4] = {0, 0, 0, 0};
    hipEvent_t stage_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned stage_next = 0;
    // asynchronous-failure flag: one word of pinned host memory a kernel sets when it finds an internal invariant broken (the
    // scatter kernels' position checks, pz_msm.hip); read and cleared by pz_check_async after a synchronisation
    volatile unsigned* async_err_h = nullptr;
    volatile unsigned* async_err_d = nullptr;   // the same word as the device addresses it
    // pz_dev_alloc / pz_dev_free block cache (pz_dev_cache_limit; off by default): freed blocks of 32 MiB and more are kept, up to
    // dev_cache_limit bytes, and handed to the next request of (nearly) that size -- a caller that builds a 116-GB proving key per
    // message pays the driver's allocation cost once, not per key
    size_t dev_cache_limit = 0, dev_cache_bytes = 0;
    std::vector<std::pair<void*, size_t>> dev_cache;
    std::map<void*, size_t> dev_live;   // sizes of the live pz_dev_alloc blocks (only tracked while the cache is on)
    // pz_dev_arena: one reserved block of device memory this context's allocations (pz_dev_alloc and the library's own buffers)
    // are carved from, so that a caller who builds and drops a proving key per message makes no driver allocation call after start-up
    struct pz_arena* arena = nullptr;
    bool prime_table_ready = false;   // the sieve primes (the odd primes below 2^16) are in ws[WS_PRIME_TAB] (pz_prime.hip)
    std::recursive_mutex mu;   // one context is serialised internally: entry points may be called from any thread
};

struct pz_bases {
    size_t n = 0;          // points
    uint32_t c = 0;        // window bits
    uint32_t nwin = 0;     // floor(253/c)+1
    void* d_table = nullptr;  // nwin x n affine points (64 B), window-major
    int lagrange = 0;
    int device = 0;
};

static inline int pz_hip_fail(pz_ctx* ctx, hipError_t e, const char* what) {
    if (ctx) snprintf(ctx->hip_err, sizeof ctx->hip_err, "%s: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PZ_ERR_OOM : PZ_ERR_HIP;
}
#define HIPCHK(ctx, x)                                              \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) return pz_hip_fail((ctx), e_, #x);    \
    } while (0)
#define PZCHK(x)                    \
    do {                            \
        int rc_ = (x);              \
        if (rc_ != PZ_OK) return rc_; \
    } while (0)

// first statement of every entry point that touches the device: serialise on the context (workspaces, caches and the
// stream order belong to it; entry points call each other, hence recursive) and select its device for this thread
#define PZ_ENTER(ctx)                                           \
    std::lock_guard<std::recursive_mutex> pz_lock_((ctx)->mu);  \
    HIPCHK((ctx), hipSetDevice((ctx)->device))

// grow-only workspace slot; contents are NOT preserved across growth
int pz_ws_get(pz_ctx* ctx, int slot, size_t bytes, void** out);
// hipMalloc for the library's own buffers: on out-of-memory the pz_dev_alloc block cache is released and the request repeated once
hipError_t pz_hip_malloc(pz_ctx* ctx, void** d, size_t bytes);
// the counterpart: a block of ANY context's arena goes back to its arena (after a device synchronisation: hipFree's own semantics, the
// callers rely on it), anything else to hipFree
hipError_t pz_hip_free(void* d);
// free device memory as the library should plan with it: the driver's figure plus what this context's arena has free
size_t pz_mem_free_bytes(pz_ctx* ctx);
void pz_dev_cache_trim(pz_ctx* ctx, size_t keep_bytes);
// cached base^i table (device, Fr Montgomery)
int pz_get_pow_table(pz_ctx* ctx, const uint64_t base[4], size_t n, void** d_out, const uint64_t* init = nullptr);
// the same table as raw 9 x 29-bit limbs per entry (n x 9 u32), cached beside it
int pz_get_pow_table_raw(pz_ctx* ctx, const uint64_t base[4], size_t n, void** d_raw_out, const uint64_t* init = nullptr);
// dst[9 i + j] = limb j (29 bits; the top limb takes the rest) of the 256-bit integer src[i]: asynchronous on the context's stream
int pz_raw29_convert(pz_ctx* ctx, const void* d_src_fr, void* d_dst_u32, size_t count);

// timing scopes: record an event pair around a kernel-class region on ctx->stream
struct pz_timer {
    pz_ctx* ctx;
    int cls;
    bool on;
    size_t idx;
    pz_timer(pz_ctx* c, int cls_);
    ~pz_timer();
};

int pz_async_err_init(pz_ctx* ctx);    // allocates the flag on first use
int pz_check_async(pz_ctx* ctx);       // after a stream synchronisation: PZ_ERR_ASYNC (and the flag cleared) if a kernel raised it
const uint64_t* pz_fr_one261();   // Montgomery one times 32: first entry of a power table kept in the 2^261 domain (fp29.cuh)
int pz_io_init(pz_ctx* ctx);
// asynchronous host -> device copy of a SMALL host argument (pageable memory the caller may free on return): staged through a
// pinned block of the context (ring of four; a block is reused only after the copy queued from it has completed)
int pz_upload_small_async(pz_ctx* ctx, void* d_dst, const void* src, size_t bytes);   // streams + events of the host-pointer pipelines; orders io_h2d after ctx->stream

// pz_permutation_sigma_part_dev for a range of columns given by its own part of the maps (pz_vkgen.hip; keygen_vk's host-pointer form)
int pz_permutation_sigma_tile(pz_ctx* ctx, const uint32_t* d_mc, const uint32_t* d_mr, size_t m_total, size_t n_cols, uint32_t k,
                              const uint64_t omega[4], const uint64_t delta[4], uint64_t* d_sigma, size_t sigma_stride);

// device buffers of one call of a host-composition entry point (pz_vk_keygen.cpp, pz_params.cpp), freed on every path out of it
// (pz_dev_free waits for the queued work)
struct pz_dev_bufs {
    pz_ctx* c;
    std::vector<void*> bufs;
    explicit pz_dev_bufs(pz_ctx* c_) : c(c_) {}
    int get(size_t bytes, void** out) {
        *out = nullptr;
        const int rc = pz_dev_alloc(c, bytes ? bytes : 1, out);
        if (rc == PZ_OK) bufs.push_back(*out);
        return rc;
    }
    ~pz_dev_bufs() {
        for (void* d : bufs) pz_dev_free(c, d);
    }
};
// n bytes of OS randomness (getrandom, /dev/urandom behind it): the verifier's fold weights, pz_params_check's rho and tau (pz_verify.cpp)
bool pz_os_random(void* buf, size_t n);

// the per-kind limits of the circuits: what the structure generator (pz_structure.hip) and the expansion (pz_witness.hip) refuse alike
#define PZ_TALLY_MAX 65536    // ciphertexts of a tally or a weighted tally (kinds 3, 4)
#define PZ_ENTRIES_MAX 1024   // entries of a ballot, an opening or a mix (kinds 6 .. 11); kind 11: count * slots, its in-circuit values
#define PZ_WORD_BITS_MAX 64   // bits of a weight, a message or a slot value: one 64-bit word
#define PZ_SLOTS_MAX 64       // slots of a packed ballot (kind 11)
static inline bool pz_count_ok(size_t count, size_t lo, size_t max) { return count >= lo && count <= max; }
static inline bool pz_word_bits_ok(uint32_t bits) { return bits >= 1 && bits <= PZ_WORD_BITS_MAX; }
static inline bool pz_short_exp_ok(uint32_t s_limbs, uint32_t limbs_n) { return s_limbs >= 1 && s_limbs <= 2 * (uint64_t)limbs_n; }   // of hs^s
static inline bool pz_slots_ok(size_t count, uint32_t slots) { return slots >= 1 && slots <= PZ_SLOTS_MAX && count * slots <= PZ_ENTRIES_MAX; }

// the circuit structure handle (pz_circuit_structure_dev, pz_structure.hip).  pz_structure_expose (pz_public.hip) adds the instance column:
// d_map_col / d_map_row are then [m + 1][2^k] and d_cell_col / d_cell_row hold the (column, row) of the n_public exposed advice cells
struct pz_structure {
    pz_ctx* ctx = nullptr;
    uint8_t* d_selectors = nullptr;
    uint32_t *d_map_col = nullptr, *d_map_row = nullptr;
    uint64_t* d_starts = nullptr;
    std::vector<uint64_t> constants;   // canonical integers, 4 words each
    std::vector<uint64_t> starts;      // host copy (n_adv + 1)
    size_t n_adv = 0, n_used = 0, n_lk = 0, max_rows = 0, n_cells = 0, n_lookups = 0, n_steps_g = 0, n_steps_r = 0;
    uint32_t k = 0;
    int kind = 0;
    uint32_t limbs_n = 0, limb_bits = 0, lookup_bits = 0;
    size_t count = 0;                  // kind 6 (the ballot): its ciphertexts; n_steps_g = 2 m_bits, n_steps_r = the records of one r^n chain.
                                       // kind 7 (a trustee's partial decryptions): its ciphertexts; n_steps_g = the records of one chain
    uint32_t slots = 0;                // kind 11 (the packed ballot): the slots of a ciphertext; count = its ciphertexts, n_steps_g = 2 m_bits,
                                       // n_steps_r = the records of one hs-chain
    size_t n_instance = 0, n_public = 0;
    uint32_t *d_cell_col = nullptr, *d_cell_row = nullptr;
};

static inline unsigned pz_div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// the device batch verifier (pz_verify.hip kernels, pz_verify.cpp orchestration).  Offsets in 4-word elements into a proof's
// evaluation array (pz_proof_evaluate's), counts of a verifying key's shape; sets in verifier / prover.query_layout's order.
#define PZ_VSETS_MAX 5
struct pz_vshape {
    uint32_t A, Lk, F, m, S;   // m counts the instance column when the key has one (n_inst = 1: the permutation's LAST column)
    uint32_t n_inst;
    uint32_t n_own;   // the proof's commitments = its own bases: A + 4 Lk + S + 6
    uint32_t n_vkb;   // fixed | sigma | g0: F + m + 1
    uint32_t n_ev;    // evaluation elements
    uint32_t e_adv, e_lka, e_fix, e_sig, e_pz, e_lz, e_ap, e_sp, e_rnd, e_h;
    uint32_t n_sets;
    uint32_t set_start[PZ_VSETS_MAX], set_count[PZ_VSETS_MAX], set_npts[PZ_VSETS_MAX];
};
// a member of a query set: (evaluation element offset, destination); the destination's top two bits say which scalar array
enum { PZ_VM_OWN = 0, PZ_VM_VK = 1, PZ_VM_H = 2 };
// per-proof scalars the host derives after replaying the transcript (Montgomery, 4 words each)
enum { VP_BETA = 0, VP_GAMMA, VP_Y, VP_BX, VP_L0, VP_LLAST, VP_LACT, VP_INV, VP_XN, VP_SY, VP_W1A, VP_W2A, VP_W2B, VP_INST, VP_COEF,
       VP_LAG = VP_COEF + PZ_VSETS_MAX, VP_COUNT = VP_LAG + 4 * PZ_VSETS_MAX };
int pz_verify_terms_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, const uint32_t* d_members, const uint64_t* d_evals,
                           const uint64_t* d_pp, const uint64_t* d_delta, uint64_t* d_h, int32_t* d_ident, uint64_t* d_own,
                           uint64_t* d_vksc, uint64_t* d_gpart);
// the instance column at each proof's challenge (pz_public.hip): d_out[p * out_stride ..+4] = sum_{i<L} v_pi l_i(x_p) for B proofs, instances
// canonical words [B][L][4], x Montgomery words at d_x + p * x_stride; d_flags[p]: bit 0 x_p lies on the domain, bit 1 a value >= r.
// Strides in 64-bit words.  Asynchronous on the context's stream.
int pz_instance_eval_launch(pz_ctx* ctx, uint32_t k, const uint64_t omega[4], const uint64_t n_inv[4], const uint64_t* d_instances, size_t L,
                            size_t B, const uint64_t* d_x, size_t x_stride, uint64_t* d_out, size_t out_stride, int32_t* d_flags);
// pz_g1_check_dev's predicate (pz_msm.hip: the identity, or canonical coordinates on the curve) over n_groups x group affine points:
// d_flags[g] = 1 if a point of group g fails it, else 0.  Asynchronous on the context's stream.
int pz_g1_check_groups_launch(pz_ctx* ctx, const uint64_t* d_points, size_t n_groups, size_t group, int32_t* d_flags);
int pz_verify_fold_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, int mode, const uint64_t* d_r, uint64_t* d_vksc,
                          const uint64_t* d_gpart, const uint64_t* d_own, uint64_t* d_cols);

// halo2 wire bytes <-> words (pz_wire.hip).  Where element i of a launch lies: proof p = i / per, member j = i % per; its 32 wire bytes
// at p * wire_stride + (j < split ? wire_off0 + 32 j : wire_off1 + 32 (j - split)), its words at p * word_stride + word_off + j * (its
// size), its status at p * st_stride + st_off + j.  Byte offsets but for the status'.  skip_last: member per - 1 has no wire bytes.
struct pz_wire_map {
    size_t per, split;
    size_t wire_stride, wire_off0, wire_off1;
    size_t word_stride, word_off;
    size_t st_stride, st_off;
    int skip_last;
};
// a batch of B proofs between wire bytes (B x 32 (n_own + n_ev - 1)) and pz_verify_batch's words; decode fills d_elem_status
// (B x (n_own + n_ev)) and d_status (B: each proof's worst element status).  Asynchronous on the context's stream.
int pz_wire_proofs_launch(pz_ctx* ctx, const pz_vshape& s, size_t B, int decode, uint8_t* d_bytes, uint64_t* d_words, int32_t* d_elem_status,
                          int32_t* d_status);
