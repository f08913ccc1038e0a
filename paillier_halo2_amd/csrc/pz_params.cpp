// pz_params.cpp -- the ParamsKZG object of the C ABI (include/pz.h): halo2's ParamsKZG::{read_custom, write_custom,
// downsize} and a consistency check of the four sections of a params file.  Host composition of the library's own entry points -- the G1
// codec and curve check (pz_g1_[de]compress_dev, pz_g1_check_dev), the MSM, the NTT, the G1 inverse FFT, the pairing check -- and of the
// G2 kernels of pz_params.hip.  No kernel of its own.
#include <stdlib.h>

#include <new>
#include <vector>

#include "../host/fr_host.hpp"
#include "pz_internal.h"

struct pz_params {
    pz_ctx* ctx = nullptr;
    uint32_t k = 0;
    void* d_g = nullptr;    // 2^k affine points each, device
    void* d_gl = nullptr;
    uint64_t g2[16] = {0}, s_g2[16] = {0};
    pz_bases* bases[2] = {nullptr, nullptr};   // window tables of g / g_lagrange, built on first request
};

namespace {
using pzh::Fr;

constexpr size_t DEFAULT_CHUNK = (size_t)1 << 20;   // points per upload / decode step: 64 MiB of raw points

size_t chunk_points() {
    const char* e = getenv("PZ_PARAMS_CHUNK");
    if (e && *e) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (*end == 0 && v > 0) return (size_t)v;
    }
    return DEFAULT_CHUNK;
}

bool format_ok(int f) { return f == PZ_SERDE_PROCESSED || f == PZ_SERDE_RAW || f == PZ_SERDE_RAW_UNCHECKED; }
size_t g1_bytes(int f) { return f == PZ_SERDE_PROCESSED ? 32 : 64; }
size_t g2_bytes(int f) { return f == PZ_SERDE_PROCESSED ? 64 : 128; }

struct ParamsGuard {   // an object under construction: released unless handed out
    pz_params* p;
    ~ParamsGuard() {
        if (p) pz_params_free(p);
    }
    pz_params* release() {
        pz_params* r = p;
        p = nullptr;
        return r;
    }
};

int new_params(pz_ctx* ctx, uint32_t k, pz_params** out) {
    pz_params* p = new (std::nothrow) pz_params();
    if (!p) return PZ_ERR_OOM;
    p->ctx = ctx;
    p->k = k;
    *out = p;
    const size_t bytes = (size_t)64 << k;
    PZCHK(pz_dev_alloc(ctx, bytes, &p->d_g));
    return pz_dev_alloc(ctx, bytes, &p->d_gl);
}

int derive_lagrange(pz_params* p) {
    const Fr w_inv = pzh::inv(pzh::omega(p->k)), n_inv = pzh::inv(pzh::from_u64((uint64_t)1 << p->k));
    return pz_srs_lagrange_from_monomial_dev(p->ctx, p->k, w_inv.v, n_inv.v, (const uint64_t*)p->d_g, (uint64_t*)p->d_gl);
}

// one G1 section of a file -> d_dst, chunk by chunk; *bad += the points refused
int decode_g1(pz_ctx* ctx, const uint8_t* src, size_t n, int format, size_t chunk, void* stage, void* d_status, std::vector<int32_t>& hst,
              uint64_t* d_dst, uint64_t* bad) {
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t cnt = n - i0 < chunk ? n - i0 : chunk;
        uint64_t* dst = d_dst + 8 * i0;
        if (format == PZ_SERDE_PROCESSED) {
            PZCHK(pz_upload(ctx, stage, src + 32 * i0, 32 * cnt));
            PZCHK(pz_g1_decompress_dev(ctx, (const uint8_t*)stage, cnt, dst, (int32_t*)d_status));
            PZCHK(pz_download(ctx, hst.data(), d_status, 4 * cnt));
            for (size_t j = 0; j < cnt; ++j) *bad += hst[j] != 0;
        } else {
            PZCHK(pz_upload(ctx, dst, src + 64 * i0, 64 * cnt));
            if (format == PZ_SERDE_RAW) {
                uint64_t b = 0;
                PZCHK(pz_g1_check_dev(ctx, dst, cnt, &b));
                *bad += b;
            }
        }
    }
    return PZ_OK;
}

int encode_g1(pz_ctx* ctx, const uint64_t* d_src, size_t n, int format, size_t chunk, void* stage, uint8_t* out) {
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t cnt = n - i0 < chunk ? n - i0 : chunk;
        if (format == PZ_SERDE_PROCESSED) {
            PZCHK(pz_g1_compress_dev(ctx, d_src + 8 * i0, cnt, (uint8_t*)stage));
            PZCHK(pz_download(ctx, out + 32 * i0, stage, 32 * cnt));
        } else {
            PZCHK(pz_download(ctx, out + 64 * i0, d_src + 8 * i0, 64 * cnt));
        }
    }
    return PZ_OK;
}

bool all_zero(const uint64_t* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (v[i]) return false;
    return true;
}

// a uniform element of Fr (up to 2^-2 bias of the 252-bit draw, as the verifier's fold weights), Montgomery
bool random_fr(Fr& out) {
    uint64_t w[4];
    if (!pz_os_random(w, sizeof w)) return false;
    w[3] &= 0x0fffffffffffffffULL;
    out = pzh::from_raw(w);
    return true;
}

// POWERS: e(A, s_g2) e(-B, g2) == 1 for A = sum_{i<n-1} rho^i g[i], B = sum_{i<n-1} rho^i g[i+1]
int check_powers(pz_params* p, const pz_bases* bg, uint32_t nwin, pz_dev_bufs& dev, void* d_mask, void* d_sc, bool* ok) {
    pz_ctx* ctx = p->ctx;
    const size_t n = (size_t)1 << p->k;
    Fr rho;
    if (!random_fr(rho)) return PZ_ERR_INTERNAL;
    // column A = [1, rho, .., rho^(n-2), 0] at element 0, column B = -[0, 1, rho, .., rho^(n-2)] at element n: ones where a power goes,
    // then the powers in place
    PZCHK(pz_dev_memset(ctx, d_mask, 1, 2 * n));
    PZCHK(pz_dev_memset(ctx, (uint8_t*)d_mask + n - 1, 0, 2));
    PZCHK(pz_fr_from_mask_dev(ctx, (const uint8_t*)d_mask, 2 * n, (uint64_t*)d_sc));
    const Fr minus_one = pzh::neg(pzh::FR_ONE);
    PZCHK(pz_fr_distribute_powers_dev(ctx, (uint64_t*)d_sc, 1, 4 * n, n - 1, rho.v, nullptr));
    PZCHK(pz_fr_distribute_powers_dev(ctx, (uint64_t*)d_sc + 4 * (n + 1), 1, 4 * n, n - 1, rho.v, minus_one.v));
    void *d_jac, *d_g1, *d_g2, *d_ok;
    PZCHK(dev.get(2 * 96, &d_jac));
    PZCHK(dev.get(2 * 64, &d_g1));
    PZCHK(dev.get(2 * 128, &d_g2));
    PZCHK(dev.get(4, &d_ok));
    PZCHK(pz_msm_g1_dev(ctx, bg, (const uint64_t*)d_sc, 2, n, 4 * n, 0, nwin, (uint64_t*)d_jac));
    uint64_t jac[24], aff[16], q[32];
    PZCHK(pz_download(ctx, jac, d_jac, sizeof jac));
    PZCHK(pz_g1_normalize(ctx, jac, 2, aff));
    memcpy(q, p->s_g2, 128);
    memcpy(q + 16, p->g2, 128);
    PZCHK(pz_upload(ctx, d_g1, aff, sizeof aff));
    PZCHK(pz_upload(ctx, d_g2, q, sizeof q));
    PZCHK(pz_pairing_check_dev(ctx, (const uint64_t*)d_g1, (const uint64_t*)d_g2, 1, 2, (int32_t*)d_ok));
    int32_t v = 0;
    PZCHK(pz_download(ctx, &v, d_ok, 4));
    *ok = v == 1;
    return PZ_OK;
}

// LAGRANGE: sum_i tau^i g_lagrange[i] == sum_j c_j g[j] for c = iNTT(tau^i): both are [f(s)] G for the f with f(omega^i) = tau^i
int check_lagrange(pz_params* p, const pz_bases* bg, const pz_bases* bl, uint32_t nwin_g, uint32_t nwin_l, pz_dev_bufs& dev, void* d_mask,
                   void* d_sc, bool* ok) {
    pz_ctx* ctx = p->ctx;
    const size_t n = (size_t)1 << p->k;
    Fr tau;
    if (!random_fr(tau)) return PZ_ERR_INTERNAL;
    PZCHK(pz_dev_memset(ctx, d_mask, 1, n));
    PZCHK(pz_fr_from_mask_dev(ctx, (const uint8_t*)d_mask, n, (uint64_t*)d_sc));
    PZCHK(pz_fr_distribute_powers_dev(ctx, (uint64_t*)d_sc, 1, 4 * n, n, tau.v, nullptr));
    uint64_t* d_coeff = (uint64_t*)d_sc + 4 * n;
    PZCHK(pz_dev_copy(ctx, d_coeff, d_sc, 32 * n));
    const Fr w_inv = pzh::inv(pzh::omega(p->k)), n_inv = pzh::inv(pzh::from_u64((uint64_t)n));
    PZCHK(pz_ntt_fr_dev(ctx, d_coeff, 1, 4 * n, w_inv.v, p->k, nullptr, n_inv.v));
    void* d_jac;
    PZCHK(dev.get(2 * 96, &d_jac));
    PZCHK(pz_msm_g1_dev(ctx, bl, (const uint64_t*)d_sc, 1, n, 4 * n, 0, nwin_l, (uint64_t*)d_jac));
    PZCHK(pz_msm_g1_dev(ctx, bg, d_coeff, 1, n, 4 * n, 0, nwin_g, (uint64_t*)d_jac + 12));
    uint64_t jac[24], aff[16];
    PZCHK(pz_download(ctx, jac, d_jac, sizeof jac));
    PZCHK(pz_g1_normalize(ctx, jac, 2, aff));
    *ok = !memcmp(aff, aff + 8, 64);
    return PZ_OK;
}

}   // namespace

extern "C" int pz_params_file_bytes(uint32_t k, int format, size_t* bytes) {
    if (!bytes || !format_ok(format) || k < 1 || k > 28) return PZ_ERR_INVALID;
    *bytes = 4 + 2 * (g1_bytes(format) << k) + 2 * g2_bytes(format);
    return PZ_OK;
}

extern "C" int pz_params_free(pz_params* p) {
    if (!p) return PZ_OK;
    for (pz_bases* b : p->bases)
        if (b) pz_bases_free(p->ctx, b);
    if (p->d_g) pz_dev_free(p->ctx, p->d_g);
    if (p->d_gl) pz_dev_free(p->ctx, p->d_gl);
    delete p;
    return PZ_OK;
}

extern "C" int pz_params_decode(pz_ctx* ctx, const uint8_t* bytes, size_t len, int format, pz_params** out, uint64_t* n_bad) {
    if (n_bad) *n_bad = 0;
    if (!ctx || !bytes || !out || !format_ok(format) || len < 4) return PZ_ERR_INVALID;
    *out = nullptr;
    uint32_t k;
    memcpy(&k, bytes, 4);
    size_t want = 0;
    if (pz_params_file_bytes(k, format, &want) != PZ_OK || want != len) return PZ_ERR_INVALID;
    const size_t n = (size_t)1 << k, pb = g1_bytes(format), qb = g2_bytes(format);
    const size_t chunk = chunk_points() < n ? chunk_points() : n;
    PZ_ENTER(ctx);
    try {
        ParamsGuard g{nullptr};
        PZCHK(new_params(ctx, k, &g.p));
        pz_dev_bufs dev(ctx);
        void *stage = nullptr, *d_status = nullptr;
        std::vector<int32_t> hst;
        if (format == PZ_SERDE_PROCESSED) {
            PZCHK(dev.get(32 * chunk, &stage));
            PZCHK(dev.get(4 * chunk, &d_status));
            hst.resize(chunk);
        }
        uint64_t bad = 0;
        PZCHK(decode_g1(ctx, bytes + 4, n, format, chunk, stage, d_status, hst, (uint64_t*)g.p->d_g, &bad));
        PZCHK(decode_g1(ctx, bytes + 4 + pb * n, n, format, chunk, stage, d_status, hst, (uint64_t*)g.p->d_gl, &bad));
        const uint8_t* q = bytes + 4 + 2 * pb * n;
        uint64_t pair[32];
        int32_t st[2] = {0, 0};
        if (format == PZ_SERDE_PROCESSED) {
            PZCHK(pz_g2_decompress(ctx, q, 2, pair, st, nullptr));
        } else {
            memcpy(pair, q, 2 * qb);
            if (format == PZ_SERDE_RAW) {
                PZCHK(pz_g2_check(ctx, pair, 2, st));
                for (int32_t& s : st)
                    if (s == 3) s = 0;   // on the twist: membership in the subgroup is pz_params_check's question
            }
        }
        bad += (st[0] != 0) + (st[1] != 0);
        if (n_bad) *n_bad = bad;
        if (bad) return PZ_ERR_INVALID;
        memcpy(g.p->g2, pair, 128);
        memcpy(g.p->s_g2, pair + 16, 128);
        PZCHK(pz_sync(ctx));
        *out = g.release();
        return PZ_OK;
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    }
}

extern "C" int pz_params_from_dev(pz_ctx* ctx, uint32_t k, const uint64_t* d_g, const uint64_t* d_g_lagrange, const uint64_t g2[16],
                                  const uint64_t s_g2[16], pz_params** out) {
    if (!ctx || !d_g || !g2 || !s_g2 || !out || k < 1 || k > 28) return PZ_ERR_INVALID;
    *out = nullptr;
    PZ_ENTER(ctx);
    ParamsGuard g{nullptr};
    PZCHK(new_params(ctx, k, &g.p));
    const size_t bytes = (size_t)64 << k;
    PZCHK(pz_dev_copy(ctx, g.p->d_g, d_g, bytes));
    if (d_g_lagrange)
        PZCHK(pz_dev_copy(ctx, g.p->d_gl, d_g_lagrange, bytes));
    else
        PZCHK(derive_lagrange(g.p));
    memcpy(g.p->g2, g2, 128);
    memcpy(g.p->s_g2, s_g2, 128);
    *out = g.release();
    return PZ_OK;
}

extern "C" int pz_params_info(const pz_params* p, uint32_t* k, uint64_t g0_affine[8], uint64_t g2[16], uint64_t s_g2[16]) {
    if (!p) return PZ_ERR_INVALID;
    if (k) *k = p->k;
    if (g2) memcpy(g2, p->g2, 128);
    if (s_g2) memcpy(s_g2, p->s_g2, 128);
    if (g0_affine) PZCHK(pz_download(p->ctx, g0_affine, p->d_g, 64));
    return PZ_OK;
}

extern "C" int pz_params_points(const pz_params* p, const uint64_t** d_g, const uint64_t** d_g_lagrange) {
    if (!p) return PZ_ERR_INVALID;
    if (d_g) *d_g = (const uint64_t*)p->d_g;
    if (d_g_lagrange) *d_g_lagrange = (const uint64_t*)p->d_gl;
    return PZ_OK;
}

extern "C" int pz_params_bases(pz_params* p, int lagrange, const pz_bases** bases) {
    if (!p || !bases) return PZ_ERR_INVALID;
    *bases = nullptr;
    const int which = lagrange ? 1 : 0;
    std::lock_guard<std::recursive_mutex> lock(p->ctx->mu);
    if (!p->bases[which]) {
        PZCHK(pz_bases_load_g1(p->ctx, (const uint64_t*)(which ? p->d_gl : p->d_g), (size_t)1 << p->k, 1, 0, &p->bases[which]));
        p->bases[which]->lagrange = which;
    }
    *bases = p->bases[which];
    return PZ_OK;
}

extern "C" int pz_params_encode(const pz_params* p, int format, uint8_t* out, size_t capacity) {
    if (!p || !out || !format_ok(format)) return PZ_ERR_INVALID;
    size_t want = 0;
    PZCHK(pz_params_file_bytes(p->k, format, &want));
    if (capacity < want) return PZ_ERR_CAPACITY;
    pz_ctx* ctx = p->ctx;
    const size_t n = (size_t)1 << p->k, pb = g1_bytes(format);
    const size_t chunk = chunk_points() < n ? chunk_points() : n;
    PZ_ENTER(ctx);
    pz_dev_bufs dev(ctx);
    void* stage = nullptr;
    if (format == PZ_SERDE_PROCESSED) PZCHK(dev.get(32 * chunk, &stage));
    memcpy(out, &p->k, 4);
    PZCHK(encode_g1(ctx, (const uint64_t*)p->d_g, n, format, chunk, stage, out + 4));
    PZCHK(encode_g1(ctx, (const uint64_t*)p->d_gl, n, format, chunk, stage, out + 4 + pb * n));
    uint8_t* q = out + 4 + 2 * pb * n;
    if (format == PZ_SERDE_PROCESSED) {
        uint64_t pair[32];
        memcpy(pair, p->g2, 128);
        memcpy(pair + 16, p->s_g2, 128);
        PZCHK(pz_g2_compress(ctx, pair, 2, q));
    } else {
        memcpy(q, p->g2, 128);
        memcpy(q + 128, p->s_g2, 128);
    }
    return PZ_OK;
}

extern "C" int pz_params_downsize(const pz_params* p, uint32_t k_new, pz_params** out) {
    if (!p || !out || k_new < 1 || k_new > p->k) return PZ_ERR_INVALID;
    *out = nullptr;
    return pz_params_from_dev(p->ctx, k_new, (const uint64_t*)p->d_g, k_new == p->k ? (const uint64_t*)p->d_gl : nullptr, p->g2, p->s_g2, out);
}

extern "C" int pz_params_check(pz_params* p, uint32_t* failed, uint32_t* skipped) {
    if (!p || !failed) return PZ_ERR_INVALID;
    *failed = 0;
    if (skipped) *skipped = 0;
    pz_ctx* ctx = p->ctx;
    const size_t n = (size_t)1 << p->k;
    PZ_ENTER(ctx);
    try {
        uint32_t f = 0;
        // ---- the points, one by one
        uint64_t bad_g = 0, bad_l = 0;
        PZCHK(pz_g1_check_dev(ctx, (const uint64_t*)p->d_g, n, &bad_g));
        PZCHK(pz_g1_check_dev(ctx, (const uint64_t*)p->d_gl, n, &bad_l));
        if (bad_g || bad_l) f |= PZ_PARAMS_BAD_G1;
        uint64_t pair[32];
        int32_t st[2];
        memcpy(pair, p->g2, 128);
        memcpy(pair + 16, p->s_g2, 128);
        PZCHK(pz_g2_check(ctx, pair, 2, st));
        if (st[0] || st[1] || all_zero(p->g2, 16) || all_zero(p->s_g2, 16)) f |= PZ_PARAMS_BAD_G2;
        uint64_t g0[8];
        PZCHK(pz_download(ctx, g0, p->d_g, 64));
        if (all_zero(g0, 8)) f |= PZ_PARAMS_BAD_G0;
        if (f) {
            *failed = f;
            if (skipped) *skipped = PZ_PARAMS_BAD_POWERS | PZ_PARAMS_BAD_LAGRANGE;
            return PZ_OK;
        }
        // ---- the relations between them
        const pz_bases *bg = nullptr, *bl = nullptr;
        PZCHK(pz_params_bases(p, 0, &bg));
        PZCHK(pz_params_bases(p, 1, &bl));
        uint32_t nwin_g = 0, nwin_l = 0;
        PZCHK(pz_bases_info(bg, nullptr, nullptr, &nwin_g));
        PZCHK(pz_bases_info(bl, nullptr, nullptr, &nwin_l));
        pz_dev_bufs dev(ctx);
        void *d_mask, *d_sc;
        PZCHK(dev.get(2 * n, &d_mask));
        PZCHK(dev.get(2 * n * 32, &d_sc));
        bool ok = false;
        PZCHK(check_powers(p, bg, nwin_g, dev, d_mask, d_sc, &ok));
        if (!ok) f |= PZ_PARAMS_BAD_POWERS;
        PZCHK(check_lagrange(p, bg, bl, nwin_g, nwin_l, dev, d_mask, d_sc, &ok));
        if (!ok) f |= PZ_PARAMS_BAD_LAGRANGE;
        *failed = f;
        return PZ_OK;
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    }
}
