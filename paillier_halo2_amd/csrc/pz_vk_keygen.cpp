// pz_vk_keygen.cpp -- keygen_vk as an entry point of its own (halo2's keygen_vk, reached in the reference at
// /root/reference/src/bench.rs:161-175): the verifying key's commitments from the circuit STRUCTURE alone, for a party that only verifies.
// Host composition of the library's entry points, sharing nothing with pz_pk_*: the selectors are committed from their bytes
// (pz_g1_commit_mask_dev), the constants and table columns in one small MSM, sigma in tiles of columns through ONE reusable buffer
// (pz_permutation_sigma_part_dev + pz_msm_g1_dev).  No transform, no extended form, nothing resident after the call; device memory beyond
// the caller's structure arrays is O(tile 2^k).
#include <new>
#include <vector>

#include "../host/fr_host.hpp"
#include "pz_internal.h"

namespace {
int vk_keygen(pz_ctx* ctx, const pz_bases* bl, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk, const uint8_t* selectors,
              const uint64_t* constants, size_t n_constants, const uint32_t* map_col, const uint32_t* map_row, size_t tile, bool on_device,
              size_t n_instance, uint64_t* fixed_affine, uint64_t* sigma_affine) {
    if (!ctx || !bl || !selectors || !map_col || !map_row || !fixed_affine || !sigma_affine || (n_constants && !constants)) return PZ_ERR_INVALID;
    if (k < 4 || k > 24 || !n_adv || !n_lk || lookup_bits >= k) return PZ_ERR_INVALID;
    if (n_instance > 1) return PZ_ERR_INVALID;
    const size_t n = (size_t)1 << k, A = n_adv, F = A + 2, m = n_adv + n_lk + 1 + n_instance;   // the instance column: the permutation's last
    if (n_constants > n) return PZ_ERR_INVALID;
    if (m > ((size_t)1 << 32) / n) return PZ_ERR_UNSUPPORTED;   // the copy-constraint map addresses cells with 32 bits
    size_t np = 0;
    uint32_t nwin = 0;
    if (pz_bases_info(bl, &np, nullptr, &nwin) != PZ_OK || np < n) return PZ_ERR_INVALID;
    if (tile == 0) tile = 64;
    if (tile > m) tile = m;
    PZ_ENTER(ctx);
    try {
        pz_dev_bufs dev(ctx);
        void *jac_f, *jac_s, *buf;
        PZCHK(dev.get(F * 96, &jac_f));
        PZCHK(dev.get(m * 96, &jac_s));
        PZCHK(dev.get((tile > 2 ? tile : 2) * n * 32, &buf));   // a tile of sigma columns; before that the two small fixed columns
        // ---- selectors: bytes -> commitments
        if (on_device) {
            PZCHK(pz_g1_commit_mask_dev(ctx, bl, selectors, A, n, n, (uint64_t*)jac_f));
        } else {
            const size_t st = tile < A ? tile : A;
            void* up;
            PZCHK(dev.get(st * n, &up));
            for (size_t c0 = 0; c0 < A; c0 += st) {
                const size_t nc = A - c0 < st ? A - c0 : st;
                PZCHK(pz_upload(ctx, up, selectors + c0 * n, nc * n));
                PZCHK(pz_g1_commit_mask_dev(ctx, bl, (const uint8_t*)up, nc, n, n, (uint64_t*)jac_f + c0 * 12));
            }
        }
        // ---- the constants column and the table column 0 .. 2^lookup_bits - 1: one MSM over the rows that can be non-zero
        {
            const size_t tb = (size_t)1 << lookup_bits, ns = n_constants > tb ? n_constants : tb;
            std::vector<pzh::Fr> cols(2 * ns);
            const pzh::Fr zero = {{0, 0, 0, 0}};
            for (size_t i = 0; i < ns; ++i) {
                cols[i] = i < n_constants ? pzh::from_raw(constants + 4 * i) : zero;
                cols[ns + i] = i < tb ? pzh::from_u64(i) : zero;
            }
            PZCHK(pz_upload(ctx, buf, cols.data(), 2 * ns * 32));
            PZCHK(pz_msm_g1_dev(ctx, bl, (const uint64_t*)buf, 2, ns, 4 * ns, 0, nwin, (uint64_t*)jac_f + A * 12));
        }
        // ---- sigma, tile by tile through the one buffer
        const pzh::Fr omega = pzh::omega(k), delta = pzh::delta();
        void *up_c = nullptr, *up_r = nullptr;
        if (!on_device) {
            PZCHK(dev.get(tile * n * 4, &up_c));
            PZCHK(dev.get(tile * n * 4, &up_r));
        }
        for (size_t c0 = 0; c0 < m; c0 += tile) {
            const size_t nc = m - c0 < tile ? m - c0 : tile;
            if (on_device) {
                PZCHK(pz_permutation_sigma_part_dev(ctx, map_col, map_row, m, c0, nc, k, omega.v, delta.v, (uint64_t*)buf, 4 * n));
            } else {
                PZCHK(pz_upload(ctx, up_c, map_col + c0 * n, nc * n * 4));
                PZCHK(pz_upload(ctx, up_r, map_row + c0 * n, nc * n * 4));
                PZCHK(pz_permutation_sigma_tile(ctx, (const uint32_t*)up_c, (const uint32_t*)up_r, m, nc, k, omega.v, delta.v, (uint64_t*)buf, 4 * n));
            }
            PZCHK(pz_msm_g1_dev(ctx, bl, (const uint64_t*)buf, nc, n, 4 * n, 0, nwin, (uint64_t*)jac_s + c0 * 12));
        }
        // ---- affine, one normalisation per family (pz_download synchronises and reports an out-of-range map image as PZ_ERR_ASYNC)
        std::vector<uint64_t> jac(12 * (F > m ? F : m));
        PZCHK(pz_download(ctx, jac.data(), jac_f, F * 96));
        PZCHK(pz_g1_normalize(ctx, jac.data(), F, fixed_affine));
        PZCHK(pz_download(ctx, jac.data(), jac_s, m * 96));
        PZCHK(pz_g1_normalize(ctx, jac.data(), m, sigma_affine));
        return PZ_OK;
    } catch (const std::bad_alloc&) {
        return PZ_ERR_OOM;
    }
}
}   // namespace

extern "C" int pz_vk_keygen_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                                const uint8_t* d_selectors, const uint64_t* constants, size_t n_constants, const uint32_t* d_map_col,
                                const uint32_t* d_map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine) {
    return vk_keygen(ctx, bases_lagrange, k, lookup_bits, n_adv, n_lk, d_selectors, constants, n_constants, d_map_col, d_map_row, tile, true, 0,
                     fixed_affine, sigma_affine);
}
extern "C" int pz_vk_keygen(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                            const uint8_t* selectors, const uint64_t* constants, size_t n_constants, const uint32_t* map_col,
                            const uint32_t* map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine) {
    return vk_keygen(ctx, bases_lagrange, k, lookup_bits, n_adv, n_lk, selectors, constants, n_constants, map_col, map_row, tile, false, 0,
                     fixed_affine, sigma_affine);
}
// the same for a structure with the optional instance column (map_col / map_row u32 [m + n_instance][2^k], sigma_affine (m + n_instance) x 8);
// n_public only has to be consistent with n_instance: the key's commitments do not depend on it
extern "C" int pz_vk_keygen_pub_dev(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                                    size_t n_instance, size_t n_public, const uint8_t* d_selectors, const uint64_t* constants, size_t n_constants,
                                    const uint32_t* d_map_col, const uint32_t* d_map_row, size_t tile, uint64_t* fixed_affine,
                                    uint64_t* sigma_affine) {
    if (n_instance ? n_public == 0 : n_public != 0) return PZ_ERR_INVALID;
    return vk_keygen(ctx, bases_lagrange, k, lookup_bits, n_adv, n_lk, d_selectors, constants, n_constants, d_map_col, d_map_row, tile, true,
                     n_instance, fixed_affine, sigma_affine);
}
extern "C" int pz_vk_keygen_pub(pz_ctx* ctx, const pz_bases* bases_lagrange, uint32_t k, uint32_t lookup_bits, size_t n_adv, size_t n_lk,
                                size_t n_instance, size_t n_public, const uint8_t* selectors, const uint64_t* constants, size_t n_constants,
                                const uint32_t* map_col, const uint32_t* map_row, size_t tile, uint64_t* fixed_affine, uint64_t* sigma_affine) {
    if (n_instance ? n_public == 0 : n_public != 0) return PZ_ERR_INVALID;
    return vk_keygen(ctx, bases_lagrange, k, lookup_bits, n_adv, n_lk, selectors, constants, n_constants, map_col, map_row, tile, false,
                     n_instance, fixed_affine, sigma_affine);
}
