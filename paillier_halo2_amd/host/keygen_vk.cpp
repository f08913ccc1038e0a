// keygen_vk.cpp -- DERIVE the verifying key from the circuit's shape alone, from plain C++ over the C ABI (include/pz.h:
// pz_circuit_structure_dev, pz_vk_keygen_dev, pz_g1_compress).  No torch, no HIP call of its own, no Python, no proving key: what a party
// that only verifies runs instead of trusting the prover's key file (halo2's keygen_vk; the reference reaches it at bench.rs:161-175).
//
// usage: keygen_vk <kzg params file> <kind> <enc_bits> <limb_bits> <lookup_bits> <k> <minimum_rows> <blinding_factors> [<exp_g hex> <exp_r hex>] <out.vk>
//   params file: srs.write_params_kzg's ParamsKZG (u32 k, g, g_lagrange, g2, s_g2): only g_lagrange is read -- never a secret
//   kind: encrypt | add | encrypt_uniform (or 0 | 1 | 2), pz_circuit_structure_dev's; encrypt and encrypt_uniform take the two exponents
//   (the message m and the modulus n, hexadecimal: only their bits shape the circuit), add takes none
//   out.vk: "PZVK", u32 version 1, k, blinding_factors, n_adv, n_lk, then the n_adv + 2 fixed and the n_adv + n_lk + 1 sigma commitments,
//   32 compressed bytes each -- the file verify_wire reads and prove_connected writes with PZ_PROVE_WIRE=1, byte for byte
// stdout: one JSON line {"k", "n_adv", "n_lk", "structure_ms", "vk_ms", "digest"}; digest: the key's 64-byte digest in hexadecimal
// (pz_key_digest: what a bound transcript starts from, equal to pz_pk_digest of the prover's key).  Exit 0 ok, 2 on malformed arguments or files or a library error.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pz.h"

namespace {

bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz : 0);
    const bool ok = sz >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

int fail(const char* what) {
    fprintf(stderr, "keygen_vk: %s\n", what);
    return 2;
}

bool parse_u64(const char* s, uint64_t& out) {
    if (!*s) return false;
    char* end = nullptr;
    out = strtoull(s, &end, 10);
    return *end == 0;
}

// hexadecimal (an optional 0x) -> `words` little-endian 64-bit words; false if it has other characters or does not fit
bool parse_hex(const char* s, size_t words, std::vector<uint64_t>& out) {
    if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) s += 2;
    const size_t len = strlen(s);
    if (!len) return false;
    out.assign(words, 0);
    for (size_t i = 0; i < len; ++i) {
        const char c = s[len - 1 - i];
        unsigned v;
        if (c >= '0' && c <= '9') v = (unsigned)(c - '0');
        else if (c >= 'a' && c <= 'f') v = (unsigned)(c - 'a') + 10;
        else if (c >= 'A' && c <= 'F') v = (unsigned)(c - 'A') + 10;
        else return false;
        if (i / 16 >= words) {
            if (v) return false;
            continue;
        }
        out[i / 16] |= (uint64_t)v << (4 * (i % 16));
    }
    return true;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 10 && argc != 12)
        return fail("usage: keygen_vk <kzg params file> <kind> <enc_bits> <limb_bits> <lookup_bits> <k> <minimum_rows> <blinding_factors> "
                    "[<exp_g hex> <exp_r hex>] <out.vk>");
    int kind;
    const std::string ks = argv[2];
    if (ks == "encrypt" || ks == "0") kind = 0;
    else if (ks == "add" || ks == "1") kind = 1;
    else if (ks == "encrypt_uniform" || ks == "2") kind = 2;
    else return fail("kind: encrypt | add | encrypt_uniform");
    if ((kind == 1) != (argc == 10)) return fail("encrypt and encrypt_uniform take <exp_g hex> <exp_r hex>, add takes none");
    uint64_t enc_bits, limb_bits, lookup_bits, k, minimum_rows, bf;
    if (!parse_u64(argv[3], enc_bits) || !parse_u64(argv[4], limb_bits) || !parse_u64(argv[5], lookup_bits) || !parse_u64(argv[6], k) ||
        !parse_u64(argv[7], minimum_rows) || !parse_u64(argv[8], bf))
        return fail("a shape argument is not a number");
    if (limb_bits < 16 || limb_bits > 90 || !enc_bits || enc_bits % limb_bits || enc_bits > (1u << 20) || k < 4 || k > 24 || lookup_bits >= k ||
        bf > 64 || minimum_rows >= ((uint64_t)1 << k))
        return fail("shape out of range");
    const uint32_t limbs_n = (uint32_t)(enc_bits / limb_bits);
    const size_t ew = (size_t)((enc_bits + 63) / 64);
    std::vector<uint64_t> exp_g(ew, 0), exp_r(ew, 0);
    if (argc == 12 && (!parse_hex(argv[9], ew, exp_g) || !parse_hex(argv[10], ew, exp_r))) return fail("an exponent is not hexadecimal or exceeds enc_bits");
    const char* out_path = argv[argc - 1];
    std::vector<uint8_t> params;
    if (!read_file(argv[1], params) || params.size() < 4) return fail("params file");
    uint32_t pk_k;
    memcpy(&pk_k, params.data(), 4);
    const size_t n = (size_t)1 << k;
    if (pk_k != k || params.size() != 4 + 2 * n * 64 + 256) return fail("params file: k or size");
    std::vector<uint64_t> gl(n * 8);
    memcpy(gl.data(), params.data() + 4 + n * 64, n * 64);
    std::vector<uint8_t>().swap(params);

    pz_ctx* ctx = nullptr;
    const int dev = 0;
    if (pz_init(1, &dev, &ctx) != PZ_OK) return fail("pz_init");
    pz_bases* bl = nullptr;
    pz_structure* st = nullptr;
    int rc = pz_srs_load_g1(ctx, (uint32_t)k, gl.data(), 1, &bl);
    const char* where = "pz_srs_load_g1";
    size_t n_adv = 0, n_lk = 0, n_constants = 0;
    double structure_ms = 0, vk_ms = 0;
    std::vector<uint8_t> vkfile;
    uint8_t digest[64] = {0};
    if (rc == PZ_OK) {
        where = "pz_circuit_structure_dev";
        const double t0 = now_ms();
        rc = pz_circuit_structure_dev(ctx, kind, limbs_n, (uint32_t)limb_bits, (uint32_t)lookup_bits, (uint32_t)k, exp_g.data(), exp_r.data(),
                                      (size_t)minimum_rows, (uint32_t)bf, &st);
        if (rc == PZ_OK) rc = pz_sync(ctx);
        structure_ms = now_ms() - t0;
    }
    if (rc == PZ_OK) {
        where = "pz_structure_info";
        rc = pz_structure_info(st, &n_adv, nullptr, &n_lk, nullptr, &n_constants, nullptr, nullptr, nullptr, nullptr);
    }
    if (rc == PZ_OK) {
        const uint8_t* d_sel = nullptr;
        const uint32_t *d_mc = nullptr, *d_mr = nullptr;
        const uint64_t* constants = nullptr;
        where = "pz_structure_arrays";
        rc = pz_structure_arrays(st, &d_sel, &d_mc, &d_mr, nullptr, &constants, nullptr);
        if (rc == PZ_OK) {
            const size_t F = n_adv + 2, m = n_adv + n_lk + 1;
            std::vector<uint64_t> pts(8 * (F + m));
            where = "pz_vk_keygen_dev";
            const double t0 = now_ms();
            rc = pz_vk_keygen_dev(ctx, bl, (uint32_t)k, (uint32_t)lookup_bits, n_adv, n_lk, d_sel, constants, n_constants, d_mc, d_mr, 0, pts.data(),
                                  pts.data() + 8 * F);
            vk_ms = now_ms() - t0;
            if (rc == PZ_OK) {
                where = "pz_key_digest";
                rc = pz_key_digest((uint32_t)k, (uint32_t)bf, n_adv, n_lk, 0, 0, pts.data(), pts.data() + 8 * F, digest);
            }
            if (rc == PZ_OK) {
                vkfile.resize(24 + 32 * (F + m));
                const uint32_t head[5] = {1, (uint32_t)k, (uint32_t)bf, (uint32_t)n_adv, (uint32_t)n_lk};
                memcpy(vkfile.data(), "PZVK", 4);
                memcpy(vkfile.data() + 4, head, 20);
                where = "pz_g1_compress";
                rc = pz_g1_compress(ctx, pts.data(), F + m, vkfile.data() + 24);
            }
        }
    }
    if (rc != PZ_OK) fprintf(stderr, "keygen_vk: %s: %s\n", where, pz_strerror(rc));
    if (st) pz_structure_free(st);
    if (bl) pz_bases_free(ctx, bl);
    pz_free(ctx);
    if (rc != PZ_OK) return 2;
    FILE* f = fopen(out_path, "wb");
    if (!f) return fail("cannot write the key file");
    const bool ok = fwrite(vkfile.data(), 1, vkfile.size(), f) == vkfile.size();
    if (fclose(f) != 0 || !ok) return fail("cannot write the key file");
    char hex[129];
    for (int i = 0; i < 64; ++i) snprintf(hex + 2 * i, 3, "%02x", digest[i]);
    printf("{\"k\": %u, \"n_adv\": %zu, \"n_lk\": %zu, \"structure_ms\": %.2f, \"vk_ms\": %.2f, \"digest\": \"%s\"}\n", (unsigned)k, n_adv, n_lk,
           structure_ms, vk_ms, hex);
    return 0;
}
