// verify_wire.cpp -- VERIFY proofs that arrive as halo2 wire bytes, from plain C++ over the C ABI (include/pz.h: pz_g1_decompress,
// pz_vk_create, pz_verify_batch_bytes).  No torch, no HIP call of its own, no Python: the compiled counterpart of
// paillier_halo2_amd/verifier.py::verify_batch_bytes, what an integrator who holds `Vec<u8>` proofs runs to check them.
//
// usage: verify_wire <vk file> <kzg params file> <proof bytes file>...
//   vk file: "PZVK", u32 version 1, k, blinding_factors, n_adv, n_lk, then the n_adv + 2 fixed and the n_adv + n_lk + 1 sigma commitments,
//   32 compressed bytes each (prove_connected with PZ_PROVE_WIRE=1 writes it; verifier.vk_to_bytes is the same format)
//   params file: srs.write_params_kzg's ParamsKZG (u32 k, g, g_lagrange, g2, s_g2): only g[0], g2 and s_g2 are read -- never a secret
//   proof bytes files: one proof each, pz_proof_wire_bytes long; proof i's transcript seed is i as 8 little-endian bytes
// PZ_VERIFY_BIND=1: the proofs are BOUND to the key (prove_connected's PZ_PROVE_BIND=1; pz_vk_bind): each replay starts from the key's digest
//   followed by that seed.  Bound proofs without it, or unbound proofs with it, do not verify (exit 1).
// stdout: one JSON line {"proofs", "verified", "per_proof", "ms"}.  Exit 0 if every proof verified, 1 if any did not, 2 on bad input (a vk
// file whose points do not decode included) or a library error.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    fprintf(stderr, "verify_wire: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return fail("usage: verify_wire <vk file> <kzg params file> <proof bytes file>...");
    std::vector<uint8_t> vkf, params;
    if (!read_file(argv[1], vkf) || vkf.size() < 24 || memcmp(vkf.data(), "PZVK", 4)) return fail("vk file");
    uint32_t head[5];
    memcpy(head, vkf.data() + 4, sizeof head);
    const uint32_t k = head[1], bf = head[2];
    const size_t n_adv = head[3], n_lk = head[4];
    if (head[0] != 1) return fail("vk file: version");
    if (k < 4 || k > 24 || !n_adv || !n_lk || n_adv + n_lk >= (1u << 24)) return fail("vk file: shape");
    const size_t F = n_adv + 2, m = n_adv + n_lk + 1;
    if (vkf.size() != 24 + 32 * (F + m)) return fail("vk file: size");
    if (!read_file(argv[2], params) || params.size() < 4) return fail("params file");
    uint32_t pk_k;
    memcpy(&pk_k, params.data(), 4);
    const size_t n = (size_t)1 << k;
    if (pk_k != k || params.size() != 4 + 2 * n * 64 + 256) return fail("params file: k or size");
    uint64_t g0[8], g2[16], s_g2[16];
    memcpy(g0, params.data() + 4, 64);
    memcpy(g2, params.data() + 4 + 2 * n * 64, 128);
    memcpy(s_g2, params.data() + 4 + 2 * n * 64 + 128, 128);
    const size_t B = (size_t)argc - 3;
    std::vector<std::vector<uint8_t>> files(B);
    for (size_t i = 0; i < B; ++i)
        if (!read_file(argv[3 + i], files[i])) return fail("proof bytes file");

    pz_ctx* ctx = nullptr;
    const int dev = 0;
    if (pz_init(1, &dev, &ctx) != PZ_OK) return fail("pz_init");
    std::vector<uint64_t> pts(8 * (F + m));
    uint64_t n_bad = 0;
    int rc = pz_g1_decompress(ctx, vkf.data() + 24, F + m, pts.data(), nullptr, &n_bad);
    if (rc != PZ_OK || n_bad) {
        if (rc != PZ_OK) fprintf(stderr, "pz_g1_decompress: %s\n", pz_strerror(rc));
        pz_free(ctx);
        return fail("vk file: a commitment does not decode");
    }
    pz_vk* vk = nullptr;
    rc = pz_vk_create(ctx, k, bf, n_adv, n_lk, pts.data(), pts.data() + 8 * F, g0, g2, s_g2, &vk);
    if (rc != PZ_OK) {
        fprintf(stderr, "pz_vk_create: %s\n", pz_strerror(rc));
        pz_free(ctx);
        return 2;
    }
    if (const char* be = getenv("PZ_VERIFY_BIND"))   // the proofs were made bound to their key (prove_connected's PZ_PROVE_BIND=1)
        if (be[0] == '1') pz_vk_bind(vk, 1);
    size_t wire = 0;
    pz_proof_wire_bytes(vk, &wire);
    std::vector<uint8_t> bytes, seeds;
    std::vector<size_t> offs{0};
    bool bad = false;
    for (size_t i = 0; i < B && !bad; ++i) {
        bad = files[i].size() != wire;
        bytes.insert(bytes.end(), files[i].begin(), files[i].end());
        for (int b = 0; b < 8; ++b) seeds.push_back((uint8_t)((uint64_t)i >> (8 * b)));
        offs.push_back(seeds.size());
    }
    if (bad) {
        pz_vk_free(vk);
        pz_free(ctx);
        return fail("proof bytes file: not the size of a proof of this key");
    }
    std::vector<int32_t> verdicts(B);
    int all_ok = 0;
    const auto t0 = std::chrono::steady_clock::now();
    rc = pz_verify_batch_bytes(vk, bytes.data(), B, seeds.data(), offs.data(), verdicts.data(), nullptr, nullptr, &all_ok);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    pz_vk_free(vk);
    pz_free(ctx);
    if (rc != PZ_OK) {
        fprintf(stderr, "pz_verify_batch_bytes: %s\n", pz_strerror(rc));
        return 2;
    }
    printf("{\"proofs\": %zu, \"verified\": %s, \"per_proof\": [", B, all_ok ? "true" : "false");
    for (size_t i = 0; i < B; ++i) printf("%s%s", i ? ", " : "", verdicts[i] ? "true" : "false");
    printf("], \"ms\": %.2f}\n", ms);
    return all_ok ? 0 : 1;
}
