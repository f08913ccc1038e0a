// verify_connected.cpp -- VERIFY prove_connected's proofs from plain C++ over the C ABI (include/pz.h: pz_vk_create, pz_verify_batch).  No
// torch, no HIP call of its own, no Python: the compiled counterpart of paillier_halo2_amd/verifier.py::verify_batch_native, what a reference
// integrator who makes proofs with the stepper runs to check them.
//
// usage: verify_connected <job file> <kzg params file> <proof file>
//   job file: prove_connected's (the shape: [2] k, [5] blinding_factors, [6] n_adv, [7] n_lk of its u64 header; nothing else is read)
//   params file: srs.write_params_kzg's ParamsKZG (u32 k, g, g_lagrange, g2, s_g2): only g[0], g2 and s_g2 are read -- never a secret
//   proof file: prove_connected's records: "vk/fixed", "vk/sigma" and each proof's "p<i>/c/..." and "p<i>/e/..."; proof i's transcript
//   seed is i as 8 little-endian bytes
// PZ_VERIFY_BIND=1: the proofs are BOUND to the key (prove_connected's PZ_PROVE_BIND=1; pz_vk_bind): each replay starts from the key's digest
//   followed by that seed.  Bound proofs without it, or unbound proofs with it, do not verify (exit 1).
// stdout: one JSON line {"proofs", "verified", "per_proof", "ms"}.  Exit 0 if every proof verified, 1 if any did not, 2 on bad input or a
// library error.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/pz.h"

namespace {

struct Rec {
    uint64_t count = 0, per = 0;
    std::vector<uint64_t> w;
};

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

bool read_records(const char* path, std::map<std::string, Rec>& out) {
    std::vector<uint8_t> b;
    if (!read_file(path, b) || b.size() % 8) return false;
    std::vector<uint64_t> w(b.size() / 8);
    memcpy(w.data(), b.data(), b.size());
    size_t p = 0;
    while (p < w.size()) {
        const uint64_t len = w[p++];
        const uint64_t nw = (len + 7) / 8;
        if (len > 4096 || p + nw + 3 > w.size()) return false;
        const std::string name((const char*)(w.data() + p), len);
        p += nw + 1;   // name, kind
        Rec r;
        r.count = w[p++];
        r.per = w[p++];
        if (r.per && r.count > (w.size() - p) / r.per) return false;
        r.w.assign(w.begin() + p, w.begin() + p + r.count * r.per);
        p += r.count * r.per;
        out[name] = std::move(r);
    }
    return true;
}

int fail(const char* what) {
    fprintf(stderr, "verify_connected: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return fail("usage: verify_connected <job file> <kzg params file> <proof file>");
    std::vector<uint8_t> job, params;
    if (!read_file(argv[1], job) || job.size() < 16 * 8) return fail("job file");
    uint64_t hdr[16];
    memcpy(hdr, job.data(), sizeof hdr);
    if (hdr[0] != 0x435A50) return fail("job file: magic");
    const uint32_t k = (uint32_t)hdr[2], bf = (uint32_t)hdr[5];
    const size_t n_adv = hdr[6], n_lk = hdr[7];
    if (k < 4 || k > 24) return fail("job file: k");
    if (!read_file(argv[2], params) || params.size() < 4) return fail("params file");
    uint32_t pk_k;
    memcpy(&pk_k, params.data(), 4);
    const size_t n = (size_t)1 << k;
    if (pk_k != k || params.size() != 4 + 2 * n * 64 + 256) return fail("params file: k or size");
    uint64_t g0[8], g2[16], s_g2[16];
    memcpy(g0, params.data() + 4, 64);
    memcpy(g2, params.data() + 4 + 2 * n * 64, 128);
    memcpy(s_g2, params.data() + 4 + 2 * n * 64 + 128, 128);
    std::map<std::string, Rec> rec;
    if (!read_records(argv[3], rec)) return fail("proof file");
    const size_t F = n_adv + 2, m = n_adv + n_lk + 1;
    auto it_f = rec.find("vk/fixed"), it_s = rec.find("vk/sigma");
    if (it_f == rec.end() || it_s == rec.end() || it_f->second.w.size() != 8 * F || it_s->second.w.size() != 8 * m)
        return fail("proof file: vk/fixed, vk/sigma");

    pz_ctx* ctx = nullptr;
    const int dev = 0;
    if (pz_init(1, &dev, &ctx) != PZ_OK) return fail("pz_init");
    pz_vk* vk = nullptr;
    int rc = pz_vk_create(ctx, k, bf, n_adv, n_lk, it_f->second.w.data(), it_s->second.w.data(), g0, g2, s_g2, &vk);
    if (rc != PZ_OK) {
        fprintf(stderr, "pz_vk_create: %s\n", pz_strerror(rc));
        pz_free(ctx);
        return 2;
    }
    if (const char* be = getenv("PZ_VERIFY_BIND"))   // the proofs were made bound to their key (prove_connected's PZ_PROVE_BIND=1)
        if (be[0] == '1') pz_vk_bind(vk, 1);
    size_t cw = 0, ew = 0;
    pz_vk_info(vk, &cw, &ew);
    // each proof in the ABI layout: the stepper's outputs in phase order, the records concatenated as they are
    static const char* const coms[10] = {"advice", "lookup_advice", "perm_inputs", "perm_tables", "perm_z", "lookup_z", "random", "h", "w1", "w2"};
    static const char* const evs[10] = {"advice", "lookup_advice", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables", "random", "h"};
    std::vector<uint64_t> proofs;
    std::vector<uint8_t> seeds;
    std::vector<size_t> offs{0};
    size_t B = 0;
    bool bad = false;
    for (;; ++B) {
        const std::string pre = "p" + std::to_string(B) + "/";
        if (!rec.count(pre + "c/advice")) break;
        const size_t start = proofs.size();
        for (const char* c : coms) {
            auto it = rec.find(pre + "c/" + c);
            if (it == rec.end()) { bad = true; break; }
            proofs.insert(proofs.end(), it->second.w.begin(), it->second.w.end());
        }
        for (const char* e : evs) {
            auto it = rec.find(pre + "e/" + e);
            if (bad || it == rec.end()) { bad = true; break; }
            proofs.insert(proofs.end(), it->second.w.begin(), it->second.w.end());
        }
        if (bad || proofs.size() - start != cw + ew) { bad = true; break; }
        for (int b = 0; b < 8; ++b) seeds.push_back((uint8_t)((uint64_t)B >> (8 * b)));
        offs.push_back(seeds.size());
    }
    if (bad || !B) {
        pz_vk_free(vk);
        pz_free(ctx);
        return fail(B ? "proof file: a proof's records do not match the key's shape" : "proof file: no proofs");
    }
    std::vector<int32_t> verdicts(B);
    int all_ok = 0;
    const auto t0 = std::chrono::steady_clock::now();
    rc = pz_verify_batch(vk, proofs.data(), B, seeds.data(), offs.data(), verdicts.data(), nullptr, nullptr, &all_ok);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    pz_vk_free(vk);
    pz_free(ctx);
    if (rc != PZ_OK) {
        fprintf(stderr, "pz_verify_batch: %s\n", pz_strerror(rc));
        return 2;
    }
    printf("{\"proofs\": %zu, \"verified\": %s, \"per_proof\": [", B, all_ok ? "true" : "false");
    for (size_t i = 0; i < B; ++i) printf("%s%s", i ? ", " : "", verdicts[i] ? "true" : "false");
    printf("], \"ms\": %.2f}\n", ms);
    return all_ok ? 0 : 1;
}
