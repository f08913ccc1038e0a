// prints the key digest (host/key_digest.hpp) of a fixed synthetic key and the challenges of a BOUND and an unbound transcript
// (host/transcript.hpp) over it; tests/test_key_digest.py compares them with hashlib and with prover.key_digest / prover.HashTranscript.
// CPU only, no library: the headers as the compiled drivers include them.
#include <cstdio>
#include <string>
#include <vector>

#include "../../paillier_halo2_amd/host/key_digest.hpp"
#include "../../paillier_halo2_amd/host/transcript.hpp"

static void hex(const char* name, const uint8_t* d, size_t n) {
    printf("%s ", name);
    for (size_t i = 0; i < n; ++i) printf("%02x", d[i]);
    printf("\n");
}

int main() {
    const uint64_t k = 12, bf = 6, n_adv = 5, n_lk = 2, n_instance = 1, n_public = 9;
    std::vector<uint64_t> fixed(8 * (n_adv + 2)), sigma(8 * (n_adv + n_lk + 1 + n_instance));
    for (size_t i = 0; i < fixed.size(); ++i) fixed[i] = 0x9e3779b97f4a7c15ULL * (i + 1);
    for (size_t i = 0; i < sigma.size(); ++i) sigma[i] = 0xbf58476d1ce4e5b9ULL * (i + 3);
    uint8_t d[pzh::KEY_DIGEST_BYTES];
    pzh::key_digest(k, bf, n_adv, n_lk, n_instance, n_public, fixed.data(), sigma.data(), d);
    hex("digest", d, 64);
    const uint64_t index = 5;
    for (int bound = 0; bound < 2; ++bound) {
        pzp::Transcript tr(bound ? d : nullptr, &index, 8);
        tr.common_points(fixed.data(), 3);
        tr.squeeze("a");
        tr.common_scalars(sigma.data(), 2);
        tr.squeeze("b");
        for (auto& c : tr.drawn) hex((std::string(bound ? "bound_" : "plain_") + c.first).c_str(), (const uint8_t*)c.second.v, 32);
    }
    return 0;
}
