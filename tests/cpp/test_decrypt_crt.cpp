// CRT decryption's host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierSecretKey::create_crt, PaillierChip::decrypt's
// CrtPath, paillier_decrypt_crt_test) on keys and ciphertexts the caller computed with integers of its own:
// argv[1] names a text file of hex values, one per line -- per key: n, g, lambda, d, p, q, the number of ciphertexts B, then B pairs
// (c, expected m); the last pair of every key is a NON-UNIT c (a multiple of a prime of n) with m = 0.
#include <cstdio>
#include <fstream>
#include <string>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static int failures = 0;
#define CHECK(cond, what)                                          \
    do {                                                           \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
        else std::printf("ok   %s\n", what);                       \
    } while (0)

static void test_key(Context& ctx, const PaillierDecryptionCrtInput& in, const BigUint& bad_c) {
    RangeChip range{10};
    char name[200];
    std::snprintf(name, sizeof name, "paillier_decrypt_crt_test: %zu-bit n, %zu ciphertexts: the CRT path = the lambda path = expected, swapped primes too",
                  in.n.bits(), in.cts.size());
    paillier_decrypt_crt_test(ctx, range, in);   // throws on any mismatch
    CHECK(true, name);
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, (unsigned)in.n.bits());
    auto sk = PaillierSecretKey::create_crt(ctx, in.n, in.g, in.lambda, in.d, in.p, in.q).unwrap();
    auto mixed = pc.decrypt(ctx, *sk, {in.cts[0], bad_c, in.cts[0]}, true, CrtPath::Yes);
    auto lam = pc.decrypt(ctx, *sk, {in.cts[0], bad_c, in.cts[0]}, true, CrtPath::No);
    CHECK(mixed.ok && mixed.val[0].unit && !mixed.val[1].unit && mixed.val[2].unit && mixed.val[1].m.is_zero() && mixed.val[1].r.is_zero() &&
              mixed.val[0].m == in.ms[0] && mixed.val[2].m == in.ms[0] && mixed.val[0].r == mixed.val[2].r,
          "a non-unit is flagged alone, its m and r are zero");
    CHECK(lam.ok && lam.val[0].r == mixed.val[0].r && !lam.val[1].unit && lam.val[2].m == mixed.val[2].m, "the lambda path of the same handle agrees");
    CHECK(pc.decrypt(ctx, *sk, {in.cts[0], in.n * in.n}, true, CrtPath::Yes).err.status == PZ_ERR_RANGE,
          "the CRT path refuses a ciphertext equal to n^2 (PZ_ERR_RANGE)");
    CHECK(pc.decrypt(ctx, *sk, {}, true, CrtPath::Yes).err.status == PZ_ERR_INVALID, "the CRT path refuses an empty batch");
    auto plain = PaillierSecretKey::create(ctx, in.n, in.g, in.lambda, in.d).unwrap();
    CHECK(!plain->has_crt() && pc.decrypt(ctx, *plain, in.cts, true, CrtPath::Yes).err.status == PZ_ERR_INVALID,
          "a handle made without the primes has no CRT part, and the CRT path refuses it");
    auto via_auto = pc.decrypt(ctx, *plain, in.cts);
    CHECK(via_auto.ok && via_auto.val[0].m == in.ms[0], "CrtPath::Auto on such a handle is the lambda path");
    CHECK(PaillierSecretKey::create_crt(ctx, in.n, in.g, in.lambda, in.d, in.p + BigUint(2), in.q).err.status == PZ_ERR_INVALID,
          "a key with p + 2 is refused");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: test_decrypt_crt <file of hex values>\n");
        return 2;
    }
    try {
        std::ifstream f(argv[1]);
        std::string s;
        auto next = [&]() {
            if (!(f >> s)) throw std::runtime_error("the input file ends early");
            return BigUint::from_hex(s);
        };
        Context ctx(0);
        size_t keys = 0;
        while (f >> s) {
            PaillierDecryptionCrtInput in;
            in.n = BigUint::from_hex(s);
            in.g = next();
            in.lambda = next();
            in.d = next();
            in.p = next();
            in.q = next();
            const BigUint count = next();
            const size_t B = count.is_zero() ? 0 : (size_t)count.l[0];
            if (B < 2) throw std::runtime_error("a key needs an honest ciphertext and the non-unit");
            BigUint bad_c;
            for (size_t i = 0; i < B; ++i) {
                BigUint c = next(), m = next();
                if (i + 1 == B) bad_c = c;
                else {
                    in.cts.push_back(c);
                    in.ms.push_back(m);
                }
            }
            test_key(ctx, in, bad_c);
            ++keys;
        }
        CHECK(keys > 0, "the input named at least one key");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
