// T-of-T threshold decryption in the host mirror (paillier_halo2_amd/host/paillier_chip.hpp: deal_shares, PaillierChip::partial_decrypt,
// PaillierChip::combine) on a key of two hard-coded 64-bit safe primes: the mirror deals T shares, every
// trustee opens K ciphertexts, the combiner returns the plaintexts PaillierChip::decrypt gives under the full key; a partial taken from
// another trustee flags its entry alone; the refusals.
#include <cstdio>
#include <random>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x7c50);
// (a test's generator: a dealer draws from a CSPRNG)
static BigUint rand_below(const BigUint& k) {
    std::vector<uint64_t> v(k.l.size() + 1);
    for (auto& w : v) w = rng();
    return BigUint::from_limbs(v.data(), v.size()) % k;
}

static int failures = 0;
#define CHECK(cond, what)                                          \
    do {                                                           \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
        else std::printf("ok   %s\n", what);                       \
    } while (0)

static void test_threshold(size_t T, bool general_g) {
    Context ctx(0);
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint one(1), p = BigUint::from_hex("A4E4E25A2BF9133F"), q = BigUint::from_hex("F6CC057211D86F37"), n = p * q, n2 = n * n;
    // a general g: a random value below n (the key handle of PaillierChip::decrypt takes g at n's width); deal_shares refuses it if n
    // does not divide its order, which a random unit's does but for a negligible fraction
    BigUint g = n + one;
    if (general_g) g = rand_below(n - BigUint(2)) + BigUint(2);
    auto dealt = deal_shares(ctx, pc, p, q, T, rand_below, true, &g).unwrap();
    const ThresholdKey& key = dealt.key;
    char name[200];
    std::snprintf(name, sizeof name, "deal_shares T=%zu %s g: T shares below n lambda, T public h_i, v's order proved", T, general_g ? "general" : "standard");
    const BigUint lambda = ((p - one) * (q - one)) / BigUint::gcd(p - one, q - one), N = n * lambda;
    bool shares_ok = dealt.shares.size() == T && key.hs.size() == T && key.v_order_proved && key.n == n && key.g == g;
    BigUint sum;
    for (const BigUint& s : dealt.shares) {
        shares_ok = shares_ok && s < N;
        sum = (sum + s) % N;
    }
    const BigUint theta = lambda * BigUint::mod_inverse(lambda, n);
    CHECK(shares_ok && sum == theta % N && theta % n == one && (theta % lambda).is_zero(), name);
    // K ciphertexts: 0, 1, n - 1, random
    std::vector<BigUint> ms{BigUint(), one, n - one, rand_below(n)}, cts;
    for (const BigUint& m : ms) cts.push_back(paillier_enc_native(ctx, n, g, m, rand_below(n - one) + one));
    std::vector<std::vector<BigUint>> partials;
    bool hs_ok = true;
    for (size_t i = 0; i < T; ++i) {
        PartialDecryption pd = pc.partial_decrypt(ctx, n, key.v, dealt.shares[i], cts).unwrap();
        hs_ok = hs_ok && pd.h == key.hs[i] && pd.us.size() == cts.size();
        partials.push_back(pd.us);
    }
    CHECK(hs_ok, "every trustee's h = v^theta_i is its entry of the public key");
    std::vector<Decryption> comb = pc.combine(ctx, key, partials).unwrap();
    auto sk = PaillierSecretKey::create(ctx, n, g, lambda, BigUint::mod_inverse(n, lambda)).unwrap();
    std::vector<Decryption> full = pc.decrypt(ctx, *sk, cts, false).unwrap();
    bool same = comb.size() == ms.size() && full.size() == ms.size();
    for (size_t j = 0; same && j < ms.size(); ++j) same = comb[j].unit && full[j].unit && comb[j].m == ms[j] && full[j].m == ms[j];
    CHECK(same, "combine == PaillierChip::decrypt under the full key == the messages");
    if (T >= 2) {
        std::vector<std::vector<BigUint>> swapped = partials;
        swapped[1][2] = partials[0][2];
        std::vector<Decryption> bad = pc.combine(ctx, key, swapped).unwrap();
        bool only = true;
        for (size_t j = 0; j < ms.size(); ++j) only = only && (j == 2 ? !bad[j].unit && bad[j].m.is_zero() : bad[j].unit && bad[j].m == ms[j]);
        CHECK(only, "a partial taken from another trustee flags its entry alone");
        std::vector<std::vector<BigUint>> over = partials;
        over[0][0] = n2;
        CHECK(pc.combine(ctx, key, over).err.status == PZ_ERR_RANGE, "combine refuses a partial of n^2 (PZ_ERR_RANGE)");
    }
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint one(1), p = BigUint::from_hex("A4E4E25A2BF9133F"), q = BigUint::from_hex("F6CC057211D86F37"), n = p * q;
    CHECK(deal_shares(ctx, pc, p, q, 0, rand_below).err.status == PZ_ERR_INVALID && deal_shares(ctx, pc, p, q, 257, rand_below).err.status == PZ_ERR_INVALID,
          "deal_shares refuses 0 and 257 trustees");
    CHECK(deal_shares(ctx, pc, p, p, 2, rand_below).err.status == PZ_ERR_INVALID, "deal_shares refuses p = q");
    const BigUint bad_g = p;
    CHECK(deal_shares(ctx, pc, p, q, 2, rand_below, false, &bad_g).err.status == PZ_ERR_INVALID, "deal_shares refuses a g whose order n does not divide");
    auto plain = deal_shares(ctx, pc, p, q, 2, rand_below).unwrap();
    CHECK(!plain.key.v_order_proved && plain.key.hs.size() == 2, "without the caller's word on safe primes the order of v is not proved");
    CHECK(pc.partial_decrypt(ctx, n, plain.key.v, plain.shares[0], {}).err.status == PZ_ERR_INVALID, "partial_decrypt refuses no ciphertext");
    CHECK(pc.partial_decrypt(ctx, n, plain.key.v, plain.shares[0], {n * n}).err.status == PZ_ERR_RANGE, "partial_decrypt refuses a ciphertext of n^2");
    CHECK(pc.partial_decrypt(ctx, n, plain.key.v, one << 256, {one}).err.status == PZ_ERR_RANGE, "partial_decrypt refuses a share of 2^256");
    CHECK(pc.combine(ctx, plain.key, {}).err.status == PZ_ERR_INVALID && pc.combine(ctx, plain.key, {{one}, {}}).err.status == PZ_ERR_INVALID,
          "combine refuses no trustee and a trustee without an answer");
}

int main() {
    try {
        test_threshold(1, false);
        test_threshold(3, false);
        test_threshold(5, true);
        test_refusals();
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
