// t-of-T threshold decryption in the host mirror (paillier_halo2_amd/host/paillier_chip.hpp: deal_shamir, PaillierChip::combine_t /
// mod_inverse) on a key of two hard-coded 64-bit safe primes: the mirror deals 3-of-5, the shares lie on one
// polynomial through theta, three trustees open K ciphertexts with the unchanged PaillierChip::partial_decrypt, combine_t returns the
// plaintexts for two different subsets, two trustees are too few; mod_inverse against BigUint arithmetic; the refusals.
#include <cstdio>
#include <random>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x7d50);
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

static const char* P_HEX = "A4E4E25A2BF9133F";
static const char* Q_HEX = "F6CC057211D86F37";

static void test_three_of_five(bool general_g) {
    Context ctx(0);
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const size_t T = 5, t = 3;
    const BigUint one(1), p = BigUint::from_hex(P_HEX), q = BigUint::from_hex(Q_HEX), n = p * q, n2 = n * n;
    BigUint g = n + one;
    if (general_g) g = rand_below(n - BigUint(2)) + BigUint(2);
    auto dealt = deal_shamir(ctx, pc, p, q, T, t, rand_below, true, &g).unwrap();
    const ShamirKey& key = dealt.key;
    const BigUint lambda = ((p - one) * (q - one)) / BigUint::gcd(p - one, q - one), N = n * lambda;
    const BigUint theta = lambda * BigUint::mod_inverse(lambda, n);
    bool shape = dealt.shares.size() == T && key.hs.size() == T && key.v_order_proved && key.n == n && key.g == g && key.trustees == T &&
                 key.threshold == t;
    for (const BigUint& s : dealt.shares) shape = shape && s < N;
    CHECK(shape, general_g ? "deal_shamir 3-of-5, general g: 5 shares below n lambda, 5 public h_i, v's order proved"
                           : "deal_shamir 3-of-5, standard g: 5 shares below n lambda, 5 public h_i, v's order proved");
    // the shares lie on ONE polynomial of degree 2 through theta: the third finite difference vanishes and Newton's backward
    // extrapolation to 0 gives theta:  f(0) = 3 f(1) - 3 f(2) + f(3),  f(4) = f(1) - 3 f(2) + 3 f(3),  f(5) = f(2) - 3 f(3) + 3 f(4)
    const std::vector<BigUint>& s = dealt.shares;
    const BigUint N3 = N.mul_small(3);
    auto comb3 = [&](const BigUint& a, const BigUint& b, const BigUint& c) { return (a + N3 - b.mul_small(3) + c.mul_small(3)) % N; };   // a - 3b + 3c
    CHECK((s[0].mul_small(3) + N3 - s[1].mul_small(3) + s[2]) % N == theta % N && comb3(s[0], s[1], s[2]) == s[3] && comb3(s[1], s[2], s[3]) == s[4],
          "the shares are the values at 1 .. 5 of one polynomial of degree 2 with f(0) = theta");
    std::vector<BigUint> ms{BigUint(), one, n - one, rand_below(n)}, cts;
    for (const BigUint& m : ms) cts.push_back(paillier_enc_native(ctx, n, g, m, rand_below(n - one) + one));
    std::vector<std::vector<BigUint>> us(T);
    bool hs_ok = true;
    for (size_t i = 0; i < T; ++i) {
        PartialDecryption pd = pc.partial_decrypt(ctx, n, key.v, dealt.shares[i], cts).unwrap();
        hs_ok = hs_ok && pd.h == key.hs[i] && pd.us.size() == cts.size();
        us[i] = pd.us;
    }
    CHECK(hs_ok, "every trustee's h = v^(s_i) is its entry of the public key");
    auto opened = [&](const std::vector<uint32_t>& ids) {
        std::vector<std::vector<BigUint>> parts;
        for (uint32_t i : ids) parts.push_back(us[i - 1]);
        std::vector<Decryption> d = pc.combine_t(ctx, key, ids, parts).unwrap();
        bool same = d.size() == ms.size();
        for (size_t j = 0; same && j < ms.size(); ++j) same = d[j].unit && d[j].m == ms[j];
        return same;
    };
    CHECK(opened({1, 2, 3}), "trustees 1, 2, 3 open the messages");
    CHECK(opened({5, 2, 4}), "trustees 5, 2, 4 open the same messages");
    {
        std::vector<Decryption> d = pc.combine_t(ctx, key, {2, 5}, {us[1], us[4]}).unwrap();
        bool none = d.size() == ms.size();
        for (size_t j = 0; none && j < ms.size(); ++j) none = !d[j].unit && d[j].m.is_zero();
        CHECK(none, "two trustees are too few: every entry is flagged and zero");
    }
    {
        std::vector<std::vector<BigUint>> parts{us[0], us[1], us[2]};
        parts[1][2] = us[1][0];
        std::vector<Decryption> d = pc.combine_t(ctx, key, {1, 2, 3}, parts).unwrap();
        bool only = true;
        for (size_t j = 0; j < ms.size(); ++j) only = only && (j == 2 ? !d[j].unit && d[j].m.is_zero() : d[j].unit && d[j].m == ms[j]);
        CHECK(only, "a partial of another ciphertext flags its entry alone");
        parts[0][0] = n2;
        CHECK(pc.combine_t(ctx, key, {1, 2, 3}, parts).err.status == PZ_ERR_RANGE, "combine_t refuses a partial of n^2 (PZ_ERR_RANGE)");
    }
}

static void test_mod_inverse() {
    Context ctx(0);
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint one(1), p = BigUint::from_hex(P_HEX), q = BigUint::from_hex(Q_HEX), n = p * q;
    std::vector<BigUint> xs{one, BigUint(2), n - one, p, BigUint(), q.mul_small(3)};
    for (int i = 0; i < 20; ++i) xs.push_back(rand_below(n));
    std::vector<BigUint> inv = pc.mod_inverse(ctx, n, xs).unwrap();
    bool ok = inv.size() == xs.size();
    for (size_t j = 0; ok && j < xs.size(); ++j) {
        const bool unit = BigUint::gcd(xs[j], n) == one;
        ok = unit ? inv[j] == BigUint::mod_inverse(xs[j], n) && (inv[j] * xs[j]) % n == one && inv[j] < n : inv[j].is_zero();
    }
    CHECK(ok, "mod_inverse == BigUint::mod_inverse for units, zero for p, 0 and 3 q, under n = p q");
    const BigUint big = (one << 4095) + (rand_below(one << 4094) << 1) + one;   // 64 words, the top bit set: x + mod overflows the capacity
    std::vector<BigUint> ys{big - one, big - BigUint(2), (big + one) >> 1, rand_below(big)};
    std::vector<BigUint> yi = pc.mod_inverse(ctx, big, ys).unwrap();
    bool ok2 = yi.size() == ys.size();
    for (size_t j = 0; ok2 && j < ys.size(); ++j)
        ok2 = BigUint::gcd(ys[j], big) == one ? (yi[j] * ys[j]) % big == one && yi[j] < big : yi[j].is_zero();
    CHECK(ok2 && yi[0] == big - one && yi[2] == BigUint(2), "mod_inverse under a 4096-bit modulus with its top bit set: x x^-1 = 1");
    CHECK(pc.mod_inverse(ctx, n, {n}).err.status == PZ_ERR_RANGE && pc.mod_inverse(ctx, n, {n + one}).err.status == PZ_ERR_RANGE,
          "mod_inverse refuses x = mod and x > mod (PZ_ERR_RANGE)");
    CHECK(pc.mod_inverse(ctx, n + one, {one}).err.status == PZ_ERR_INVALID && pc.mod_inverse(ctx, one, {BigUint()}).err.status == PZ_ERR_INVALID &&
              pc.mod_inverse(ctx, BigUint(), {one}).err.status == PZ_ERR_ZERO_MODULUS && pc.mod_inverse(ctx, n, {}).err.status == PZ_ERR_INVALID,
          "mod_inverse refuses an even modulus, 1, 0 and an empty batch");
}

static void test_refusals() {
    Context ctx(0);
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
    const BigUint one(1), p = BigUint::from_hex(P_HEX), q = BigUint::from_hex(Q_HEX);
    auto st = [&](size_t T, size_t t) { return deal_shamir(ctx, pc, p, q, T, t, rand_below).err.status; };
    CHECK(st(0, 1) == PZ_ERR_INVALID && st(257, 1) == PZ_ERR_INVALID && st(3, 0) == PZ_ERR_INVALID && st(3, 4) == PZ_ERR_INVALID,
          "deal_shamir refuses 0 and 257 trustees and a threshold of 0 or above the trustees");
    CHECK(deal_shamir(ctx, pc, p, p, 3, 2, rand_below).err.status == PZ_ERR_INVALID, "deal_shamir refuses p = q");
    CHECK(deal_shamir(ctx, pc, BigUint(5), BigUint(7), 5, 2, rand_below).err.status == PZ_ERR_INVALID, "deal_shamir refuses primes that do not exceed the trustees");
    const BigUint bad_g = p;
    CHECK(deal_shamir(ctx, pc, p, q, 3, 2, rand_below, false, &bad_g).err.status == PZ_ERR_INVALID, "deal_shamir refuses a g whose order n does not divide");
    auto plain = deal_shamir(ctx, pc, p, q, 1, 1, rand_below).unwrap();
    CHECK(!plain.key.v_order_proved && plain.key.hs.size() == 1, "1-of-1 without the caller's word on safe primes: the order of v is not proved");
    CHECK(pc.combine_t(ctx, plain.key, {}, {}).err.status == PZ_ERR_INVALID && pc.combine_t(ctx, plain.key, {1}, {{one}, {one}}).err.status == PZ_ERR_INVALID &&
              pc.combine_t(ctx, plain.key, {2}, {{one}}).err.status == PZ_ERR_INVALID,
          "combine_t refuses no member, answers without ids and an id above the trustees");
}

int main() {
    try {
        test_three_of_five(false);
        test_three_of_five(true);
        test_mod_inverse();
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
