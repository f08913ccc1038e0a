// Prime generation in the host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::is_probable_prime / prime_search,
// generate_prime, generate_key, primes_are_safe): the device's verdicts on values whose primality is known,
// generated 64-bit primes checked by a host test that is deterministic for 64 bits, a safe 128-bit key whose safety primes_are_safe
// derives and deal_shares then proves v's order for, three trustees opening a ciphertext under it; the refusals.
#include <cstdio>
#include <random>

#include "../../paillier_halo2_amd/host/paillier_chip.hpp"

using namespace pz;

static std::mt19937_64 rng(0x7e60);
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

// Miller-Rabin over the first twelve primes: deterministic for every 64-bit value
static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((unsigned __int128)a * b % m); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t m) {
    uint64_t r = 1;
    for (a %= m; e; e >>= 1, a = mulmod(a, a, m))
        if (e & 1) r = mulmod(r, a, m);
    return r;
}
static bool is_prime_u64(uint64_t x) {
    if (x < 2) return false;
    for (uint64_t s : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37})
        if (x % s == 0) return x == s;
    uint64_t d = x - 1;
    unsigned r = 0;
    while (!(d & 1)) d >>= 1, ++r;
    for (uint64_t a : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37}) {
        uint64_t y = powmod(a, d, x);
        if (y == 1 || y == x - 1) continue;
        bool comp = true;
        for (unsigned i = 1; i < r && comp; ++i) {
            y = mulmod(y, y, x);
            comp = y != x - 1;
        }
        if (comp) return false;
    }
    return true;
}

struct Rig {
    Context ctx{0};
    RangeChip range{13};
    BigUintChip chip = BigUintChip::construct(&range, 64);
    PaillierChip pc = PaillierChip::construct(&chip, 128);
};

static void test_verdicts(Rig& g) {
    const BigUint one(1);
    const std::vector<uint64_t> bases{2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47};
    const std::vector<BigUint> xs{BigUint(), one, BigUint(2), BigUint(3), BigUint(4), BigUint(561), BigUint(3215031751ull),
                                  (one << 61) - one, (one << 127) - one, (one << 64) + one, ((one << 61) - one) * ((one << 61) - one),
                                  BigUint::from_hex("2BE6951ADC5B22410A5FD"),   // 3317044064679887385961981: passes 2 .. 41, fails 43
                                  (one << 2048) - BigUint(1557), (one << 2048) - BigUint(1559), BigUint(13) * (one << 1000) + one};
    const std::vector<bool> want{false, false, true, true, false, false, false, true, true, false, false, false, true, false, true};
    auto got = g.pc.is_probable_prime(g.ctx, xs, bases).unwrap();
    CHECK(got == want, "is_probable_prime over the bases 2 .. 47: small ends, pseudoprimes, Mersenne primes, a Fermat number, a square, 2^2048 - 1557");
    CHECK(g.pc.is_probable_prime(g.ctx, {one << 2048}, bases).err.status == PZ_ERR_RANGE && g.pc.is_probable_prime(g.ctx, {}, bases).err.status == PZ_ERR_INVALID &&
              g.pc.is_probable_prime(g.ctx, {one}, {}).err.status == PZ_ERR_INVALID && g.pc.is_probable_prime(g.ctx, {one}, {1}).err.status == PZ_ERR_INVALID,
          "is_probable_prime refuses a 2049-bit value, an empty batch, no base and a base below 2");
}

static void test_generate(Rig& g) {
    bool ok = true;
    for (int safe = 0; safe <= 1; ++safe)
        for (int k = 0; k < 3; ++k) {
            const BigUint p = generate_prime(g.ctx, g.pc, 64, safe != 0, 8, rand_below).unwrap();
            const uint64_t v = p.to_limbs(1)[0];
            ok = ok && p.bits() == 64 && (v >> 62) == 3 && is_prime_u64(v) && (!safe || ((v & 3) == 3 && is_prime_u64((v - 1) / 2)));
        }
    CHECK(ok, "generate_prime: 64-bit primes and safe primes with the two top bits set, by a host test that is deterministic at 64 bits");
    const BigUint big = generate_prime(g.ctx, g.pc, 1024, false, 16, rand_below).unwrap();
    CHECK(big.bits() == 1024 && big.bit(1022) && big.bit(0) && g.pc.is_probable_prime(g.ctx, {big}, {2, 3, 5, 7}).unwrap()[0],
          "generate_prime: a 1024-bit prime, two top bits set, passes the bases 2, 3, 5, 7 again");
    CHECK(generate_prime(g.ctx, g.pc, 39, false, 8, rand_below).err.status == PZ_ERR_INVALID && generate_prime(g.ctx, g.pc, 2049, false, 8, rand_below).err.status == PZ_ERR_INVALID &&
              generate_prime(g.ctx, g.pc, 64, false, 0, rand_below).err.status == PZ_ERR_INVALID && generate_prime(g.ctx, g.pc, 64, false, 65, rand_below).err.status == PZ_ERR_INVALID &&
              generate_prime(g.ctx, g.pc, 64, false, 8, rand_below, ((size_t)1 << 20) + 1).err.status == PZ_ERR_INVALID,
          "generate_prime refuses bits outside 40 .. 2048, rounds outside 1 .. 64 and a window above 2^20");
}

static void test_safe_key_into_the_dealer(Rig& g) {
    const BigUint one(1), two(2);
    const PrimePair k = generate_key(g.ctx, g.pc, 128, true, 16, rand_below).unwrap();
    const BigUint n = k.p * k.q, n2 = n * n;
    const uint64_t p = k.p.to_limbs(1)[0], q = k.q.to_limbs(1)[0];
    CHECK(k.p != k.q && n.bits() == 128 && BigUint::gcd(n, (k.p - one) * (k.q - one)) == one && is_prime_u64(p) && is_prime_u64(q) &&
              is_prime_u64((p - 1) / 2) && is_prime_u64((q - 1) / 2),
          "generate_key(128, safe): distinct safe primes, n of exactly 128 bits, gcd(n, phi(n)) = 1");
    const bool safe = primes_are_safe(g.ctx, g.pc, k.p, k.q, 16, rand_below).unwrap();
    const PrimePair plain = generate_key(g.ctx, g.pc, 128, false, 16, rand_below).unwrap();
    const bool plain_safe = is_prime_u64((plain.p.to_limbs(1)[0] - 1) / 2) && is_prime_u64((plain.q.to_limbs(1)[0] - 1) / 2);
    CHECK(safe && primes_are_safe(g.ctx, g.pc, plain.p, plain.q, 16, rand_below).unwrap() == plain_safe &&
              !primes_are_safe(g.ctx, g.pc, k.p, k.p, 16, rand_below).unwrap() && !primes_are_safe(g.ctx, g.pc, (one << 61) - one, k.q, 16, rand_below).unwrap() &&
              primes_are_safe(g.ctx, g.pc, k.p, k.q, 0, rand_below).err.status == PZ_ERR_INVALID,
          "primes_are_safe: true for the safe key, the host's verdict for a plain key, false for p = q and for 2^61 - 1; refuses 0 rounds");
    auto dealt = deal_shares(g.ctx, g.pc, k.p, k.q, 3, rand_below, safe).unwrap();
    CHECK(dealt.key.v_order_proved && dealt.key.n == n && dealt.shares.size() == 3, "deal_shares on the generated key with the derived safe_primes: v's order proved");
    const BigUint m = rand_below(n), c = paillier_enc_native(g.ctx, n, dealt.key.g, m, rand_below(n - one) + one);
    std::vector<std::vector<BigUint>> us;
    bool hs_ok = true;
    for (size_t i = 0; i < 3; ++i) {
        PartialDecryption pd = g.pc.partial_decrypt(g.ctx, n, dealt.key.v, dealt.shares[i], {c}).unwrap();
        hs_ok = hs_ok && pd.h == dealt.key.hs[i];
        us.push_back(pd.us);
    }
    auto opened = g.pc.combine(g.ctx, dealt.key, us).unwrap();
    CHECK(hs_ok && opened.size() == 1 && opened[0].unit && opened[0].m == m, "three trustees open a ciphertext under the generated key");
}

int main() {
    try {
        Rig g;
        test_verdicts(g);
        test_generate(g);
        test_safe_key_into_the_dealer(g);
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
